#!/usr/bin/env python
"""Local scaling (evaluator._local_scaled_from_slab, one rank) on an N x N fp32 slab, for a rocprofv3 kernel trace: time and
achieved bytes/s of nr_localscale_apply next to nr_sinknorm_apply at the same shape (the same traffic: one slab read, two
vectors, one slab write), and the share of the list kernels (top-k rows, top-k columns) in the run.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/localscale_profile.py N [k] [repeats]
    python tools/localscale_profile.py --summary DIR N     # per-kernel totals of the trace, bytes/s from the slab size
"""
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# slab passes (4 N^2 bytes each) one launch of the kernel makes; the vectors and the [N, k] lists are left out
# (the applies are nr_slab.h's skeleton, named after the family struct it is instantiated with)
PASSES = {"nr_ls_apply": 2, "nr_sn_apply": 2}
SHOWN = ("nr_localscale", "nr_ls_apply", "nr_sn_apply", "nr_topk", "nr_slab_topk")


def run(N, k, repeats):
    import torch
    from neighborretr_amd import evaluator, ops
    g = torch.Generator(device="cuda").manual_seed(4242)
    S = torch.randn((N, N), generator=g, device="cuda") * 0.1               # a planted hub and a diagonal, as a test set has
    S += 0.35 * torch.eye(N, device="cuda")
    S[:, 7] += 0.25
    u, v = torch.zeros((N,), device="cuda"), torch.zeros((N,), device="cuda")
    for mode in evaluator.LOCAL_SCALING_MODES:                              # warm-up: every kernel once
        evaluator._local_scaled_from_slab(S, N, N, 1, 0, mode, k)
    ops.sinknorm_apply(S, 20.0, u, v)
    torch.cuda.synchronize()
    for mode in evaluator.LOCAL_SCALING_MODES:
        t0 = time.perf_counter()
        for _ in range(repeats):
            T = evaluator._local_scaled_from_slab(S, N, N, 1, 0, mode, k)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / repeats * 1e3
        hits = int((T.argmax(1) == 7).sum()), int((S.argmax(1) == 7).sum())
        print(f"N = {N}, k = {k}, {mode}: {ms:.2f} ms per scaling (lists, statistics and apply, host included);  "
              f"top-1 hits of the hub {hits[1]} -> {hits[0]}")
    for _ in range(3 * repeats):                                            # the yardstick: as many launches as the three modes
        ops.sinknorm_apply(S, 20.0, u, v)
    torch.cuda.synchronize()


def _kernel_totals(d):
    """[(name, calls, total us)] of the trace rocprofv3 wrote under d: its kernel_stats.csv (-f csv), or the `top_kernels` view
    of its database."""
    import csv
    import sqlite3
    tables = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if tables:
        with open(tables[0], newline="") as f:
            return [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3) for r in csv.DictReader(f)]
    path = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))[0]
    return list(sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"))


def summary(d, N):
    rows = _kernel_totals(d)
    slab = 4.0 * N * N
    total = lists = 0.0
    for name, calls, us in rows:
        if not any(s in name for s in SHOWN):
            continue
        if "nr_sn_apply" not in name:
            total += us
            if "topk" in name:
                lists += us
        passes = next((p for key, p in PASSES.items() if key in name), 0)
        rate = f"{passes * slab * calls / (us * 1e-6) / 1e12:6.2f} TB/s" if passes else "            "
        print(f"{us:12.1f} us  {calls:5d} calls  {us / calls:9.2f} us each  {rate}  {name[:90]}")
    share = 100.0 * lists / total if total else 0.0
    print(f"N = {N}: slab {slab / 1e6:.1f} MB; local-scaling kernels {total:.1f} us in all, the list kernels {lists:.1f} us ({share:.0f} %)")


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]))
    else:
        run(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 10, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
