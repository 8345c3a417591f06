#!/usr/bin/env python
"""Mutual proximity (evaluator._mutual_proximity_from_slab, one rank) on an N x N fp32 slab, for a rocprofv3 kernel trace: the time
of the two count kernels (N^3 compare pairs each) next to the paper estimate of DESIGN.md "Mutual proximity", and of the moment
and apply kernels.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/mutualprox_profile.py N [repeats]
    python tools/mutualprox_profile.py --summary DIR N [repeats]     # per-kernel totals of the trace, pairs/s of the count kernels
"""
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNT_KERNELS = ("nr_mp_row_counts_kernel", "nr_mp_col_counts_kernel")      # N^3 compare pairs per launch
VALU_PER_PAIR = 4                                                           # two compares, a select and an add with carry
SHOWN = ("nr_mp_",)


def run(N, repeats):
    import torch
    from neighborretr_amd import evaluator
    g = torch.Generator(device="cuda").manual_seed(4242)
    S = torch.randn((N, N), generator=g, device="cuda") * 0.1               # a planted hub and a diagonal, as a test set has
    S += 0.35 * torch.eye(N, device="cuda")
    S[:, 7] += 0.25
    for mode in evaluator.MUTUAL_PROXIMITY_MODES:                           # warm-up: every kernel once
        evaluator._mutual_proximity_from_slab(S, N, N, 1, 0, mode)
    torch.cuda.synchronize()
    for mode in evaluator.MUTUAL_PROXIMITY_MODES:
        t0 = time.perf_counter()
        for _ in range(repeats):
            T = evaluator._mutual_proximity_from_slab(S, N, N, 1, 0, mode)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / repeats * 1e3
        hits = int((T.argmax(1) == 7).sum()), int((S.argmax(1) == 7).sum())
        print(f"N = {N}, {mode}: {ms:.2f} ms per correction (every kernel, host included);  top-1 hits of the hub {hits[1]} -> {hits[0]}")


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
    pairs = float(N) ** 3
    total = counts = 0.0
    for name, calls, us in _kernel_totals(d):
        if not any(s in name for s in SHOWN):
            continue
        total += us
        rate = "                                  "
        if any(k in name for k in COUNT_KERNELS):
            counts += us
            per = us / calls * 1e-6
            rate = f"{pairs / per / 1e12:6.2f} Tpairs/s {VALU_PER_PAIR * pairs / per / 1e12:6.1f} Tlane-op/s"
        print(f"{us:12.1f} us  {calls:5d} calls  {us / calls:10.2f} us each  {rate}  {name[:80]}")
    share = 100.0 * counts / total if total else 0.0
    print(f"N = {N}: {pairs:.3e} pairs per count launch; mutual-proximity kernels {total:.1f} us in all, the count kernels "
          f"{counts:.1f} us ({share:.0f} %)")


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]))
    else:
        run(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 3)
