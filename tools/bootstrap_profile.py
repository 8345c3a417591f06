#!/usr/bin/env python
"""The bootstrap of the rank statistics (ops.bootstrap_rank_stats, DESIGN.md "Bootstrap confidence intervals") for a rocprofv3 kernel
trace: n_boot resamples of U single-entry units, one ranking and a paired call, next to the host time of the NumPy restatement of
the hit counts alone.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/bootstrap_profile.py U [n_boot] [repeats]
    python tools/bootstrap_profile.py --summary DIR U [n_boot]      # per-launch time of the kernel in the trace, draws/s
    python tools/bootstrap_profile.py --host U [n_boot]             # the NumPy restatement alone (no GPU)
"""
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KERNEL = "nr_bootstrap_rank_stats_kernel"


def _ranks(U):
    import numpy as np
    rng = np.random.default_rng(4242)                     # R@1 near 45 %, a long tail: what a test set of U queries looks like
    return np.where(rng.random(U) < 0.45, 0, rng.geometric(0.02, U)).astype(np.int32)


def host(U, n_boot):
    import bootstrap_ref as B
    ranks = _ranks(U)
    t0 = time.perf_counter()
    hits = (ranks[B.draws_matrix(0, 0, n_boot, U)] < 1).sum(1)
    print(f"U = {U}, n_boot = {n_boot}: NumPy restatement, draws and one hit count, no medians: {time.perf_counter() - t0:.3f} s "
          f"(mean R@1 {100 * hits.mean() / U:.1f})")


def run(U, n_boot, repeats):
    import torch
    from neighborretr_amd import ops
    ranks = torch.from_numpy(_ranks(U)).cuda()
    other = torch.flip(ranks, (0,)).contiguous()
    end = torch.arange(U, dtype=torch.int32, device="cuda")
    for paired in (False, True):
        args = (ranks, end, other, end) if paired else (ranks, end)
        ops.bootstrap_rank_stats(*args, n_boot=n_boot)                          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeats):
            out = ops.bootstrap_rank_stats(*args, n_boot=n_boot)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / repeats * 1e3
        r1 = 100.0 * out[:, 0, 4].double().mean().item() / U
        print(f"U = {U}, n_boot = {n_boot}, V = {2 if paired else 1}: {ms:.2f} ms per call (the wrapper's checks and the host "
              f"included);  mean R@1 {r1:.1f}")


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


def summary(d, U, n_boot):
    for name, calls, us in _kernel_totals(d):
        if KERNEL in name:
            print(f"U = {U}, n_boot = {n_boot}: {us:12.1f} us  {calls:5d} calls  {us / calls:10.2f} us each (V = 1 and V = 2 launches "
                  f"together)  {float(U) * n_boot / (us / calls * 1e-6) / 1e9:8.2f} G draws/s per pass  {name[:60]}")


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 10000)
    elif sys.argv[1] == "--host":
        host(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 10000)
    else:
        run(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 10000, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
