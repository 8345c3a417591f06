#!/usr/bin/env python
"""The paired permutation test's two kernels (ops.permtest_rank_stats, ops.permtest_unit_sums, DESIGN.md "Paired permutation tests")
for a rocprofv3 kernel trace: n_perm relabellings of two rankings of U single-entry units, and of two sets of IR columns.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/permtest_profile.py U [n_perm] [repeats]
    python tools/permtest_profile.py --summary DIR U [n_perm]      # per-launch time of both kernels in the trace
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("nr_permtest_rank_stats_kernel", "nr_permtest_unit_sums_kernel")


def run(U, n_perm, repeats):
    import numpy as np
    import torch
    from bootstrap_profile import _ranks                  # the rankings of the bootstrap's profile: R@1 near 45 %, a long tail
    from neighborretr_amd import ops
    from neighborretr_amd.metrics import RetrievalMetrics
    ranks = torch.from_numpy(_ranks(U)).cuda()
    other = torch.flip(ranks, (0,)).contiguous()
    end = torch.arange(U, dtype=torch.int32, device="cuda")
    cols = [torch.from_numpy(RetrievalMetrics.ir_unit_columns(r.cpu().numpy())).cuda() for r in (ranks, other)]
    for name, call in (("rank_stats", lambda: ops.permtest_rank_stats(ranks, end, other, end, n_perm=n_perm)),
                       ("unit_sums", lambda: ops.permtest_unit_sums(cols[0], cols[1], n_perm=n_perm))):
        call()                                                                   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeats):
            out = call()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / repeats * 1e3
        print(f"U = {U}, n_perm = {n_perm}, {name}: {ms:.2f} ms per call (the wrapper's checks and the host included);  "
              f"checksum {int(np.asarray(out.sum().cpu()))}")


def summary(d, U, n_perm):
    from bootstrap_profile import _kernel_totals
    for name, calls, us in _kernel_totals(d):
        if any(k in name for k in KERNELS):
            print(f"U = {U}, n_perm = {n_perm}: {us:12.1f} us  {calls:5d} calls  {us / calls:10.2f} us each  "
                  f"{float(U) * n_perm / (us / calls * 1e-6) / 1e9:8.2f} G units/s per launch  {name[:60]}")


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 10000)
    else:
        run(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 10000, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
