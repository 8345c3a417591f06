#!/usr/bin/env python
"""The test-time Sinkhorn normalisation (evaluator._sinkhorn_potentials + nr_sinknorm_apply, one rank) on an N x N fp32 slab,
for a rocprofv3 kernel trace: time and achieved bytes/s of the half-step kernels.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/sinknorm_profile.py N [n_iter] [repeats]
    python tools/sinknorm_profile.py --summary DIR N     # per-kernel totals of the trace database, bytes/s from the slab size
"""
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# slab passes (4 N^2 bytes each) one launch of the kernel makes; the vectors and the 1/32-slab workspace are left out
# (the kernels are nr_slab.h's skeletons, named after the family struct they are instantiated with)
PASSES = {"nr_sn_row": 1, "nr_sn_col": 1, "nr_sn_apply": 2}


def run(N, n_iter, repeats):
    import torch
    from neighborretr_amd import evaluator, ops
    g = torch.Generator(device="cuda").manual_seed(4242)
    S = torch.randn((N, N), generator=g, device="cuda") * 0.1               # a planted hub and a diagonal, as a test set has
    S += 0.35 * torch.eye(N, device="cuda")
    S[:, 7] += 0.25
    log_mu, log_nu = evaluator._log_marginals(N, N, None, "cuda")
    evaluator._sinkhorn_potentials(S, 20.0, log_mu, log_nu, 2, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        u, v, err = evaluator._sinkhorn_potentials(S, 20.0, log_mu, log_nu, n_iter, 1)
        T = ops.sinknorm_apply(S, 20.0, u, v)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / repeats * 1e3
    hits = int((T.argmax(1) == 7).sum()), int((S.argmax(1) == 7).sum())
    print(f"N = {N}, {n_iter} iterations: {ms:.2f} ms per normalisation ({ms / n_iter * 1e3:.1f} us per iteration, host included);  "
          f"marginal_err {err:.3e};  top-1 hits of the hub {hits[1]} -> {hits[0]}")


def summary(d, N):
    """Per-kernel totals of the trace database rocprofv3 wrote under d (its `top_kernels` view: name, calls, total us)."""
    import sqlite3
    path = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))[0]
    rows = list(sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"))
    slab = 4.0 * N * N
    total = 0.0
    for name, calls, us in rows:
        if "nr_sn_" not in name and "nr_hn_" not in name:
            continue
        total += us
        passes = next((p for k, p in PASSES.items() if k in name), 0)
        rate = f"{passes * slab * calls / (us * 1e-6) / 1e12:6.2f} TB/s" if passes else "            "
        print(f"{us:12.1f} us  {calls:5d} calls  {us / calls:9.2f} us each  {rate}  {name[:90]}")
    print(f"N = {N}: slab {slab / 1e6:.1f} MB; normalisation kernels {total:.1f} us in all")


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]))
    else:
        run(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 50, int(sys.argv[3]) if len(sys.argv) > 3 else 2)
