#!/usr/bin/env python
"""The evaluation with hubness (sharded_metrics_with_hubness, k = 15, one rank) at a given size, for a rocprofv3 kernel trace:
the share of the top-k / occurrence kernels against the slab similarity.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/hubness_profile.py N Nt Nv [iters]
    python tools/hubness_profile.py --summary DIR       # per-kernel totals of the trace database and the share
"""
import glob
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOPK = ("nr_topk_lines_kernel", "nr_topk_merge_kernel", "nr_topk_occurrences_kernel")


def run(N, Nt, Nv, iters):
    import torch
    from neighborretr_amd import modeling, synth
    from neighborretr_amd.evaluator import sharded_metrics_with_hubness
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(7).items()}, strict=False)
    m = m.cuda().eval()
    t, v, tm, vm = (torch.from_numpy(a).cuda() for a in synth.make_samples(4242, "test", N, Nt, Nv))
    args = SimpleNamespace(world_size=1)
    sharded_metrics_with_hubness(m, t, v, tm.float(), vm.float(), args, 15)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        t2v, v2t = sharded_metrics_with_hubness(m, t, v, tm.float(), vm.float(), args, 15)
    torch.cuda.synchronize()
    print(f"N = {N}, tokens {Nt} x {Nv}: {(time.perf_counter() - t0) / iters * 1e3:.2f} ms per evaluation with hubness@15;  "
          f"t2v R@1 {t2v['R1']:.1f} skew {t2v['hubness']['skewness']:.2f};  v2t R@1 {v2t['R1']:.1f} skew {v2t['hubness']['skewness']:.2f}")


def summary(d):
    """Per-kernel totals of the trace database rocprofv3 wrote under d (its `top_kernels` view: name, calls, total us)."""
    import sqlite3
    path = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))[0]
    rows = list(sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"))
    sim = sum(us for name, _, us in rows if name.startswith("void nr_sim"))
    scorer = sum(us for name, _, us in rows if name.startswith("void nr_mlp_kernel") or name.startswith("void nr_prepare_kernel"))
    topk = sum(us for name, _, us in rows if any(k in name for k in TOPK))
    for name, calls, us in rows[:12]:
        print(f"{us:12.1f} us  {calls:5d} calls  {name[:100]}")
    for name, calls, us in rows:
        if any(k in name for k in TOPK):
            print(f"  top-k: {us:10.1f} us  {calls:5d} calls  {name[:100]}")
    print(f"similarity kernel (nr_sim*) {sim:.1f} us; with its token scorer / prepare launches {sim + scorer:.1f} us; "
          f"top-k + occurrence kernels {topk:.1f} us = {100.0 * topk / max(sim, 1e-9):.2f} % of the similarity kernel, "
          f"{100.0 * topk / max(sim + scorer, 1e-9):.2f} % with the scorer")


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 3)
