#!/usr/bin/env python
"""Two-stage retrieval against the exhaustive search at a given size (text -> video, top 10 of every query, one rank, synthetic
features): wall times with a device synchronise around them, or -- under rocprofv3 -- the kernels behind them.

    python tools/two_stage_profile.py N Nt Nv [iters [C,C,...]]       # one table row per search: ms per search, R@1, recall
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/two_stage_profile.py N Nt Nv [iters [C,C,...]]
    python tools/two_stage_profile.py --summary DIR                    # per-kernel totals of the trace database

The exhaustive search is evaluator._slab_similarity + ops.slab_topk_rows (GalleryIndex.search with n_candidates = 0); the two-stage
searches run at C = 16, 64, 128 on one GalleryIndex, whose preparation is timed on its own: it is paid once per gallery.  Every
search is warmed up once at the shape it is timed at; the searches alternate inside every repeat, so that drift of the shared
machine lands on all of them alike.
"""
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CANDIDATES = (0, 16, 64, 128)              # 0: exhaustive
K = 10


def run(N, Nt, Nv, iters):
    import numpy as np
    import torch
    from neighborretr_amd import modeling, search, synth
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(7).items()}, strict=False)
    m = m.cuda().eval()
    t, v, tm, vm = (torch.from_numpy(a).cuda() for a in synth.make_samples(4242, "test", N, Nt, Nv))
    tm, vm = tm.float(), vm.float()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    search.GalleryIndex(m, v, vm)                                      # warm-up of the preparation
    index, build_ms = timed(lambda: search.GalleryIndex(m, v, vm))
    ms = {C: [] for C in CANDIDATES}
    lists = {}
    for C in CANDIDATES:                                               # warm-up: every search once at its shape
        lists[C] = index.search(t, tm, K, C)[0]
    for _ in range(iters):
        for C in CANDIDATES:
            ms[C].append(timed(lambda: index.search(t, tm, K, C))[1])
    gt = torch.arange(N, device="cuda", dtype=torch.int32)[:, None]
    truth = lists[0]
    print(f"N = {N}, tokens {Nt} x {Nv}, {N} queries, top {K}; gallery prepared in {build_ms:.1f} ms (once per gallery); "
          f"{iters} repeats, median [min .. max] ms per search")
    base = float(np.median(ms[0]))
    for C in CANDIDATES:
        r1 = float((lists[C][:, :1] == gt).any(1).float().mean()) * 100
        r10 = float((lists[C] == gt).any(1).float().mean()) * 100
        same = float((lists[C][:, 0] == truth[:, 0]).float().mean()) * 100
        med = float(np.median(ms[C]))
        name = "exhaustive" if C == 0 else f"two-stage C={C}"
        print(f"  {name:18s} {med:10.2f} [{min(ms[C]):.2f} .. {max(ms[C]):.2f}] ms  x{base / med:6.2f}  R@1 {r1:5.1f}  R@10 {r10:5.1f}  "
              f"top-1 equal to the exhaustive search's {same:5.1f} %")


def summary(d):
    """Per-kernel totals of the trace database rocprofv3 wrote under d (its `top_kernels` view: name, calls, total us)."""
    import sqlite3
    path = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))[0]
    rows = list(sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"))
    for name, calls, us in rows[:14]:
        print(f"{us:12.1f} us  {calls:6d} calls  {us / max(calls, 1):10.1f} us/call  {name[:110]}")
    cand = sum(us for name, _, us in rows if "nr_sim_cand_kernel" in name)
    sim = sum(us for name, _, us in rows if name.startswith("void nr_sim") and "nr_sim_cand_kernel" not in name)
    coarse = sum(us for name, _, us in rows if "nr_gemm_nt_f32_kernel" in name)
    topk = sum(us for name, _, us in rows if "nr_topk" in name)
    print(f"exhaustive similarity kernels (nr_sim*) {sim:.1f} us; candidate scorer (nr_sim_cand_kernel) {cand:.1f} us; "
          f"coarse scores (nr_gemm_nt_f32_kernel) {coarse:.1f} us; top-k kernels {topk:.1f} us")


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        if len(sys.argv) > 5:                              # e.g. 0,64: only these searches (a trace with one list length)
            CANDIDATES = (0,) + tuple(int(c) for c in sys.argv[5].split(",") if int(c))      # the exhaustive search is the yardstick
        run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 3)
