#!/usr/bin/env python
"""What mutual proximity costs two-stage retrieval (text -> video, every text a query, one rank, synthetic
features): wall times with a device synchronise around them, or -- under rocprofv3 -- the kernels behind them.

    python tools/two_stage_mutualprox_profile.py N Nt Nv C M [iters]      # median [min .. max] ms of each search and of attach_mutualprox
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/two_stage_mutualprox_profile.py N Nt Nv C M [iters]
    python tools/two_stage_mutualprox_profile.py --summary DIR             # per-kernel totals of the trace database

Timed: the raw search (`index.search(t, tm, 10, C)`: candidates + the four launches of search.rerank; the code path of the parent
commit, which this feature does not touch -- the yardstick), the searches with `mutual_proximity="emp" | "gauss"` (candidates + ONE
nr_cand_mutualprox_rerank launch), `local_scaling="csls"` and `norm="is"` (the sibling kernels, so that one trace holds all three)
and `attach_mutualprox` with M bank texts, which is paid once per gallery.  Every call is warmed up once at its shape; the searches
alternate inside every repeat, so that drift of the shared machine lands on all of them alike.
"""
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, LS_K = 10, 10
MODES = ("emp", "gauss")
KERNELS = ("nr_cand_mutualprox_rerank_kernel<0>", "nr_cand_mutualprox_rerank_kernel<1>", "nr_cand_localscale_rerank_kernel",
           "nr_cand_norm_rerank_kernel")


def run(N, Nt, Nv, C, M, iters):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from neighborretr_amd import modeling, search, synth
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(7).items()}, strict=False)
    m = m.cuda().eval()
    t, v, tm, vm = (torch.from_numpy(a).cuda() for a in synth.make_samples(4242, "test", N, Nt, Nv))
    bt, _, btm, _ = (torch.from_numpy(a).cuda() for a in synth.make_samples(77, "train", M, Nt, Nv))
    tm, vm, btm = tm.float(), vm.float(), btm.float()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    index = search.GalleryIndex(m, v, vm).attach_mutualprox(bt, btm).attach_localscale(bt, btm, LS_K).attach_querybank(bt, btm)
    calls = {"raw search": lambda: index.search(t, tm, K, C)}
    for mode in MODES:
        calls[f"search {mode}"] = lambda mode=mode: index.search(t, tm, K, C, mutual_proximity=mode)
    calls["search csls"] = lambda: index.search(t, tm, K, C, local_scaling="csls")
    calls["search norm=is"] = lambda: index.search(t, tm, K, C, norm="is")
    calls["attach_mutualprox"] = lambda: index.attach_mutualprox(bt, btm)
    out = {name: fn() for name, fn in calls.items()}                   # warm-up: every call once at its shape
    ms = {name: [] for name in calls}
    for _ in range(iters):
        for name, fn in calls.items():
            ms[name].append(timed(fn)[1])
    n_slots = int((index.candidates(t, tm, C)[0] >= 0).sum())
    print(f"N = {N}, tokens {Nt} x {Nv}, {N} queries, C = {C}, top {K}, bank of {M} texts ({4e-6 * M * N:.1f} MB of item lines; emp reads "
          f"{4e-6 * M * n_slots:.0f} MB of them per search); {iters} repeats, median [min .. max] ms")
    for name in calls:
        print(f"  {name:20s} {float(np.median(ms[name])):9.3f} [{min(ms[name]):.3f} .. {max(ms[name]):.3f}] ms")
    gt = torch.arange(N, device="cuda", dtype=torch.int32)[:, None]
    for name in ["raw search"] + [f"search {mode}" for mode in MODES]:
        idx = out[name][0]
        occ = torch.bincount(idx[:, 0].clamp(min=0).long(), minlength=N)
        print(f"  {name:20s} R@1 {float((idx[:, :1] == gt).any(1).float().mean()) * 100:5.1f}  R@10 "
              f"{float((idx == gt).any(1).float().mean()) * 100:5.1f}  max N_1 {int(occ.max())}")


def summary(d):
    """Per-kernel totals of the trace database rocprofv3 wrote under d (its `top_kernels` view: name, calls, total us)."""
    import sqlite3
    path = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))[0]
    rows = list(sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"))
    for name, calls, us in rows[:16]:
        print(f"{us:12.1f} us  {calls:6d} calls  {us / max(calls, 1):10.1f} us/call  {name[:110]}")
    for name, calls, us in rows:
        for kernel in KERNELS:
            if kernel in name:
                print(f"{kernel}: {us / max(calls, 1):.1f} us per launch over {calls} launches")


if __name__ == "__main__":
    argv = sys.argv[1:]
    if len(argv) < 2 or (argv[0] != "--summary" and len(argv) < 5):
        sys.exit("usage: two_stage_mutualprox_profile.py N Nt Nv C M [iters]  |  --summary DIR")
    if argv[0] == "--summary":
        summary(argv[1])
    else:
        N, Nt, Nv, C, M = (int(a) for a in argv[:5])
        run(N, Nt, Nv, C, M, int(argv[5]) if len(argv) > 5 else 5)
