#!/usr/bin/env python
"""The inverted-file prefilter of two-stage retrieval against the exact prefilter at a given size (text -> video,
every text a query, top 10, one rank, synthetic features): wall times with a device synchronise around them, or -- under rocprofv3
-- the kernels behind them.

    python tools/ivf_profile.py N Nt Nv [iters [C,C,... [L,L,... [D,D,...]]]]     # the table of one gallery size
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/ivf_profile.py N Nt Nv 2 16 128 8
    python tools/ivf_profile.py --summary DIR                                       # per-kernel totals of the trace database

C: candidates per query (default 16,64); L: lists (default 64,128; 0: the exact prefilter alone, for a trace of its own); D: the
divisors of L that give the probes, P = L / D (default 16,8,4).  Two figures per search, each the median over `iters` repeats:
  (a) the candidates stage alone: the queries' preparation and pooled vectors and everything up to the candidate lists, i.e. all
      of GalleryIndex.candidates before ops.local_level_cand
  (b) the whole search (GalleryIndex.search)
The exact prefilter (nprobe=None) is timed in the same process, alternating with the inverted file inside every repeat, so that
drift of a shared machine lands on both alike.  Every call is warmed up once at the shape it is timed at.  build = build_ivf with
its defaults (10 rounds), paid once per gallery; pool = the mean pool length / N; kept = the mean share of the exact prefilter's
candidates that the inverted file's lists hold.
"""
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 10


def run(N, Nt, Nv, iters, cands, lists, divisors):
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

    def stage_a(index, C, P):
        with torch.no_grad():
            q = search._Side(index.model, t, tm, index.query_side)
            return index._prefilter(q.pooled, C, 256, P)[0]

    med = lambda x: float(np.median(x))                                                   # noqa: E731
    gt = torch.arange(N, device="cuda", dtype=torch.int32)[:, None]
    print(f"N = {N}, tokens {Nt} x {Nv}, {N} queries, top {K}; {iters} repeats, median ms; (a) = the candidates stage, (b) = the whole search")
    for L in lists:
        index = search.GalleryIndex(m, v, vm)
        if L:                                                                             # L = 0: the exact prefilter alone (a trace of its own)
            index.build_ivf(L)                                                            # warm-up of the build
            _, build_ms = timed(lambda: index.build_ivf(L))
            sizes = index.ivf.sizes
            print(f"  L = {L}: build_ivf {build_ms:.1f} ms (once per gallery); list sizes min {min(sizes)} / median {int(np.median(sizes))} / max {max(sizes)}")
        for C in cands:
            probes = [None] + ([max(1, L // D) for D in divisors] if L else [])
            a, b, out = {P: [] for P in probes}, {P: [] for P in probes}, {}
            for P in probes:                                                              # warm-up: every call once at its shape
                stage_a(index, C, P)
                out[P] = index.search(t, tm, K, C, nprobe=P)[0]
            for _ in range(iters):
                for P in probes:
                    a[P].append(timed(lambda: stage_a(index, C, P))[1])
                    b[P].append(timed(lambda: index.search(t, tm, K, C, nprobe=P))[1])
            for P in probes:
                r10 = float((out[P] == gt).any(1).float().mean()) * 100
                if P is None:
                    print(f"    C = {C:3d}  exact prefilter   (a) {med(a[P]):8.2f} [{min(a[P]):.2f} .. {max(a[P]):.2f}]  (b) {med(b[P]):8.2f} "
                          f"[{min(b[P]):.2f} .. {max(b[P]):.2f}]  R@10 {r10:5.1f}")
                    continue
                stats = index.candidates(t, tm, C, nprobe=P, ivf_stats=True)[2].double()
                kept = float(torch.where(stats[:, 2] > 0, stats[:, 1] / stats[:, 2].clamp(min=1), torch.ones_like(stats[:, 1])).mean())
                print(f"    C = {C:3d}  IVF P = {P:3d} (L/{L // P:<2d})  (a) {med(a[P]):8.2f} [{min(a[P]):.2f} .. {max(a[P]):.2f}]  (b) {med(b[P]):8.2f} "
                      f"[{min(b[P]):.2f} .. {max(b[P]):.2f}]  (a) / exact (a) = {med(a[P]) / med(a[None]):5.2f}  (b) / exact (b) = "
                      f"{med(b[P]) / med(b[None]):5.2f}  pool {float(stats[:, 0].mean()) / N * 100:5.1f} %  kept {kept * 100:5.1f} %  R@10 {r10:5.1f}")


def summary(d):
    """Per-kernel totals of the trace database rocprofv3 wrote under d (its `top_kernels` view: name, calls, total us)."""
    import sqlite3
    path = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))[0]
    rows = list(sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"))
    for name, calls, us in rows[:24]:
        print(f"{us:12.1f} us  {calls:6d} calls  {us / max(calls, 1):10.1f} us/call  {name[:110]}")
    for what, key in (("candidate scorer (nr_sim_cand_kernel)", "nr_sim_cand_kernel"), ("coarse scores (nr_gemm_nt_f32_kernel)", "nr_gemm_nt_f32_kernel"),
                      ("top-k (nr_topk_lines_kernel)", "nr_topk_lines_kernel"), ("nr_ivf_scan_kernel", "nr_ivf_scan_kernel"),
                      ("nr_ivf_select_kernel", "nr_ivf_select_kernel"), ("nr_ivf_list_sums_kernel", "nr_ivf_list_sums_kernel")):
        hit = [(calls, us) for name, calls, us in rows if key in name]
        print(f"{what}: {sum(us for _, us in hit):.1f} us over {sum(c for c, _ in hit)} launches")
    print(f"all kernels: {sum(us for _, _, us in rows):.1f} us over {sum(c for _, c, _ in rows)} launches")


if __name__ == "__main__":
    if sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        ints = lambda i, default: tuple(int(x) for x in sys.argv[i].split(",")) if len(sys.argv) > i else default       # noqa: E731
        run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 5, ints(5, (16, 64)),
            ints(6, (64, 128)), ints(7, (16, 8, 4)))
