#!/usr/bin/env python
"""The kernel of the paired permutation test of hubness (ops.permtest_hubness, DESIGN.md "Permutation test of hubness") for a rocprofv3
kernel trace, at the two shapes the design notes price: MSR-VTT (1000 lists over a gallery of 1000, k = 15) and MSVD video->text (670
lists over its 27 763 sentences, k = 15).  Lists of popularity + noise: a hubby ranking A against a flatter ranking B.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/hubperm_profile.py [n_perm] [repeats]
    python tools/hubperm_profile.py --summary DIR [n_perm]      # per-launch time of the kernel in the trace, by shape
    python tools/hubperm_profile.py --host [n_perm]             # the NumPy restatement's time for the same calls, one thread
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
KERNEL = "nr_permtest_hubness_kernel"
SHAPES = (("MSR-VTT", 1000, 1000, 15), ("MSVD video->text", 670, 27763, 15))      # name, n_lists, G, k


def _lists(n_lists, G, k, weight, seed):
    """Top-k lists int32 [n_lists, k] of weight * popularity + noise over G items."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pop = np.random.default_rng(4242).standard_normal(G)
    out = np.empty((n_lists, k), dtype=np.int32)
    for q in range(n_lists):
        score = weight * pop + rng.standard_normal(G)
        top = np.argpartition(-score, k)[:k]
        out[q] = top[np.argsort(-score[top], kind="stable")]
    return out


def _case(n_lists, G, k):
    import numpy as np
    gt = (np.arange(n_lists) * (G // n_lists)).astype(np.int32)
    return _lists(n_lists, G, k, 1.0, 1), _lists(n_lists, G, k, 0.5, 2), np.arange(n_lists, dtype=np.int32), G, gt, gt + max(1, G // n_lists)


def run(n_perm, repeats):
    import numpy as np
    import torch
    from neighborretr_amd import ops
    for name, n_lists, G, k in SHAPES:
        a, b, end, _, gb, ge = (torch.from_numpy(x).cuda() if not isinstance(x, int) else x for x in _case(n_lists, G, k))
        call = lambda: ops.permtest_hubness(a, b, end, G, gb, ge, n_perm=n_perm)
        call()                                                                   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeats):
            out = call()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / repeats * 1e3
        print(f"{name}: {n_lists} lists, G = {G}, k = {k}, n_perm = {n_perm}: {ms:.2f} ms per call (the wrapper's checks, the two "
              f"occurrence launches and the host included);  checksum {int(np.asarray(out.sum().cpu()))}")


def summary(d, n_perm):
    """The kernel's launches in trace order are SHAPES in turn, (1 + repeats) each: the stats table has one row per kernel, so the
    per-shape split comes from the kernel trace itself."""
    import csv
    import glob
    traces = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    with open(traces[0], newline="") as f:
        rows = [r for r in csv.DictReader(f) if KERNEL in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = len(rows) // len(SHAPES)
    for i, (name, n_lists, G, k) in enumerate(SHAPES):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * per:(i + 1) * per]]
        med = sorted(us)[len(us) // 2]
        words = float(n_perm) * n_lists * k
        print(f"{name}: {n_lists} lists, G = {G}, k = {k}, n_perm = {n_perm}: {len(us)} launches, median {med:10.1f} us, "
              f"min {min(us):10.1f} us, max {max(us):10.1f} us;  {words / (med * 1e-6) / 1e9:6.2f} G list words/s, LDS "
              f"{4 * G + 576} bytes per workgroup, grid {n_perm} x {rows[i * per].get('Workgroup_Size_X', '?')} threads")


def host(n_perm, sample=5):
    """The restatement's plain loops at 10 000 permutations run for minutes: `sample` permutations are timed and scaled."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hubperm_ref as H
    for name, n_lists, G, k in SHAPES:
        case = _case(n_lists, G, k)
        t0 = time.perf_counter()
        H.hubness_stats(*case, seed=0, p0=0, n_perm=sample)
        s = (time.perf_counter() - t0) / sample
        print(f"{name}: NumPy / Python restatement, one thread: {s * 1e3:.1f} ms per permutation ({sample} timed), "
              f"{s * n_perm:.0f} s for n_perm = {n_perm}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summary":
        summary(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 10000)
    elif len(sys.argv) > 1 and sys.argv[1] == "--host":
        host(int(sys.argv[2]) if len(sys.argv) > 2 else 10000)
    else:
        run(int(sys.argv[1]) if len(sys.argv) > 1 else 10000, int(sys.argv[2]) if len(sys.argv) > 2 else 4)
