"""CPU: what tests/test_linear_gpu.py relies on, checked without a GPU -- the tile choice of the split-bf16 linear engine as a pure
host function (nr_linear_plan) on every GPU case, the coverage of every kernel variant a shape can reach, the fp32 twin's share
of the rounding bound on the inputs of the GPU cases (the stored FRAC figures are held to it), planted defects against the bars
the GPU tests apply, and the argument checks of the launch."""
import ctypes
import functools
import os
import re

import torch

import linear_ref as L
from neighborretr_amd import hip
from test_frontend_cpu import _held

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUP = hip.NR_EINVAL, hip.NR_EUNSUPPORTED


def _plan(case, probs=None):
    return hip.linear_plan(L.plan_args(case, probs), single=case.family == "x3")


# ---- the dispatch -----------------------------------------------------------------------------------------------------------------
def test_every_case_runs_the_variant_it_names():
    for c in L.CASES:
        assert _plan(c) == (0, c.variant), c.name
        assert len(c.probs) <= hip.LINEAR_GROUP_MAX and (c.family == "group" or len(c.probs) == 1)
    # the problems of the mixed group one by one, and the chunks of eleven, take the same blocks as the group: their outputs are
    # compared bit for bit
    mixed = L.BY_NAME["grp/mixed8"]
    assert list(mixed.probs) == L.MIXED8
    for p in L.CHUNKED11:
        assert _plan(mixed, [p]) == (0, L.G124)
    assert _plan(mixed, L.CHUNKED11[:8]) == _plan(mixed, L.CHUNKED11[8:]) == (0, L.G124)
    assert hip.linear_plan(L.plan_args(mixed, L.CHUNKED11))[0] == EUNSUP                    # more than 8 in ONE launch


def test_the_instantiation_list_is_the_source():
    """L.INSTANTIATIONS = the kernel instantiations of a release build, read from csrc/nr_linear.hip (tuning-only ones left out)."""
    src = open(os.path.join(ROOT, "neighborretr_amd", "csrc", "nr_linear.hip")).read()
    src = re.sub(r"#ifdef NR_TUNE.*?#endif", "", src, flags=re.S)
    src = "\n".join(ln for ln in src.split("\n") if not ln.lstrip().startswith("#define"))
    ints = lambda s: tuple(int(v) for v in s.split(","))
    group = set()
    for m in re.finditer(r"NR_LG1_CASE\(([\d, ]+)\)", src):
        mi, ni, st, wc = ints(m.group(1))
        group.add((mi, ni, st, wc, 0, 1))
    for m in re.finditer(r"NR_LGC_CASE\(([\d, ]+)\)", src):
        group.add(ints(m.group(1)) + (2, 1, 0))
    for m in re.finditer(r"NR_LG8_CASE\(([\d, ]+)\)", src):
        group.add(ints(m.group(1)) + (4, 0, 0))
    for m in re.finditer(r"NR_LG_CASE\(([\d, ]+)\)", src):
        group.add(ints(m.group(1)) + (2, 0, 0))
    x3 = {ints(m.group(1)) + (2, 0, 0) for m in re.finditer(r"nr_linear_launch_s<([\d, ]+)>\(a, st\)", src)}
    assert group == L.INSTANTIATIONS["group"] and x3 == L.INSTANTIATIONS["x3"]


def _sweep():
    """Every variant the dispatcher picks for some shape: tile counts one under, at and one over each threshold (256, 640, 1536
    tiles of 32 x 64; 1024 of 128 x 128; 1024 and 2048 for one pass; 192 and 512 for nr_linear_x3), single problems and the same
    totals cut into groups, plus a coarse grid of shapes."""
    seen = set()

    def ask(family, probs):
        rc, plan = hip.linear_plan(probs, single=family == "x3")
        assert rc == 0, (family, probs)
        seen.add((family, plan))

    around = lambda ts: sorted({t + d for t in ts for d in (-1, 0, 1)})
    for t in around((256, 640, 1536, 1024, 2048)) + [1, 2, 5000, 20000]:
        for one in (False, True):
            ask("group", [(32 * t, 64, 64, 0, 0, one)])                                    # t tiles of 32 x 64, t / 4 of 128 x 128
            ask("group", [(32 * (t - t // 2), 64, 64, 0, 0, one), (32, 64 * (t // 2), 128, 0, 0, one)] if t > 1 else [(1, 1, 64, 0, 0, one)])
        ask("group", [(32 * t, 64, 192, 0, 32)])                                            # conv: samples of 32 rows
    for t in around((1024,)):
        for one in (False, True):
            ask("group", [(128 * t, 128, 64, 0, 0, one)])                                  # t tiles of 128 x 128, 8 t of 32 x 64
        ask("group", [(128 * t, 128, 192, 0, 16)])
    for t in around((192, 512)) + [1, 100, 383, 2000]:
        ask("x3", [(128 * t, 128, 64)])
        ask("x3", [(128, 128 * t, 64)])
        ask("x3", [(64 * t, 128, 64)])                                                      # 64-row blocks: t workgroups
    for M in (1, 100, 700, 3000, 9000):
        for N in (1, 64, 500, 2048, 9000):
            for one in (False, True):
                ask("group", [(M, N, 64, 0, 0, one)])
            ask("group", [(M, N, 192, 0, 1)])
            ask("x3", [(M, N, 64)])
    return seen


def test_the_cases_cover_every_variant_a_shape_can_reach():
    reachable = _sweep()
    every = {(f, v) for f, vs in L.INSTANTIATIONS.items() for v in vs}
    assert reachable <= every
    never = every - reachable
    print("unreachable instantiations:", sorted(never))
    assert never == L.UNREACHABLE
    covered = {(c.family, c.variant) for c in L.CASES}
    assert covered == reachable, (sorted(reachable - covered), sorted(covered - reachable))
    # why the two are dead, in the dispatcher's own terms: one pass on 4 waves means t32x64 / 4 < 256, a one-deep ring there needs
    # t32x64 / 2 >= 512; nr_linear_x3's 64 x 128 block means t128 < 192, so at most 2 t128 < 384 workgroups, one-deep needs 512
    assert 4 * 256 // 2 <= 512 and 2 * 191 < 512
    # randn and coherent inputs, all four flag combinations, in every variant
    for fv in sorted(reachable):
        mine = [c for c in L.CASES if (c.family, c.variant) == fv]
        assert {c.kind for c in mine} == {"randn", "coh"}, fv
        for kind in ("randn", "coh"):
            assert {(p.bias, p.res) for c in mine if c.kind == kind for p in c.probs} == set(L.FLAGS), (fv, kind)


def test_the_cases_stand_on_the_edges_they_name():
    rings = {}
    for c in L.CASES:
        BM, BN = L.block(c.variant)
        for p in c.probs:
            rings.setdefault((c.family, c.variant), set()).add(p.K // 64)
            assert p.K % 64 == 0 and (not p.conv_n or (p.K % 192 == 0 and p.M % p.conv_n == 0 and p.K // 3 <= 1024)), c.name
            if p.ld:
                assert p.ld % 8 == 0 and p.off % 64 == 0 and p.off + p.K <= p.ld and not p.conv_n, c.name
        if c.name.split("/")[-1] == "edges" or "/edges/" in c.name:
            ms, ns = {p.M for p in c.probs}, {p.N for p in c.probs}
            assert {1, BM - 1, BM, BM + 1} <= ms and {1, 15, 16, 17, BN - 1, BN + 1} <= ns, c.name
    ms, ns = ({p.M for c in L.CASES if c.variant == L.X242 for p in c.probs}, {p.N for c in L.CASES if c.variant == L.X242 for p in c.probs})
    assert {1, 63, 64, 65} <= ms and {1, 15, 16, 17, 127, 129} <= ns
    for v in (L.X442, L.X441):                                                              # one past a block multiple, both ways
        assert all(p.M % 128 == 1 and p.N % 128 == 1 for c in L.CASES if (c.family, c.variant) == ("x3", v) for p in c.probs)
    # the rings: fewer slices than stages, as many, more
    G = lambda v: rings[("group", v)]
    assert {1, 2, 3, 4, 5, 24} <= G(L.G124) and {1, 2, 3} <= G(L.G122) and {1, 2, 3} <= G(L.O222) and {1, 2, 3} <= G(L.O228)
    assert all({1, 2, 3} <= rings[("x3", v)] for v in (L.X242, L.X442, L.X441)) and {3, 6, 24} <= G(L.C124)
    for v in (L.G124, L.C124, L.O222, L.X242):                                              # one K = 1536 case per family
        assert any(p.K == 1536 for c in L.CASES if c.variant == v for p in c.probs)
    # conv samples: every size with C in {64, 128, 512}; a sample that ends exactly on a block edge, one that spans two blocks
    for C in (64, 128, 512):
        assert {p.conv_n for c in L.CASES for p in c.probs if p.K == 3 * C} >= set(L.CONV_N)
    assert L.CONV_SAMPLES[32] * 32 == 64 and L.CONV_SAMPLES[33] == 2 and L.CONV_SAMPLES[65] == 1
    lds = {(p.ld - p.K, p.ld // p.K) for c in L.CASES if c.name.startswith("ld/") for p in c.probs}
    assert {(8, 1), (64, 1)} <= lds and any(m == 4 for _, m in lds)
    assert {c.one_pass for c in L.CASES if c.name.startswith("ld/")} == {False, True}
    # tile totals 1, 7, 8, 9 of the small-grid variant (XCD order: the grid is padded to a multiple of 8 workgroups)
    for t in (1, 7, 8, 9):
        c = L.BY_NAME[f"grp/tiles{t}"]
        assert sum(-(-p.M // 32) * -(-p.N // 64) for p in c.probs) == t
    assert len({(p.M, p.N, p.K) for p in L.MIXED8}) == 8 and {(p.bias, p.res) for p in L.MIXED8} == set(L.FLAGS)
    mid = L.BY_NAME["grp/one_tile_between"].probs[1]
    assert mid.M <= 32 and mid.N <= 64


# ---- the reference is right ---------------------------------------------------------------------------------------------------------
def test_the_conv_reference_is_conv1d():
    c = L.Case("cpu/conv", "group", "randn", False, (L.P(6 * 5, 7, 3 * 64, 1, 1, conv_n=5),), L.C124)
    p, q = c.probs[0], L.make_inputs(c, 0)
    r = L.reference(p, q)
    x = (L._val(q.xh, torch.float64) + L._val(q.xl, torch.float64)).view(6, 5, 64)
    w = (L._val(q.wh, torch.float64) + L._val(q.wl, torch.float64)).view(7, 3, 64).permute(0, 2, 1)      # [out, in, tap]
    want = torch.nn.functional.conv1d(x.permute(0, 2, 1), w, padding=1).permute(0, 2, 1).reshape(30, 7)
    want = want + q.bias.double() + q.res.double()
    assert float((r.ref - want).abs().max()) <= 1e-12
    assert float((r.ref3 - r.ref).abs().max()) > 0 and bool((r.working <= r.rigorous).all())
    # the twin stays inside the working bar it defines, and a sequential fp32 sum inside the rigorous one
    t = L.twin(p, q)
    assert bool(((t.double() - r.ref).abs() <= r.working).all())


# ---- the bars are earned ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twin_frac():
    frac = {}
    for c in L.CASES:
        if c.kind != "randn":
            continue
        for i, p in enumerate(c.probs):
            q = L.make_inputs(c, i)
            rows = L.twin_rows(p)
            r = L.reference(p, q)
            t = L.twin(p, q, rows, epilogue=False)
            key = (c.one_pass, p.K)
            frac[key] = max(frac.get(key, 0.0), float(((t.double() - r.prod3[rows]).abs() / r.unit[rows]).max()))
    return frac


def test_stored_frac_is_the_twin_s():
    frac = _twin_frac()
    assert {K for one, K in frac if not one} == set(L.FRAC3) and {K for one, K in frac if one} == set(L.FRAC1)
    for (one, K), f in sorted(frac.items()):
        _held(f"linear {'one pass' if one else 'split'} K={K}", f, (L.FRAC1 if one else L.FRAC3)[K])
        assert L.FACTOR * (L.FRAC1 if one else L.FRAC3)[K] < 1.0                           # the working bar is the tighter one
    assert L.FACTOR == 8.0


def _applied_bar(c, r):
    """The tightest bar tests/test_linear_gpu.py holds a case to: working on randn inputs, rigorous on coherent ones."""
    return r.working if c.kind == "randn" else r.rigorous


def _defect_shows(c, i, **defect):
    p, q = c.probs[i], L.make_inputs(c, i)
    rows = L.twin_rows(p)[:64]
    r = L.reference(p, q)
    bar = _applied_bar(c, r)[rows]
    clean = (L.twin(p, q, rows).double() - r.ref[rows]).abs()
    assert bool((clean <= bar).all()), (c.name, i)                                         # the twin itself passes
    bad = (L.twin(p, q, rows, **defect).double() - r.ref[rows]).abs()
    return float((bad / bar).max()), float((bad / bar).min())


def test_planted_defects_exceed_the_bars():
    n = {k: 0 for k in ("drop", "tap", "cross", "last", "bias")}
    for c in L.CASES:
        for i, p in enumerate(c.probs):
            if p.M * p.N > 2 ** 14 and i > 0:                                              # (the fillers: first problem only)
                continue
            if c.kind == "coh" and not c.one_pass and p.K <= 512:
                for drop in ("lh", "hl"):
                    worst, least = _defect_shows(c, i, drop=drop)
                    assert least > 1.0, (c.name, i, drop, least)                           # EVERY entry is outside the bar
                    n["drop"] += 1
            if c.kind == "randn" and p.conv_n > 1:
                assert _defect_shows(c, i, taps=(-2, 0, 1))[0] > 100.0, (c.name, i)
                assert _defect_shows(c, i, cross=True)[0] > 100.0 or p.M == p.conv_n, (c.name, i)
                n["tap"] += 1
                n["cross"] += p.M != p.conv_n
            if c.kind == "randn" and p.K >= 128 and p.conv_n != 1:                          # (samples of one token: the last tap is all zeros)
                assert _defect_shows(c, i, skip_last=True)[0] > 100.0, (c.name, i)
                n["last"] += 1
            if c.kind == "randn" and p.bias and p.N > 16:
                for d in (16, -16):
                    assert _defect_shows(c, i, bias_shift=d)[0] > 100.0, (c.name, i)
                n["bias"] += 1
    print("planted defects shown:", n)
    assert min(n.values()) >= 8


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_linear_launch_refuses_bad_arguments_before_any_launch():
    """The statuses tests/test_host_cpu.py does not cover, through nr_linear_group itself (refused on the host, nothing launched) and
    through nr_linear_plan, which answers the same."""
    lib = hip.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)

    def probs(n=1, **kw):
        lp = (hip.LinearProblem * n)()
        for a in lp:
            a.x_hi = a.x_lo = a.w_hi = a.w_lo = a.out = ptr
            a.M, a.N, a.K = 64, 64, 192
            for k, v in kw.items():
                setattr(a, k, v)
        return lp

    def both(lp, n=None):
        n = len(lp) if n is None else n
        words = (ctypes.c_int32 * hip.LINEAR_PLAN_WORDS)()
        rc = lib.nr_linear_plan(n, lp, 0, words)
        assert rc != 0 and lib.nr_linear_group(n, lp, None) == rc                           # (refused: nothing is launched)
        return rc

    assert hip.linear_plan(probs()) == (0, L.G124)
    assert both(probs(K=96)) == EINVAL                                                      # K % 64
    assert both(probs(K=128, conv_n=4)) == EINVAL                                           # conv: K % 192
    assert hip.linear_plan(probs(K=192, conv_n=4)) == (0, L.C124)
    assert both(probs(K=64, ld=68)) == EINVAL                                               # ld % 8
    assert hip.linear_plan(probs(K=64, ld=72)) == (0, L.G124)
    assert both(probs(K=192, ld=256, conv_n=4)) == EINVAL                                   # a row pitch together with conv
    lp = probs(2)
    lp[1].conv_n = 4
    assert both(lp) == EINVAL                                                               # conv flags that differ inside a launch
    lp[0].conv_n = 4
    assert hip.linear_plan(lp) == (0, L.C124)
    assert both(probs(conv_n=-1)) == EINVAL
    assert both(probs(9)) == EUNSUP                                                         # n > 8
    assert hip.linear_plan(probs(8))[0] == 0
    assert both(probs(x_lo=None, w_lo=None, conv_n=4)) == EUNSUP                            # one pass has no conv form
    assert both(probs(x_lo=None)) == EINVAL                                                 # half a pair
    words = (ctypes.c_int32 * hip.LINEAR_PLAN_WORDS)()
    assert lib.nr_linear_plan(1, probs(), 0, None) == EINVAL and lib.nr_linear_plan(0, probs(), 0, words) == EINVAL
    # nr_linear_x3's form: one split-bf16 problem, no conv
    assert lib.nr_linear_plan(2, probs(2), 1, words) == EINVAL
    assert lib.nr_linear_plan(1, probs(x_lo=None, w_lo=None), 1, words) == EINVAL
    assert lib.nr_linear_plan(1, probs(conv_n=4), 1, words) == EINVAL
    assert lib.nr_linear_plan(1, probs(K=96), 1, words) == EINVAL
    assert lib.nr_linear_x3(ptr, ptr, ptr, ptr, None, None, 64, 64, 96, ptr, None) == EINVAL
    assert lib.nr_linear_x3(ptr, None, ptr, ptr, None, None, 64, 64, 64, ptr, None) == EINVAL
