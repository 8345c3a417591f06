"""GPU: every tile form of the split-bf16 linear engine (nr_linear_group by way of cluster_backward_hip._linear_group, and
nr_linear_x3) against the fp64 restatement of tests/linear_ref.py, launch by launch over linear_ref.CASES:

  non-conv split-bf16 blocks <1,2,4>, <1,2,2>, <2,2,1>, <2,2,1> on 8 waves, <4,4,1>; the k=3 token convolution read in place on
  <1,2,4>, <1,2,2>, <2,2,1>; one pass on 4 and 8 waves, ring depth 1 and 2; nr_linear_x3's 64 x 128 and 128 x 128 blocks; K-slices
  of wider matrices (row pitch); groups of up to 8 problems and the Python caller's chunking

at block edges, ring edges (fewer K slices than stages, as many, more), all four bias / residual combinations, random and
coherent inputs (tests/test_linear_cpu.py holds the case lists to every variant the dispatcher can pick, and the bars to the
fp32 twin).  Every launch is checked for: the rigorous bar on every entry; the working bar on random inputs; the tighter of the
two that applies once more WITHOUT its A_ll term against the reference without the lo * lo product; finite outputs
although every operand column outside a K-slice and every operand row behind the last one holds NaN; the sentinel words around
and between the outputs; the same bits from a second launch.  The worst ratio to each bar is printed before it is asserted."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import linear_ref as L
from neighborretr_amd import hip
from neighborretr_amd.cluster_backward_hip import _linear_group

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256                                     # sentinel words in front of, between and behind the outputs
PAD_ROWS = 3                                    # NaN rows behind every operand


def _operand(bits, p, rows):
    """Operand bits [rows, k] on the device -> (buffer, address of element [0, 0] of the operand inside it): the leading rows of a
    buffer whose trailing rows are NaN; with a row pitch, columns [off, off + K) of a [rows + PAD_ROWS, ld] matrix of NaN."""
    if bits is None:
        return None, None
    k = bits.shape[1]
    buf = torch.full((rows + PAD_ROWS, p.ld if p.ld else k), L.NAN16, dtype=torch.int16, device=DEV)
    buf[:rows, p.off:p.off + k] = bits
    return buf, buf.data_ptr() + 2 * p.off


@functools.lru_cache(maxsize=2)
def _prepared(name):
    """Inputs, buffers and fp64 references of a case on the device -- made once, shared, never written to."""
    case = L.BY_NAME[name] if name in L.BY_NAME else EXTRA[name]
    out = []
    for i, p in enumerate(case.probs):
        q = L.make_inputs(case, i)
        qd = SimpleNamespace(**{k: None if v is None else v.to(DEV) for k, v in vars(q).items()})
        bufs = [_operand(qd.xh, p, p.M), _operand(qd.xl, p, p.M), _operand(qd.wh, p, p.N), _operand(qd.wl, p, p.N)]
        out.append(SimpleNamespace(p=p, q=qd, keep=[b for b, _ in bufs], addr=[a for _, a in bufs], r=L.reference(p, qd)))
    return case, out


def _launch(case, items):
    """One launch of the case's problems into a fresh sentinel-filled arena -> (arena as int32, [(first, last) word of each output])."""
    where, off = [], GUARD
    for it in items:
        where.append((off, off + it.p.M * it.p.N))
        off += it.p.M * it.p.N + GUARD
    arena = torch.full((off,), L.SENT32, dtype=torch.int32, device=DEV)
    outs = [arena.data_ptr() + 4 * a for a, _ in where]
    if case.family == "x3":
        (it,), vp = items, ctypes.c_void_p
        hip.call("nr_linear_x3", vp(it.addr[0]), vp(it.addr[1]), vp(it.addr[2]), vp(it.addr[3]), hip.ptr(it.q.bias, allow_none=True),
                 hip.ptr(it.q.res, allow_none=True), it.p.M, it.p.N, it.p.K, vp(outs[0]), hip.stream_ptr())
    else:
        _linear_group([(*it.addr, it.q.bias, it.q.res, o, it.p.M, it.p.N, it.p.K, it.p.ld, it.p.conv_n) for it, o in zip(items, outs)])
    torch.cuda.synchronize()
    return arena, where


def _outside_untouched(arena, where):
    keep = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    for a, b in where:
        keep[a:b] = False
    return bool((arena[keep] == L.SENT32).all())


def _check(case, items, arena, where):
    worst_r = worst_w = worst_3 = 0.0
    for i, (it, (a, b)) in enumerate(zip(items, where)):
        got = arena[a:b].view(torch.float32).view(it.p.M, it.p.N).double()
        assert bool(torch.isfinite(got).all()), (case.name, i, "a NaN operand column or row was read into a product")
        err = (got - it.r.ref).abs()
        rr = float((err / it.r.rigorous).max())
        rw = float((err / it.r.working).max()) if case.kind == "randn" else 0.0
        # the rounding alone: the engine leaves lo * lo out exactly, so against the reference WITHOUT that product the same bar
        # holds without its A_ll term (on random signs A_ll is most of the working bar at small K)
        bar3 = (it.r.working if case.kind == "randn" else it.r.rigorous) - it.r.a_ll
        worst_3 = max(worst_3, float(((got - it.r.ref3).abs() / bar3).max()))
        worst_r, worst_w = max(worst_r, rr), max(worst_w, rw)
        if rr > 1.0 or rw > 1.0:
            print(f"linear {case.name} problem {i} {tuple(it.p)}: max|err| {float(err.max()):.3e}, {rr:.3f} of rigorous, {rw:.3f} of working")
    v = "x3" + str(case.variant[:3]) if case.family == "x3" else str(case.variant)
    print(f"linear {v} {case.kind} {case.name}: rigorous {worst_r:.4f} working {worst_w:.4f} rounding-alone {worst_3:.4f}")
    assert worst_r <= 1.0 and worst_w <= 1.0 and worst_3 <= 1.0
    assert _outside_untouched(arena, where), "a launch wrote outside its outputs"


@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_linear_matches_fp64(name):
    case, items = _prepared(name)
    arena, where = _launch(case, items)
    _check(case, items, arena, where)
    again, _ = _launch(case, items)
    assert torch.equal(arena, again), "two launches of the same case differ"


EXTRA = {"grp/chunked11": L.Case("grp/chunked11", "group", "randn", False, tuple(L.CHUNKED11), L.G124)}


@pytest.mark.parametrize("name", ["grp/mixed8", "grp/chunked11"])
def test_group_equals_its_problems_launched_one_by_one(name):
    """Eight different problems in one grid, and eleven through the caller's chunking (8 + 3): the same bits as every problem in a
    launch of its own (the same blocks either way: tests/test_linear_cpu.py), and each inside the bars."""
    case, items = _prepared(name)
    arena, where = _launch(case, items)
    _check(case, items, arena, where)
    for it, (a, b) in zip(items, where):
        single, ((sa, sb),) = _launch(case, [it])
        assert _outside_untouched(single, [(sa, sb)])
        assert torch.equal(single[sa:sb], arena[a:b]), tuple(it.p)
