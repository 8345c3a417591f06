"""GPU: every launch form of the fused similarity forward (nr_local_level_fwd: csrc/nr_sim_reg.hip, csrc/nr_sim.hip, the tile
engine csrc/nr_gemm_tile.h) against the fp64 restatement of tests/simfwd_ref.py.

Each case FIRST asserts, through nr_local_level_plan, that its shape runs the form it was chosen for (simfwd_ref.FORMS) and fails
-- not skips -- if a picker has moved.  Then, on operand planes made in stock torch on the CPU (the very planes the twin of
tests/test_simfwd_cpu.py ran on), with the reference evaluated in fp64 on the device:

  operand tier   S on all pairs, the pooled maxima and the row / column sum forms against the same function of the bf16 planes;
                 bars = simfwd_ref.bars (8 x the fp32 twin, capped by the any-order bound and by today's bars), never set from
                 the kernel's output.  Arg-max: the reference's product at the kernel's index equals the reference's maximum
                 within the bar (near-ties make anything stricter a coin toss).
  exact tier     S against fp64 of the fp32 inputs at today's bars: 2e-6 split-bf16, 1e-3 one pass.
  tie tier       operands whose every sum is exact in fp32 in any order (simfwd_ref.make_exact_inputs): S, pmax, qmax and both
                 sum forms equal fp64 bit for bit, the arg-max indices equal the FIRST maximum, ties among masked tokens included.

Every output lives in a sentinel-filled allocation: 256 elements on either side of it do not move, and it is written whole.
The measured maxima are printed per case (pytest -s)."""
import ctypes
import functools
import math

import pytest
import torch

import simfwd_ref as R
from neighborretr_amd import hip, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
PREC = {"bf16": hip.PREC_BF16, "x3": hip.PREC_BF16X3}
GUARD, SENT = 256, -77.25
MODES = (hip.OUT_FULL, hip.OUT_ROWSUM, hip.OUT_COLSUM)


def _id(c):
    return "-".join(map(str, c))


def _plan_of(case):
    return next(c[6] for c in R.FORMS if c[:6] == case)


def _assert_plan(case):
    Nt, Nv, A, Bv, d, p = case
    want, got = _plan_of(case), hip.local_level_plan(A, Nt, Bv, Nv, d, PREC[p])
    assert got == want, f"{case}: the launch is now {got}, this case was chosen for {want}"
    return want


class Guarded:
    """A tensor inside a sentinel-filled allocation."""

    def __init__(self, shape, dtype=torch.float32):
        self.n = math.prod(shape)
        self.sent = SENT if dtype == torch.float32 else 0xA5
        self.buf = torch.full((self.n + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)

    def untouched_around(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[GUARD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.buf == self.sent).all())


@functools.lru_cache(maxsize=2)
def _device_inputs(case, exact):
    x = (R.make_exact_inputs if exact else R.make_inputs)(case)
    planes = tuple(p.to(DEV).contiguous() for p in x["planes"])
    return x, planes, x["w_t"].to(DEV).contiguous(), x["w_v"].to(DEV).contiguous()


def _out_shape(case, mode):
    Nt, Nv, A, Bv, d, p = case
    if mode == hip.OUT_FULL:
        return (A, Bv)
    nr, nc = hip.local_level_tiles(A, Nt, Bv, Nv, PREC[p])
    return (nc, A) if mode == hip.OUT_ROWSUM else (nr, Bv)


def _launch(case, planes, w_t, w_v, mode, want_arg, expect=0):
    """One nr_local_level_fwd call into guarded outputs -> (out, aux or None) as tensors; asserts the return code, that nothing
    around an output moved and that (expect == 0) every output element was written, or (a refusal) none."""
    Nt, Nv, A, Bv, d, p = case
    out = Guarded(_out_shape(case, mode))
    aux = None
    if want_arg:
        aux = (Guarded((A, Bv, Nt), torch.uint8), Guarded((A, Bv, Nv), torch.uint8), Guarded((A, Bv, Nt)), Guarded((A, Bv, Nv)))
    ptrs = [hip.ptr(g.t) for g in aux] if aux else [None] * 4
    rc = hip.lib().nr_local_level_fwd(hip.ptr(planes[0]), hip.ptr(planes[1]), hip.ptr(planes[2]), hip.ptr(planes[3]),
                                      hip.ptr(w_t), hip.ptr(w_v), A, Nt, Bv, Nv, d, PREC[p], mode, hip.ptr(out.t), *ptrs,
                                      hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (case, mode, rc)
    every = (out,) + (aux or ())
    assert all(g.untouched_around() for g in every), (case, mode)
    if expect != 0:
        assert all(g.untouched() for g in every), (case, mode)
        return None, None
    assert bool((out.t != SENT).all()) and (aux is None or bool((aux[2].t != SENT).all() and (aux[3].t != SENT).all()))
    return out.t, (tuple(g.t for g in aux) if aux else None)


def _block_sums(S, n, size):
    """S [rows, n] fp32 -> fp64 sums over consecutive groups of `size` columns: [ceil(n / size), rows], and the sums of |S|."""
    nb = -(-n // size)
    pad = torch.zeros(S.shape[0], nb * size, dtype=torch.float64, device=S.device)
    pad[:, :n] = S.double()
    return pad.view(S.shape[0], nb, size).sum(-1).t(), pad.abs().view(S.shape[0], nb, size).sum(-1).t()


def _run_all(case, exact):
    """The five launches of a case -> (x, S, aux, row parts, column parts); the want_arg launch's S bit-equal to the plain one."""
    x, planes, w_t, w_v = _device_inputs(case, exact)
    S, _ = _launch(case, planes, w_t, w_v, hip.OUT_FULL, False)
    S_arg, aux = _launch(case, planes, w_t, w_v, hip.OUT_FULL, True)
    assert torch.equal(S, S_arg), case
    rs, _ = _launch(case, planes, w_t, w_v, hip.OUT_ROWSUM, False)
    cs, _ = _launch(case, planes, w_t, w_v, hip.OUT_COLSUM, False)
    return x, S, aux, rs, cs


@pytest.mark.parametrize("case", R.CASES, ids=_id)
def test_every_launch_form_against_fp64(case):
    plan = _assert_plan(case)
    Nt, Nv, A, Bv, d, p = case
    texts, videos = plan[6:8]
    x, S, (arg_v, arg_t, pmax, qmax), rs, cs = _run_all(case, False)
    ref = R.forward(R.operand_terms(*x["planes"], A, Nt, Bv, Nv, p == "x3"), x["w_t"], x["w_v"], device=DEV, keep_R=True)
    ex = R.forward(R.exact_terms(x["t"], x["tm"], x["v"], x["vm"]), x["w_t"], x["w_v"], device=DEV)
    bar_R, bar_S = R.bars(p, d)
    dev = lambda a, b: float((a.double() - b).abs().max())
    d_S, d_p, d_q, d_ex = dev(S, ref["S"]), dev(pmax, ref["pmax"]), dev(qmax, ref["qmax"]), dev(S, ex["S"])
    at_v = torch.gather(ref["R"], 3, arg_v.long()[..., None]).squeeze(-1)
    at_t = torch.gather(ref["R"], 2, arg_t.long()[:, :, None, :]).squeeze(2)
    d_av, d_at = float((at_v - ref["pmax"]).abs().max()), float((at_t - ref["qmax"]).abs().max())
    # the sum forms: reduced, against fp64 (as means: bar_S + what a sequential fp32 sum of one block's S can lose); and part by
    # part against the kernel's own S of that block, which pins the layout of the parts to the tiling the plan reports
    s_max = float(ref["S"].abs().max())
    d_rs = float((rs.double().sum(0) / Bv - ref["rowsum"] / Bv).abs().max())
    d_cs = float((cs.double().sum(0) / A - ref["colsum"] / A).abs().max())
    bar_rs = bar_S + 1.01 * videos * 2.0 ** -24 * s_max
    bar_cs = bar_S + 1.01 * texts * 2.0 ** -24 * s_max
    own_r, abs_r = _block_sums(S, Bv, videos)
    own_c, abs_c = _block_sums(S.t().contiguous(), A, texts)
    part_r = float(((rs.double() - own_r).abs() - 1.01 * videos * 2.0 ** -24 * abs_r).max())
    part_c = float(((cs.double() - own_c).abs() - 1.01 * texts * 2.0 ** -24 * abs_c).max())
    line = (f"simfwd {_id(case)} {plan[:6]}: S {d_S:.2e} (bar {bar_S:.2e}) pmax {d_p:.2e} qmax {d_q:.2e} (bar {bar_R:.2e}) "
            f"arg_v {d_av:.2e} arg_t {d_at:.2e}; rows {d_rs:.2e} ({bar_rs:.2e}) cols {d_cs:.2e} ({bar_cs:.2e}); "
            f"exact S {d_ex:.2e} (bar {R.TODAY[p]:.0e})")
    print(line)
    assert rs.shape == (plan[8], A) and cs.shape == (plan[9], Bv), line
    assert all(bool(torch.isfinite(t).all()) for t in (S, pmax, qmax, rs, cs)), line
    assert d_S <= bar_S, line
    assert d_p <= bar_R and d_q <= bar_R, line
    assert int(arg_v.max()) < Nv and int(arg_t.max()) < Nt, line
    assert d_av <= bar_R and d_at <= bar_R, line
    assert d_rs <= bar_rs and d_cs <= bar_cs, line
    assert part_r <= 0.0 and part_c <= 0.0, line
    assert d_ex <= R.TODAY[p], line
    ma, mb = R.masked_samples(A, Bv)
    assert float(S[ma].abs().max()) == 0.0 and float(S[:, mb].abs().max()) == 0.0, line
    assert float(pmax[ma].abs().max()) == 0.0 and float(qmax[:, mb].abs().max()) == 0.0, line


@pytest.mark.parametrize("case", R.one_case_per_form(), ids=_id)
def test_exact_sums_and_ties_bit_for_bit(case):
    """The tie tier on one case of every form: every K sum and every pooled sum is exact in fp32 in any order, so S, pmax, qmax
    and both sum forms equal fp64 bit for bit and the arg-max indices are the first maximum -- among them the masked tokens' tie
    at 0 in the pairs whose live products are all negative."""
    plan = _assert_plan(case)
    Nt, Nv, A, Bv, d, p = case
    x, S, (arg_v, arg_t, pmax, qmax), rs, cs = _run_all(case, True)
    ref = R.forward(R.operand_terms(*x["planes"], A, Nt, Bv, Nv, p == "x3"), x["w_t"], x["w_v"], device=DEV)
    eq = lambda a, b: bool(torch.equal(a.double(), b.double()))
    bad = [k for k, a, b in (("S", S, ref["S"]), ("pmax", pmax, ref["pmax"]), ("qmax", qmax, ref["qmax"]),
                             ("arg_v", arg_v, ref["arg_v"]), ("arg_t", arg_t, ref["arg_t"]),
                             ("rowsum", rs.double().sum(0), ref["rowsum"]), ("colsum", cs.double().sum(0), ref["colsum"]))
           if not eq(a, b)]
    n_tie = int(((ref["pmax"] == 0) & (ref["arg_v"] > 0)).sum()) + int(((ref["qmax"] == 0) & (ref["arg_t"] > 0)).sum())
    print(f"simfwd ties {_id(case)} {plan[:6]}: differing {bad or 'none'}; maxima that are a masked token's 0 behind live tokens: {n_tie}")
    assert not bad, (case, bad)
    assert n_tie > 0 or min(Nt, Nv) <= 2


@pytest.mark.parametrize("case", R.REFUSED, ids=_id)
def test_refusals_write_nothing(case):
    """Over the LDS budget (2 x 2 tokens at 65 x 65 in split-bf16, one token per sample at 90 x 90) or more than 128 tokens per
    sample: the plan reports the refusal, nr_local_level_fwd returns NR_EUNSUPPORTED in every mode and no output moves."""
    assert _assert_plan(case) is None
    Nt, Nv, A, Bv, d, p = case
    g = torch.Generator().manual_seed(1)
    planes = tuple(torch.randint(-3, 3, (n, d), generator=g, dtype=torch.int16).to(DEV) for n in (A * Nt, A * Nt, Bv * Nv, Bv * Nv))
    w_t, w_v = torch.rand(A, Nt, generator=g).to(DEV), torch.rand(Bv, Nv, generator=g).to(DEV)
    for mode in MODES:
        Nt_, Nv_ = min(Nt, 128), min(Nv, 128)                       # (nr_local_level_tiles refuses these shapes too: any buffer will do)
        out = Guarded((max(A, Bv), max(A, Bv)))
        aux = (Guarded((A, Bv, Nt_), torch.uint8), Guarded((A, Bv, Nv_), torch.uint8), Guarded((A, Bv, Nt_)), Guarded((A, Bv, Nv_)))
        for with_aux in (False, True):
            ptrs = [hip.ptr(a.t) for a in aux] if with_aux else [None] * 4
            rc = hip.lib().nr_local_level_fwd(*(hip.ptr(q) for q in planes), hip.ptr(w_t), hip.ptr(w_v), A, Nt, Bv, Nv, d, PREC[p],
                                              mode, hip.ptr(out.t), *ptrs, hip.stream_ptr())
            torch.cuda.synchronize()
            assert rc == hip.NR_EUNSUPPORTED, (case, mode, rc)
            assert out.untouched() and all(a.untouched() for a in aux), (case, mode)


def _problem(case, mode):
    Nt, Nv, A, Bv, d, p = case
    x, planes, w_t, w_v = _device_inputs(case, False)
    pt = ops.Prepared(planes[0], planes[1], None, None, A * Nt, d)
    pv = ops.Prepared(planes[2], planes[3], None, None, Bv * Nv, d)
    return (pt, pv, w_t, w_v, A, Nt, Bv, Nv, PREC[p], mode)


@pytest.mark.parametrize("kinds", [(0, 0), (1, 0, 1), (0, 0, 1)], ids=["chained-pair", "group-of-three", "pair-then-one"])
def test_grouped_and_chained_launches_equal_the_single_ones(kinds):
    """nr_local_level_group at d = 128 on the smallest groupable product of each kind (0: one pass on 192 x 384 blocks, 1:
    split-bf16 on 96 x 192): two kind-0 products in front run as chained tile pairs (nr_sim_pair_kernel), everything else in
    the grouped grid.  Outputs bit for bit those of the single launches -- which test_every_launch_form_against_fp64 holds to
    fp64 -- in all three output modes, one entry point call per group."""
    for k in set(kinds):
        case = R.GROUP_KIND[k]
        _assert_plan(case)
        Nt, Nv, A, Bv, d, p = case
        assert hip.local_level_group_kind(A, Nt, Bv, Nv, d, PREC[p]) == k
    for modes in (MODES, MODES[1:] + MODES[:1], MODES[2:] + MODES[:2]):
        probs = [_problem(R.GROUP_KIND[k], modes[i % 3]) for i, k in enumerate(kinds)]
        single = [ops.local_level(*q)[0] for q in probs]
        n0 = hip.N_CALLS
        got = ops.local_level_group(probs)
        torch.cuda.synchronize()
        assert hip.N_CALLS - n0 == 1
        for i, (a, b) in enumerate(zip(got, single)):
            assert a.shape == b.shape and torch.equal(a, b), (kinds, modes, i)
