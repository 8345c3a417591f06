"""GPU: the one-pass fp16 precision (hip.PREC_F16) of the similarity forward, the token scorer, the prepare kernels and the
training plan's step.

bit-exact tier  Operand planes whose values are numbers of BOTH formats (multiples of 2^-6, |k| <= 128, dense rows: every K
                sum stays under 2^11 on a 2^-12 grid, exact in fp32 in any order): the bf16 bits with PREC_BF16 and the fp16 bits
                with PREC_F16 run the same blocks in the same order and must give the same bits -- S, the row / column
                sum forms, pooled maxima, arg-max bytes (an exact tie included), scorer logits and weights.  One case per fp16
                form that is built; the block shapes without an fp16 kernel must refuse with nothing written.
operand tier    Random inputs against the fp64 restatements of tests/simfwd_ref.py / tests/scorer_ref.py evaluated on the
                fp16-rounded operands.  What separates kernel and reference is the fp32 accumulation alone, as for one bf16
                pass, so the bars are made the same way: similarity 8 x the error of the sequential fp32 twin (simfwd_ref.twin,
                run here on the fp16 planes' subsample, and never under the stored figure of the bf16 planes), capped by the
                any-order bound; scorer the one-pass bars of tests/test_scorer_gpu.py (10 x its fp32 twin: logits 1e-5, weights
                2e-6).  Never from the kernel's output.  Measured maxima are printed (pytest -s).
prepare         the fp16 plane is torch's fp32 -> fp16 rounding of the kernel's fp32 values bit for bit; hi, lo, norms and
                column sums do not depend on it; masked rows are zero.
head            the training plan against the reference fixtures and against the "bf16x3" plan: |dL| <= 5e-4 (half the
                project's 1e-3 bar, the condition under which a launch was switched to fp16); a captured step replays bit for
                bit."""
import functools

import numpy as np
import pytest
import torch

import nr_oracle as O
import scorer_ref as SR
import simfwd_ref as R
from neighborretr_amd import head, hip, modeling, ops, synth
from util import golden, noise, params, problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENT = 256, -77.25
DL_BAR = 5e-4

# (Nt, Nv, A, Bv, d): one case per one-pass register form of simfwd_ref.FORMS; built = an fp16 kernel exists for its block
BUILT = [(24, 12, 5, 3, 64), (24, 12, 5, 3, 512), (24, 12, 37, 19, 128), (24, 12, 92, 184, 128), (24, 12, 121, 481, 128),
         (24, 12, 121, 481, 64), (64, 64, 64, 61, 128), (64, 64, 64, 61, 64)]
NOT_BUILT = [(24, 12, 121, 241, 128), (24, 12, 121, 241, 64), (64, 64, 3, 5, 128), (64, 64, 31, 64, 128), (24, 64, 5, 3, 128),
             (64, 12, 3, 21, 128)]
SCORER_SETS = [(17, 24), (5, 64), (34, 64), (66, 64), (257, 24)]


def _id(c):
    return "x".join(map(str, c))


def _bits(x, dtype):
    """fp32 values that are numbers of `dtype` -> their bit patterns as int16 (asserted exact)."""
    y = x.to(dtype)
    assert torch.equal(y.float(), x)
    return y.view(torch.int16).contiguous()


def _grid_values(seed, tag, shape):
    """k / 64 with integer |k| <= 128: numbers of bf16 (8 significand bits) and of fp16.  A sum of up to 512 products of two of
    them is a multiple of 2^-12 below 2^11: 23 bits, exact in fp32 whatever the order."""
    k = np.clip(synth.randint(seed, tag + "/k", -128, 128, shape), -128, 128).astype(np.float32)
    return torch.from_numpy(k / 64.0)


class Guarded:
    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.sent = SENT if dtype == torch.float32 else 0xA5
        self.buf = torch.full((self.n + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)

    def around(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[GUARD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.buf == self.sent).all())


def _sim_launch(case, prec, t_plane, v_plane, w_t, w_v, mode, want_arg, expect=0):
    Nt, Nv, A, Bv, d = case
    if mode == hip.OUT_FULL:
        shape = (A, Bv)
    else:
        nr, nc = hip.local_level_tiles(A, Nt, Bv, Nv, prec)
        shape = (nc, A) if mode == hip.OUT_ROWSUM else (nr, Bv)
    out = Guarded(shape)
    aux = (Guarded((A, Bv, Nt), torch.uint8), Guarded((A, Bv, Nv), torch.uint8), Guarded((A, Bv, Nt)), Guarded((A, Bv, Nv))) if want_arg else None
    ptrs = [hip.ptr(g.t) for g in aux] if aux else [None] * 4
    rc = hip.lib().nr_local_level_fwd(hip.ptr(t_plane), None, hip.ptr(v_plane), None, hip.ptr(w_t), hip.ptr(w_v), A, Nt, Bv, Nv, d,
                                      prec, mode, hip.ptr(out.t), *ptrs, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (case, prec, mode, rc)
    every = (out,) + (aux or ())
    assert all(g.around() for g in every), (case, mode)
    if expect != 0:
        assert all(g.untouched() for g in every), (case, mode)
        return None, None
    assert bool((out.t != SENT).all())
    return out.t, (tuple(g.t for g in aux) if aux else None)


@functools.lru_cache(maxsize=2)
def _grid_case(case):
    """Exactly representable operands of one case: prefix masks (masked rows zero), one fully masked text and video, and EXACT
    TIES: text 0 keeps two tokens, the second a copy of the first, and video 0 two such frames -- every maximum over text 0's
    tokens (video 0's frames) is attained twice, by tokens 0 and 1 or, where their product is negative, by the zeros of the
    masked tokens 2, 3, ...: the first index is 0 or 2."""
    Nt, Nv, A, Bv, d = case
    seed, tag = 6100 + d, f"f16/{Nt}x{Nv}/{A}x{Bv}"
    t, v = _grid_values(seed, tag + "/t", (A, Nt, d)), _grid_values(seed, tag + "/v", (Bv, Nv, d))
    tm = torch.from_numpy((np.arange(Nt)[None] < synth.randint(seed, tag + "/tm", 2, Nt, (A, 1))).astype(np.float32))
    vm = torch.from_numpy((np.arange(Nv)[None] < synth.randint(seed, tag + "/vm", 2, Nv, (Bv, 1))).astype(np.float32))
    ma, mb = R.masked_samples(A, Bv)
    if ma is not None:
        tm[ma] = 0
    if mb is not None:
        vm[mb] = 0
    t[0, 1], v[0, 1] = t[0, 0], v[0, 0]
    tm[0], vm[0] = 0, 0
    tm[0, :2], vm[0, :2] = 1, 1
    t, v = t * tm[..., None], v * vm[..., None]
    w_t = torch.from_numpy(synth.randint(seed, tag + "/wt", 0, 4, (A, Nt)).astype(np.float32) / 64.0)
    w_v = torch.from_numpy(synth.randint(seed, tag + "/wv", 0, 4, (Bv, Nv)).astype(np.float32) / 64.0)
    return t, v, w_t, w_v


@pytest.mark.parametrize("case", BUILT, ids=_id)
def test_similarity_fp16_equals_bf16_bit_for_bit_on_common_numbers(case):
    Nt, Nv, A, Bv, d = case
    plan = hip.local_level_plan(A, Nt, Bv, Nv, d, hip.PREC_F16)
    assert plan is not None and plan == hip.local_level_plan(A, Nt, Bv, Nv, d, hip.PREC_BF16)
    t, v, w_t, w_v = _grid_case(case)
    w_t, w_v = w_t.to(DEV), w_v.to(DEV)
    planes = {p: (_bits(t.reshape(A * Nt, d), dt).to(DEV), _bits(v.reshape(Bv * Nv, d), dt).to(DEV))
              for p, dt in ((hip.PREC_BF16, torch.bfloat16), (hip.PREC_F16, torch.float16))}
    got = {}
    for p, (tp, vp) in planes.items():
        S, _ = _sim_launch(case, p, tp, vp, w_t, w_v, hip.OUT_FULL, False)
        S_arg, aux = _sim_launch(case, p, tp, vp, w_t, w_v, hip.OUT_FULL, True)
        rs, _ = _sim_launch(case, p, tp, vp, w_t, w_v, hip.OUT_ROWSUM, False)
        cs, _ = _sim_launch(case, p, tp, vp, w_t, w_v, hip.OUT_COLSUM, False)
        assert torch.equal(S, S_arg)
        got[p] = (S, rs, cs) + aux
    for a, b, name in zip(got[hip.PREC_BF16], got[hip.PREC_F16], ("S", "rowsum", "colsum", "arg_v", "arg_t", "pmax", "qmax")):
        assert torch.equal(a, b), (case, name)
    # ... and the common answer is the right one: every sum is exact, so fp64 of the same numbers gives the same S and pools,
    # and the arg-max bytes are the FIRST maximum (the tie: frame 0 before frame 1, token 0 before token 1)
    ref = R.forward([(t, v)], w_t, w_v, device=DEV)
    S, _, _, arg_v, arg_t, pmax, qmax = got[hip.PREC_F16]
    assert torch.equal(pmax.double(), ref["pmax"]) and torch.equal(qmax.double(), ref["qmax"])
    assert torch.equal(arg_v.long(), ref["arg_v"]) and torch.equal(arg_t.long(), ref["arg_t"])
    assert float((S.double() - ref["S"]).abs().max()) <= 2.0 ** -20 * float(ref["S"].abs().max())      # (the weighted sums round)
    assert bool(((ref["arg_t"][0] == 0) | (ref["arg_t"][0] == 2)).all()) and bool(((ref["arg_v"][:, 0] == 0) | (ref["arg_v"][:, 0] == 2)).all())


@pytest.mark.parametrize("case", NOT_BUILT, ids=_id)
def test_similarity_fp16_refuses_blocks_without_a_kernel_and_writes_nothing(case):
    Nt, Nv, A, Bv, d = case
    assert hip.local_level_plan(A, Nt, Bv, Nv, d, hip.PREC_F16) is None
    assert hip.local_level_plan(A, Nt, Bv, Nv, d, hip.PREC_BF16)[0] == "reg"
    tp = torch.zeros((A * Nt, d), dtype=torch.int16, device=DEV)
    vp = torch.zeros((Bv * Nv, d), dtype=torch.int16, device=DEV)
    w_t, w_v = torch.zeros((A, Nt), device=DEV), torch.zeros((Bv, Nv), device=DEV)
    for mode, arg in ((hip.OUT_FULL, True), (hip.OUT_ROWSUM, False), (hip.OUT_COLSUM, False)):
        _sim_launch(case, hip.PREC_F16, tp, vp, w_t, w_v, mode, arg, expect=hip.NR_EUNSUPPORTED)


def _scorer_params(exact_grid):
    P = params()
    b1, w2, b2 = (P["text_weight_fc." + k].float() for k in ("0.bias", "2.weight", "2.bias"))
    W1 = _grid_values(6200, "f16/W1", (1024, 512)) if exact_grid else P["text_weight_fc.0.weight"].float()
    return W1, b1, w2.reshape(-1), b2.reshape(1)


@pytest.mark.parametrize("n,N", SCORER_SETS, ids=lambda v: str(v))
def test_scorer_fp16_equals_bf16_bit_for_bit_on_common_numbers(n, N):
    d, H = 512, 1024
    assert hip.token_scorer_plan(n * N, H, hip.PREC_F16, N) == hip.token_scorer_plan(n * N, H, hip.PREC_BF16, N) is not None
    W1, b1, w2, b2 = _scorer_params(True)
    x = _grid_values(6300 + n, f"f16/scorer/{n}x{N}", (n * N, d))
    mask = torch.from_numpy((np.arange(N)[None] < synth.randint(6300 + n, "f16/scorer/mask", 1, N, (n, 1))).astype(np.float32))
    if n >= 3:
        mask[1] = 0
    x = x * mask.reshape(-1, 1)
    norm = torch.from_numpy(0.5 + 4.0 * synth.uniform(6300 + n, "f16/scorer/norm", (n * N,)).astype(np.float32)).to(DEV)
    b1, w2, b2, mask = b1.to(DEV), w2.to(DEV), b2.to(DEV), mask.to(DEV)
    out = {}
    for p, dt in ((hip.PREC_BF16, torch.bfloat16), (hip.PREC_F16, torch.float16)):
        plane, w1 = _bits(x, dt).to(DEV), _bits(W1, dt).to(DEV)
        prep = ops.Prepared(plane if p == hip.PREC_BF16 else torch.zeros_like(plane), None, norm, None, n * N, d,
                            plane if p == hip.PREC_F16 else None)
        w, lg = ops.token_weights(prep, w1, None, b1, w2, b2, mask, n, N, p, want_logits=True)
        parts = ops.token_logit_parts(prep, w1, None, b1, w2, p)
        torch.cuda.synchronize()
        out[p] = (w, lg, parts)
    for a, b, name in zip(out[hip.PREC_BF16], out[hip.PREC_F16], ("weights", "logits", "logit parts")):
        assert torch.equal(a, b), (n, N, name)
    w, lg, _ = out[hip.PREC_F16]
    assert bool(torch.isfinite(lg).all()) and float((w.sum(-1) - 1).abs().max()) <= 1e-5


# ---- operand tier ------------------------------------------------------------------------------------------------------------
def _f16_planes(x, mask):
    """fp16 plane [n N, d] (int16 bits) of the fp32 rounding of normalize(x) * mask computed in fp64, as simfwd_ref.operands."""
    n, N, d = x.shape
    return R.normalised(x, mask).float().reshape(n * N, d).to(torch.float16).view(torch.int16)


@pytest.mark.parametrize("case", [(24, 12, 5, 3, 512), (24, 12, 37, 19, 128), (24, 12, 92, 184, 128), (24, 12, 121, 481, 128),
                                  (64, 64, 64, 61, 128)], ids=_id)
def test_similarity_fp16_against_fp64_of_its_operands(case):
    Nt, Nv, A, Bv, d = case
    x = R.make_inputs(case + ("bf16",))
    tp, vp = _f16_planes(x["t"], x["tm"]), _f16_planes(x["v"], x["vm"])
    T, V = tp.view(torch.float16).float().view(A, Nt, d), vp.view(torch.float16).float().view(Bv, Nv, d)
    # the bars, from the sequential fp32 twin on the subsample of THESE planes (never under the stored bf16-plane figure)
    sa, sb = R.subsample(A), R.subsample(Bv)
    sub = [(T[sa], V[sb])]
    tw, rf = R.twin(sub, x["w_t"][sa], x["w_v"][sb]), R.forward(sub, x["w_t"][sa], x["w_v"][sb], keep_R=True)
    e_R = max(float((tw["R"].double() - rf["R"]).abs().max()), R.TWIN["bf16"][0])
    e_S = max(float((tw["S"].double() - rf["S"]).abs().max()), R.TWIN["bf16"][1])
    mag = float(torch.einsum("atd,bvd->abtv", T[sa].double().abs(), V[sb].double().abs()).max())
    bound_R = 1.01 * d * 2.0 ** -24 * mag
    bar_R, bar_S = min(R.BAR_FACTOR * e_R, bound_R), min(R.BAR_FACTOR * e_S, bound_R + 1.01 * (Nt + Nv + 1) * 2.0 ** -24 * mag)
    w_t, w_v = x["w_t"].to(DEV), x["w_v"].to(DEV)
    S, aux = _sim_launch(case, hip.PREC_F16, tp.to(DEV), vp.to(DEV), w_t, w_v, hip.OUT_FULL, True)
    ref = R.forward([(T, V)], x["w_t"], x["w_v"], device=DEV)
    d_S = float((S.double() - ref["S"]).abs().max())
    d_p = float((aux[2].double() - ref["pmax"]).abs().max())
    d_q = float((aux[3].double() - ref["qmax"]).abs().max())
    # against fp64 of the fp32 inputs: what fp16 operands cost S (reported; one bf16 pass is held to 1e-3 there)
    ex = R.forward(R.exact_terms(x["t"], x["tm"], x["v"], x["vm"]), x["w_t"], x["w_v"], device=DEV)
    d_ex = float((S.double() - ex["S"]).abs().max())
    print(f"\n[f16 sim {_id(case)}] operand tier: S {d_S:.3g} (bar {bar_S:.3g}), pmax {d_p:.3g}, qmax {d_q:.3g} (bar {bar_R:.3g}); "
          f"S against fp64 of the fp32 inputs {d_ex:.3g}")
    assert d_S <= bar_S and d_p <= bar_R and d_q <= bar_R
    assert d_ex <= R.TODAY["bf16"]


@pytest.mark.parametrize("n,N", [(17, 24), (66, 64), (257, 24)], ids=lambda v: str(v))
def test_scorer_fp16_against_fp64_of_its_operands(n, N):
    d, H = 512, 1024
    W1, b1, w2, b2 = _scorer_params(False)
    x, mask = SR.make_case(31, n, N, d)
    _, _, norm = SR.prepare_tokens(x, mask)
    xn = (x.reshape(-1, d).float() / norm[:, None]) * mask.reshape(-1, 1).float()
    plane, w1 = xn.to(torch.float16), W1.to(torch.float16)
    prep = ops.Prepared(torch.zeros((n * N, d), dtype=torch.int16, device=DEV), None, norm.to(DEV), None, n * N, d,
                        plane.view(torch.int16).to(DEV))
    w, lg = ops.token_weights(prep, w1.view(torch.int16).to(DEV), None, b1.to(DEV), w2.to(DEV), b2.to(DEV), mask.float().to(DEV), n, N,
                              hip.PREC_F16, want_logits=True)
    torch.cuda.synchronize()
    X, W = plane.to(DEV).double(), w1.to(DEV).double()
    h = (X @ W.t()) * norm.to(DEV).double()[:, None] + b1.to(DEV).double()
    lg_ref = (torch.relu(h) @ w2.to(DEV).double() + b2.to(DEV).double()).view(n, N)
    w_ref = torch.softmax(lg_ref.masked_fill(mask.to(DEV) == 0, SR.NEG_BIG), dim=-1)
    valid = mask.to(DEV) != 0
    d_lg, d_w = float((lg.double() - lg_ref)[valid].abs().max()), float((w.double() - w_ref).abs().max())
    print(f"\n[f16 scorer {n}x{N}] operand tier: logits {d_lg:.3g} (bar 1e-5), weights {d_w:.3g} (bar 2e-6)")
    assert d_lg <= 1e-5 and d_w <= 2e-6


# ---- prepare -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tok", [1, 63, 64, 65, 3072])
def test_prepare_fp16_plane(n_tok):
    d = 512
    x = torch.from_numpy(synth.normal(77, f"f16/prep/{n_tok}", (n_tok, d)).astype(np.float32)).to(DEV) * 3.0
    mask = torch.from_numpy((synth.uniform(77, f"f16/prep/mask/{n_tok}", (n_tok,)) > 0.25).astype(np.float32)).to(DEV)
    if n_tok > 2:
        mask[1], mask[2] = 0.0, 1.0
    a = ops.prepare_tokens(x, mask, want_lo=True, want_colsum=True, want_f16=False)
    b = ops.prepare_tokens(x, mask, want_lo=True, want_colsum=True, want_f16=True)
    c = ops.prepare_tokens(x, mask, want_lo=False, want_f16=True)
    torch.cuda.synchronize()
    assert a.f16 is None and b.f16 is not None and c.lo is None
    for k in ("hi", "lo", "norm", "colsum"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(c.hi, a.hi) and torch.equal(c.norm, a.norm) and torch.equal(c.f16, b.f16)
    want = ((x * (1.0 / b.norm)[:, None]) * mask[:, None]).to(torch.float16)
    assert torch.equal(b.f16.view(torch.float16), want)
    # (a masked row is x * 0: zeros of either sign, as in the bf16 planes)
    assert bool((b.f16.view(torch.float16)[mask == 0] == 0).all()) and bool((b.hi.view(torch.bfloat16)[mask == 0] == 0).all())
    # the pair launch writes the same planes
    p0, p1 = ops.prepare_tokens_pair(x, mask, x.flip(0).contiguous(), None, want_lo=False, want_colsum=True, want_f16=True)
    torch.cuda.synchronize()
    assert torch.equal(p0.f16, b.f16) and torch.equal(p0.hi, a.hi) and torch.equal(p0.colsum, a.colsum) and p0.lo is None
    assert torch.equal(p1.f16.view(torch.float16), (x.flip(0) * (1.0 / p1.norm)[:, None]).to(torch.float16))
    w = torch.from_numpy(synth.normal(78, "f16/w", (64, d)).astype(np.float32)).to(DEV)
    assert torch.equal(ops.split_f16(w).view(torch.float16), w.to(torch.float16))


# ---- head ----------------------------------------------------------------------------------------------------------------------
def _model(precision, K, **cfg):
    m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K, **cfg), precision=precision)
    m.load_state_dict(params(), strict=False)
    m = m.to(DEV)
    with torch.no_grad():
        m.clip.logit_scale.fill_(float(np.log(100.0)))
    return m.train()


def _step(m, x, nz, K):
    c = m.config
    with torch.no_grad():
        return torch.stack(m._compute_losses(x["text_feat"], x["video_feat"], x["text_mask"], x["video_mask"], x["mb_feat_t"],
                                             x["mb_feat_v"], x["mb_mask_t"], x["mb_mask_v"], c.centrality_scale, c.beta, K,
                                             c.temperature, m.clip.logit_scale.exp(), noise=nz))


@pytest.mark.parametrize("name", ["c1_b16", "c2_b128", "c4_b8", "r32_blank"])
def test_training_plan_losses_against_the_reference_fixtures(name):
    g = golden(name)
    B, Nt, Nv, M, K = (int(g[k]) for k in ("B", "Nt", "Nv", "M", "K"))
    x = problem(int(g["seed"]), B, Nt, Nv, M, device=DEV, blank_video=int(g["blank_video"]))
    nz = noise(int(g["seed"]), B, Nt, Nv, device=DEV)
    plan = head.precision_plan(head.PREC_MIXED, (B, Nt, Nv, 512, 1024))
    multi = name == "c4_b8"          # the reference's centrality term raises at its shape: the documented "mean" reduction
    m = _model("bf16", K, **(dict(centrality_multi_token="mean") if multi else {}))
    got = _step(m, x, nz, K).cpu().numpy()
    if multi:
        hp = dict(synth.DEFAULT_HP, num_neighbors=K)
        with torch.no_grad():
            ref = O.compute_losses(*(x[k].cpu() for k in ("text_feat", "video_feat", "text_mask", "video_mask", "mb_feat_t", "mb_feat_v",
                                                          "mb_mask_t", "mb_mask_v")), params(), hp, torch.tensor(100.0),
                                   {k: v.cpu() for k, v in nz.items()}, centrality_multi_token="mean")
        ref = np.array([float(r) for r in ref])
    else:
        ref = np.asarray(g["losses"], dtype=np.float64)
    ok = np.isfinite(ref)
    dL = float(np.abs(got - ref)[ok].max()) if ok.any() else 0.0
    print(f"\n[f16 head {name}] plan (B x B, batch scorers, bank) = {plan}; max|dL| over {int(ok.sum())} finite reference losses {dL:.3g} (bar {DL_BAR:g})")
    assert plan[1] == hip.PREC_F16 and plan[2] == hip.PREC_BF16
    assert np.array_equal(np.isfinite(got), ok), (got, ref)
    assert dL <= DL_BAR


# seeds of tools/prec_probe_f16.random_shapes with B <= 24: every reference loss is finite there (profiles/f16_prec_probe.txt)
@pytest.mark.parametrize("seed", [3004, 3005, 3009, 3011, 3015, 3016, 3018, 3020])
def test_training_plan_against_the_split_plan_on_random_shapes(seed):
    r = np.random.RandomState(seed)
    B = int(r.randint(3, 41))
    M, K = int(r.choice([32, 64, 96, 128])), int(r.randint(1, min(B, 20) + 1))
    assert 3 <= B <= 24
    x, nz = problem(seed, B, 24, 12, M, device=DEV), noise(seed, B, 24, 12, device=DEV)
    a = _step(_model("bf16", K), x, nz, K).cpu().numpy()
    b = _step(_model("bf16x3", K), x, nz, K).cpu().numpy()
    assert np.isfinite(b).all() and np.isfinite(a).all()
    dL = float(np.abs(a - b).max())
    print(f"\n[f16 head random seed {seed} B={B} M={M} K={K}] max|dL| training plan vs bf16x3 {dL:.3g} (bar {DL_BAR:g})")
    assert dL <= DL_BAR


def test_captured_step_replays_the_eager_step_bit_for_bit():
    g = golden("c1_b16")
    B, Nt, Nv, M, K = (int(g[k]) for k in ("B", "Nt", "Nv", "M", "K"))
    x, nz = problem(int(g["seed"]), B, Nt, Nv, M, device=DEV), noise(int(g["seed"]), B, Nt, Nv, device=DEV)
    m = _model("bf16", K)
    eager = _step(m, x, nz, K).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), m.graph_capture_mode():
        for _ in range(2):
            _step(m, x, nz, K)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with m.graph_capture_mode(), torch.cuda.graph(gr):
        losses = _step(m, x, nz, K)
    for _ in range(2):
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(losses, eager)
