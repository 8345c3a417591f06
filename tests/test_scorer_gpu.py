"""GPU: every launch form of the token scorer (csrc/nr_mlp.hip) against the fp64 references of tests/scorer_ref.py.

Each case FIRST asserts, through nr_token_scorer_plan, that its token set runs the form it was chosen for (scorer_ref.FORMS:
block rows x hidden units, ring depth, fused softmax or the two launches) and fails -- not skips -- if the picker has moved.

Two tiers, both evaluated in stock fp64 torch on the device:

  operand tier   the same function on the very bf16 operands the kernel reads.  What separates kernel and reference is the
                 order and the precision (fp32) of the sums alone.  Evaluating the reference's own sums in plain fp32 instead
                 of fp64 (CPU, 16 threads, 257 x 24, 130 x 64, 575 x 64, 381 x 24, 192 x 64 tokens of this file's inputs) moves
                     one pass:     logits 9.8e-7 .. 1.31e-6, weights 1.8e-7 .. 2.7e-7
                     three terms:  logits 9.6e-7 .. 1.21e-6, weights 1.8e-7 .. 2.4e-7
                 The bars are ten times that, because the MFMA accumulation order is not the CPU's: one pass 1e-5 / 2e-6 (set
                 on an earlier measurement of 8.1e-7 .. 9.5e-7 / 1.0e-7 .. 1.4e-7, kept), three terms 1.2e-5 / 2.4e-6.  Never
                 set from the kernel's output.  Pre-mask logits are compared on ALL tokens (masked tokens have zero operand
                 rows: relu(b1) . w2 + b2).
  exact tier     the project's bars against the fp32 inputs (test_token_weights): split-bf16 weights 2e-5 and logits of valid
                 tokens 2e-4; one pass logits of valid tokens 3e-2 (its weights are held by the operand tier alone: the
                 plan itself is up to 2.8e-3 away from the exact weights at these sizes).

Structure: rows sum to 1 (1e-5), masked tokens exactly 0, a single valid token exactly 1, a fully masked sample 1/N (1e-7),
the softmax counter pool all zero after every fused call, three launches on the same inputs bit-identical."""
import ctypes
import functools

import pytest
import torch

import scorer_ref as R
from neighborretr_amd import hip, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
PREC = {"bf16": hip.PREC_BF16, "x3": hip.PREC_BF16X3}
OPERAND_BARS = {"bf16": (1e-5, 2e-6), "x3": (1.2e-5, 2.4e-6)}        # (logits, weights), absolute
EXACT_BARS = {"bf16": (3e-2, None), "x3": (2e-4, 2e-5)}             # (logits of valid tokens, weights)


def _np(a):
    return torch.from_numpy(a.astype("float32")).to(DEV)


@functools.lru_cache(maxsize=None)
def _params(d=512, H=1024):
    """(W1, b1, w2, b2, w1_hi, w1_lo) on the device: the head's own scorer (synth.make_params(7)) at 512 x 1024, fresh
    N(0, 0.02) weights / N(0, 0.01) biases at any other width."""
    if (d, H) == (512, 1024):
        P = synth.make_params(7)
        W1, b1 = _np(P["text_weight_fc.0.weight"]), _np(P["text_weight_fc.0.bias"])
        w2, b2 = _np(P["text_weight_fc.2.weight"]).reshape(-1).contiguous(), _np(P["text_weight_fc.2.bias"])
    else:
        W1, b1 = _np(0.02 * synth.normal(7, "scorer/w1", (H, d))), _np(0.01 * synth.normal(7, "scorer/b1", (H,)))
        w2, b2 = _np(0.02 * synth.normal(7, "scorer/w2", (H,))), _np(0.01 * synth.normal(7, "scorer/b2", (1,)))
    hi, lo = ops.split_bf16(W1)
    return W1, b1, w2, b2, hi, lo


@functools.lru_cache(maxsize=2)
def _tokens(seed, n, N, d=512):
    """(x, mask, prepared operands) on the device; the two precisions of one shape share them."""
    x, mask = R.make_case(seed, n, N, d)
    x, mask = x.to(DEV), mask.to(DEV)
    if d % 256 == 0:
        prep = ops.prepare_tokens(x, mask)
    else:                                       # nr_prepare_tokens takes d % 256 == 0 only: the same operands from stock torch
        hi, lo, norm = R.prepare_tokens(x, mask)
        prep = ops.Prepared(hi.contiguous(), lo.contiguous(), norm.contiguous(), None, n * N, d)
    return x, mask, prep


def _counters_clear():
    st = ops._COUNTERS.get(("softmax", torch.empty(0, device=DEV).device))
    return st is None or int((st[0] != 0).sum()) == 0


def _check(tag, p, x, mask, prep, par, w, lg):
    """Both tiers and the structural checks for one scorer output; prints the measured maxima."""
    W1, b1, w2, b2, w1h, w1l = par
    n, N = mask.shape
    w_o, lg_o = R.operand(prep.hi, prep.lo, prep.norm, w1h, w1l, b1, w2, b2, mask, n, N, p == "x3", device=DEV)
    w_e, lg_e = R.exact(x, mask, W1, b1, w2, b2, device=DEV)
    valid = mask.bool()
    d_w_o = float((w.double() - w_o).abs().max())
    d_w_e = float((w.double() - w_e).abs().max())
    d_sum = float((w.double().sum(-1) - 1.0).abs().max())
    line = f"scorer {tag} {p}: operand tier w {d_w_o:.2e}"
    if lg is not None:
        d_lg_o = float((lg.double() - lg_o).abs().max())
        d_lg_e = float((lg.double() - lg_e)[valid].abs().max()) if bool(valid.any()) else 0.0
        line += f" logits {d_lg_o:.2e}; exact tier w {d_w_e:.2e} logits(valid) {d_lg_e:.2e}; row sums {d_sum:.1e}"
    else:
        line += f"; exact tier w {d_w_e:.2e}; row sums {d_sum:.1e}"
    print(line)
    assert bool(torch.isfinite(w).all())
    bar_lg, bar_w = OPERAND_BARS[p]
    assert d_w_o <= bar_w, line
    ex_lg, ex_w = EXACT_BARS[p]
    if ex_w is not None:
        assert d_w_e <= ex_w, line
    if lg is not None:
        assert bool(torch.isfinite(lg).all())
        assert d_lg_o <= bar_lg, line
        assert d_lg_e <= ex_lg, line
    assert d_sum <= 1e-5, line
    some = valid.any(-1)                                             # samples with at least one valid token
    off = w[some][~valid[some]]
    assert off.numel() == 0 or float(off.abs().max()) == 0.0, line
    blank = ~some
    if bool(blank.any()):
        assert float((w[blank] - 1.0 / N).abs().max()) <= 1e-7, line
    single = valid.sum(-1) == 1
    if bool(single.any()):
        assert bool((w[single][valid[single]] == 1.0).all()), line


def _form_cases():
    for call, precs, n, N, form in R.FORMS:
        for p in precs:
            yield pytest.param(call, p, n, N, form, id=f"{call}-{p}-{n}x{N}")


@pytest.mark.parametrize("call,p,n,N,form", list(_form_cases()))
def test_every_launch_form_against_fp64(call, p, n, N, form):
    """One row of scorer_ref.FORMS through ops.token_weights (H = 1024, d = 512, the head's own parameters)."""
    prec = PREC[p]
    fused = hip.token_scorer_plan(n * N, 1024, prec, N)
    if call == "fused":
        assert fused == form, f"{n} x {N} {p}: the picker now runs {fused}, this case was chosen for {form}"
    else:
        assert fused is None, f"{n} x {N} {p}: nr_token_weights_fwd now takes this set ({fused})"
        got = hip.token_scorer_plan(n * N, 1024, prec, 0)
        assert got == form, f"{n} x {N} {p}: the picker now runs {got}, this case was chosen for {form}"
    x, mask, prep = _tokens(1001, n, N)
    par = _params()
    W1, b1, w2, b2, w1h, w1l = par
    runs = []
    for _ in range(3 if call == "fused" else 1):
        n0 = hip.N_CALLS
        w, lg = ops.token_weights(prep, w1h, w1l, b1, w2, b2, mask, n, N, prec, want_logits=True)
        torch.cuda.synchronize()
        assert hip.N_CALLS - n0 == (1 if call == "fused" else 3)     # one launch, or refusal + the two launches
        if call == "fused":
            assert _counters_clear()
        runs.append((w, lg))
    for w_k, lg_k in runs[1:]:                                       # the hand-off is deterministic
        assert torch.equal(w_k, runs[0][0]) and torch.equal(lg_k, runs[0][1])
    _check(f"{call} {n}x{N} {form}", p, x, mask, prep, par, *runs[0])
    if N == 1:                                                       # N = 1 fuses; the two launches for it, by hand
        parts = ops.token_logit_parts(prep, w1h, w1l, b1, w2, prec)
        _check(f"two launches {n}x{N}", p, x, mask, prep, par, *ops.token_softmax(parts, b2, mask, n, N, want_logits=True))


@pytest.mark.parametrize("d,H", [(64, 1024), (192, 1024), (512, 128), (512, 256), (512, 1152)])
@pytest.mark.parametrize("p", ["bf16", "x3"])
def test_widths_the_abi_admits(d, H, p):
    """d % 64 == 0 and H % 128 == 0 beyond the head's 512 x 1024: one and three K slices through the two-deep ring, 1 / 2 / 9
    logit parts (9: the second round of the fused epilogue's 8-wide part loop), at 17 x 24 and 257 x 24 tokens."""
    prec = PREC[p]
    par = _params(d, H)
    W1, b1, w2, b2, w1h, w1l = par
    for n, N in ((17, 24), (257, 24)):
        form = hip.token_scorer_plan(n * N, H, prec, N)
        want = (192, 256, 2) if (H, p, n) == (1024, "bf16", 257) else (96, 128, 2)
        assert form == want, (d, H, p, n, form)
        x, mask, prep = _tokens(1003, n, N, d)
        w, lg = ops.token_weights(prep, w1h, w1l, b1, w2, b2, mask, n, N, prec, want_logits=True)
        torch.cuda.synchronize()
        assert _counters_clear()
        _check(f"d={d} H={H} {n}x{N} {form}", p, x, mask, prep, par, w, lg)


def _problem(prep, par, mask, n, N, w, parts, counters, logits=None):
    W1, b1, w2, b2, w1h, w1l = par
    q = hip.TokenWeightsProblem()
    q.tok_hi, q.tok_lo, q.norm = hip.ptr(prep.hi), hip.ptr(prep.lo), hip.ptr(prep.norm)
    q.w1_hi, q.w1_lo = hip.ptr(w1h), hip.ptr(w1l)
    q.b1, q.w2, q.b2 = hip.ptr(b1), hip.ptr(w2), hip.ptr(b2)
    q.mask, q.logit_part, q.counters = hip.ptr(mask), hip.ptr(parts), hip.ptr(counters)
    q.w, q.logits = hip.ptr(w), hip.ptr(logits, allow_none=True)
    q.n_samples, q.N, q.d, q.H, q.n_counters = n, N, prep.d, W1.shape[0], counters.numel()
    return q


def test_grouped_form_refuses_a_width_its_block_does_not_divide():
    """H = 1152 (H % 256 != 0): nr_token_weights_fwd_group returns NR_EUNSUPPORTED and writes nothing."""
    n, N = 17, 24
    par = _params(512, 1152)
    x, mask, prep = _tokens(1003, n, N)
    w = torch.full((n, N), float("nan"), device=DEV)
    parts = torch.full((1152 // 128, n * N), float("nan"), device=DEV)
    counters = torch.zeros(64, dtype=torch.int32, device=DEV)
    arr = (hip.TokenWeightsProblem * 1)()
    m = mask.float().contiguous()
    q = _problem(prep, par, m, n, N, w, parts, counters)
    ctypes.memmove(ctypes.addressof(arr), ctypes.addressof(q), ctypes.sizeof(q))
    rc = hip.lib().nr_token_weights_fwd_group(arr, (ctypes.c_int * 1)(hip.PREC_BF16), 1, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == hip.NR_EUNSUPPORTED
    assert bool(torch.isnan(w).all()) and bool(torch.isnan(parts).all()) and int(counters.abs().sum()) == 0


def _softmax_ref(parts, b2, mask, n, N):
    lg = parts.double().sum(0).view(n, N) + b2.double()
    w = torch.softmax(lg.masked_fill(mask.view(n, N) == 0, R.NEG_BIG), dim=-1)
    return w, lg


@pytest.mark.parametrize("N", [1, 63, 64, 65, 128, 129, 192, 255, 256])
def test_token_softmax_alone(N):
    """nr_token_softmax on synthetic partial logits: n_parts 1 / 8 / 9, 1 and 5 samples (5: not a multiple of a block's 4
    waves), logits spread over +-80, one sample whose largest logit sits on a masked token.  The parts are multiples of 2^-10
    whose partial sums stay below 128, so every fp32 sum of parts is exact and the pre-mask logits must EQUAL the fp64 sums; what is
    left for the weights is expf and one division: 1e-6 absolute, rows summing to 1 within 1e-6, everything finite."""
    for n_parts in (1, 8, 9):
        for n in (1, 5):
            u = synth.uniform(11 * N + n_parts, f"softmax/{n}", (n_parts, n * N))
            parts = torch.from_numpy(((2.0 * u - 1.0) * 5.0 * 1024).round() / 1024)          # +-5 each ...
            target = torch.from_numpy(((2.0 * synth.uniform(11 * N + n_parts, f"softmax/sum/{n}", (n * N,)) - 1.0) * 80.0 * 1024).round() / 1024)
            parts[-1] = target - parts[:-1].sum(0)                                           # ... summing to +-80
            parts = parts.float()
            mask = torch.from_numpy(synth.uniform(11 * N + n_parts, f"softmax/mask/{n}", (n, N)) > 0.3).float()
            lg = parts.double().sum(0).view(n, N)
            assert torch.equal(lg.view(-1), target)
            mask[0, int(lg[0].argmax())] = 0.0                       # the first sample's maximum is masked
            b2 = torch.tensor([0.125])
            w_ref, lg_ref = _softmax_ref(parts, b2, mask, n, N)
            w, lg_k = ops.token_softmax(parts.to(DEV), b2.to(DEV), mask.to(DEV), n, N, want_logits=True)
            w, lg_k = w.cpu(), lg_k.cpu()
            d_w = float((w.double() - w_ref).abs().max())
            d_sum = float((w.double().sum(-1) - 1.0).abs().max())
            print(f"softmax N={N} parts={n_parts} n={n}: w {d_w:.2e} row sums {d_sum:.1e} max|logit| {float(lg_ref.abs().max()):.1f}")
            assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(lg_k).all())
            assert torch.equal(lg_k.double(), lg_ref)
            assert d_w <= 1e-6 and d_sum <= 1e-6
            some = mask.sum(-1) > 0
            off = w[some][mask[some] == 0]
            assert off.numel() == 0 or float(off.abs().max()) == 0.0


def test_token_softmax_refuses_more_than_256_tokens():
    n, N = 2, 257
    parts = torch.zeros((1, n * N), device=DEV)
    w = torch.full((n, N), float("nan"), device=DEV)
    b2 = torch.zeros(1, device=DEV)
    rc = hip.lib().nr_token_softmax(hip.ptr(parts), 1, hip.ptr(b2), None, n, N, hip.ptr(w), None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == hip.NR_EUNSUPPORTED and bool(torch.isnan(w).all())


def test_grouped_form_against_fp64():
    """ONE nr_token_weights_fwd_group launch (192 x 256 blocks; split-bf16 sets as three accumulated passes) against the
    references, not only against the single launches: two split-bf16 and two one-pass sets."""
    sets = [(17, 24, "x3"), (17, 12, "x3"), (40, 12, "bf16"), (40, 24, "bf16")]
    par = _params()
    W1, b1, w2, b2, w1h, w1l = par
    data = []
    for k, (n, N, p) in enumerate(sets):
        x, mask = R.make_case(1005 + k, n, N)
        x, mask = x.to(DEV), mask.to(DEV)
        data.append((x, mask, ops.prepare_tokens(x, mask)))
    calls = [(prep, w1h, w1l, b1, w2, b2, mask, n, N) for (x, mask, prep), (n, N, p) in zip(data, sets)]
    n0 = hip.N_CALLS
    out = ops.token_weights_group(calls, [PREC[p] for _, _, p in sets], want_logits=True)
    torch.cuda.synchronize()
    assert out is not None and hip.N_CALLS - n0 == 1
    assert _counters_clear()
    for (x, mask, prep), (n, N, p), (w, lg) in zip(data, sets, out):
        _check(f"grouped {n}x{N} (192, 256, 2)", p, x, mask, prep, par, w, lg)


def test_paired_form_against_fp64():
    """ONE nr_token_weights_fwd_pair launch at (512, 24, 12) tokens in split-bf16 (96 x 128 blocks on a one-deep ring)."""
    par = _params()
    W1, b1, w2, b2, w1h, w1l = par
    data = []
    for k, N in enumerate((24, 12)):
        x, mask = R.make_case(1009 + k, 512, N)
        x, mask = x.to(DEV), mask.to(DEV)
        data.append((x, mask, ops.prepare_tokens(x, mask)))
    assert hip.token_scorer_plan(512 * 24, 1024, hip.PREC_BF16X3, 24)[:2] == (96, 128)
    assert hip.token_scorer_plan(512 * 12, 1024, hip.PREC_BF16X3, 12)[:2] == (96, 128)
    calls = [(prep, w1h, w1l, b1, w2, b2, mask, 512, mask.shape[1]) for x, mask, prep in data]
    n0 = hip.N_CALLS
    out = ops.token_weights_pair(calls, hip.PREC_BF16X3, want_logits=True)
    torch.cuda.synchronize()
    assert hip.N_CALLS - n0 == 1
    assert _counters_clear()
    for (x, mask, prep), (w, lg) in zip(data, out):
        _check(f"paired 512x{mask.shape[1]} (96, 128, 1)", "x3", x, mask, prep, par, w, lg)
