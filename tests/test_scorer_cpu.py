"""CPU: the token scorer's fp64 references (tests/scorer_ref.py) checked against themselves -- a token-by-token loop in Python
doubles, and the operand reference against the exact one within the bars the GPU tests use (tests/test_scorer_gpu.py).
The launch-form table those tests rely on is pinned in tests/test_host_cpu.py (test_token_scorer_plan_no_gpu_needed)."""
import torch

import scorer_ref as R
from neighborretr_amd import synth


def _params(H, d, seed=7):
    W1 = torch.from_numpy((0.02 * synth.normal(seed, "scorer/w1", (H, d))).astype("float32"))
    b1 = torch.from_numpy((0.01 * synth.normal(seed, "scorer/b1", (H,))).astype("float32"))
    w2 = torch.from_numpy((0.02 * synth.normal(seed, "scorer/w2", (H,))).astype("float32"))
    b2 = torch.from_numpy((0.01 * synth.normal(seed, "scorer/b2", (1,))).astype("float32"))
    return W1, b1, w2, b2


def test_references_equal_a_token_by_token_loop():
    """3 samples x 5 tokens (one fully masked, one with a single valid token), d = 64, H = 128: `exact` and `operand` (one
    pass and three terms) against the same sums written as Python loops over doubles.  fp64 against fp64: 1e-12."""
    n, N, d, H = 3, 5, 64, 128
    x, mask = R.make_case(3, n, N, d)
    assert int(mask[1].sum()) == 0 and int(mask[2].sum()) == 1
    W1, b1, w2, b2 = _params(H, d)
    w, lg = R.exact(x, mask, W1, b1, w2, b2)
    w_n, lg_n = R.naive([(x, W1)], None, mask, b1, w2, b2)
    assert (w - w_n).abs().max() < 1e-12 and (lg - lg_n).abs().max() < 1e-12
    assert torch.equal(w[1], torch.full((N,), 1.0 / N, dtype=torch.float64))         # fully masked: uniform
    assert float(w[2, 0]) == 1.0 and float(w[2, 1:].abs().max()) == 0.0              # one valid token
    hi, lo, norm = R.prepare_tokens(x, mask)
    wh, wl = R.split_bf16(W1)
    Xh, Xl = (R.bf16_bits(t).double().view(n, N, d) for t in (hi, lo))
    Wh, Wl = (R.bf16_bits(t).double() for t in (wh, wl))
    for three, terms in ((False, [(Xh, Wh)]), (True, [(Xh, Wh), (Xh, Wl), (Xl, Wh)])):
        w, lg = R.operand(hi, lo, norm, wh, wl, b1, w2, b2, mask, n, N, three)
        w_n, lg_n = R.naive(terms, norm.view(n, N), mask, b1, w2, b2)
        assert (w - w_n).abs().max() < 1e-12 and (lg - lg_n).abs().max() < 1e-12, three
    # masked tokens have zero operand rows: their pre-mask logit is relu(b1) . w2 + b2
    blank = float(torch.relu(b1.double()) @ w2.double() + b2.double())
    assert (lg[mask == 0] - blank).abs().max() < 1e-12


def test_three_term_operands_stay_within_the_split_bf16_bars_of_the_exact_reference():
    """The plan's three terms on bf16 halves against the fp32 inputs, 17 x 24 tokens at the head's own width and parameters:
    weights within 2e-5, logits of valid tokens within 2e-4 (the exact tier of the GPU tests); the single bf16 pass is two
    orders of magnitude away, so the bars tell the two plans apart."""
    n, N = 17, 24
    x, mask = R.make_case(1001, n, N)
    P = {k: torch.from_numpy(v) for k, v in synth.make_params(7).items()}
    W1, b1 = P["text_weight_fc.0.weight"], P["text_weight_fc.0.bias"]
    w2, b2 = P["text_weight_fc.2.weight"].reshape(-1), P["text_weight_fc.2.bias"]
    hi, lo, norm = R.prepare_tokens(x, mask)
    wh, wl = R.split_bf16(W1)
    w_e, lg_e = R.exact(x, mask, W1, b1, w2, b2)
    valid = mask.bool()
    w3, lg3 = R.operand(hi, lo, norm, wh, wl, b1, w2, b2, mask, n, N, True)
    assert (w3 - w_e).abs().max() <= 2e-5 and (lg3 - lg_e)[valid].abs().max() <= 2e-4
    w1, lg1 = R.operand(hi, lo, norm, wh, wl, b1, w2, b2, mask, n, N, False)
    assert (lg1 - lg_e)[valid].abs().max() > 2e-4 and (lg1 - lg_e)[valid].abs().max() <= 3e-2
