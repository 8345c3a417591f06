"""CPU probe: what ONE low-precision pass on the batch side costs the losses (bf16 against fp16).

The training plan runs the batch x batch product and the two batch scorers on operands of fewer bits than fp32.  This tool
measures, on the CPU oracle, what that does to the five losses: `oracle/nr_oracle.local_level_parts` is patched so that ONLY
its first call of a `compute_losses` (the batch x batch one; the two bank products follow) rounds

    the normalised, masked text tokens, the normalised, masked video tokens, and W1 of both scorers

to the candidate type.  Everything else stays fp32, products accumulate in fp32, and the scorer's pre-activation is
(x_hat . W1) * ||x|| + b1, as the kernels compute it.  Reported per case: max |dL| over the five losses (entries whose
reference is finite) for one bf16 pass, one fp16 pass and one fp16 pass with fp16 subnormals flushed to zero, max |dS| of the
fp16 pass, and max |x| of every fp16 operand (fp16 overflows past 65504 and loses bits under 6.1e-5).

    python tools/prec_probe_f16.py > profiles/f16_prec_probe.txt

Cases: the inputs of the reference fixtures c1_b16, c2_b128, c4_b8, r32_blank and 20 seeded random small shapes (B 3..40) whose
reference losses are all finite.  A launch is switched to fp16 only if its worst |dL| here stays <= 5e-4.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nr_oracle as O  # noqa: E402
from neighborretr_amd import synth  # noqa: E402

BAR = 5e-4
FIXTURES = ("c1_b16", "c2_b128", "c4_b8", "r32_blank")
F16_TINY = 2.0 ** -14          # smallest normal fp16


def _round(x, kind):
    if kind == "bf16":
        return x.to(torch.bfloat16).float()
    y = x.to(torch.float16).float()
    if kind == "f16_ftz":
        y = torch.where(y.abs() < F16_TINY, torch.zeros_like(y), y)
    return y


def _rounded_parts(kind, seen):
    """local_level_parts with its operands rounded to `kind` (the arithmetic of the kernels: see the module docstring)."""
    def parts(text_feat, video_feat, text_mask, video_mask, P, prefix_t="text_weight_fc", prefix_v="video_weight_fc"):
        dt = text_feat.dtype
        nt = text_feat.norm(dim=-1).clamp_min(1e-12)
        nv = video_feat.norm(dim=-1).clamp_min(1e-12)
        tn = _round(F.normalize(text_feat, dim=-1) * text_mask.to(dt)[..., None], kind)
        vn = _round(F.normalize(video_feat, dim=-1) * video_mask.to(dt)[..., None], kind)
        w1t, w1v = _round(P[prefix_t + ".0.weight"], kind), _round(P[prefix_v + ".0.weight"], kind)
        for name, t in (("x_hat text", tn), ("x_hat video", vn), ("W1 text", w1t), ("W1 video", w1v)):
            seen[name] = max(seen.get(name, 0.0), float(t.abs().max()))

        def weights(xn, nrm, mask, w1, prefix):
            h = F.relu((xn @ w1.t()) * nrm[..., None] + P[prefix + ".0.bias"])
            logit = F.linear(h, P[prefix + ".2.weight"], P[prefix + ".2.bias"]).squeeze(-1)
            return torch.softmax(logit.masked_fill((1 - mask).to(torch.bool), O.NEG_BIG), dim=-1)

        w_t, w_v = weights(tn, nt, text_mask, w1t, prefix_t), weights(vn, nv, video_mask, w1v, prefix_v)
        A, Nt, d = tn.shape
        Bv, Nv, _ = vn.shape
        R = (tn.reshape(A * Nt, d) @ vn.reshape(Bv * Nv, d).t()).reshape(A, Nt, Bv, Nv).permute(0, 2, 1, 3)
        R = R * text_mask.to(dt)[:, None, :, None] * video_mask.to(dt)[None, :, None, :]
        pmax, arg_v = R.max(dim=-1)
        qmax, arg_t = R.max(dim=-2)
        t2v, v2t = (pmax * w_t[:, None, :]).sum(-1), (qmax * w_v[None, :, :]).sum(-1)
        return (t2v + v2t) / 2.0, t2v, v2t, w_t, w_v, arg_v, arg_t
    return parts


def _losses(x, P, nz, hp, kind=None, seen=None):
    """(losses [5], S) of the oracle; kind: None = fp32, else the batch x batch call's operands rounded to it."""
    plain, calls = O.local_level_parts, [0]
    rounded = _rounded_parts(kind, seen if seen is not None else {}) if kind else None

    def patched(*a, **kw):
        calls[0] += 1
        return rounded(*a, **kw) if (rounded is not None and calls[0] == 1) else plain(*a, **kw)

    O.local_level_parts = patched
    try:
        kw = dict(return_parts=True)
        try:
            out, parts = O.compute_losses(x["text_feat"], x["video_feat"], x["text_mask"], x["video_mask"], x["mb_feat_t"], x["mb_feat_v"],
                                          x["mb_mask_t"], x["mb_mask_v"], P, hp, torch.tensor(100.0), nz, **kw)
        except RuntimeError:          # more than one global token per sample: the documented "mean" reduction
            calls[0] = 0
            out, parts = O.compute_losses(x["text_feat"], x["video_feat"], x["text_mask"], x["video_mask"], x["mb_feat_t"], x["mb_feat_v"],
                                          x["mb_mask_t"], x["mb_mask_v"], P, hp, torch.tensor(100.0), nz, centrality_multi_token="mean", **kw)
    finally:
        O.local_level_parts = plain
    return torch.stack([o.detach() for o in out]).double(), parts["S"].detach().double()


def probe(seed, B, Nt, Nv, M, K, blank_video=-1, param_seed=7):
    """-> dict(dL_bf16, dL_f16, dL_f16_ftz, dS_f16, finite (count of finite reference losses), max_abs {operand: max |x|})."""
    p = synth.make_problem(seed, B, Nt, Nv, M, ragged=True)
    if blank_video >= 0:
        p["video_mask"][blank_video] = 0
    x = {k: torch.from_numpy(v) for k, v in p.items()}
    P = {k: torch.from_numpy(v) for k, v in synth.make_params(param_seed).items()}
    nz = {k: torch.from_numpy(v) for k, v in synth.make_noise(seed, B, Nt, Nv).items()}
    hp = dict(synth.DEFAULT_HP, num_neighbors=K)
    with torch.no_grad():
        ref, S_ref = _losses(x, P, nz, hp)
        ok = torch.isfinite(ref)
        res = dict(finite=int(ok.sum()), max_abs={})
        for kind in ("bf16", "f16", "f16_ftz"):
            seen = {}
            got, S = _losses(x, P, nz, hp, kind, seen)
            res["dL_" + kind] = float((got - ref)[ok].abs().max()) if bool(ok.any()) else float("nan")
            if not bool(torch.isfinite(got[ok]).all()):
                res["dL_" + kind] = float("inf")
            if kind == "f16":
                res["dS_f16"], res["max_abs"] = float((S - S_ref).abs().max()), seen
    return res


def probe_fixture(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    B, Nt, Nv, M, K = (int(g[k]) for k in ("B", "Nt", "Nv", "M", "K"))
    return (int(g["seed"]), B, Nt, Nv, M, K), probe(int(g["seed"]), B, Nt, Nv, M, K, int(g["blank_video"]), int(g["param_seed"]))


def random_shapes(n=20, first_seed=3001):
    """n seeded small shapes (B 3..40, MSR-VTT token counts) whose reference losses are all finite."""
    out, seed = [], first_seed
    while len(out) < n:
        r = np.random.RandomState(seed)
        B = int(r.randint(3, 41))
        shape = (seed, B, 24, 12, int(r.choice([32, 64, 96, 128])), int(r.randint(1, min(B, 20) + 1)))
        res = probe(*shape)
        if res["finite"] == 5:
            out.append((shape, res))
        seed += 1
    return out


def _line(label, shape, r):
    ops_ = ", ".join(f"{k} {v:.4g}" for k, v in r["max_abs"].items())
    return (f"{label:<12} (seed,B,Nt,Nv,M,K)={shape}  finite losses {r['finite']}/5  max|dL| bf16 {r['dL_bf16']:.3g}  f16 {r['dL_f16']:.3g}  "
            f"f16 flushed {r['dL_f16_ftz']:.3g}  max|dS| f16 {r['dS_f16']:.3g}  max|x| of the fp16 operands: {ops_}")


def main():
    worst = dict(bf16=0.0, f16=0.0, f16_ftz=0.0)
    print("one low-precision pass on the batch x batch product and the batch scorers, CPU oracle (tools/prec_probe_f16.py)")
    rows = [(name,) + probe_fixture(name) for name in FIXTURES] + [("random",) + sr for sr in random_shapes()]
    for label, shape, r in rows:
        print(_line(label, shape, r))
        for k in worst:
            if np.isfinite(r["dL_" + k]):
                worst[k] = max(worst[k], r["dL_" + k])
    print(f"worst max|dL|: bf16 {worst['bf16']:.3g}  f16 {worst['f16']:.3g}  f16 flushed {worst['f16_ftz']:.3g}   bar {BAR:g} "
          f"-> fp16 {'clears' if worst['f16'] <= BAR else 'MISSES'} it, bf16 {'clears' if worst['bf16'] <= BAR else 'misses'} it")
    return 0 if worst["f16"] <= BAR else 1


if __name__ == "__main__":
    sys.exit(main())
