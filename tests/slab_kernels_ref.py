"""Pinned bits of the exhaustive test-time correction kernels (nr_hubnorm.hip, nr_sinknorm.hip, nr_localscale.hip and the two
applies of nr_mutualprox.hip): the inputs of every case, the calls of every family and the recorder of their digests.

The kernels claim bitwise reproducibility, so what a refactor of them has to keep is bits, not closeness.  golden/slab_kernels.json
holds, per (family, case), the sha256 of every input's bytes -- a generator that drifts (another NumPy, an edited line below) is a
loud failure, not a silent mismatch -- and the sha256 of every output's bytes, recorded on the commit before the kernels moved onto
the shared skeletons of csrc/nr_slab.h (three runs, identical digests).  This file imports nothing of the package but ops, so the
same file runs on both sides of such a change:

    python tests/slab_kernels_ref.py --out digests.json          # on the GPU; then compare or replace golden/slab_kernels.json

Inputs: NumPy default_rng on the host.  S = 0.1 * standard_normal in fp32 (its products with beta are inexact, so a fused and an
unfused multiply-add differ) with signed zeros, -inf, NaN, an all-NaN row and column, a row of -inf and one +inf.  Potentials and
statistics are random fp32, counts random int32 in range.

Shapes: (1, 1) the degenerate slab; (3, 37) the scalar path, less than one wave-stride; (130, 129) three row blocks, the last of 2
rows, odd L, three lane strides per row; (130, 1028) the vector path with a second column block (257 groups), also with S 4 bytes
off a 16-byte boundary (every kernel's scalar fallback) and with one vector operand misaligned.  That operand is one the 16-byte
path reads 16 bytes wide where the family has one -- sinknorm_steps (v, and the partial pairs' workspace), localscale_apply
(col_stat), mp_emp_apply (col_cnt), mp_gauss_apply (col_sd) -- and forces the fallback there; hubnorm_apply (col_norm),
sinknorm_apply (v) and hubnorm_stats (parts) read theirs entry by entry, so those cases pin the 16-byte path with a misaligned
operand instead.  For the applies alone: (2049, 2049) misaligned, more than 16384 x 256 entries, and (4100, 4100) aligned, more
than 16384 x 256 x 4: the second trip of the grid-stride loop on the scalar and on the vector path (hubnorm_apply in its gated
form only there: the other forms run the same loop)."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neighborretr_amd import ops  # noqa: E402

DEV = "cuda"
PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slab_kernels.json")

# case -> (n, L, beta, what is misaligned: None | "S" | "vec")
CASES = {
    "1x1": (1, 1, 20.0, None),
    "3x37": (3, 37, 20.0, None),
    "130x129": (130, 129, 20.0, None),
    "130x129-beta17.3": (130, 129, 17.3, None),
    "130x1028": (130, 1028, 20.0, None),
    "130x1028-S-off": (130, 1028, 20.0, "S"),
    "130x1028-vec-off": (130, 1028, 20.0, "vec"),
    "2049x2049-S-off": (2049, 2049, 20.0, "S"),
    "4100x4100": (4100, 4100, 20.0, None),
}
BIG = ("2049x2049-S-off", "4100x4100")                        # the applies alone
NO_BETA = ("localscale_apply", "mp_emp_apply", "mp_gauss_apply")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=1)
def inputs(case):
    """name -> host array of every input of every family at this case; one generator, drawn in a fixed order."""
    n, L, _, _ = CASES[case]
    rng = np.random.default_rng(1000003 * n + L)
    S = (0.1 * rng.standard_normal((n, L))).astype(np.float32)
    flat = S.reshape(-1)
    for val, frac in ((0.0, 0.05), (-0.0, 0.05), (-np.inf, 0.02), (np.nan, 0.05)):
        flat[rng.choice(flat.size, max(1, int(frac * flat.size)), replace=False)] = val
    if n > 2:
        S[0] = np.nan                                         # a row that is entirely NaN
        S[1, :] = -np.inf                                     # a row of -inf only
        S[n - 1, L - 1] = np.inf
    if L > 3:
        S[:, 2] = np.nan                                      # a column that is entirely NaN
        S[:, 3] = 0.0
        S[::2, 3] = -0.0                                      # a column of signed zeros only

    def f32(size, scale=1.0, shift=0.0):
        return (shift + scale * rng.standard_normal(size)).astype(np.float32)

    def spread(size):                                         # a deviation: mostly positive, with a zero, a tiny one and a NaN
        x = np.abs(f32(size, 0.1)) + np.float32(1e-3)
        x[rng.integers(0, size)] = 0.0
        x[rng.integers(0, size)] = 1e-9
        x[rng.integers(0, size)] = np.nan
        return x

    def i32(size, hi):
        return rng.integers(0, hi + 1, size=size, dtype=np.int32)

    d = {"S": S}
    d["u"], d["v"] = f32(n, 2.0), f32(L, 2.0)
    d["log_mu"], d["log_nu"] = f32(n, 0.1, -np.log(n)), f32(L, 0.1, -np.log(L))
    d["row_norm"], d["col_norm"] = f32(n, 1.0, 3.0), f32(L, 1.0, 3.0)
    d["row_gate"], d["col_gate"] = i32(n, 1), i32(L, 1)
    d["row_stat"], d["col_stat"] = f32(n, 0.5, 0.6), f32(L, 0.5, 0.6)      # some above 1: the floor of the distance scale
    d["row_stat"][rng.integers(0, n)] = np.nan
    d["col_stat"][rng.integers(0, L)] = np.nan
    d["row_mean"], d["row_sd"], d["col_mean"], d["col_sd"] = f32(n, 0.1), spread(n), f32(L, 0.1), spread(L)
    d["row_cnt"], d["col_cnt"] = i32(n, 1000), i32(L, 1000)                # a count of 0 among them: 0 / 0
    d["r2"] = (rng.random((n, L)) * (2 * d["row_cnt"][:, None] + 1)).astype(np.int32)
    d["c2"] = (rng.random((n, L)) * (2 * d["col_cnt"][None, :] + 1)).astype(np.int32)
    if case not in BIG:
        P = 3                                                 # pairs to merge: ties of the max, empty pairs, infinite maxima
        m = (np.round(rng.standard_normal((P, L)) * 4) / 4).astype(np.float32)
        s = (0.5 + 4 * rng.random((P, L))).astype(np.float32)
        s[rng.random((P, L)) < 0.2] = 0.0
        m[rng.random((P, L)) < 0.05] = -np.inf
        m[rng.random((P, L)) < 0.05] = np.inf
        d["parts"] = np.ascontiguousarray(np.stack([m, s], axis=1))
    return d


def _put(a, off=False):
    """The array on the device; off: its storage starts 4 bytes past a 16-byte boundary (the kernels' scalar paths)."""
    t = torch.from_numpy(a)
    if not off:
        out = t.to(DEV)
        assert out.data_ptr() % 16 == 0
        return out
    out = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# family -> (the inputs it reads, the one misaligned in the "vec" cases, its calls)
def _hubnorm_stats(t, beta, case):
    stats, lse = ops.hubnorm_combine(t["parts"], want_stats=True)
    return {"row_lse": ops.hubnorm_row_lse(t["S"], beta), "col_stats": ops.hubnorm_col_stats(t["S"], beta),
            "combine_lse": ops.hubnorm_combine(t["parts"]), "combine_stats": stats, "combine_stats_lse": lse}


def _hubnorm_apply(t, beta, case):
    out = {}
    for mode in ("is", "dsl"):
        forms = {"gated": dict(col_norm=t["col_norm"], row_gate=t["row_gate"], row_norm=t["row_norm"], col_gate=t["col_gate"])}
        if case not in BIG:
            forms["plain"] = dict(col_norm=t["col_norm"], row_norm=t["row_norm"])
            forms["t_only"] = dict(col_norm=t["col_norm"], row_gate=t["row_gate"], want_v=False)
            forms["v_only"] = dict(row_norm=t["row_norm"], col_gate=t["col_gate"], want_t=False)
        for form, kw in forms.items():
            T, V = ops.hubnorm_apply(t["S"], beta, mode, **kw)
            assert (T is None) == (form == "v_only") and (V is None) == (form == "t_only")
            if T is not None:
                out[f"{mode}_{form}_T"] = T
            if V is not None:
                out[f"{mode}_{form}_V"] = V
    return out


def _sinknorm_steps(t, beta, case):
    n, L = t["S"].shape
    ws = ops.sinknorm_workspace(n, L, DEV)
    if CASES[case][3] == "vec":                               # the partial pairs' workspace 4 bytes off as well
        ws = torch.empty(ws.numel() + 4, dtype=torch.uint8, device=DEV)[4:]
        assert ws.data_ptr() % 16 == 4
    blocks = ops.sinknorm_col_stats(t["S"], beta, t["u"], workspace=ws, want_stats=False)
    return {"row": ops.sinknorm_row(t["S"], beta, t["v"], t["log_mu"]),
            "row_err": ops.sinknorm_row_err(t["S"], beta, t["u"], t["v"], t["log_mu"]),
            "col_blocks": blocks.clone(), "finish_blocks": ops.sinknorm_finish_cols(blocks, t["log_nu"]),
            "col_stats": ops.sinknorm_col_stats(t["S"], beta, t["u"]),
            "finish_parts": ops.sinknorm_finish_cols(t["parts"], t["log_nu"])}


FAMILIES = {
    "hubnorm_stats": (("S", "parts"), "parts", _hubnorm_stats),
    "hubnorm_apply": (("S", "col_norm", "row_norm", "row_gate", "col_gate"), "col_norm", _hubnorm_apply),
    "sinknorm_steps": (("S", "u", "v", "log_mu", "log_nu", "parts"), "v", _sinknorm_steps),
    "sinknorm_apply": (("S", "u", "v"), "v", lambda t, beta, case: {"T": ops.sinknorm_apply(t["S"], beta, t["u"], t["v"])}),
    "localscale_apply": (("S", "row_stat", "col_stat"), "col_stat", lambda t, beta, case: {
        mode: ops.localscale_apply(t["S"], mode, t["row_stat"], t["col_stat"]) for mode in ("csls", "nicdm", "ls")}),
    "mp_emp_apply": (("S", "r2", "c2", "row_cnt", "col_cnt"), "col_cnt", lambda t, beta, case: {
        "T": ops.mp_emp_apply(t["S"], t["r2"], t["c2"], t["row_cnt"], t["col_cnt"])}),
    "mp_gauss_apply": (("S", "row_mean", "row_sd", "col_mean", "col_sd"), "col_sd", lambda t, beta, case: {
        "T": ops.mp_gauss_apply(t["S"], t["row_mean"], t["row_sd"], t["col_mean"], t["col_sd"])}),
}


def pairs():
    """Every (family, case) that is pinned: the reductions leave out the two large shapes, a family without beta its second beta."""
    for family in FAMILIES:
        for case in CASES:
            if case in BIG and not family.endswith("_apply"):
                continue
            if family in NO_BETA and "beta" in case:
                continue
            yield family, case


def record(family, case):
    """{"inputs": name -> sha256, "outputs": name -> sha256} of one family at one case, computed on the GPU."""
    names, vec_operand, calls = FAMILIES[family]
    _, _, beta, off = CASES[case]
    host = inputs(case)
    t = {name: _put(host[name], off=(off == "S" and name == "S") or (off == "vec" and name == vec_operand)) for name in names}
    out = calls(t, beta, case)
    torch.cuda.synchronize()
    return {"inputs": {name: digest(host[name]) for name in names},
            "outputs": {name: digest(x.cpu().numpy()) for name, x in out.items()}}


def pinned():
    with open(PINNED) as f:
        return json.load(f)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True, help="where to write the digests (JSON)")
    args = ap.parse_args()
    result = {f"{family}/{case}": record(family, case) for family, case in sorted(pairs(), key=lambda fc: (fc[1], fc[0]))}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(result)} (family, case) pairs, {sum(len(r['outputs']) for r in result.values())} outputs -> {args.out}")
