"""Tensor-level wrappers, one per C entry point of libnr_hip.so (no autograd here).

Each function allocates its outputs with torch (device memory plumbing only), enqueues the HIP
kernel on torch's current stream and returns without synchronising.
"""
import ctypes
import math
from collections import namedtuple

import torch

from . import hip

# hi / lo: the bf16 pair; f16: the fp16 plane of the same values (the operand of hip.PREC_F16 contractions) or None
Prepared = namedtuple("Prepared", "hi lo norm colsum n_tok d f16", defaults=(None,))


def _planes(prep, prec):
    """(first, second) operand planes of a Prepared for a contraction precision: the bf16 pair, or (fp16 plane, None)."""
    if int(prec) == hip.PREC_F16:
        if prep.f16 is None:
            raise hip.NrHipError("PREC_F16 needs the fp16 plane: prepare the tokens with want_f16=True")
        return prep.f16, None
    return prep.hi, prep.lo


_COUNTERS = {}


def _f32(t):
    return t if t.dtype == torch.float32 else t.float()


def prepare_tokens(x, mask=None, normalize=True, want_lo=None, want_norm=True, want_colsum=False, want_f16=None):
    """x [..., d] f32 -> bf16 hi/lo of normalize(x)*mask  (nr_prepare_tokens), with want_f16 also their fp16 plane in the same
    pass (nr_prepare_tokens_f16).  A caller that names no plane (want_lo and want_f16 both left out) gets every plane of the
    normalised tokens, so that the result serves whatever precision it is handed to next."""
    if want_f16 is None:
        want_f16 = want_lo is None and bool(normalize)
    if want_lo is None:
        want_lo = True
    x = _f32(x).contiguous()
    d = x.shape[-1]
    n_tok = x.numel() // d
    dev = x.device
    hi = torch.empty((n_tok, d), dtype=torch.int16, device=dev)
    lo = torch.empty((n_tok, d), dtype=torch.int16, device=dev) if want_lo else None
    f16 = torch.empty((n_tok, d), dtype=torch.int16, device=dev) if want_f16 else None
    norm = torch.empty((n_tok,), dtype=torch.float32, device=dev) if want_norm else None
    colsum = None
    if want_colsum:
        colsum = torch.empty((hip.prepare_parts(n_tok), d), dtype=torch.float32, device=dev)
    m = None
    if mask is not None:
        m = _f32(mask).contiguous()
        if m.numel() != n_tok:
            raise ValueError("mask does not match the token count")
    if f16 is not None:
        hip.call("nr_prepare_tokens_f16", hip.ptr(x, torch.float32), hip.ptr(m, allow_none=True), n_tok, d,
                 1 if normalize else 0, hip.ptr(hi), hip.ptr(lo, allow_none=True), hip.ptr(f16), hip.ptr(norm, allow_none=True),
                 hip.ptr(colsum, allow_none=True), hip.stream_ptr())
        return Prepared(hi, lo, norm, colsum, n_tok, d, f16)
    hip.call("nr_prepare_tokens", hip.ptr(x, torch.float32), hip.ptr(m, allow_none=True), n_tok, d,
             1 if normalize else 0, hip.ptr(hi), hip.ptr(lo, allow_none=True), hip.ptr(norm, allow_none=True),
             hip.ptr(colsum, allow_none=True), hip.stream_ptr())
    return Prepared(hi, lo, norm, colsum, n_tok, d)


def prepare_tokens_pair(x0, mask0, x1, mask1, want_lo=True, want_colsum=False, want_f16=False):
    """prepare_tokens of two token tensors of the same width in ONE launch (nr_prepare_tokens_pair; with want_f16 the fp16 planes
    too: nr_prepare_tokens_pair_f16) -> (Prepared, Prepared)."""
    x0, x1 = _f32(x0).contiguous(), _f32(x1).contiguous()
    d = x0.shape[-1]
    if x1.shape[-1] != d:
        raise ValueError("both tensors must have the same feature width")
    dev = x0.device
    out, argv = [], []
    for x, mask in ((x0, mask0), (x1, mask1)):
        n_tok = x.numel() // d
        hi = torch.empty((n_tok, d), dtype=torch.int16, device=dev)
        lo = torch.empty((n_tok, d), dtype=torch.int16, device=dev) if want_lo else None
        f16 = torch.empty((n_tok, d), dtype=torch.int16, device=dev) if want_f16 else None
        norm = torch.empty((n_tok,), dtype=torch.float32, device=dev)
        colsum = torch.empty((hip.prepare_parts(n_tok), d), dtype=torch.float32, device=dev) if want_colsum else None
        m = None
        if mask is not None:
            m = _f32(mask).contiguous()
            if m.numel() != n_tok:
                raise ValueError("mask does not match the token count")
        argv += [hip.ptr(x, torch.float32), hip.ptr(m, allow_none=True), n_tok, hip.ptr(hi), hip.ptr(lo, allow_none=True)]
        argv += [hip.ptr(f16)] if want_f16 else []
        argv += [hip.ptr(norm), hip.ptr(colsum, allow_none=True)]
        out.append((Prepared(hi, lo, norm, colsum, n_tok, d, f16), m))
    hip.call("nr_prepare_tokens_pair_f16" if want_f16 else "nr_prepare_tokens_pair", *argv, d, 1, hip.stream_ptr())
    return out[0][0], out[1][0]


def split_bf16(w, want_lo=True):
    w = _f32(w).contiguous()
    hi = torch.empty(w.shape, dtype=torch.int16, device=w.device)
    lo = torch.empty(w.shape, dtype=torch.int16, device=w.device) if want_lo else None
    hip.call("nr_split_bf16", hip.ptr(w, torch.float32), w.numel(), hip.ptr(hi), hip.ptr(lo, allow_none=True),
             hip.stream_ptr())
    return hi, lo


def split_f16(w):
    """fp32 -> fp16 plane (int16 storage) of a weight matrix (nr_split_f16): the PREC_F16 image of a scorer's W1."""
    w = _f32(w).contiguous()
    f16 = torch.empty(w.shape, dtype=torch.int16, device=w.device)
    hip.call("nr_split_f16", hip.ptr(w, torch.float32), w.numel(), hip.ptr(f16), hip.stream_ptr())
    return f16


def token_logit_parts(prep, w1_hi, w1_lo, b1, w2, prec):
    """[H/128, n_tok] partial logits of the token scorer (nr_token_logits_fwd)."""
    H = w1_hi.shape[0]
    parts = torch.empty((H // 128, prep.n_tok), dtype=torch.float32, device=prep.hi.device)
    t_a, t_b = _planes(prep, prec)
    hip.call("nr_token_logits_fwd", hip.ptr(t_a), hip.ptr(t_b, allow_none=True), hip.ptr(prep.norm), prep.n_tok,
             prep.d, hip.ptr(w1_hi), hip.ptr(w1_lo, allow_none=True), hip.ptr(b1, torch.float32),
             hip.ptr(w2, torch.float32), H, prec, hip.ptr(parts), hip.stream_ptr())
    return parts


def token_softmax(parts, b2, mask, n_samples, N, want_logits=False):
    w = torch.empty((n_samples, N), dtype=torch.float32, device=parts.device)
    logits = torch.empty((n_samples, N), dtype=torch.float32, device=parts.device) if want_logits else None
    m = _f32(mask).contiguous() if mask is not None else None
    hip.call("nr_token_softmax", hip.ptr(parts), parts.shape[0], hip.ptr(b2, torch.float32), hip.ptr(m, allow_none=True),
             n_samples, N, hip.ptr(w), hip.ptr(logits, allow_none=True), hip.stream_ptr())
    return w, logits


FUSE_TOKEN_SOFTMAX = True      # scorer MLP + masked softmax in one launch (nr_token_weights_fwd); False: two launches (A/B)
_SOFTMAX_SLOTS, _SOFTMAX_SLOT_LEN = 16, 4096


def _softmax_counters(dev, n_tok):
    """Zeroed per-row-tile counters for one nr_token_weights_fwd launch.  Scorer launches of one step may run side by side on
    different streams, so consecutive calls take different slots of a per-device pool (16 slots: a step issues at most six
    scorer launches; a slot comes round again only behind launches that are ordered after its previous user).  The kernel
    leaves its counters zeroed."""
    need = (n_tok + 63) // 64
    if need > _SOFTMAX_SLOT_LEN:
        return None
    key = ("softmax", dev)
    st = _COUNTERS.get(key)
    if st is None:
        st = _COUNTERS[key] = [torch.zeros((_SOFTMAX_SLOTS, _SOFTMAX_SLOT_LEN), dtype=torch.int32, device=dev), 0]
    st[1] = (st[1] + 1) % _SOFTMAX_SLOTS
    return st[0][st[1]]


def token_weights(prep, w1_hi, w1_lo, b1, w2, b2, mask, n_samples, N, prec, want_logits=False):
    """Token scorer + masked softmax (modeling.py:485-492): (w [n,N], logits or None).  One launch
    (nr_token_weights_fwd: the last column block of every row tile does the tile's softmax) when a block shape holds whole
    samples, else nr_token_logits_fwd + nr_token_softmax.  prec = hip.PREC_F16: w1_hi is the fp16 image of W1 (split_f16), w1_lo
    None, and the tokens' fp16 plane is read."""
    dev = prep.hi.device
    t_a, t_b = _planes(prep, prec)
    counters = _softmax_counters(dev, prep.n_tok) if FUSE_TOKEN_SOFTMAX else None
    if counters is not None:
        H = w1_hi.shape[0]
        parts = torch.empty((H // 128, prep.n_tok), dtype=torch.float32, device=dev)
        w = torch.empty((n_samples, N), dtype=torch.float32, device=dev)
        logits = torch.empty((n_samples, N), dtype=torch.float32, device=dev) if want_logits else None
        m = _f32(mask).contiguous() if mask is not None else None
        hip.N_CALLS += 1
        rc = hip.lib().nr_token_weights_fwd(
            hip.ptr(t_a), hip.ptr(t_b, allow_none=True), hip.ptr(prep.norm), n_samples, N, prep.d, hip.ptr(w1_hi),
            hip.ptr(w1_lo, allow_none=True), hip.ptr(b1, torch.float32), hip.ptr(w2, torch.float32), hip.ptr(b2, torch.float32),
            H, prec, hip.ptr(m, allow_none=True), hip.ptr(parts), hip.ptr(counters), counters.numel(), hip.ptr(w),
            hip.ptr(logits, allow_none=True), hip.stream_ptr())
        if rc == 0:
            return w, logits
        if rc != hip.NR_EUNSUPPORTED:
            hip._check("nr_token_weights_fwd", rc)
    parts = token_logit_parts(prep, w1_hi, w1_lo, b1, w2, prec)
    return token_softmax(parts, b2, mask, n_samples, N, want_logits)


def token_weights_pair(calls, prec, want_logits=False):
    """Two token_weights calls of one precision in ONE launch (nr_token_weights_fwd_pair; bit-identical to the single calls).
    calls: two tuples (prep, w1_hi, w1_lo, b1, w2, b2, mask, n_samples, N).  -> [(w, logits or None), (w, logits or None)]; falls
    back to two launches when the two do not run the same block shape."""
    dev = calls[0][0].hi.device
    probs, outs, keep = [], [], []
    for prep, w1_hi, w1_lo, b1, w2, b2, mask, n_samples, N in calls:
        counters = _softmax_counters(dev, prep.n_tok) if FUSE_TOKEN_SOFTMAX else None
        if counters is None:
            probs = None
            break
        H = w1_hi.shape[0]
        parts = torch.empty((H // 128, prep.n_tok), dtype=torch.float32, device=dev)
        w = torch.empty((n_samples, N), dtype=torch.float32, device=dev)
        m = _f32(mask).contiguous() if mask is not None else None
        q = hip.TokenWeightsProblem()
        t_a, t_b = _planes(prep, prec)
        q.tok_hi, q.tok_lo, q.norm = hip.ptr(t_a), hip.ptr(t_b, allow_none=True), hip.ptr(prep.norm)
        q.w1_hi, q.w1_lo = hip.ptr(w1_hi), hip.ptr(w1_lo, allow_none=True)
        q.b1, q.w2, q.b2 = hip.ptr(b1, torch.float32), hip.ptr(w2, torch.float32), hip.ptr(b2, torch.float32)
        q.mask, q.logit_part, q.counters = hip.ptr(m, allow_none=True), hip.ptr(parts), hip.ptr(counters)
        logits = torch.empty((n_samples, N), dtype=torch.float32, device=dev) if want_logits else None
        q.w, q.logits = hip.ptr(w), hip.ptr(logits, allow_none=True)
        q.n_samples, q.N, q.d, q.H, q.n_counters = int(n_samples), int(N), int(prep.d), int(H), counters.numel()
        probs.append(q)
        outs.append((w, logits))
        keep += [parts, m]
    if probs is not None:
        hip.N_CALLS += 1
        rc = hip.lib().nr_token_weights_fwd_pair(ctypes.byref(probs[0]), ctypes.byref(probs[1]), prec, hip.stream_ptr())
        if rc == 0:
            return outs
        if rc != hip.NR_EUNSUPPORTED:
            hip._check("nr_token_weights_fwd_pair", rc)
        hip.N_CALLS -= 1
    return [token_weights(*c, prec, want_logits) for c in calls]


def token_weights_group(calls, precs, want_logits=False):
    """Up to four token_weights calls, each in its own precision, in ONE launch (nr_token_weights_fwd_group: 192 x 256 blocks,
    split-bf16 sets as three accumulated passes).  calls: tuples (prep, w1_hi, w1_lo, b1, w2, b2, mask, n_samples, N); precs: one
    hip.PREC_* per call.  -> [(w, logits or None), ...], or None when a set does not fit the grouped form (nothing launched: the caller
    issues the calls one by one)."""
    if not FUSE_TOKEN_SOFTMAX or not 0 < len(calls) <= 4:
        return None
    dev = calls[0][0].hi.device
    arr = (hip.TokenWeightsProblem * len(calls))()
    outs, keep = [], []
    for q, (prep, w1_hi, w1_lo, b1, w2, b2, mask, n_samples, N) in zip(arr, calls):
        counters = _softmax_counters(dev, prep.n_tok)
        if counters is None:
            return None
        H = w1_hi.shape[0]
        parts = torch.empty((H // 128, prep.n_tok), dtype=torch.float32, device=dev)
        w = torch.empty((n_samples, N), dtype=torch.float32, device=dev)
        m = _f32(mask).contiguous() if mask is not None else None
        q.tok_hi, q.tok_lo, q.norm = hip.ptr(prep.hi), hip.ptr(prep.lo, allow_none=True), hip.ptr(prep.norm)
        q.w1_hi, q.w1_lo = hip.ptr(w1_hi), hip.ptr(w1_lo, allow_none=True)
        q.b1, q.w2, q.b2 = hip.ptr(b1, torch.float32), hip.ptr(w2, torch.float32), hip.ptr(b2, torch.float32)
        q.mask, q.logit_part, q.counters = hip.ptr(m, allow_none=True), hip.ptr(parts), hip.ptr(counters)
        logits = torch.empty((n_samples, N), dtype=torch.float32, device=dev) if want_logits else None
        q.w, q.logits = hip.ptr(w), hip.ptr(logits, allow_none=True)
        q.n_samples, q.N, q.d, q.H, q.n_counters = int(n_samples), int(N), int(prep.d), int(H), counters.numel()
        outs.append((w, logits))
        keep += [parts, m]
    pa = (ctypes.c_int * len(calls))(*[int(p) for p in precs])
    hip.N_CALLS += 1
    rc = hip.lib().nr_token_weights_fwd_group(arr, pa, len(calls), hip.stream_ptr())
    if rc == 0:
        return outs
    hip.N_CALLS -= 1
    if rc != hip.NR_EUNSUPPORTED:
        hip._check("nr_token_weights_fwd_group", rc)
    return None


def local_level(prep_t, prep_v, w_t, w_v, A, Nt, Bv, Nv, prec=hip.PREC_BF16, out_mode=hip.OUT_FULL, want_arg=False):
    """Fused token-token similarity (nr_local_level_fwd).  Returns (out, aux); aux = None or
    (arg_v, arg_t, pmax, qmax) kept for the backward pass."""
    dev = prep_t.hi.device
    if prep_t.n_tok != A * Nt or prep_v.n_tok != Bv * Nv:
        raise ValueError("prepared token counts do not match A*Nt / Bv*Nv")
    if out_mode == hip.OUT_FULL:
        out = torch.empty((A, Bv), dtype=torch.float32, device=dev)
    else:
        nr, nc = hip.local_level_tiles(A, Nt, Bv, Nv, prec)
        out = torch.empty((nc, A) if out_mode == hip.OUT_ROWSUM else (nr, Bv), dtype=torch.float32, device=dev)
    arg_v = arg_t = pmax = qmax = None
    if want_arg:
        arg_v = torch.empty((A, Bv, Nt), dtype=torch.uint8, device=dev)
        arg_t = torch.empty((A, Bv, Nv), dtype=torch.uint8, device=dev)
        pmax = torch.empty((A, Bv, Nt), dtype=torch.float32, device=dev)
        qmax = torch.empty((A, Bv, Nv), dtype=torch.float32, device=dev)
    (t_a, t_b), (v_a, v_b) = _planes(prep_t, prec), _planes(prep_v, prec)
    hip.call("nr_local_level_fwd", hip.ptr(t_a), hip.ptr(t_b, allow_none=True), hip.ptr(v_a),
             hip.ptr(v_b, allow_none=True), hip.ptr(w_t, torch.float32), hip.ptr(w_v, torch.float32),
             A, Nt, Bv, Nv, prep_t.d, prec, out_mode, hip.ptr(out), hip.ptr(arg_v, allow_none=True),
             hip.ptr(arg_t, allow_none=True), hip.ptr(pmax, allow_none=True), hip.ptr(qmax, allow_none=True),
             hip.stream_ptr())
    return out, ((arg_v, arg_t, pmax, qmax) if want_arg else None)


def local_level_cand(prep_q, prep_g, w_q, w_g, n_q, Nq, n_g, Ng, cand, prec=hip.PREC_BF16X3):
    """out [n_q, C] fp32: the local_level score of query i and gallery item cand[i, c] (nr_local_level_cand); cand [n_q, C]
    int32, 1 <= C <= 128.  Entries outside [0, n_g), the padding -1 included, give -inf."""
    if prep_q.n_tok != n_q * Nq or prep_g.n_tok != n_g * Ng:
        raise ValueError("prepared token counts do not match n_q*Nq / n_g*Ng")
    if prep_q.d != prep_g.d:
        raise ValueError("queries and gallery must have the same feature width")
    if cand.dim() != 2 or cand.shape[0] != n_q:
        raise ValueError(f"cand must be [n_q, C] = [{n_q}, C], got {tuple(cand.shape)}")
    C = int(cand.shape[1])
    out = torch.empty((n_q, C), dtype=torch.float32, device=prep_q.hi.device)
    hip.call("nr_local_level_cand", hip.ptr(prep_q.hi), hip.ptr(prep_q.lo, allow_none=True), hip.ptr(prep_g.hi),
             hip.ptr(prep_g.lo, allow_none=True), hip.ptr(w_q, torch.float32), hip.ptr(w_g, torch.float32),
             int(n_q), int(Nq), int(n_g), int(Ng), prep_q.d, int(prec), hip.ptr(cand, torch.int32), C, hip.ptr(out),
             hip.stream_ptr())
    return out


def local_level_group(problems):
    """Several loss-only products of one step: [(prep_t, prep_v, w_t, w_v, A, Nt, Bv, Nv, prec, out_mode), ...] -> list of
    outputs as local_level(...)[0] would return them.  One grid for all of them (nr_local_level_group) when every product
    can join a group; one launch each otherwise."""
    if not problems:
        return []
    groupable = 1 < len(problems) <= hip.LOCAL_LEVEL_GROUP_MAX and all(
        hip.local_level_group_kind(A, Nt, Bv, Nv, pt.d, prec) >= 0 for (pt, pv, wt, wv, A, Nt, Bv, Nv, prec, mode) in problems)
    if not groupable:
        return [local_level(*q)[0] for q in problems]
    arr = (hip.LocalLevelProblem * len(problems))()
    outs = []
    for i, (pt, pv, wt, wv, A, Nt, Bv, Nv, prec, mode) in enumerate(problems):
        dev = pt.hi.device
        if pt.n_tok != A * Nt or pv.n_tok != Bv * Nv:
            raise ValueError("prepared token counts do not match A*Nt / Bv*Nv")
        if mode == hip.OUT_FULL:
            out = torch.empty((A, Bv), dtype=torch.float32, device=dev)
        else:
            nr, nc = hip.local_level_tiles(A, Nt, Bv, Nv, prec)
            out = torch.empty((nc, A) if mode == hip.OUT_ROWSUM else (nr, Bv), dtype=torch.float32, device=dev)
        outs.append(out)
        q = arr[i]
        q.t_hi, q.v_hi = hip.ptr(pt.hi), hip.ptr(pv.hi)
        q.t_lo, q.v_lo = hip.ptr(pt.lo, allow_none=True), hip.ptr(pv.lo, allow_none=True)
        q.w_t, q.w_v, q.out = hip.ptr(wt, torch.float32), hip.ptr(wv, torch.float32), hip.ptr(out)
        q.A, q.Nt, q.Bv, q.Nv, q.d, q.prec, q.out_mode = A, Nt, Bv, Nv, pt.d, int(prec), int(mode)
    hip.call("nr_local_level_group", len(problems), arr, hip.stream_ptr())
    return outs


def reduce_parts(parts, scale):
    out = torch.empty((parts.shape[1],), dtype=torch.float32, device=parts.device)
    hip.call("nr_reduce_parts", hip.ptr(parts, torch.float32), parts.shape[0], parts.shape[1], float(scale), hip.ptr(out),
             hip.stream_ptr())
    return out


def colsum_pair(a, scale_a, b, scale_b):
    """(scale_a * column sums of a, scale_b * column sums of b) in one launch (nr_colsum_group); fixed summation order."""
    from .cluster_backward_hip import _colsum_group
    oa = torch.empty((a.shape[1],), dtype=torch.float32, device=a.device)
    ob = torch.empty((b.shape[1],), dtype=torch.float32, device=b.device)
    _colsum_group([(a, oa, a.shape[0], a.shape[1], scale_a), (b, ob, b.shape[0], b.shape[1], scale_b)])
    return oa, ob


def gemm_nt_f32(a, b):
    a, b = _f32(a).contiguous(), _f32(b).contiguous()
    M, K = a.shape
    N = b.shape[0]
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    hip.call("nr_gemm_nt_f32", hip.ptr(a), hip.ptr(b), M, N, K, hip.ptr(c), hip.stream_ptr())
    return c


def centrality_weights(g, colsum, n_tok, scale, want_aux=False):
    g = _f32(g).contiguous()
    B, d = g.shape
    w = torch.empty((B,), dtype=torch.float32, device=g.device)
    gnorm = torch.empty((B,), dtype=torch.float32, device=g.device) if want_aux else None
    mean = torch.empty((d,), dtype=torch.float32, device=g.device) if want_aux else None
    hip.call("nr_centrality_weights", hip.ptr(g), B, d, hip.ptr(colsum, torch.float32), colsum.shape[0], n_tok,
             float(scale), hip.ptr(w), hip.ptr(gnorm, allow_none=True), hip.ptr(mean, allow_none=True), hip.stream_ptr())
    return w, gnorm, mean


def centrality_weights_pair(gt, gv, mean_t, mean_v, scale, want_aux=False):
    """(w_text [B], w_video [B], aux) from finished token means (nr_centrality_weights_pair).
    gt [B,d] or [B,Gt,d], gv likewise: with several global tokens per sample the weight is the mean over them
    (config.centrality_multi_token = "mean").  aux = None or (gnorm_t, gnorm_v, wtok_t, wtok_v), per global token."""
    if gt.dim() == 2:
        gt, gv = gt[:, None, :], gv[:, None, :]
    B, n_gt, d = gt.shape
    n_gv = gv.shape[1]
    dev = gt.device
    w_t = torch.empty((B,), dtype=torch.float32, device=dev)
    w_v = torch.empty((B,), dtype=torch.float32, device=dev)
    aux = None
    if want_aux:
        aux = tuple(torch.empty((B * n,), dtype=torch.float32, device=dev) for n in (n_gt, n_gv, n_gt, n_gv))
    a = aux or (None,) * 4
    hip.call("nr_centrality_weights_pair", hip.ptr(gt, torch.float32), hip.ptr(gv, torch.float32), B, n_gt, n_gv, d,
             hip.ptr(mean_t, torch.float32), hip.ptr(mean_v, torch.float32), float(scale), hip.ptr(w_t), hip.ptr(w_v),
             hip.ptr(a[0], allow_none=True), hip.ptr(a[1], allow_none=True), hip.ptr(a[2], allow_none=True),
             hip.ptr(a[3], allow_none=True), hip.stream_ptr())
    return w_t, w_v, aux


def dpc_knn_assign(x, cluster_num, k, mask=None, noise=None):
    """Cluster id [B,N] (int64) of every token by DPC-KNN (nr_dpc_knn_assign)."""
    x = _f32(x.detach()).contiguous()
    B, N, C = x.shape
    if noise is None:
        noise = torch.rand((B, N), device=x.device, dtype=torch.float32)
    noise = _f32(noise).contiguous()
    m = _f32(mask).contiguous() if mask is not None else None
    assign = torch.empty((B, N), dtype=torch.int64, device=x.device)
    ws = torch.empty((int(hip.lib().nr_dpc_workspace_bytes(B, N)),), dtype=torch.uint8, device=x.device)
    hip.call("nr_dpc_knn_assign", hip.ptr(x), hip.ptr(m, allow_none=True), hip.ptr(noise), B, N, C, int(k), int(cluster_num),
             hip.ptr(assign), hip.ptr(ws), hip.stream_ptr())
    return assign


def sinkhorn_targets(G, beta, iters=50):
    G = _f32(G).contiguous()
    B = G.shape[0]
    tr = torch.empty_like(G)
    tc = torch.empty_like(G)
    ws = torch.empty((hip.sinkhorn_workspace_bytes(B),), dtype=torch.uint8, device=G.device)
    hip.call("nr_sinkhorn_targets", hip.ptr(G), B, float(beta), int(iters), hip.ptr(tr), hip.ptr(tc), hip.ptr(ws),
             hip.stream_ptr())
    return tr, tc


def sinkhorn_uniform_rows(G, beta, T, rowloss, iters=50):
    """Sinkhorn solve writing the uniform-CE row terms straight into rowloss[:, 1, :] (nr_sinkhorn_uniform_rows);
    the targets themselves are not materialised.  False if the shape is not covered (B > 128 or B % 4)."""
    G = _f32(G).contiguous()
    B = G.shape[0]
    if B > 128 or B % 4:
        return False
    ws = torch.empty((hip.sinkhorn_workspace_bytes(B),), dtype=torch.uint8, device=G.device)
    base = rowloss.view(-1)[B:]                    # rowloss [2,4,B]: term 1 of direction d starts at (4 d + 1) B
    hip.call("nr_sinkhorn_uniform_rows", hip.ptr(G), B, float(beta), int(iters), float(T), hip.ptr(base, torch.float32), 4 * B,
             None, None, hip.ptr(ws), hip.stream_ptr())
    return True


def split_tail_counter(dev, slot=0):
    """The zero-initialised device word shared by the two self-finalizing launches of the split tail (one per
    device: the launch that finishes last resets it, and steps on one device are ordered; steps whose tails may overlap --
    consecutive steps of a pipelined graph, modeling.StepPipeline -- take different `slot`s)."""
    key = ("split_tail", dev, int(slot))
    c = _COUNTERS.get(key)
    if c is None:
        c = _COUNTERS[key] = torch.zeros((1,), dtype=torch.int32, device=dev)
    return c


def forget_split_tail_counter(dev, slot=0):
    """Drops the device's shared finalize word (the next split_tail_counter call allocates a zeroed one)."""
    _COUNTERS.pop(("split_tail", dev, int(slot)), None)


def sinkhorn_uniform_rows_final(G, beta, T, rowloss, counter, wu, wn, wkl, losses, iters=50):
    """nr_sinkhorn_uniform_rows_final: Sinkhorn + uniform-CE row terms into rowloss[:, 1, :], taking part in the shared
    finalize (see row_losses_no_uniform_final)."""
    G = _f32(G).contiguous()
    B = G.shape[0]
    ws = torch.empty((hip.sinkhorn_workspace_bytes(B),), dtype=torch.uint8, device=G.device)
    hip.call("nr_sinkhorn_uniform_rows_final", hip.ptr(G), B, float(beta), int(iters), float(T), hip.ptr(rowloss, torch.float32),
             hip.ptr(counter, torch.int32), float(wu), float(wn), float(wkl), hip.ptr(losses, torch.float32), hip.ptr(ws),
             hip.stream_ptr())


def row_losses_no_uniform_final(S, G, c0_parts, c1_parts, c_scale, wc_text, wc_video, logit_scale, K, T, rowloss, counter,
                                wu, wn, wkl, losses):
    """nr_row_losses_fwd_no_uniform_final: the other row terms from the bank products' partial sums; the workgroup (of
    either launch) that finishes last writes the five losses."""
    B = S.shape[0]
    hip.call("nr_row_losses_fwd_no_uniform_final", hip.ptr(S, torch.float32), hip.ptr(G, torch.float32),
             hip.ptr(c0_parts, torch.float32), c0_parts.shape[0], hip.ptr(c1_parts, torch.float32), c1_parts.shape[0],
             float(c_scale), hip.ptr(wc_text, torch.float32), hip.ptr(wc_video, torch.float32),
             hip.ptr(logit_scale, torch.float32), B, int(K), float(T), hip.ptr(rowloss, torch.float32),
             hip.ptr(counter, torch.int32), float(wu), float(wn), float(wkl), hip.ptr(losses, torch.float32), hip.stream_ptr())


def row_losses_no_uniform_final_cw(S, G, c0_parts, c1_parts, c_scale, g_text, g_video, mean_text, mean_video, centrality_scale,
                                   logit_scale, K, T, rowloss, counter, wu, wn, wkl, losses):
    """nr_row_losses_fwd_no_uniform_final_cw: row_losses_no_uniform_final with the centrality weights computed by the row's own
    wave (one global token per sample: g_text / g_video [B, d], mean_text / mean_video [d])."""
    B, d = S.shape[0], g_text.shape[-1]
    hip.call("nr_row_losses_fwd_no_uniform_final_cw", hip.ptr(S, torch.float32), hip.ptr(G, torch.float32),
             hip.ptr(c0_parts, torch.float32), c0_parts.shape[0], hip.ptr(c1_parts, torch.float32), c1_parts.shape[0],
             float(c_scale), hip.ptr(g_text, torch.float32), hip.ptr(g_video, torch.float32), hip.ptr(mean_text, torch.float32),
             hip.ptr(mean_video, torch.float32), int(d), float(centrality_scale), hip.ptr(logit_scale, torch.float32), B, int(K),
             float(T), hip.ptr(rowloss, torch.float32), hip.ptr(counter, torch.int32), float(wu), float(wn), float(wkl),
             hip.ptr(losses, torch.float32), hip.stream_ptr())


def row_losses_no_uniform(S, G, bank_c0, bank_c1, wc_text, wc_video, logit_scale, K, T, rowloss):
    """Centrality / neighbour / KL row terms into rowloss[:, (0, 2, 3), :] (nr_row_losses_fwd_no_uniform)."""
    B = S.shape[0]
    hip.call("nr_row_losses_fwd_no_uniform", hip.ptr(S, torch.float32), hip.ptr(G, torch.float32), hip.ptr(bank_c0, torch.float32),
             hip.ptr(bank_c1, torch.float32), hip.ptr(wc_text, torch.float32), hip.ptr(wc_video, torch.float32),
             hip.ptr(logit_scale, torch.float32), B, int(K), float(T), hip.ptr(rowloss, torch.float32), hip.stream_ptr())


def row_losses(S, G, tgt_rows, tgt_cols, bank_c0, bank_c1, wc_text, wc_video, logit_scale, K, T):
    B = S.shape[0]
    rowloss = torch.empty((2, 4, B), dtype=torch.float32, device=S.device)
    hip.call("nr_row_losses_fwd", hip.ptr(S, torch.float32), hip.ptr(G, torch.float32), hip.ptr(tgt_rows), hip.ptr(tgt_cols),
             hip.ptr(bank_c0, torch.float32), hip.ptr(bank_c1, torch.float32), hip.ptr(wc_text, torch.float32),
             hip.ptr(wc_video, torch.float32), hip.ptr(logit_scale, torch.float32), B, int(K), float(T),
             hip.ptr(rowloss), hip.stream_ptr())
    return rowloss


def row_losses_slab(S_rows, S_cols, row0, G, tgt_rows, tgt_cols, bank_c0, bank_c1, wc_text, wc_video, logit_scale, K, T):
    """Row terms [2,4,B] of the rows [row0, row0 + n) only (zero elsewhere) from the two slabs of S a rank owns."""
    n, B = S_rows.shape
    rowloss = torch.zeros((2, 4, B), dtype=torch.float32, device=S_rows.device)
    hip.call("nr_row_losses_fwd_slab", hip.ptr(S_rows, torch.float32), hip.ptr(S_cols, torch.float32), int(row0), int(n),
             hip.ptr(G, torch.float32), hip.ptr(tgt_rows), hip.ptr(tgt_cols), hip.ptr(bank_c0, torch.float32),
             hip.ptr(bank_c1, torch.float32), hip.ptr(wc_text, torch.float32), hip.ptr(wc_video, torch.float32),
             hip.ptr(logit_scale, torch.float32), B, int(K), float(T), hip.ptr(rowloss), hip.stream_ptr())
    return rowloss


def row_losses_bwd_slab(S_rows, S_cols, row0, G, tgt_rows, tgt_cols, bank_c0, bank_c1, wc_text, wc_video, logit_scale, K, T, g_rowloss):
    """Backward of row_losses_slab (nr_row_losses_bwd_slab) -> dS_dir, dG_dir, d_c_rows [2,n,B], d_wc, d_ls_rows [2,n]."""
    n, B = S_rows.shape
    dev = S_rows.device
    dS = torch.empty((2, n, B), dtype=torch.float32, device=dev)
    dG = torch.empty((2, n, B), dtype=torch.float32, device=dev)
    dC = torch.empty((2, n, B), dtype=torch.float32, device=dev)
    dwc = torch.empty((2, n), dtype=torch.float32, device=dev)
    dls = torch.empty((2, n), dtype=torch.float32, device=dev)
    hip.call("nr_row_losses_bwd_slab", hip.ptr(S_rows, torch.float32), hip.ptr(S_cols, torch.float32), int(row0), int(n),
             hip.ptr(G, torch.float32), hip.ptr(tgt_rows), hip.ptr(tgt_cols), hip.ptr(bank_c0, torch.float32),
             hip.ptr(bank_c1, torch.float32), hip.ptr(wc_text, torch.float32), hip.ptr(wc_video, torch.float32),
             hip.ptr(logit_scale, torch.float32), B, int(K), float(T), hip.ptr(g_rowloss, torch.float32), hip.ptr(dS), hip.ptr(dG),
             hip.ptr(dC), hip.ptr(dwc), hip.ptr(dls), hip.stream_ptr())
    return dS, dG, dC, dwc, dls


def row_losses_final(S, G, tgt_rows, tgt_cols, bank_c0, bank_c1, wc_text, wc_video, logit_scale, K, T, wu, wn, wkl):
    """Row terms [2,4,B] AND the five losses from one launch (nr_row_losses_fwd_final)."""
    B = S.shape[0]
    dev = S.device
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)     # one counter per stream: launches on one stream are ordered
    counter = _COUNTERS.get(key)
    if counter is None:
        counter = _COUNTERS[key] = torch.zeros((1,), dtype=torch.int32, device=dev)
    rowloss = torch.empty((2, 4, B), dtype=torch.float32, device=dev)
    losses = torch.empty((5,), dtype=torch.float32, device=dev)
    hip.call("nr_row_losses_fwd_final", hip.ptr(S, torch.float32), hip.ptr(G, torch.float32), hip.ptr(tgt_rows), hip.ptr(tgt_cols),
             hip.ptr(bank_c0, torch.float32), hip.ptr(bank_c1, torch.float32), hip.ptr(wc_text, torch.float32),
             hip.ptr(wc_video, torch.float32), hip.ptr(logit_scale, torch.float32), B, int(K), float(T),
             hip.ptr(rowloss), hip.ptr(counter), float(wu), float(wn), float(wkl), hip.ptr(losses), hip.stream_ptr())
    return rowloss, losses


def loss_finalize(rowloss, wu, wn, wkl):
    B = rowloss.shape[-1]
    losses = torch.empty((5,), dtype=torch.float32, device=rowloss.device)
    hip.call("nr_loss_finalize", hip.ptr(rowloss), B, float(wu), float(wn), float(wkl), hip.ptr(losses), hip.stream_ptr())
    return losses


def row_losses_bwd(S, G, tgt_rows, tgt_cols, bank_c0, bank_c1, wc_text, wc_video, logit_scale, K, T, g_rowloss):
    """-> dS_dir [2,B,B], dG_dir [2,B,B], d_c_rows [2,B,B], d_wc [2,B], d_ls_rows [2,B]  (nr_row_losses_bwd)."""
    B = S.shape[0]
    dev = S.device
    dS = torch.empty((2, B, B), dtype=torch.float32, device=dev)
    dG = torch.empty((2, B, B), dtype=torch.float32, device=dev)
    dC = torch.empty((2, B, B), dtype=torch.float32, device=dev)
    dwc = torch.empty((2, B), dtype=torch.float32, device=dev)
    dls = torch.empty((2, B), dtype=torch.float32, device=dev)
    hip.call("nr_row_losses_bwd", hip.ptr(S, torch.float32), hip.ptr(G, torch.float32), hip.ptr(tgt_rows), hip.ptr(tgt_cols),
             hip.ptr(bank_c0, torch.float32), hip.ptr(bank_c1, torch.float32), hip.ptr(wc_text, torch.float32),
             hip.ptr(wc_video, torch.float32), hip.ptr(logit_scale, torch.float32), B, int(K), float(T),
             hip.ptr(g_rowloss, torch.float32), hip.ptr(dS), hip.ptr(dG), hip.ptr(dC), hip.ptr(dwc), hip.ptr(dls),
             hip.stream_ptr())
    return dS, dG, dC, dwc, dls


def rowloss_coef(gs, hp, B):
    """g_rowloss [2,4,B] from the gradients of the five losses (tensors or None) in one launch (nr_rowloss_coef)."""
    dev = next(g for g in gs if g is not None).device
    gs = [None if g is None else _f32(g).contiguous() for g in gs]
    coef = torch.empty((2, 4, B), dtype=torch.float32, device=dev)
    hip.call("nr_rowloss_coef", *[hip.ptr(g, allow_none=True) for g in gs], float(hp["uniform_weight"]),
             float(hp["neighbor_weight"]), float(hp["kl_weight"]), int(B), hip.ptr(coef), hip.stream_ptr())
    return coef


def rowloss_bwd_finish(dS_dir, dG_dir, dC_rows, dls_rows):
    """-> dS [B,B], dG [B,B], d_c0 [B], d_c1 [B], d_ls [] in one launch (nr_rowloss_bwd_finish)."""
    B = dS_dir.shape[1]
    f32 = dict(dtype=torch.float32, device=dS_dir.device)
    dS, dG = torch.empty((B, B), **f32), torch.empty((B, B), **f32)
    dc = torch.empty((2, B), **f32)
    d_ls = torch.empty((1,), **f32)
    hip.call("nr_rowloss_bwd_finish", hip.ptr(dS_dir, torch.float32), hip.ptr(dG_dir, torch.float32), hip.ptr(dC_rows, torch.float32),
             hip.ptr(dls_rows, torch.float32), B, hip.ptr(dS), hip.ptr(dG), hip.ptr(dc[0]), hip.ptr(dc[1]), hip.ptr(d_ls),
             hip.stream_ptr())
    return dS, dG, dc[0], dc[1], d_ls[0]


def centrality_weights_bwd_pair(g_t, gnorm_t, mean_t, w_t, dw_t, g_v, gnorm_v, mean_v, w_v, dw_v, scale):
    """centrality_weights_bwd for both modalities in one launch -> dg_t, dmean_t, dg_v, dmean_v."""
    B, d = g_t.shape
    if g_v.shape != g_t.shape:
        raise ValueError("text and video global tokens of one batch have the same shape")
    dg_t, dg_v = torch.empty_like(g_t), torch.empty_like(g_v)
    dmean = torch.empty((2, d), dtype=torch.float32, device=g_t.device)
    hip.call("nr_centrality_weights_bwd_pair", hip.ptr(g_t, torch.float32), hip.ptr(gnorm_t), hip.ptr(mean_t), hip.ptr(w_t),
             hip.ptr(dw_t.contiguous(), torch.float32), hip.ptr(g_v, torch.float32), hip.ptr(gnorm_v), hip.ptr(mean_v), hip.ptr(w_v),
             hip.ptr(dw_v.contiguous(), torch.float32), B, d, float(scale), hip.ptr(dg_t), hip.ptr(dmean[0]), hip.ptr(dg_v),
             hip.ptr(dmean[1]), hip.stream_ptr())
    return dg_t, dmean[0], dg_v, dmean[1]


def global_logits_bwd(dG, gt2, gv2, add_t, add_v):
    """d_gt = dG gv + add_t, d_gv = dG^T gt + add_v in one launch (nr_global_logits_bwd)."""
    B, d = gt2.shape
    d_gt, d_gv = torch.empty_like(gt2), torch.empty_like(gv2)
    hip.call("nr_global_logits_bwd", hip.ptr(dG, torch.float32), hip.ptr(gt2, torch.float32), hip.ptr(gv2, torch.float32),
             hip.ptr(add_t, torch.float32), hip.ptr(add_v, torch.float32), B, d, hip.ptr(d_gt), hip.ptr(d_gv), hip.stream_ptr())
    return d_gt, d_gv


def add_transposed(a, b):
    """a + b.T for square fp32 matrices."""
    B = a.shape[0]
    out = torch.empty((B, B), dtype=torch.float32, device=a.device)
    hip.call("nr_add_transposed", hip.ptr(a, torch.float32), hip.ptr(b, torch.float32), B, hip.ptr(out), hip.stream_ptr())
    return out


def colsum(a):
    rows, cols = a.shape
    out = torch.empty((cols,), dtype=torch.float32, device=a.device)
    hip.call("nr_colsum", hip.ptr(a, torch.float32), rows, cols, hip.ptr(out), hip.stream_ptr())
    return out


USE_MFMA_BACKWARD = True        # False: the scalar arg-max walk for d_x too (reference for the MFMA path in the tests)


def transpose_prepared(preps, use_lo=True):
    """Several Prepared token sets in the order nr_local_level_bwd_group reads its "other" operand (fragment-major, whole
    slices of 96 tokens) in ONE launch (nr_sim_bwd_operand_group) -> [(hi_f, lo_f or None, tokens covered), ...]."""
    out = []
    for k in range(0, len(preps), hip.SIM_BWD_GROUP_MAX):
        chunk = preps[k:k + hip.SIM_BWD_GROUP_MAX]
        arr = (hip.SimBwdOperand * len(chunk))()
        for a, p in zip(arr, chunk):
            n_tok, d = p.hi.view(-1, p.d).shape
            ldk = (n_tok + 95) // 96 * 96
            dev = p.hi.device
            hi_f = torch.empty((ldk * d,), dtype=torch.int16, device=dev)
            lo_f = torch.empty((ldk * d,), dtype=torch.int16, device=dev) if (use_lo and p.lo is not None) else None
            a.hi, a.lo = p.hi.data_ptr(), (p.lo.data_ptr() if p.lo is not None else None)
            a.out_hi, a.out_lo = hi_f.data_ptr(), (lo_f.data_ptr() if lo_f is not None else None)
            a.n_tok, a.d = int(n_tok), int(d)
            out.append((hi_f, lo_f, ldk))
        hip.call("nr_sim_bwd_operand_group", len(chunk), arr, hip.stream_ptr())
    return out


def local_level_bwd_group(items, use_lo=True):
    """d_x of up to four fused products in one launch + one summing launch (nr_local_level_bwd_group).  items: dicts with
        side, dS, ds_mode, ds_scale, other_T=(hi_t, lo_t, ldk) from transpose_prepared, w_self, w_other, aux, A, Nt, Bv, Nv,
        d_x [n_self_tokens, d] f32 (items with the same d_x are summed), accumulate (first item of a d_x: keep its content)."""
    if not 0 < len(items) <= hip.SIM_BWD_GROUP_MAX:
        raise ValueError("1..%d products per launch" % hip.SIM_BWD_GROUP_MAX)
    arr = (hip.SimBwdItem * len(items))()
    keep = []
    for a, it in zip(arr, items):
        hi_t, lo_t, ldk = it["other_T"]
        arg_v, arg_t = it["aux"][0], it["aux"][1]
        dS = _f32(it["dS"]).contiguous()
        w_s, w_o = _f32(it["w_self"]).contiguous(), _f32(it["w_other"]).contiguous()
        keep += [dS, w_s, w_o]
        a.dS, a.oT_hi, a.oT_lo = dS.data_ptr(), hi_t.data_ptr(), (lo_t.data_ptr() if (use_lo and lo_t is not None) else None)
        a.w_self, a.w_other, a.arg_v, a.arg_t = w_s.data_ptr(), w_o.data_ptr(), arg_v.data_ptr(), arg_t.data_ptr()
        a.d_x, a.ds_scale = it["d_x"].data_ptr(), float(it["ds_scale"])
        a.side, a.ds_mode, a.ldk = int(it["side"]), int(it["ds_mode"]), int(ldk)
        a.A, a.Nt, a.Bv, a.Nv, a.d = int(it["A"]), int(it["Nt"]), int(it["Bv"]), int(it["Nv"]), int(hi_t.numel() // ldk)
        a.accumulate = 1 if it.get("accumulate") else 0
    nbytes = int(hip.lib().nr_local_level_bwd_group_workspace_bytes(len(items), arr))
    if nbytes == 0:
        raise hip.NrHipError("nr_local_level_bwd_group: shape outside the matrix-core backward (nr_local_level_bwd_mfma_supported)")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=items[0]["d_x"].device)
    hip.call("nr_local_level_bwd_group", len(items), arr, hip.ptr(ws), nbytes, hip.stream_ptr())


def pool_weight_bwd_group(jobs):
    """d_w of several token-weight vectors in one launch (nr_pool_weight_bwd_group).  jobs: dicts with side, N, d_w [n_self*N]
    f32, accumulate, srcs = [(dS, ds_mode, ds_scale, pooled [A,Bv,N] f32, A, Bv), ...] (one or two products)."""
    if not 0 < len(jobs) <= hip.POOLW_GROUP_MAX:
        raise ValueError("1..%d jobs per launch" % hip.POOLW_GROUP_MAX)
    arr = (hip.PoolWJob * len(jobs))()
    keep = []
    for a, j in zip(arr, jobs):
        a.n_src, a.side, a.N, a.accumulate = len(j["srcs"]), int(j["side"]), int(j["N"]), 1 if j.get("accumulate") else 0
        a.d_w = j["d_w"].data_ptr()
        for k, (dS, mode, scale, pool, A, Bv) in enumerate(j["srcs"]):
            dS = _f32(dS).contiguous()
            keep.append(dS)
            a.src[k].dS, a.src[k].pool, a.src[k].ds_scale = dS.data_ptr(), pool.data_ptr(), float(scale)
            a.src[k].ds_mode, a.src[k].A, a.src[k].Bv = int(mode), int(A), int(Bv)
    hip.call("nr_pool_weight_bwd_group", len(jobs), arr, hip.stream_ptr())


class TokenSet(namedtuple("TokenSet", "prep w T", defaults=(None,))):
    """One operand of the similarity backward: its Prepared tokens, its softmax weights [n, N] (n samples of N tokens), and
    optionally T, its transposed form from transpose_prepared when the caller has made it already."""
    n = property(lambda self: self.w.shape[0])
    N = property(lambda self: self.w.shape[1])


# One fused product text x video with its upstream gradient dS (ds_mode 0: [A, Bv]; 1 / 2: a row / column mean's [A] / [Bv]
# vector, times ds_scale) and the forward's aux = (arg_v, arg_t, pmax, qmax).  A and Bv are the two sets' n.
SimProduct = namedtuple("SimProduct", "text video dS ds_mode ds_scale aux")
# One token set whose gradient is wanted, the products it is an operand of in summation order (at most two: PoolWJob has two
# sources), and whether d_x is wanted besides d_w (a memory-bank set: weights only).
SimTarget = namedtuple("SimTarget", "set products want_dx", defaults=(True,))


def sim_backward_launches(targets, group_max=hip.SIM_BWD_GROUP_MAX):
    """Host only, by identity (`is`) of the sets and products: the launches of a table of SimTargets ->
        d_x launches  [[(set, product, side), ...], ...]   the targets in order, each one's products in order, cut every group_max
        jobs          [(set, [(product, side), ...]), ...]  one weight sum per target
        transposes    [[set, ...], ...]                     the distinct "other" operands of the d_x items in first-use order
    side: 0 where the set is the product's text operand (its pooled maxima are aux[2]), 1 where the video operand (aux[3]).
    The mapping is fixed because it is part of the result: nr_local_level_bwd_group chooses its chunking, and with it the
    summation order of d_x, from the composition of a launch, and sums the products of one d_x in item order."""
    items, jobs, others = [], [], []
    for k, tg in enumerate(targets):
        if any(tg.set is u.set for u in targets[:k]):
            raise ValueError("a token set is the target of one entry")
        sides = [(p, 0 if p.text is tg.set else 1) for p in tg.products]
        if not (1 <= len(sides) <= 2 and all((p.text, p.video)[side] is tg.set and side == sides[0][1] for p, side in sides)):
            raise ValueError("a target is the same operand (text or video) of its one or two products")
        jobs.append((tg.set, sides))
        for p, side in sides if tg.want_dx else ():
            items.append((tg.set, p, side))
            other = p.video if side == 0 else p.text
            if not any(other is o for o in others):
                others.append(other)
    cut = lambda xs: [xs[k:k + group_max] for k in range(0, len(xs), group_max)]      # noqa: E731
    return cut(items), jobs, cut(others)


def _pool_src(p, side):
    """A product as a source of nr_pool_weight_bwd_group: the pooled maxima of the operand's side (pmax = aux[2] / qmax = aux[3])."""
    return p.dS, p.ds_mode, p.ds_scale, p.aux[2 + side], p.text.n, p.video.n


def sim_backward(targets, use_lo=True, out=None, accumulate=False, scalar_dw=False, fallback=True):
    """The token side of the similarity backward from ONE description of each product: (d_x [n N, d] or None, d_w [n N]) per
    SimTarget, written into the buffers that `out` gives (None: a new one).  The only place that decides between the matrix-core
    kernel (nr_local_level_bwd_group, launches as sim_backward_launches states them, one nr_pool_weight_bwd_group for every d_w)
    and, with USE_MFMA_BACKWARD off or token counts the kernel refuses, nr_local_level_bwd's entry-by-entry walk: target by
    target, product by product, a target's second product accumulating (fallback=False: NrHipError instead).
    accumulate: keep the buffers' content.  scalar_dw: d_w from the walk's own sum (the cross-check of the tests)."""
    launches, jobs, transposes = sim_backward_launches(targets)
    d = next(s.prep.d for tg in targets for p in tg.products for s in (p.text, p.video) if s.prep is not None)
    dev = targets[0].set.w.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
    out = [((d_x if d_x is not None else new(tg.set.n * tg.set.N, d)) if tg.want_dx else None,
            d_w if d_w is not None else new(tg.set.n * tg.set.N)) for tg, (d_x, d_w) in zip(targets, out or [(None, None)] * len(targets))]
    buf = {id(tg.set): o for tg, o in zip(targets, out)}
    P0 = targets[0].products[0]
    mfma = bool(launches) and USE_MFMA_BACKWARD and bool(hip.lib().nr_local_level_bwd_mfma_supported(P0.text.N, P0.video.N, d))
    if launches and not (mfma or fallback):
        raise hip.NrHipError("the matrix-core similarity backward is required here (USE_MFMA_BACKWARD off, or token counts "
                             "outside nr_local_level_bwd_mfma_supported)")
    if mfma:
        T = {}
        for chunk in transposes:
            todo = [s for s in chunk if s.T is None]
            T.update([(id(s), s.T) for s in chunk if s.T is not None])
            T.update(zip(map(id, todo), transpose_prepared([s.prep for s in todo], use_lo=use_lo)))
        first = {id(tg.set): tg.products[0] for tg in targets}
        for launch in launches:
            local_level_bwd_group([
                dict(side=side, dS=p.dS, ds_mode=p.ds_mode, ds_scale=p.ds_scale, other_T=T[id((p.video, p.text)[side])],
                     w_self=s.w, w_other=(p.video, p.text)[side].w, aux=p.aux, A=p.text.n, Nt=p.text.N, Bv=p.video.n, Nv=p.video.N,
                     d_x=buf[id(s)][0], accumulate=accumulate and p is first[id(s)]) for s, p, side in launch], use_lo=use_lo)
        if not scalar_dw:
            pool_weight_bwd_group([dict(side=sides[0][1], N=s.N, d_w=buf[id(s)][1], accumulate=accumulate,
                                        srcs=[_pool_src(p, side) for p, side in sides]) for s, sides in jobs])
    if not mfma or scalar_dw:
        for s, sides in jobs:
            d_x, d_w = (None if mfma else buf[id(s)][0]), buf[id(s)][1]
            for k, (p, side) in enumerate(sides):
                acc = accumulate or k > 0
                if d_x is not None or scalar_dw:
                    other = (p.video, p.text)[side]
                    ws = torch.empty((int(hip.lib().nr_local_level_bwd_workspace_bytes(side, p.text.n, p.text.N, p.video.n, p.video.N,
                                                                                       d)),), dtype=torch.uint8, device=dev)
                    hip.call("nr_local_level_bwd", side, hip.ptr(p.dS, torch.float32), int(p.ds_mode), float(p.ds_scale),
                             hip.ptr(other.prep.hi), hip.ptr(other.prep.lo if use_lo else None, allow_none=True),
                             hip.ptr(s.w, torch.float32), hip.ptr(other.w, torch.float32), *(hip.ptr(a) for a in p.aux),
                             p.text.n, p.text.N, p.video.n, p.video.N, d, hip.ptr(d_x, allow_none=True),
                             hip.ptr(d_w if scalar_dw else None, allow_none=True), 1 if acc else 0, hip.ptr(ws), hip.stream_ptr())
                if not scalar_dw:
                    pool_weight_bwd_group([dict(side=side, N=s.N, d_w=d_w, accumulate=acc, srcs=[_pool_src(p, side)])])
    return out


def local_level_bwd(side, dS, ds_mode, ds_scale, other, w_self, w_other, aux, A, Nt, Bv, Nv, d_x=None, d_w=None,
                    want_dx=True, accumulate=False, use_lo=True, other_T=None, scalar_dw=False):
    """Arg-max-routed gradient for one operand: sim_backward of one target with one product.  `other` is the Prepared token set
    of the opposite operand (other_T: its transposed form, where the caller made it already).
    Returns (d_x [n_self*N, d] or None, d_w [n_self*N])."""
    if accumulate and ((want_dx and d_x is None) or d_w is None):
        raise ValueError("accumulate=True needs existing d_x / d_w buffers")
    me = TokenSet(None, w_self.reshape((A, Nt) if side == 0 else (Bv, Nv)))
    ot = TokenSet(other, w_other.reshape((Bv, Nv) if side == 0 else (A, Nt)), other_T)
    P = SimProduct(*((me, ot) if side == 0 else (ot, me)), dS, ds_mode, ds_scale, aux)
    return sim_backward([SimTarget(me, [P], want_dx)], use_lo, [(d_x, d_w)], accumulate, scalar_dw)[0]


def normalize_bwd(x, norm, mask, d_xn, dmean):
    x = _f32(x).contiguous()
    d = x.shape[-1]
    n_tok = x.numel() // d
    dx = torch.empty_like(x)
    m = _f32(mask).contiguous() if mask is not None else None
    hip.call("nr_normalize_bwd", hip.ptr(x), hip.ptr(norm, torch.float32), hip.ptr(m, allow_none=True),
             hip.ptr(d_xn, allow_none=True), hip.ptr(dmean, allow_none=True), n_tok, d, hip.ptr(dx), hip.stream_ptr())
    return dx


def token_softmax_bwd(w, dw):
    n, N = w.shape
    out = torch.empty_like(w)
    hip.call("nr_token_softmax_bwd", hip.ptr(w, torch.float32), hip.ptr(dw.contiguous(), torch.float32), n, N, hip.ptr(out),
             hip.stream_ptr())
    return out


def centrality_weights_bwd(g, gnorm, mean, w, dw, scale):
    B, d = g.shape
    dg = torch.empty_like(g)
    dmean = torch.empty((d,), dtype=torch.float32, device=g.device)
    hip.call("nr_centrality_weights_bwd", hip.ptr(g, torch.float32), hip.ptr(gnorm), hip.ptr(mean), hip.ptr(w),
             hip.ptr(dw.contiguous(), torch.float32), B, d, float(scale), hip.ptr(dg), hip.ptr(dmean), hip.stream_ptr())
    return dg, dmean


def bank_push(bank, batch, scratch=None):
    """In-place FIFO push: bank <- cat(batch, bank)[:capacity]  (nr_bank_push)."""
    cap, n_new = bank.shape[0], batch.shape[0]
    row_bytes = bank[0].numel() * bank.element_size()
    if batch.dtype != bank.dtype or batch[0].numel() != bank[0].numel():
        raise ValueError("bank / batch row layout mismatch")
    if scratch is None and n_new < cap:
        scratch = torch.empty_like(bank)
    hip.call("nr_bank_push", hip.ptr(bank), hip.ptr(batch.contiguous()), cap, n_new, row_bytes,
             hip.ptr(scratch, allow_none=True), hip.stream_ptr())
    return bank


def mask_piece(mask):
    """(tensor, kind) of a mask for pack_shard: int64 / fp32 masks are converted to the record's u8 by the pack kernel itself
    (kind 1 / 2), u8 ones travel as they are; anything else is converted here."""
    m = mask.contiguous()
    if m.dtype == torch.int64:
        return m, 1
    if m.dtype == torch.float32:
        return m, 2
    return (m if m.dtype == torch.uint8 else m.to(torch.uint8)), 0


def pack_shard(tensors, packed, offsets, kinds=None):
    """nr_pack_shard(_convert): the (contiguous GPU) tensors' bytes at `offsets` inside the uint8 buffer `packed`; a piece of
    kind 1 / 2 (mask_piece) is converted to u8 on the way and takes one byte per ELEMENT."""
    n = len(tensors)
    for t in tensors:
        hip.ptr(t)
    kinds = list(kinds) if kinds is not None else [0] * n
    srcs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    nbytes = (ctypes.c_size_t * n)(*[t.numel() * (1 if k else t.element_size()) for t, k in zip(tensors, kinds)])
    offs = (ctypes.c_size_t * n)(*offsets)
    if any(kinds):
        hip.call("nr_pack_shard_convert", n, srcs, nbytes, offs, (ctypes.c_int * n)(*kinds), hip.ptr(packed, torch.uint8), hip.stream_ptr())
    else:
        hip.call("nr_pack_shard", n, srcs, nbytes, offs, hip.ptr(packed, torch.uint8), hip.stream_ptr())


def copy_group(dsts, srcs):
    """nr_copy_group: dsts[k] <- srcs[k] (contiguous GPU tensors of equal size and dtype, at most 12) in one launch."""
    n = len(dsts)
    for d_, s_ in zip(dsts, srcs):
        hip.ptr(d_)
        hip.ptr(s_)
        if d_.dtype != s_.dtype or d_.numel() != s_.numel():
            raise ValueError("copy_group: source and destination differ in size or dtype")
    hip.call("nr_copy_group", n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in dsts]),
             (ctypes.c_size_t * n)(*[t.numel() * t.element_size() for t in srcs]), hip.stream_ptr())


def unpack_gathered(gathered, world, record_bytes, nbytes, offsets, outs, u8_to_f32):
    """nr_unpack_gathered: [world, record_bytes] uint8 -> the rank-major output tensors `outs`."""
    n = len(outs)
    for t in outs:
        hip.ptr(t)
    hip.call("nr_unpack_gathered", n, hip.ptr(gathered, torch.uint8), int(world), int(record_bytes),
             (ctypes.c_size_t * n)(*nbytes), (ctypes.c_size_t * n)(*offsets), (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs]),
             (ctypes.c_int * n)(*[1 if c else 0 for c in u8_to_f32]), hip.stream_ptr())


def bank_absorb_gathered(recv, lay, bank, shadow, ring_head, capacity, rng_state):
    """nr_bank_absorb_gathered: the gathered batch in `recv` (dist.packed_gather_raw) goes straight into the memory bank's ring --
    fp32 rows, masks, ids -- and, prepared, into its bf16 shadow; the ring head moves back by the batch and the noise stream's
    counter advances.  bank: dict of the five mb_* tensors; shadow: (text Prepared, video Prepared) or None."""
    dev = recv.device
    key = ("absorb", dev)
    counter = _COUNTERS.get(key)
    if counter is None:                 # the launch's two-level ticket: nr_bank_absorb_counter_words() zeroed words, left zeroed
        counter = _COUNTERS[key] = torch.zeros((hip.lib().nr_bank_absorb_counter_words(),), dtype=torch.int32, device=dev)
    a = hip.BankAbsorbDesc()
    a.gathered = hip.ptr(recv, torch.uint8)
    a.record_bytes = lay["record"]
    a.off_text, a.off_video, a.off_index, a.off_text_mask, a.off_video_mask = lay["offs"]
    (Nt, d), (Nv, _) = lay["shapes"][0], lay["shapes"][1]
    a.world, a.per_rank, a.Nt, a.Nv, a.d, a.capacity = lay["W"], lay["b"], Nt, Nv, d, int(capacity)
    a.bank_text, a.bank_video = hip.ptr(bank["mb_feat_t"], torch.float32), hip.ptr(bank["mb_feat_v"], torch.float32)
    a.bank_text_mask, a.bank_video_mask = hip.ptr(bank["mb_mask_t"], torch.float32), hip.ptr(bank["mb_mask_v"], torch.float32)
    a.bank_index = hip.ptr(bank["mb_ind"], torch.int64)
    if shadow is not None:
        st, sv = shadow
        a.shadow_text_hi, a.shadow_text_lo, a.shadow_text_norm = hip.ptr(st.hi), hip.ptr(st.lo), hip.ptr(st.norm, torch.float32)
        a.shadow_video_hi, a.shadow_video_lo, a.shadow_video_norm = hip.ptr(sv.hi), hip.ptr(sv.lo), hip.ptr(sv.norm, torch.float32)
    a.ring_head = hip.ptr(ring_head, torch.int32)
    a.rng_state = hip.ptr(rng_state, torch.int64)
    a.counter = hip.ptr(counter, torch.int32)
    hip.call("nr_bank_absorb_gathered", a, hip.stream_ptr())


def step_prologue(mask0, mask1, logit_scale, rng_state, n_noise, ring=None):
    """nr_step_prologue: (mask0 fp32, mask1 fp32, exp(logit_scale) [1] or None, noise [n_noise] or None).
    int64 masks are converted by the kernel; fp32 masks pass through untouched.
    ring = (head int32[1] device tensor, advance, capacity): the bank's ring head is moved back by `advance`."""
    dev = (mask0 if mask0 is not None else rng_state).device
    f32 = dict(dtype=torch.float32, device=dev)

    def conv(m):
        if m is None or m.dtype == torch.float32:
            return None, m
        if m.dtype != torch.int64:
            return None, m.float()
        m = m.contiguous()
        return m, torch.empty(m.shape, **f32)
    i0, o0 = conv(mask0)
    i1, o1 = conv(mask1)
    ls_exp = ls = None
    if logit_scale is not None:
        ls = logit_scale.detach().float().reshape(1).contiguous()
        ls_exp = torch.empty((1,), **f32)
    noise = torch.empty((n_noise,), **f32) if n_noise > 0 else None
    if i0 is not None or i1 is not None or ls is not None or noise is not None or ring is not None:
        hip.call("nr_step_prologue", hip.ptr(i0, allow_none=True), i0.numel() if i0 is not None else 0,
                 hip.ptr(o0 if i0 is not None else None, allow_none=True),
                 hip.ptr(i1, allow_none=True), i1.numel() if i1 is not None else 0,
                 hip.ptr(o1 if i1 is not None else None, allow_none=True),
                 hip.ptr(ls, allow_none=True), hip.ptr(ls_exp, allow_none=True),
                 hip.ptr(rng_state if noise is not None else None, torch.int64, allow_none=True),
                 hip.ptr(noise, allow_none=True), int(n_noise),
                 hip.ptr(ring[0] if ring else None, torch.int32, allow_none=True), int(ring[1]) if ring else 0,
                 int(ring[2]) if ring else 0, hip.stream_ptr())
    return o0, o1, ls_exp, noise


def bank_ring_push(banks, batches, head_new, head_dev=None):
    """Ring-buffer push of several bank tensors in one launch (nr_bank_ring_push).  head_dev: int32 [1] device
    tensor holding the head (overrides head_new)."""
    n = len(banks)
    cap, n_new = banks[0].shape[0], batches[0].shape[0]
    bs = [b.contiguous() for b in batches]
    for bank, batch in zip(banks, bs):
        if bank.dtype != batch.dtype or bank[0].numel() != batch[0].numel() or bank.shape[0] != cap:
            raise ValueError("bank / batch layout mismatch")
    PA = ctypes.c_void_p * n
    pb = PA(*[b.data_ptr() for b in banks])
    pn = PA(*[b.data_ptr() for b in bs])
    rb = (ctypes.c_size_t * n)(*[b[0].numel() * b.element_size() for b in banks])
    for b in list(banks) + bs:
        hip.ptr(b)                      # device / contiguity check
    hip.call("nr_bank_ring_push", n, pb, pn, rb, cap, int(head_new), hip.ptr(head_dev, torch.int32, allow_none=True), n_new,
             hip.stream_ptr())


def diag_ranks(S):
    S = _f32(S).contiguous()
    N = S.shape[0]
    g = torch.empty((N,), dtype=torch.int32, device=S.device)
    e = torch.empty((N,), dtype=torch.int32, device=S.device)
    hip.call("nr_diag_ranks", hip.ptr(S), N, hip.ptr(g), hip.ptr(e), hip.stream_ptr())
    return g, e


def slab_ranks(S_slab, row0, diag):
    """(greater_rows, equal_rows [n], greater_cols, equal_cols [N]) of a row slab against the full diagonal (nr_slab_ranks)."""
    S_slab = _f32(S_slab).contiguous()
    n, N = S_slab.shape
    dev = S_slab.device
    gr = torch.empty((n,), dtype=torch.int32, device=dev)
    er = torch.empty((n,), dtype=torch.int32, device=dev)
    gc = torch.empty((N,), dtype=torch.int32, device=dev)
    ec = torch.empty((N,), dtype=torch.int32, device=dev)
    hip.call("nr_slab_ranks", hip.ptr(S_slab), n, N, int(row0), hip.ptr(diag, torch.float32), hip.ptr(gr), hip.ptr(er),
             hip.ptr(gc), hip.ptr(ec), hip.stream_ptr())
    return gr, er, gc, ec


def group_slab_ranks(S_slab, row0, group_end):
    """(greater_rows, equal_before_rows [n] int32, group_max [G,V] fp32) of a sentence-row slab (nr_group_slab_ranks);
    group_end [G] int32 on the device, its last entry >= row0 + n (the caller built it: not re-read here)."""
    S_slab = _f32(S_slab).contiguous()
    n, V = S_slab.shape
    G = group_end.shape[0]
    dev = S_slab.device
    gr = torch.empty((n,), dtype=torch.int32, device=dev)
    eb = torch.empty((n,), dtype=torch.int32, device=dev)
    gmax = torch.empty((G, V), dtype=torch.float32, device=dev)
    hip.call("nr_group_slab_ranks", hip.ptr(S_slab), n, V, int(row0), hip.ptr(group_end, torch.int32), G, hip.ptr(gr),
             hip.ptr(eb), hip.ptr(gmax), hip.stream_ptr())
    return gr, eb, gmax


def _check_k(k):
    k = int(k)
    if not 1 <= k <= hip.TOPK_MAX:
        raise ValueError(f"k must lie in [1, {hip.TOPK_MAX}], got {k}")
    return k


def slab_topk_rows(S_slab, k):
    """(idx [n,k] int32, val [n,k] fp32): the top-k list of every row of S_slab [n,N] (nr_slab_topk_rows): score descending,
    ties by lower column, NaN never selected, padded with -1 / -inf."""
    k = _check_k(k)
    S_slab = _f32(S_slab).contiguous()
    if S_slab.dim() != 2:
        raise ValueError("S_slab must be 2-D")
    n, N = S_slab.shape
    idx = torch.empty((n, k), dtype=torch.int32, device=S_slab.device)
    val = torch.empty((n, k), dtype=torch.float32, device=S_slab.device)
    hip.call("nr_slab_topk_rows", hip.ptr(S_slab), n, N, k, hip.ptr(idx), hip.ptr(val), hip.stream_ptr())
    return idx, val


def slab_topk_cols(S_slab, row0, k):
    """(idx [N,k] int32, val [N,k] fp32): every column's top-k list over this slab's rows only, indices row0 + i
    (nr_slab_topk_cols) -- the partial lists topk_merge combines."""
    k = _check_k(k)
    S_slab = _f32(S_slab).contiguous()
    if S_slab.dim() != 2:
        raise ValueError("S_slab must be 2-D")
    n, N = S_slab.shape
    idx = torch.empty((N, k), dtype=torch.int32, device=S_slab.device)
    val = torch.empty((N, k), dtype=torch.float32, device=S_slab.device)
    hip.call("nr_slab_topk_cols", hip.ptr(S_slab), n, N, int(row0), k, hip.ptr(idx), hip.ptr(val), hip.stream_ptr())
    return idx, val


def topk_merge(idx, val):
    """idx [W,n,k] int32, val [W,n,k] fp32 (W partial lists per item, each in the top-k order) -> the merged (idx, val)
    [n,k] (nr_topk_merge)."""
    if idx.dim() != 3 or idx.shape != val.shape:
        raise ValueError("idx and val must both be [n_lists, n_items, k]")
    W, n, k = idx.shape
    k = _check_k(k)
    idx, val = idx.contiguous(), val.contiguous()
    out_i = torch.empty((n, k), dtype=torch.int32, device=idx.device)
    out_v = torch.empty((n, k), dtype=torch.float32, device=idx.device)
    hip.call("nr_topk_merge", W, hip.ptr(idx, torch.int32), hip.ptr(val, torch.float32), n, k, hip.ptr(out_i), hip.ptr(out_v),
             hip.stream_ptr())
    return out_i, out_v


def topk_occurrences(idx, n_gallery, gt_begin, gt_end):
    """(occ, good) [n_gallery] int32 k-occurrence counts of the lists idx [n_q,k] int32 (nr_topk_occurrences); query q's
    ground truth is the gallery range [gt_begin[q], gt_end[q]) (int32 [n_q] on the device)."""
    if idx.dim() != 2:
        raise ValueError("idx must be [n_queries, k]")
    n_q, k = idx.shape
    k = _check_k(k)
    if gt_begin.shape != (n_q,) or gt_end.shape != (n_q,):
        raise ValueError("gt_begin / gt_end must have one entry per query")
    idx = idx.contiguous()
    occ = torch.empty((n_gallery,), dtype=torch.int32, device=idx.device)
    good = torch.empty((n_gallery,), dtype=torch.int32, device=idx.device)
    hip.call("nr_topk_occurrences", hip.ptr(idx, torch.int32), n_q, k, int(n_gallery), hip.ptr(gt_begin.contiguous(), torch.int32),
             hip.ptr(gt_end.contiguous(), torch.int32), hip.ptr(occ), hip.ptr(good), hip.stream_ptr())
    return occ, good


HUBNORM_MODES = {"is": hip.HUBNORM_IS, "dsl": hip.HUBNORM_DSL}


def _check_beta(beta):
    beta = float(beta)
    if not (beta > 0 and math.isfinite(beta)):
        raise ValueError(f"beta must be finite and > 0, got {beta}")
    return beta


def _slab_2d(S):
    S = _f32(S).contiguous()
    if S.dim() != 2:
        raise ValueError("S must be 2-D")
    return S


def hubnorm_row_lse(S, beta):
    """lse [n] fp32: log-sum-exp of every row of beta * S [n, L] over its non-NaN entries, -inf for a row with none
    (nr_hubnorm_row_lse)."""
    beta = _check_beta(beta)
    S = _slab_2d(S)
    n, L = S.shape
    lse = torch.empty((n,), dtype=torch.float32, device=S.device)
    if n:
        hip.call("nr_hubnorm_row_lse", hip.ptr(S), n, L, beta, hip.ptr(lse), hip.stream_ptr())
    return lse


def hubnorm_col_stats(S, beta):
    """stats [2, L] fp32 = (max, sum of exp(beta x - max)) of every column of beta * S [n, L] (nr_hubnorm_col_stats): the
    partial pairs a row slab contributes, merged over the slabs by hubnorm_combine."""
    beta = _check_beta(beta)
    S = _slab_2d(S)
    n, L = S.shape
    ws = torch.empty((int(hip.lib().nr_hubnorm_col_workspace(n, L)),), dtype=torch.uint8, device=S.device)
    stats = torch.empty((2, L), dtype=torch.float32, device=S.device)
    hip.call("nr_hubnorm_col_stats", hip.ptr(S), n, L, beta, hip.ptr(ws), hip.ptr(stats), hip.stream_ptr())
    return stats


def hubnorm_combine(parts, want_stats=False):
    """parts [P, 2, L] fp32 (max, sum) pairs -> lse [L], merged in index order (nr_hubnorm_combine); want_stats: (stats [2, L],
    lse)."""
    parts = _f32(parts).contiguous()
    if parts.dim() != 3 or parts.shape[1] != 2:
        raise ValueError("parts must be [P, 2, L]")
    P, _, L = parts.shape
    lse = torch.empty((L,), dtype=torch.float32, device=parts.device)
    stats = torch.empty((2, L), dtype=torch.float32, device=parts.device) if want_stats else None
    hip.call("nr_hubnorm_combine", P, hip.ptr(parts), L, hip.ptr(stats, allow_none=True), hip.ptr(lse), hip.stream_ptr())
    return (stats, lse) if want_stats else lse


def hubnorm_apply(S, beta, mode, col_norm=None, row_gate=None, row_norm=None, col_gate=None, want_t=True, want_v=True):
    """(T, V) [n, L] fp32 from one read of S [n, L] (nr_hubnorm_apply); mode "is" | "dsl".  T uses the column normaliser
    col_norm [L] on the rows where row_gate [n] (int32, None: every row) is non-zero and keeps S elsewhere; V uses the row
    normaliser row_norm [n] on the columns where col_gate [L] is non-zero.  An output not wanted is None."""
    beta = _check_beta(beta)
    if mode not in HUBNORM_MODES:
        raise ValueError(f"mode must be one of {sorted(HUBNORM_MODES)}, got {mode!r}")
    if not (want_t or want_v):
        raise ValueError("nothing to compute")
    S = _slab_2d(S)
    n, L = S.shape
    dev = S.device

    def vec(x, size, dtype, what):
        if x is None:
            return None
        x = x.to(device=dev, dtype=dtype).contiguous()
        if x.shape != (size,):
            raise ValueError(f"{what} must have shape ({size},), got {tuple(x.shape)}")
        return x

    col_norm, row_norm = vec(col_norm, L, torch.float32, "col_norm"), vec(row_norm, n, torch.float32, "row_norm")
    row_gate, col_gate = vec(row_gate, n, torch.int32, "row_gate"), vec(col_gate, L, torch.int32, "col_gate")
    if (want_t and col_norm is None) or (want_v and row_norm is None):
        raise ValueError("T needs col_norm, V needs row_norm")
    T = torch.empty_like(S) if want_t else None
    V = torch.empty_like(S) if want_v else None
    if n == 0 or L == 0:
        return T, V
    p = lambda x: hip.ptr(x, allow_none=True)                  # noqa: E731
    hip.call("nr_hubnorm_apply", hip.ptr(S), n, L, beta, HUBNORM_MODES[mode], p(col_norm), p(row_gate), p(T), p(row_norm),
             p(col_gate), p(V), hip.stream_ptr())
    return T, V


def _cand_lines(fine, cand, n_gallery, k, want_corr):
    """The front the candidate re-rank wrappers share: checks (fine, cand, n_gallery, k) and allocates the outputs every one of
    them has -> (fine, cand, n, C, n_gallery, k, idx [n, k] int32, val [n, k] fp32, corr [n, C] fp32 or None)."""
    if fine.dim() != 2 or cand.dim() != 2 or fine.shape != cand.shape:
        raise ValueError(f"fine and cand must both be [n, C], got {tuple(fine.shape)} and {tuple(cand.shape)}")
    n, C = cand.shape
    n_gallery, k = int(n_gallery), _check_k(k)
    if not 1 <= C <= hip.TOPK_MAX or k > C:
        raise ValueError(f"1 <= k <= C <= {hip.TOPK_MAX} expected, got k = {k}, C = {C}")
    if n_gallery < 1:
        raise ValueError("the gallery is empty")
    dev = fine.device
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    val = torch.empty((n, k), dtype=torch.float32, device=dev)
    corr = torch.empty((n, C), dtype=torch.float32, device=dev) if want_corr else None
    return _f32(fine).contiguous(), cand.contiguous(), n, C, n_gallery, k, idx, val, corr


def cand_norm_rerank(fine, cand, n_gallery, k, norm=None, active=None, beta=20.0, want_corr=True):
    """(idx [n, k] int32, val [n, k] fp32, corr [n, C] fp32 or None, gate [n] int32) of candidate lists cand [n, C] int32 (ascending
    gallery index, entries outside [0, n_gallery) absent) with fine scores fine [n, C], in one launch (nr_cand_norm_rerank).
    norm [n_gallery] fp32: the gallery's normalisers, active [n_gallery] int32: the activation set.  norm None: gate 0, corr =
    fine -- search.rerank; active None: every query takes corr = fl(fl(beta fine) - norm[cand]) (mode "is"); with active only
    the queries whose top-1 candidate is active (mode "qbnorm").  idx / val: the top k of corr, ties by lower position, -1 / -inf
    where the line has fewer than k present non-NaN slots.  1 <= k <= C <= 128."""
    fine, cand, n, C, n_gallery, k, idx, val, corr = _cand_lines(fine, cand, n_gallery, k, want_corr)
    if active is not None and norm is None:
        raise ValueError("an activation set needs the normalisers")
    beta = _check_beta(beta) if norm is not None else 0.0
    dev = fine.device
    for x, dtype, what in ((norm, torch.float32, "norm"), (active, torch.int32, "active")):
        if x is not None and (x.dtype != dtype or x.shape != (n_gallery,) or x.device != dev):
            raise ValueError(f"{what} must be a {dtype} vector of {n_gallery} entries on {dev}")
    gate = torch.empty((n,), dtype=torch.int32, device=dev)
    if n:
        p = lambda x: hip.ptr(None if x is None else x.contiguous(), allow_none=True)        # noqa: E731
        hip.call("nr_cand_norm_rerank", hip.ptr(fine), hip.ptr(cand, torch.int32), n, C, n_gallery, p(norm), p(active), beta, k,
                 hip.ptr(idx), hip.ptr(val), p(corr), hip.ptr(gate), hip.stream_ptr())
    return idx, val, corr, gate


def _ivf_index(list_items, list_offsets):
    """(n_items, n_lists) of an inverted-file index given as list_items [n_items] / list_offsets [n_lists + 1] int32."""
    for x, what in ((list_items, "list_items"), (list_offsets, "list_offsets")):
        if x.dim() != 1 or x.dtype != torch.int32:
            raise ValueError(f"{what} must be a torch.int32 vector, got {x.dtype} {tuple(x.shape)}")
    n_items, n_lists = int(list_items.shape[0]), int(list_offsets.shape[0]) - 1
    if not 1 <= n_lists <= n_items:
        raise ValueError(f"1 <= n_lists <= n_items expected, got {n_lists} lists of {n_items} items")
    return n_items, n_lists


def ivf_list_sums(x, list_items, list_offsets):
    """sums [L, d] fp32: the rows x[list_items[list_offsets[l] : list_offsets[l + 1]]] of every list added in list order, one
    sequential fp32 addition per component (nr_ivf_list_sums)."""
    n_items, n_lists = _ivf_index(list_items, list_offsets)
    if x.dim() != 2 or x.shape[0] != n_items:
        raise ValueError(f"x must be [n_items, d] = [{n_items}, d], got {tuple(x.shape)}")
    x = _f32(x).contiguous()
    d = int(x.shape[1])
    sums = torch.empty((n_lists, d), dtype=torch.float32, device=x.device)
    hip.call("nr_ivf_list_sums", hip.ptr(x), hip.ptr(list_items.contiguous(), torch.int32), hip.ptr(list_offsets.contiguous(), torch.int32),
             n_items, n_lists, d, hip.ptr(sums), hip.stream_ptr())
    return sums


def ivf_scan(q, rows, list_items, list_offsets, probes, stride, max_list_size, out=None):
    """(pool_score [n, stride] fp32, pool_item [n, stride] int32, pool_len [n] int32): the pools of the queries q [n, d] over the
    lists probes [n, P] int32 names in probe order (nr_ivf_scan).  rows [n_items, d] = the indexed vectors list
    by list.  Every score has the bits gemm_nt_f32 gives its (query, item) pair; slots from pool_len on are NOT written.  stride
    >= the sum of the P largest list sizes and max_list_size >= the largest come from the host's copy of the sizes: nothing here
    reads the device.  out: (pool_score, pool_item, pool_len) buffers to write into (at least n rows of `stride`).  The grouping
    of the (query, probe) pairs by list -- a stable sort and two prefix sums -- is device plumbing in torch."""
    n_items, n_lists = _ivf_index(list_items, list_offsets)
    if q.dim() != 2 or rows.dim() != 2 or rows.shape[0] != n_items or q.shape[1] != rows.shape[1]:
        raise ValueError(f"q must be [n, d] and rows [{n_items}, d], got {tuple(q.shape)} and {tuple(rows.shape)}")
    n, d = int(q.shape[0]), int(q.shape[1])
    if probes.dim() != 2 or probes.shape[0] != n or probes.dtype != torch.int32:
        raise ValueError(f"probes must be a torch.int32 [n, P] = [{n}, P] tensor, got {probes.dtype} {tuple(probes.shape)}")
    P, stride, max_list_size = int(probes.shape[1]), int(stride), int(max_list_size)
    if not 1 <= P <= min(n_lists, hip.IVF_MAX_PROBE):
        raise ValueError(f"the number of probes must lie in [1, min(n_lists, {hip.IVF_MAX_PROBE}) = {min(n_lists, hip.IVF_MAX_PROBE)}], got {P}")
    if d % 16 != 0:
        raise ValueError(f"d must be a multiple of 16, got {d}")
    if stride < 1 or not 0 <= max_list_size <= n_items:
        raise ValueError(f"stride >= 1 and 0 <= max_list_size <= n_items expected, got {stride} and {max_list_size}")
    dev = q.device
    if out is None:
        out = (torch.empty((n, stride), dtype=torch.float32, device=dev), torch.empty((n, stride), dtype=torch.int32, device=dev),
               torch.empty((n,), dtype=torch.int32, device=dev))
    score, item, length = out
    if tuple(score.shape) != (n, stride) or tuple(item.shape) != (n, stride) or tuple(length.shape) != (n,):
        raise ValueError(f"out must be ([n, stride], [n, stride], [n]) = ([{n}, {stride}], [{n}, {stride}], [{n}])")
    if n == 0:
        return score, item, length
    q, rows, probes = _f32(q).contiguous(), _f32(rows).contiguous(), probes.contiguous()
    bucket = torch.where((probes >= 0) & (probes < n_lists), probes, torch.full_like(probes, n_lists)).reshape(-1)
    ordered, order = torch.sort(bucket, stable=True)
    order = order.to(torch.int32)
    group = torch.searchsorted(ordered, torch.arange(n_lists + 2, dtype=torch.int32, device=dev), out_int32=True)
    tiles = torch.zeros((n_lists + 2,), dtype=torch.int32, device=dev)
    tiles[1:] = torch.cumsum((group[1:] - group[:-1] + 15) // 16, 0)
    hip.call("nr_ivf_scan", hip.ptr(q), n, hip.ptr(rows), hip.ptr(list_items.contiguous(), torch.int32),
             hip.ptr(list_offsets.contiguous(), torch.int32), n_items, n_lists, d, hip.ptr(probes, torch.int32), P,
             hip.ptr(order, torch.int32), hip.ptr(group, torch.int32), hip.ptr(tiles, torch.int32), max_list_size,
             hip.ptr(score, torch.float32), hip.ptr(item, torch.int32), hip.ptr(length, torch.int32), stride, hip.stream_ptr())
    return score, item, length


def ivf_select(pool_score, pool_item, pool_len, C, want_score=False):
    """cand [n, C] int32 (and, with want_score, their scores [n, C] fp32): the top C of the first pool_len[i] entries of every pool
    line by (score descending, gallery index ascending; NaN never taken), in ASCENDING GALLERY INDEX, padded with -1 / -inf
    (nr_ivf_select).  The items of a line must be distinct."""
    if pool_score.dim() != 2 or pool_score.shape != pool_item.shape or pool_item.dtype != torch.int32:
        raise ValueError(f"pool_score (fp32) and pool_item (int32) must both be [n, stride], got {tuple(pool_score.shape)} and "
                         f"{pool_item.dtype} {tuple(pool_item.shape)}")
    n, stride = (int(s) for s in pool_score.shape)
    if pool_len.dtype != torch.int32 or tuple(pool_len.shape) != (n,):
        raise ValueError(f"pool_len must be a torch.int32 vector of {n} entries, got {pool_len.dtype} {tuple(pool_len.shape)}")
    C = int(C)
    if not 1 <= C <= hip.TOPK_MAX:
        raise ValueError(f"C must lie in [1, {hip.TOPK_MAX}], got {C}")
    if stride < 1:
        raise ValueError("the pool lines are empty (stride < 1)")
    dev = pool_score.device
    cand = torch.empty((n, C), dtype=torch.int32, device=dev)
    score = torch.empty((n, C), dtype=torch.float32, device=dev) if want_score else None
    if n:
        hip.call("nr_ivf_select", hip.ptr(_f32(pool_score).contiguous()), hip.ptr(pool_item.contiguous(), torch.int32),
                 hip.ptr(pool_len.contiguous(), torch.int32), n, stride, C, hip.ptr(cand), hip.ptr(score, allow_none=True),
                 hip.stream_ptr())
    return (cand, score) if want_score else cand


def _flat_vec(x, size, what, dtype=torch.float32):
    """x, a vector operand of a slab kernel, taken as it is: refused (never converted) unless contiguous, of `dtype` and `size`."""
    if x.dtype != dtype or x.shape != (size,) or not x.is_contiguous():
        name = "fp32" if dtype == torch.float32 else dtype
        raise ValueError(f"{what} must be a contiguous {name} vector of {size} entries, got {x.dtype} {tuple(x.shape)}")
    return x


def sinknorm_workspace(n, L, device):
    """The column half-step's workspace for a slab [n, L]: uint8, nr_hubnorm_col_workspace(n, L) bytes."""
    return torch.empty((int(hip.lib().nr_hubnorm_col_workspace(int(n), int(L))),), dtype=torch.uint8, device=device)


def sinknorm_row(S, beta, v, log_mu, out=None):
    """u [n] = log_mu - LSE_j(fma(beta, S, v[j])) of every row of S [n, L], 0 for a row whose LSE is not finite
    (nr_sinknorm_row; until_module.py:249).  out: the u to overwrite."""
    beta = _check_beta(beta)
    S = _slab_2d(S)
    n, L = S.shape
    u = torch.empty((n,), dtype=torch.float32, device=S.device) if out is None else _flat_vec(out, n, "out")
    if n and L:
        hip.call("nr_sinknorm_row", hip.ptr(S), n, L, beta, hip.ptr(_flat_vec(v, L, "v")), hip.ptr(_flat_vec(log_mu, n, "log_mu")),
                 hip.ptr(u), hip.stream_ptr())
    else:
        u.zero_()
    return u


def sinknorm_col_stats(S, beta, u, workspace=None, want_stats=True):
    """The (max, sum) pairs of fma(beta, S, u[i]) down the columns of S [n, L] (nr_sinknorm_col_stats; until_module.py:250).
    want_stats: stats [2, L], this slab's pairs merged in block order (what a rank contributes to the cross-rank gather).
    Otherwise the blocks' pairs [ceil(n / 64), 2, L], a view of `workspace`, for sinknorm_finish_cols."""
    beta = _check_beta(beta)
    S = _slab_2d(S)
    n, L = S.shape
    ws = sinknorm_workspace(n, L, S.device) if workspace is None else workspace
    need = int(hip.lib().nr_hubnorm_col_workspace(n, L))
    if ws.dtype != torch.uint8 or ws.numel() < need:
        raise ValueError(f"workspace must be uint8 with at least {need} bytes")
    stats = torch.empty((2, L), dtype=torch.float32, device=S.device) if want_stats else None
    if L and (n or want_stats):
        hip.call("nr_sinknorm_col_stats", hip.ptr(S) if n else None, n, L, beta, hip.ptr(_flat_vec(u, n, "u")) if n else None,
                 hip.ptr(ws) if need else None, hip.ptr(stats, allow_none=True), hip.stream_ptr())
    return stats if want_stats else ws[:need].view(torch.float32).view((n + 63) // 64, 2, L)


def sinknorm_finish_cols(parts, log_nu, out=None):
    """v [L] = log_nu - lse of the pairs parts [P, 2, L] merged in index order, 0 where the lse is not finite
    (nr_sinknorm_finish_cols; until_module.py:250).  out: the v to overwrite."""
    if parts.dtype != torch.float32 or parts.dim() != 3 or parts.shape[1] != 2 or not parts.is_contiguous():
        raise ValueError("parts must be a contiguous fp32 [P, 2, L]")
    P, _, L = parts.shape
    v = torch.empty((L,), dtype=torch.float32, device=parts.device) if out is None else _flat_vec(out, L, "out")
    if L:
        hip.call("nr_sinknorm_finish_cols", P, hip.ptr(parts) if P else None, L, hip.ptr(_flat_vec(log_nu, L, "log_nu")), hip.ptr(v),
                 hip.stream_ptr())
    return v


def sinknorm_apply(S, beta, u, v):
    """T [n, L] = fl(fma(beta, S, u[i]) + v[j]), two roundings (nr_sinknorm_apply; until_module.py:253-257 in the log domain)."""
    beta = _check_beta(beta)
    S = _slab_2d(S)
    n, L = S.shape
    T = torch.empty_like(S)
    if n and L:
        hip.call("nr_sinknorm_apply", hip.ptr(S), n, L, beta, hip.ptr(_flat_vec(u, n, "u")), hip.ptr(_flat_vec(v, L, "v")), hip.ptr(T),
                 hip.stream_ptr())
    return T


def sinknorm_row_err(S, beta, u, v, log_mu):
    """err [n] = |exp(LSE_j(T[i, j]) - log_mu[i]) - 1|, T as sinknorm_apply gives it, 0 for a row whose LSE is not finite
    (nr_sinknorm_row_err)."""
    beta = _check_beta(beta)
    S = _slab_2d(S)
    n, L = S.shape
    err = torch.zeros((n,), dtype=torch.float32, device=S.device)
    if n and L:
        hip.call("nr_sinknorm_row_err", hip.ptr(S), n, L, beta, hip.ptr(_flat_vec(u, n, "u")), hip.ptr(_flat_vec(v, L, "v")),
                 hip.ptr(_flat_vec(log_mu, n, "log_mu")), hip.ptr(err), hip.stream_ptr())
    return err


LOCALSCALE_MODES = {"csls": hip.LOCALSCALE_CSLS, "nicdm": hip.LOCALSCALE_NICDM, "ls": hip.LOCALSCALE_LS}


def localscale_stats(idx, val):
    """(mean, kth) [n] fp32 of the top-k lists idx [n, k] int32 / val [n, k] fp32 (nr_localscale_stats): the mean of a list's
    present values (idx >= 0), summed one by one in list order, and the last of them; NaN for a list with none."""
    if idx.dim() != 2 or idx.shape != val.shape or idx.dtype != torch.int32 or val.dtype != torch.float32:
        raise ValueError("idx (int32) and val (fp32) must both be [n, k]")
    n, k = idx.shape
    k = _check_k(k)
    idx, val = idx.contiguous(), val.contiguous()
    mean = torch.empty((n,), dtype=torch.float32, device=idx.device)
    kth = torch.empty((n,), dtype=torch.float32, device=idx.device)
    if n:
        hip.call("nr_localscale_stats", hip.ptr(idx), hip.ptr(val), n, k, hip.ptr(mean), hip.ptr(kth), hip.stream_ptr())
    return mean, kth


def localscale_apply(S, mode, row_stat, col_stat):
    """T [n, L] fp32 from one read of S [n, L] (nr_localscale_apply); mode "csls" | "nicdm" | "ls".  row_stat [n] / col_stat [L]:
    the neighbourhood means (csls, nicdm) or k-th values (ls) of localscale_stats.  S may be a view whose rows lie back to back
    (a slice of a flat buffer): it is not copied, a misaligned one takes the kernel's scalar path."""
    if mode not in LOCALSCALE_MODES:
        raise ValueError(f"mode must be one of {sorted(LOCALSCALE_MODES)}, got {mode!r}")
    S = _slab_2d(S)
    n, L = S.shape
    T = torch.empty_like(S)
    if n and L:
        hip.call("nr_localscale_apply", hip.ptr(S), n, L, LOCALSCALE_MODES[mode], hip.ptr(_flat_vec(row_stat, n, "row_stat")),
                 hip.ptr(_flat_vec(col_stat, L, "col_stat")), hip.ptr(T), hip.stream_ptr())
    return T


def cand_localscale_rerank(fine, cand, n_gallery, k, g_stat, mode, ls_k, query_is_row, want_corr=True):
    """(idx [n, k] int32, val [n, k] fp32, corr [n, C] fp32 or None, qstat [n, 2] fp32) of candidate lists cand [n, C] int32
    (ascending gallery index, entries outside [0, n_gallery) absent) with fine scores fine [n, C], in one launch
    (nr_cand_localscale_rerank).  mode "csls" | "nicdm" | "ls"; g_stat [n_gallery] fp32: the gallery items' neighbourhood statistic
    (localscale_stats' mean for csls / nicdm, its kth for ls).  qstat = (mean, kth) of every query's top-ls_k list of its raw
    scores; corr = the formula of `mode` on (fine, the query's statistic, g_stat[cand]), the query being the row where
    query_is_row, else the column; absent slots -inf.  idx / val: the top k of corr, ties by lower position, -1 / -inf where the
    line has fewer than k present non-NaN slots.  1 <= k <= C <= 128, 1 <= ls_k <= C."""
    fine, cand, n, C, n_gallery, k, idx, val, corr = _cand_lines(fine, cand, n_gallery, k, want_corr)
    if mode not in LOCALSCALE_MODES:
        raise ValueError(f"mode must be one of {sorted(LOCALSCALE_MODES)}, got {mode!r}")
    if isinstance(ls_k, bool) or not isinstance(ls_k, int) or not 1 <= ls_k <= C:
        raise ValueError(f"ls_k must be an integer in [1, C = {C}], got {ls_k!r}")
    if not isinstance(query_is_row, (bool, int)) or query_is_row not in (0, 1):
        raise ValueError(f"query_is_row must be True or False, got {query_is_row!r}")
    dev = fine.device
    if not torch.is_tensor(g_stat) or g_stat.dtype != torch.float32 or g_stat.shape != (n_gallery,) or g_stat.device != dev:
        raise ValueError(f"g_stat must be a {torch.float32} vector of {n_gallery} entries on {dev}")
    qstat = torch.empty((n, 2), dtype=torch.float32, device=dev)
    if n:
        hip.call("nr_cand_localscale_rerank", hip.ptr(fine), hip.ptr(cand, torch.int32), n, C, n_gallery, hip.ptr(g_stat.contiguous()),
                 LOCALSCALE_MODES[mode], ls_k, int(query_is_row), k, hip.ptr(idx), hip.ptr(val), hip.ptr(corr, allow_none=True),
                 hip.ptr(qstat), hip.stream_ptr())
    return idx, val, corr, qstat


def _mp_matrix(x, dtype, shape, what):
    if x.dtype != dtype or x.dim() != 2 or not x.is_contiguous() or (shape is not None and tuple(x.shape) != tuple(shape)):
        want = "2-D" if shape is None else f"{tuple(shape)}"
        raise ValueError(f"{what} must be a contiguous {dtype} matrix, {want}, got {x.dtype} {tuple(x.shape)}")
    return x


def _mp_line(length, what):
    if length >= hip.MP_LINE_MAX:
        raise ValueError(f"{what}: a reference line of {length} entries is too long for exact counts (at most {hip.MP_LINE_MAX - 1})")


def mp_row_counts(S, R):
    """r2 [n, L] int32: r2[i, j] = 2 #{x in R[i, :] : x < S[i, j]} + #{x == S[i, j]} (nr_mp_row_counts); S [n, L], R [n, Lr] fp32.
    NaN entries count nothing, a NaN score counts 0."""
    S = _slab_2d(S)
    n, L = S.shape
    R = _mp_matrix(R, torch.float32, None, "R")
    if R.shape[0] != n:
        raise ValueError(f"R must have the {n} rows of S, got {tuple(R.shape)}")
    _mp_line(R.shape[1], "mp_row_counts")
    r2 = torch.empty((n, L), dtype=torch.int32, device=S.device)
    if n and L:
        hip.call("nr_mp_row_counts", hip.ptr(S), n, L, hip.ptr(R), R.shape[1], hip.ptr(r2), hip.stream_ptr())
    return r2


def mp_col_counts(S, Q, out=None):
    """c2 [n, L] int32: c2[i, j] = 2 #{x in Q[:, j] : x < S[i, j]} + #{x == S[i, j]} (nr_mp_col_counts); S [n, L], Q [m, L] fp32.
    out: the counts of earlier blocks of reference rows, added to in place and returned (integers: any blocking of the rows gives
    the same result)."""
    S = _slab_2d(S)
    n, L = S.shape
    Q = _mp_matrix(Q, torch.float32, None, "Q")
    if Q.shape[1] != L:
        raise ValueError(f"Q must have the {L} columns of S, got {tuple(Q.shape)}")
    m = Q.shape[0]
    _mp_line(m, "mp_col_counts")
    c2 = torch.empty((n, L), dtype=torch.int32, device=S.device) if out is None else _mp_matrix(out, torch.int32, (n, L), "out")
    if n and L and (m or out is None):
        hip.call("nr_mp_col_counts", hip.ptr(S), n, L, hip.ptr(Q) if m else None, m, hip.ptr(c2), 0 if out is None else 1,
                 hip.stream_ptr())
    return c2


def mp_line_counts(R=None, Q=None):
    """(row_cnt [n] of R [n, Lr], col_cnt [L] of Q [m, L]) int32: the non-NaN entries of every row of R and of every column of
    this slab of Q (nr_mp_line_counts); None for an input not given."""
    if R is None and Q is None:
        raise ValueError("nothing to count")
    row_cnt = col_cnt = None
    n = Lr = m = L = 0
    if R is not None:
        R = _mp_matrix(R, torch.float32, None, "R")
        n, Lr = R.shape
        row_cnt = torch.zeros((n,), dtype=torch.int32, device=R.device)
    if Q is not None:
        Q = _mp_matrix(Q, torch.float32, None, "Q")
        m, L = Q.shape
        col_cnt = torch.zeros((L,), dtype=torch.int32, device=Q.device)
    p = lambda x, live: hip.ptr(x) if (x is not None and live) else None             # noqa: E731
    rows, cols = bool(n and Lr), bool(m and L)
    if rows or cols:
        hip.call("nr_mp_line_counts", p(R, rows), n if rows else 0, Lr, p(row_cnt, rows), p(Q, cols), m, L if cols else 0,
                 p(col_cnt, cols), hip.stream_ptr())
    return row_cnt, col_cnt


def mp_emp_apply(S, r2, c2, row_cnt, col_cnt):
    """T [n, L] fp32 = fl(fl(r2 / 2 row_cnt[i]) fl(c2 / 2 col_cnt[j])), NaN where S is (nr_mp_emp_apply).  r2, c2 [n, L] int32 as
    mp_row_counts / mp_col_counts give them, row_cnt [n], col_cnt [L] int32 the lines' non-NaN counts.  S may be a view whose rows
    lie back to back (a slice of a flat buffer): it is not copied, a misaligned one takes the kernel's scalar path."""
    S = _slab_2d(S)
    n, L = S.shape
    r2, c2 = _mp_matrix(r2, torch.int32, (n, L), "r2"), _mp_matrix(c2, torch.int32, (n, L), "c2")
    row_cnt, col_cnt = _flat_vec(row_cnt, n, "row_cnt", torch.int32), _flat_vec(col_cnt, L, "col_cnt", torch.int32)
    T = torch.empty_like(S)
    if n and L:
        hip.call("nr_mp_emp_apply", hip.ptr(S), n, L, hip.ptr(r2), hip.ptr(c2), hip.ptr(row_cnt), hip.ptr(col_cnt), hip.ptr(T),
                 hip.stream_ptr())
    return T


def mp_row_moments(R):
    """(mean, sd) [n] fp32 of the rows of R [n, Lr] over their non-NaN entries (nr_mp_row_moments): fp64 accumulation, population
    standard deviation; NaN for a row with no entry."""
    R = _mp_matrix(_f32(R), torch.float32, None, "R")
    n, Lr = R.shape
    mean = torch.empty((n,), dtype=torch.float32, device=R.device)
    sd = torch.empty((n,), dtype=torch.float32, device=R.device)
    if n:
        hip.call("nr_mp_row_moments", hip.ptr(R) if Lr else None, n, Lr, hip.ptr(mean), hip.ptr(sd), hip.stream_ptr())
    return mean, sd


def mp_col_moments(Q):
    """parts [3, L] fp64 = (count, mean, M2) of the columns of this slab Q [m, L] over their non-NaN entries (nr_mp_col_moments):
    what a rank contributes to the cross-rank gather, merged by mp_moments_combine."""
    Q = _mp_matrix(_f32(Q), torch.float32, None, "Q")
    m, L = Q.shape
    parts = torch.zeros((3, L), dtype=torch.float64, device=Q.device)
    if m and L:
        hip.call("nr_mp_col_moments", hip.ptr(Q), m, L, hip.ptr(parts), hip.stream_ptr())
    return parts


def mp_moments_combine(parts):
    """parts [P, 3, L] fp64 -> (mean, sd) [L] fp32, merged by Chan's update in index order (nr_mp_moments_combine); NaN for a
    column with no entry in any part."""
    if parts.dtype != torch.float64 or parts.dim() != 3 or parts.shape[1] != 3 or not parts.is_contiguous():
        raise ValueError("parts must be a contiguous fp64 [P, 3, L]")
    P, _, L = parts.shape
    mean = torch.empty((L,), dtype=torch.float32, device=parts.device)
    sd = torch.empty((L,), dtype=torch.float32, device=parts.device)
    if L:
        hip.call("nr_mp_moments_combine", P, hip.ptr(parts) if P else None, L, hip.ptr(mean), hip.ptr(sd), hip.stream_ptr())
    return mean, sd


def mp_gauss_apply(S, row_mean, row_sd, col_mean, col_sd):
    """T [n, L] fp32 = -(Q_r + Q_c - Q_r Q_c), Q the upper tail 0.5 erfc(z / sqrt 2) of the row's / the column's normal at S[i, j]
    (nr_mp_gauss_apply).  S may be a row-contiguous view, as for mp_emp_apply."""
    S = _slab_2d(S)
    n, L = S.shape
    T = torch.empty_like(S)
    vecs = (_flat_vec(row_mean, n, "row_mean"), _flat_vec(row_sd, n, "row_sd"), _flat_vec(col_mean, L, "col_mean"),
            _flat_vec(col_sd, L, "col_sd"))
    if n and L:
        hip.call("nr_mp_gauss_apply", hip.ptr(S), n, L, *(hip.ptr(x) for x in vecs), hip.ptr(T), hip.stream_ptr())
    return T


MUTUALPROX_MODES = {"emp": hip.MUTUALPROX_EMP, "gauss": hip.MUTUALPROX_GAUSS}


def cand_mutualprox_rerank(fine, cand, n_gallery, k, mode, g_line=None, g_cnt=None, g_mean=None, g_sd=None, want_corr=True):
    """(idx [n, k] int32, val [n, k] fp32, corr [n, C] fp32 or None, qstat [n, 3] fp32) of candidate lists cand [n, C] int32
    (ascending gallery index, entries outside [0, n_gallery) absent) with fine scores fine [n, C], in one launch
    (nr_cand_mutualprox_rerank).  mode "emp": g_line [n_gallery, M] fp32 (item-major: item g's M bank scores) and g_cnt [n_gallery]
    int32 (their non-NaN counts, mp_line_counts); mode "gauss": g_mean, g_sd [n_gallery] fp32 (the lines' moments, mp_row_moments or
    mp_col_moments + mp_moments_combine); a mode reads its own arrays only.  qstat = (c_q, mean, sd) of every query's own line, the
    selectable slots' raw scores (fp64 sums in position order, population sd), in both modes.  corr = the formula of mp_emp_apply /
    mp_gauss_apply with the query's line on one side and the item's on the other; absent slots -inf.  idx / val: the top k of corr,
    ties by lower position, -1 / -inf where the line has fewer than k present slots with a non-NaN corr.  1 <= k <= C <= 128."""
    fine, cand, n, C, n_gallery, k, idx, val, corr = _cand_lines(fine, cand, n_gallery, k, want_corr)
    if not isinstance(mode, str) or mode not in MUTUALPROX_MODES:
        raise ValueError(f"mode must be one of {sorted(MUTUALPROX_MODES)}, got {mode!r}")
    dev = fine.device
    M = 0
    if mode == "emp":
        if (not torch.is_tensor(g_line) or g_line.dtype != torch.float32 or g_line.dim() != 2 or g_line.shape[0] != n_gallery
                or g_line.shape[1] < 1 or g_line.device != dev or not g_line.is_contiguous()):
            raise ValueError(f"g_line must be a contiguous {torch.float32} matrix of {n_gallery} rows (M >= 1 columns) on {dev}")
        M = g_line.shape[1]
        _mp_line(M, "cand_mutualprox_rerank")
        needs = ((g_cnt, torch.int32, "g_cnt"),)
    else:
        needs = ((g_mean, torch.float32, "g_mean"), (g_sd, torch.float32, "g_sd"))
    for x, dtype, what in needs:
        if not torch.is_tensor(x) or x.dtype != dtype or x.shape != (n_gallery,) or x.device != dev:
            raise ValueError(f"{what} must be a {dtype} vector of {n_gallery} entries on {dev}")
    qstat = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n:
        emp = mode == "emp"
        # the mode's own arrays, contiguous, held in `used` until the call has returned; the other mode's are not passed
        used = [x.contiguous() if on else None for x, on in ((g_line, emp), (g_cnt, emp), (g_mean, not emp), (g_sd, not emp))]
        line, cnt, mean, sd = (hip.ptr(x, allow_none=True) for x in used)
        hip.call("nr_cand_mutualprox_rerank", hip.ptr(fine), hip.ptr(cand, torch.int32), n, C, n_gallery, MUTUALPROX_MODES[mode],
                 line, cnt, M, mean, sd, k, hip.ptr(idx), hip.ptr(val), hip.ptr(corr, allow_none=True), hip.ptr(qstat),
                 hip.stream_ptr())
    return idx, val, corr, qstat


def _boot_cuts(cuts):
    cuts = [c for c in cuts]
    if not 1 <= len(cuts) <= hip.BOOT_MAX_CUTS:
        raise ValueError(f"cuts must hold 1 to {hip.BOOT_MAX_CUTS} cut-offs, got {len(cuts)}")
    if any(isinstance(c, bool) or int(c) != c for c in cuts):
        raise ValueError(f"cuts must be integers, got {cuts!r}")
    cuts = [int(c) for c in cuts]
    if cuts[0] < 1 or cuts[-1] >= 1 << 31 or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"cuts must be positive and strictly increasing, got {cuts!r}")
    return cuts


def _boot_ranking(ranks, unit_end, which, dev=None, U=None):
    """The checked (ranks, unit_end, E) of one ranking of bootstrap_rank_stats."""
    for name, t in ((f"ranks_{which}", ranks), (f"unit_end_{which}", unit_end)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D int32 tensor")
        if not t.is_cuda or (dev is not None and t.device != dev):
            raise ValueError(f"{name} must be on the GPU, on one device with the other operands (no CPU fallback)")
    if ranks.device != unit_end.device:
        raise ValueError(f"ranks_{which} and unit_end_{which} must be on one device")
    ranks, unit_end = ranks.contiguous(), unit_end.contiguous()
    E, n_units = ranks.numel(), unit_end.numel()
    if not 1 <= n_units <= hip.BOOT_MAX_UNITS or (U is not None and n_units != U):
        raise ValueError(f"unit_end_{which} must hold the same 1 to 2^24 units as the other ranking, got {n_units}")
    if E and (int(ranks.min()) < 0 or int(ranks.max()) >= hip.BOOT_RANK_LIMIT):
        raise ValueError(f"ranks_{which} must lie in [0, 2^30)")
    ends = unit_end.to(torch.int64)
    size = torch.diff(ends, prepend=ends.new_full((1,), -1))
    if int(size.min()) < 0 or int(ends[-1]) != E - 1:
        raise ValueError(f"unit_end_{which} must be non-decreasing from -1 and end at E - 1 = {E - 1}")
    if n_units * int(size.max()) >= 1 << 32:
        raise ValueError(f"ranking {which}: a resample could hold 2^32 entries or more (units times the largest unit)")
    if E == 0:
        ranks = torch.zeros((1,), dtype=torch.int32, device=ranks.device)        # never read: a pointer for the entry point
    return ranks, unit_end, E


def _resample_range(seed, first, count, names):
    """The checked integers (seed, first, count) of a resampling call; names = what the last two are called."""
    for name, v in (("seed", seed), (names[0], first), (names[1], count)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer, got {v!r}")
    seed, first, count = int(seed), int(first), int(count)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
    if first < 0 or count < 0 or first + count > (1 << 31) - 1:
        raise ValueError(f"{names[0]} and {names[1]} must be >= 0 with {names[0]} + {names[1]} <= 2^31 - 1, got {first} and {count}")
    return seed, first, count


def _resample_values(values, name):
    """The checked contiguous [U, Q] int64 values of a unit-sum call: on the GPU, U and Q in range, no sum can overflow."""
    if not torch.is_tensor(values) or values.dtype != torch.int64 or values.dim() != 2:
        raise ValueError(f"{name} must be a 2-D int64 tensor [U, Q]")
    if not values.is_cuda:
        raise ValueError(f"{name} must be on the GPU (no CPU fallback)")
    U, Q = values.shape
    if not 1 <= U <= hip.BOOT_MAX_UNITS or not 1 <= Q <= hip.BOOT_MAX_COLS:
        raise ValueError(f"{name} must be [U, Q] with U in [1, 2^24] and Q in [1, {hip.BOOT_MAX_COLS}], got {tuple(values.shape)}")
    largest = max(int(values.max()), -int(values.min()))
    if U * largest >= hip.BOOT_SUM_LIMIT:
        raise ValueError(f"{name}: U max|value| = {U} x {largest} reaches 2^62: a resample's sum could overflow")
    return values.contiguous()


def bootstrap_rank_stats(ranks_a, unit_end_a, ranks_b=None, unit_end_b=None, cuts=(1, 5, 10, 50), seed=0, b0=0, n_boot=1000):
    """int64 [n_boot, V, 4 + K] on the device (nr_bootstrap_rank_stats): for resamples b0 .. b0 + n_boot - 1 of the U units drawn
    with replacement and ranking v (V = 2 with ranks_b / unit_end_b, paired: the same draws), over the entries of the drawn units:
    n, the sum of ranks, the order statistics at positions (n - 1) // 2 and n // 2 (-1 when n = 0) and #{r < cuts[k]}.  ranks_v
    [E_v] int32 in [0, 2^30); unit_end_v [U] int32 = the index of the last entry of unit u (non-decreasing, from -1, ends at
    E_v - 1).  The result depends on (seed, b, inputs) alone."""
    cuts = _boot_cuts(cuts)
    if (ranks_b is None) != (unit_end_b is None):
        raise ValueError("ranks_b and unit_end_b come together")
    seed, b0, n_boot = _resample_range(seed, b0, n_boot, ("b0", "n_boot"))
    ra, ea, E_a = _boot_ranking(ranks_a, unit_end_a, "a")
    U = ea.numel()
    rb = eb = None
    E_b = 0
    if ranks_b is not None:
        rb, eb, E_b = _boot_ranking(ranks_b, unit_end_b, "b", ra.device, U)
    V = 1 if rb is None else 2
    K = len(cuts)
    out = torch.empty((n_boot, V, 4 + K), dtype=torch.int64, device=ra.device)
    if n_boot:
        hip.call("nr_bootstrap_rank_stats", hip.ptr(ra), hip.ptr(ea), E_a, hip.ptr(rb, allow_none=True), hip.ptr(eb, allow_none=True),
                 E_b, U, (ctypes.c_int32 * K)(*cuts), K, ctypes.c_uint64(seed), b0, n_boot, hip.ptr(out), hip.stream_ptr())
    return out


def pair_ranks(M_slab, row0, group_end, own, want_row=True, want_col=True):
    """(row_rank [n] int32 | None, col_ahead [n_total] int32 | None) of the row slab M[row0 : row0 + n, :] (nr_pair_ranks): pair s is
    (row s, column g(s)) with group_end [V] int32 on the device (video g owns the rows [group_end[g-1], group_end[g]), increasing from
    above 0 and ending at n_total: every video owns a sentence) and own [n_total] fp32 = M[s, g(s)].  row_rank: the complete 0-based text->video rank of the slab's pairs, -1
    where own is NaN or infinite; col_ahead: this slab's part of every pair's video->text rank among all sentences (0 where
    unranked): the sum over the slabs of a split is the rank.  group_end is checked on the device: ValueError."""
    for name, t, dtype in (("M_slab", M_slab, torch.float32), ("group_end", group_end, torch.int32), ("own", own, torch.float32)):
        if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda:
            raise ValueError(f"{name} must be a {dtype} tensor on the GPU (no CPU fallback)")
    if M_slab.dim() != 2 or group_end.dim() != 1 or own.dim() != 1:
        raise ValueError("M_slab must be [n, V], group_end [V] and own [n_total]")
    if not (M_slab.device == group_end.device == own.device):
        raise ValueError("M_slab, group_end and own must be on one device")
    if isinstance(row0, bool) or int(row0) != row0:
        raise ValueError(f"row0 must be an integer, got {row0!r}")
    M_slab, group_end, own = M_slab.contiguous(), group_end.contiguous(), own.contiguous()
    n, V = M_slab.shape
    n_total, row0 = own.numel(), int(row0)
    if V < 1 or group_end.numel() != V:
        raise ValueError(f"group_end must hold one entry per column, got {group_end.numel()} for {V} columns")
    if row0 < 0 or row0 + n > n_total:
        raise ValueError(f"rows [{row0}, {row0 + n}) do not lie in the {n_total} pairs")
    ends = group_end.to(torch.int64)
    if int(ends[0]) < 1 or int(ends[-1]) != n_total or (V > 1 and int(torch.diff(ends).min()) < 1):
        raise ValueError(f"group_end must be positive, increasing and end at n_total = {n_total}")
    dev = M_slab.device
    row_rank = torch.empty((n,), dtype=torch.int32, device=dev) if want_row else None
    col_ahead = torch.empty((n_total,), dtype=torch.int32, device=dev) if want_col else None
    if n_total:                                           # an empty slab has no storage: the entry point takes NULL for it
        hip.call("nr_pair_ranks", hip.ptr(M_slab) if n else None, n, V, row0, n_total, hip.ptr(group_end), hip.ptr(own),
                 hip.ptr(row_rank) if want_row and n else None, hip.ptr(col_ahead, allow_none=True), hip.stream_ptr())
    return row_rank, col_ahead


def bootstrap_unit_sums(values, seed=0, b0=0, n_boot=1000):
    """int64 [n_boot, Q] on the device (nr_bootstrap_unit_sums): out[i, q] = the sum of values[u, q] over the U units u that resample
    b0 + i draws with replacement -- the draws of bootstrap_rank_stats for the same (seed, b, U).  values [U, Q] int64 on the
    device, U in [1, 2^24], Q in [1, 16], U max|value| < 2^62 (no sum can overflow)."""
    values = _resample_values(values, "values")
    seed, b0, n_boot = _resample_range(seed, b0, n_boot, ("b0", "n_boot"))
    U, Q = values.shape
    out = torch.empty((n_boot, Q), dtype=torch.int64, device=values.device)
    if n_boot:
        hip.call("nr_bootstrap_unit_sums", hip.ptr(values), U, Q, ctypes.c_uint64(seed), b0, n_boot, hip.ptr(out), hip.stream_ptr())
    return out


def permtest_rank_stats(ranks_a, unit_end_a, ranks_b, unit_end_b, cuts=(1, 5, 10, 50), seed=0, p0=0, n_perm=1000):
    """int64 [n_perm, 2, 4 + K] on the device (nr_permtest_rank_stats): for permutations p0 .. p0 + n_perm - 1 and the sides X, Y of
    the relabelling -- X takes unit u's entries from ranking a when the swap bit s(p, u) is 0 and from b when it is 1, Y the other
    ranking's -- over the side's entries: n, the sum of ranks, the order statistics at positions (n - 1) // 2 and n // 2 (-1 when
    n = 0) and #{r < cuts[k]}.  Rankings as in bootstrap_rank_stats (checked on the device: ValueError); both are required.  The
    result depends on (seed, p, inputs) alone."""
    cuts = _boot_cuts(cuts)
    seed, p0, n_perm = _resample_range(seed, p0, n_perm, ("p0", "n_perm"))
    ra, ea, E_a = _boot_ranking(ranks_a, unit_end_a, "a")
    U = ea.numel()
    rb, eb, E_b = _boot_ranking(ranks_b, unit_end_b, "b", ra.device, U)
    K = len(cuts)
    out = torch.empty((n_perm, 2, 4 + K), dtype=torch.int64, device=ra.device)
    if n_perm:
        hip.call("nr_permtest_rank_stats", hip.ptr(ra), hip.ptr(ea), E_a, hip.ptr(rb), hip.ptr(eb), E_b, U, (ctypes.c_int32 * K)(*cuts),
                 K, ctypes.c_uint64(seed), p0, n_perm, hip.ptr(out), hip.stream_ptr())
    return out


def permtest_unit_sums(values_a, values_b, seed=0, p0=0, n_perm=1000):
    """int64 [n_perm, Q] on the device (nr_permtest_unit_sums): out[i, q] = the sum over the units u of values_b[u, q] where the swap
    bit s(p0 + i, u) of permtest_rank_stats is 1 and of values_a[u, q] where it is 0: side X; side Y is the two inputs' totals minus
    it.  values_a, values_b [U, Q] int64 on one device, U in [1, 2^24], Q in [1, 16], U max|value| < 2^62 for either."""
    values_a, values_b = _resample_values(values_a, "values_a"), _resample_values(values_b, "values_b")
    if values_a.shape != values_b.shape or values_a.device != values_b.device:
        raise ValueError(f"values_a and values_b must have one shape and one device, got {tuple(values_a.shape)} and "
                         f"{tuple(values_b.shape)}")
    seed, p0, n_perm = _resample_range(seed, p0, n_perm, ("p0", "n_perm"))
    U, Q = values_a.shape
    out = torch.empty((n_perm, Q), dtype=torch.int64, device=values_a.device)
    if n_perm:
        hip.call("nr_permtest_unit_sums", hip.ptr(values_a), hip.ptr(values_b), U, Q, ctypes.c_uint64(seed), p0, n_perm, hip.ptr(out),
                 hip.stream_ptr())
    return out


def permtest_hubness(idx_a, idx_b, unit_end, n_gallery, gt_begin, gt_end, seed=0, p0=0, n_perm=1000):
    """int64 [n_perm, 2, 9] on the device (nr_permtest_hubness): for permutations p0 .. p0 + n_perm - 1 and the sides X, Y of the
    relabelling -- X takes unit u's top-k lists from ranking a when the swap bit s(p, u) of permtest_rank_stats is 0 and from b when
    it is 1, Y the other ranking's -- the integers S1, S2, S3 (power sums of the k-occurrence counts N over the gallery), #{N = 0},
    #{N G > 2 S1}, the sum of N over those hubs, #{hub and N - GN > GN}, sum GN and max N.  idx_a, idx_b [n_lists, k] int32 as
    slab_topk_rows / topk_merge write them; unit_end [U] int32 = the index of the last list of unit u (non-decreasing, from -1, ends
    at n_lists - 1; checked on the device: ValueError); gt_begin / gt_end [n_lists] int32 as for topk_occurrences.  At most
    32 768 gallery items and 65 535 lists.  The result depends on (seed, p, inputs) alone."""
    tensors = (("idx_a", idx_a, 2), ("idx_b", idx_b, 2), ("unit_end", unit_end, 1), ("gt_begin", gt_begin, 1), ("gt_end", gt_end, 1))
    for name, t, dim in tensors:
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != dim:
            raise ValueError(f"{name} must be a {dim}-D int32 tensor")
        if not t.is_cuda or t.device != idx_a.device:
            raise ValueError(f"{name} must be on the GPU, on one device with the other operands (no CPU fallback)")
    if idx_a.shape != idx_b.shape:
        raise ValueError(f"idx_a and idx_b must have one shape, got {tuple(idx_a.shape)} and {tuple(idx_b.shape)}")
    n_lists, k = idx_a.shape
    k = _check_k(k)
    if isinstance(n_gallery, bool) or int(n_gallery) != n_gallery or int(n_gallery) < 1:
        raise ValueError(f"n_gallery must be a positive integer, got {n_gallery!r}")
    n_gallery = int(n_gallery)
    if n_gallery > hip.HUBPERM_MAX_GALLERY:
        raise ValueError(f"n_gallery = {n_gallery} is above the {hip.HUBPERM_MAX_GALLERY} items whose counters one workgroup's LDS holds")
    if n_lists > hip.HUBPERM_MAX_LISTS:
        raise ValueError(f"{n_lists} lists are above the limit of {hip.HUBPERM_MAX_LISTS}: a counter keeps N in 16 bits")
    if gt_begin.shape != (n_lists,) or gt_end.shape != (n_lists,):
        raise ValueError("gt_begin / gt_end must have one entry per list")
    seed, p0, n_perm = _resample_range(seed, p0, n_perm, ("p0", "n_perm"))
    U = unit_end.numel()
    if not 1 <= U <= hip.BOOT_MAX_UNITS:
        raise ValueError(f"unit_end must hold 1 to 2^24 units, got {U}")
    ends = unit_end.to(torch.int64)
    if int(torch.diff(ends, prepend=ends.new_full((1,), -1)).min()) < 0 or int(ends[-1]) != n_lists - 1:
        raise ValueError(f"unit_end must be non-decreasing from -1 and end at n_lists - 1 = {n_lists - 1}")
    idx_a, idx_b, unit_end, gt_begin, gt_end = (t.contiguous() for t in (idx_a, idx_b, unit_end, gt_begin, gt_end))
    out = torch.empty((n_perm, 2, 9), dtype=torch.int64, device=idx_a.device)
    if not n_perm:
        return out
    occ_a, good_a = topk_occurrences(idx_a, n_gallery, gt_begin, gt_end)
    occ_b, good_b = topk_occurrences(idx_b, n_gallery, gt_begin, gt_end)
    occ_ab, good_ab = occ_a + occ_b, good_a + good_b
    if n_lists == 0:
        idx_a = idx_b = gt_begin = gt_end = torch.zeros((1,), dtype=torch.int32, device=out.device)      # never read: pointers for the entry point
    hip.call("nr_permtest_hubness", hip.ptr(idx_a), hip.ptr(idx_b), n_lists, k, hip.ptr(unit_end), U, n_gallery, hip.ptr(gt_begin),
             hip.ptr(gt_end), hip.ptr(occ_ab), hip.ptr(good_ab), ctypes.c_uint64(seed), p0, n_perm, hip.ptr(out), hip.stream_ptr())
    return out


def linear_x3(x, w, bias=None, residual=None):
    """Y = X W^T (+ bias) (+ residual) on the split-bf16 MFMA tile engine (nr_linear_x3): x [M,K], w [N,K] fp32, K padded to
    a multiple of 64 with zeros.  ~fp32-grade products (3 bf16 passes); used for the clustering GEMMs and for the
    backward of the token-scorer MLP."""
    x, w = _f32(x).contiguous(), _f32(w).contiguous()
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError("inner dimensions differ")
    if K % 64:
        pad = 64 - K % 64
        x = torch.nn.functional.pad(x, (0, pad))
        w = torch.nn.functional.pad(w, (0, pad))
        K += pad
    xh, xl = split_bf16(x)
    wh, wl = split_bf16(w)
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    b = _f32(bias).contiguous() if bias is not None else None
    r = _f32(residual).contiguous() if residual is not None else None
    hip.call("nr_linear_x3", hip.ptr(xh), hip.ptr(xl), hip.ptr(wh), hip.ptr(wl), hip.ptr(b, allow_none=True), hip.ptr(r, allow_none=True),
             M, N, K, hip.ptr(out), hip.stream_ptr())
    return out


def bertadam_plan(entries, groups):
    """Host-only check of a BertAdam table before its upload (nr_bertadam_plan): `entries` a ctypes array of hip.OptimTensor,
    `groups` one of hip.OptimGroup.  Writes every entry's chunk0 -> the number of chunks; raises on a null / misaligned pointer,
    a negative count, a group index out of range or a bad schedule id."""
    n_chunks = ctypes.c_int(0)
    hip._check("nr_bertadam_plan", hip.lib().nr_bertadam_plan(entries, len(entries), groups, len(groups), ctypes.byref(n_chunks)))
    return int(n_chunks.value)


def bertadam_workspace_bytes(n_tensors, n_chunks):
    return int(hip.lib().nr_bertadam_workspace_bytes(int(n_tensors), int(n_chunks)))


def bertadam_step(groups_dev, n_groups, table_dev, n_tensors, n_chunks, workspace, global_max_norm=None, table_offset=0):
    """The three launches of the multi-tensor BertAdam update (nr_bertadam_step) on the current stream.  groups_dev / table_dev:
    uint8 device tensors holding the uploaded hip.OptimGroup / hip.OptimTensor arrays that bertadam_plan checked (the table
    starts `table_offset` bytes into table_dev); workspace: uint8, bertadam_workspace_bytes(n_tensors, n_chunks) or more."""
    if workspace.numel() < bertadam_workspace_bytes(n_tensors, n_chunks):
        raise hip.NrHipError("bertadam_step: workspace too small")
    gmn = -1.0 if global_max_norm is None else float(global_max_norm)
    hip.call("nr_bertadam_step", ctypes.c_void_p(hip.ptr(table_dev, torch.uint8).value + int(table_offset)), int(n_tensors),
             int(n_chunks), hip.ptr(groups_dev, torch.uint8), int(n_groups), ctypes.c_float(gmn), hip.ptr(workspace, torch.uint8),
             hip.stream_ptr())


def bertadam_step_guarded(groups_dev, n_groups, table_dev, n_tensors, n_chunks, workspace, guard, ring, global_max_norm=None,
                          table_offset=0, losses=None):
    """bertadam_step with the non-finite guard (nr_bertadam_step_guarded): a step whose sum of squared gradients is not finite
    leaves p, m, v and the step counters as they were.  guard: uint8 device tensor holding one hip.StepGuard (zeroed by the
    caller, last_skipped = -1); ring: uint8 device tensor of n_ring hip.StepRecord, n_ring a power of two in [1, 4096]; losses:
    None or a contiguous float32 device tensor of at most 8 values, copied into the step's record when the launches execute."""
    if workspace.numel() < bertadam_workspace_bytes(n_tensors, n_chunks):
        raise hip.NrHipError("bertadam_step_guarded: workspace too small")
    rec = ctypes.sizeof(hip.StepRecord)
    n_ring = ring.numel() // rec
    if guard.numel() < ctypes.sizeof(hip.StepGuard) or n_ring * rec != ring.numel():
        raise hip.NrHipError("bertadam_step_guarded: guard / ring do not have the size of NrStepGuard / a whole number of NrStepRecord")
    n_losses = 0 if losses is None else int(losses.numel())
    gmn = -1.0 if global_max_norm is None else float(global_max_norm)
    hip.call("nr_bertadam_step_guarded", ctypes.c_void_p(hip.ptr(table_dev, torch.uint8).value + int(table_offset)), int(n_tensors),
             int(n_chunks), hip.ptr(groups_dev, torch.uint8), int(n_groups), ctypes.c_float(gmn), hip.ptr(workspace, torch.uint8),
             hip.ptr(guard, torch.uint8), hip.ptr(losses, torch.float32, allow_none=True), n_losses, hip.ptr(ring, torch.uint8),
             int(n_ring), hip.stream_ptr())


def bertadam_step_ema(groups_dev, n_groups, table_dev, n_tensors, n_chunks, workspace, shadows_dev, state, guard=None, ring=None,
                      global_max_norm=None, table_offset=0, shadows_offset=0, losses=None):
    """bertadam_step / bertadam_step_guarded (guard and ring given) with the weight EMA inside (nr_bertadam_step_ema).
    shadows_dev: uint8 device tensor holding, `shadows_offset` bytes in, n_tensors 8-byte pointers parallel to the table (0: that
    tensor is not averaged); state: uint8 device tensor holding one hip.EmaState."""
    if workspace.numel() < bertadam_workspace_bytes(n_tensors, n_chunks):
        raise hip.NrHipError("bertadam_step_ema: workspace too small")
    if state.numel() < ctypes.sizeof(hip.EmaState) or shadows_dev.numel() < int(shadows_offset) + 8 * int(n_tensors):
        raise hip.NrHipError("bertadam_step_ema: state / shadows do not have the size of NrEmaState / n_tensors pointers")
    n_ring = n_losses = 0
    if guard is not None:
        rec = ctypes.sizeof(hip.StepRecord)
        n_ring = ring.numel() // rec
        if guard.numel() < ctypes.sizeof(hip.StepGuard) or n_ring * rec != ring.numel():
            raise hip.NrHipError("bertadam_step_ema: guard / ring do not have the size of NrStepGuard / a whole number of NrStepRecord")
        n_losses = 0 if losses is None else int(losses.numel())
    else:
        losses = None
    gmn = -1.0 if global_max_norm is None else float(global_max_norm)
    hip.call("nr_bertadam_step_ema", ctypes.c_void_p(hip.ptr(table_dev, torch.uint8).value + int(table_offset)), int(n_tensors),
             int(n_chunks), hip.ptr(groups_dev, torch.uint8), int(n_groups), ctypes.c_float(gmn), hip.ptr(workspace, torch.uint8),
             hip.ptr(guard, torch.uint8, allow_none=True), hip.ptr(losses, torch.float32, allow_none=True), n_losses,
             hip.ptr(ring, torch.uint8, allow_none=True) if guard is not None else None, int(n_ring),
             ctypes.c_void_p(hip.ptr(shadows_dev, torch.uint8).value + int(shadows_offset)), hip.ptr(state, torch.uint8),
             hip.stream_ptr())


def ema_plan(entries, state):
    """Host-only check of a weight-EMA table and state before their upload (nr_ema_plan): `entries` a ctypes array of
    hip.EmaTensor, `state` a hip.EmaState.  Writes every entry's chunk0 -> the number of chunks; raises on a null / misaligned
    pointer, a negative count or a decay outside [0, 1)."""
    n_chunks = ctypes.c_int(0)
    hip._check("nr_ema_plan", hip.lib().nr_ema_plan(entries, len(entries), ctypes.byref(state), ctypes.byref(n_chunks)))
    return int(n_chunks.value)


def ema_update(table_dev, n_tensors, n_chunks, state):
    """One stand-alone update of every shadow of the uploaded hip.EmaTensor table (nr_ema_update: two launches on the current
    stream); state: uint8 device tensor holding one hip.EmaState."""
    if state.numel() < ctypes.sizeof(hip.EmaState) or table_dev.numel() < int(n_tensors) * ctypes.sizeof(hip.EmaTensor):
        raise hip.NrHipError("ema_update: state / table do not have the size of NrEmaState / n_tensors NrEmaTensor")
    hip.call("nr_ema_update", hip.ptr(table_dev, torch.uint8), int(n_tensors), int(n_chunks), hip.ptr(state, torch.uint8),
             hip.stream_ptr())


def ema_swap(table_dev, n_tensors, n_chunks):
    """Exchanges the contents of every (parameter, shadow) pair of the uploaded hip.EmaTensor table in place (nr_ema_swap)."""
    if table_dev.numel() < int(n_tensors) * ctypes.sizeof(hip.EmaTensor):
        raise hip.NrHipError("ema_swap: the table does not hold n_tensors NrEmaTensor")
    hip.call("nr_ema_swap", hip.ptr(table_dev, torch.uint8), int(n_tensors), int(n_chunks), hip.stream_ptr())
