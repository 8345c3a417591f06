"""Every form of the DPC-KNN assignment against the decision-exact reference of tests/dpc_ref.py, each on the distance matrix the
kernel itself left behind: the stand-alone kernel (nr_dpc_knn_assign), the first form of the back half (nr_ctm_front +
nr_ctm_back, and the grouped stage at C = 256 or more than 16 clusters), the second form beside the kv GEMM (masked stages:
back forms 4 and 16) and fused behind the front half (unmasked stages: the 256- and the 512-thread kernel).  Per launch: the
matrix (symmetric bits, zero diagonal, smax its maximum, entries inside the bars of dist_ref, 0 between identical rows), the
assignment on every decided sample, the forms among each other on the same bits, the shares and cluster means, sentinels.

What cannot be done from outside: nr_dpc_knn_assign computes its matrix itself and takes none, so it meets the crafted matrices
only through the reference (its own matrix, its own assignment), not through the other forms' bits; the grouped stage allocates
`assign` itself and carves `merged_pb` out of its workspace, so the guards sit behind the buffers of the entry points that take
them as arguments (nr_dpc_knn_assign, nr_ctm_back)."""
import ctypes

import pytest
import torch

import dpc_ref as R
from neighborretr_amd import cluster, hip
from neighborretr_amd.cluster_fused import ctm_stage_group

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -0x5A5A5A5A5A5A5A5B                    # int64 guard pattern
EPS = 1e-5


def _g(t):
    return None if t is None else t.to(DEV).contiguous()


# ---- the checks ---------------------------------------------------------------------------------------------------------------
def check_matrix(dist, smax, xn, label):
    """1: bit-symmetric, zero diagonal, smax the exact maximum, entries inside the rigorous bound and the working bar of
    dist_ref(xn), exactly 0 between bit-identical rows (their bound is 0).  -> the largest share of the rigorous bound."""
    d, xn = dist.cpu(), xn.cpu()
    assert torch.equal(d, d.transpose(1, 2)), label
    assert not d.diagonal(dim1=1, dim2=2).any(), label
    assert torch.equal(smax.cpu(), d.flatten(1).max(-1)[0]), label
    ref, rig, work = R.dist_ref(xn)
    err = (d.double() - ref).abs()
    assert bool((err <= rig).all()) and bool((err <= work).all()), (label, float((err / rig.clamp_min(1e-300)).max()))
    on = rig > 0
    share = float((err[on] / rig[on]).max()) if bool(on.any()) else 0.0
    print(f"{label}: distances use {share:.4f} of the rigorous bound")
    return share


def check_assign(dist, mask, noise, k, cnum, got, label, edges=(), all_decided=False):
    """2: equal to assign_ref of THAT matrix on every decided sample (padding tokens included); undecided samples counted, at
    most CAP of them, none of the named ones; ids in range everywhere.  -> the reference."""
    ref = R.assign_ref(dist.cpu(), None if mask is None else mask.cpu(), noise.cpu(), k, cnum)
    got = got.cpu()
    B = got.shape[0]
    dec = ref.decided
    und = int((~dec).sum())
    moved = [b for b in range(B) if not torch.equal(got[b], ref.assign[b])]
    print(f"{label}: {und}/{B} undecided; differs from the reference on samples {moved}")
    assert int(got.min()) >= 0 and int(got.max()) < cnum, label
    assert not [b for b in moved if dec[b]], (label, [b for b in moved if dec[b]])
    assert und <= R.CAP * B, (label, und)
    assert all(bool(dec[b]) for b in edges), (label, dec.tolist())
    assert not all_decided or und == 0, (label, dec.tolist())
    return ref


def check_merge(xn, w, assign, cnum, P, merged_pb, label, qn=None, qn_hi=None, qn_lo=None):
    """4: merged_pb inside the N-term bound of merge_ref at the kernel's OWN assignment, xn and w; clusters of padding alone are
    the bias exactly; norm1(merged), as fp32 or as the bf16 pair, to 2^-16 of its largest entry.  -> largest share of the bound."""
    xn, w, assign = xn.cpu(), w.cpu(), assign.cpu()
    B, N, C = xn.shape
    pb = P["proj_b"].cpu()
    share, want, A, merged = R.merge_ref(xn, w, assign, cnum, pb)
    got = merged_pb.cpu().view(B, cnum, C)
    bound = R.merge_bound(N, A, want)
    err = (got.double() - want).abs()
    assert bool((err <= bound).all()), (label, float((err / bound).max()))
    onehot = torch.nn.functional.one_hot(assign, cnum).double()
    empty = torch.einsum("bnc,bn->bc", onehot, w.double()) == 0
    assert torch.equal(got[empty], pb.expand(B, cnum, C)[empty]), label
    q = R.norm1_ref(merged, P["n1_w"].cpu(), P["n1_b"].cpu(), EPS)
    rec = qn.cpu().double() if qn is not None else qn_hi.cpu().view(torch.bfloat16).double() + qn_lo.cpu().view(torch.bfloat16).double()
    qerr = float((rec.view(B, cnum, C) - q).abs().max())
    assert qerr <= 2.0 ** -16 * float(q.abs().max()), (label, qerr)
    sh = float((err / bound).max())
    print(f"{label}: merged_pb uses {sh:.4f} of its bound, {int(empty.sum())} all-padding clusters, norm1 off by {qerr:.2e}")
    return sh


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def params(C, seed=11):
    g = torch.Generator().manual_seed(R.SEED + seed + C)
    vec = lambda n, s=1.0: (torch.randn(n, generator=g) * s).to(DEV)
    # (LayerNorm of the clustering at weight 1, bias 0: the random token sets are layer-normed already, so the kernels' rows are
    # the makers' rows up to rounding and the pinned draws of tests/dpc_ref.py keep their neighbour structure)
    return dict(ln_w=torch.ones(C, device=DEV), ln_b=torch.zeros(C, device=DEV), sc_w=vec(C, 0.05).reshape(1, C), sc_b=vec(1, 0.01), n1_w=1 + vec(C, 0.05),
                n1_b=vec(C, 0.01), proj_b=vec(C, 0.01))


def standalone(x, mask, noise, k, cnum):
    """nr_dpc_knn_assign -> (assign, dist, smax): the matrix and the maxima from its workspace (dist [B,N,N] then smax [B])."""
    B, N, C = x.shape
    ws = torch.empty(int(hip.lib().nr_dpc_workspace_bytes(B, N)), dtype=torch.uint8, device=DEV)
    buf = torch.full((B * N + 64,), SENT, dtype=torch.int64, device=DEV)
    hip.call("nr_dpc_knn_assign", hip.ptr(x), hip.ptr(mask, allow_none=True), hip.ptr(noise), B, N, C, k, cnum, hip.ptr(buf), hip.ptr(ws),
             hip.stream_ptr())
    torch.cuda.synchronize()
    assert bool((buf[B * N:] == SENT).all())
    f = ws.view(torch.float32)
    return buf[:B * N].view(B, N).clone(), f[:B * N * N].view(B, N, N).clone(), f[B * N * N: B * N * N + B].clone()


def front(y, mask, P):
    """nr_ctm_front -> dict(xn, score, w, dist, smax)."""
    B, N, C = y.shape
    f = lambda *s: torch.empty(*s, device=DEV)
    o = dict(xn=f(B, N, C), kvn=f(B * N, C), score=f(B, N), w=f(B, N), dist=f(B, N, N), smax=f(B))
    hip.call("nr_ctm_front", hip.ptr(y), hip.ptr(mask, allow_none=True), B, N, C, hip.ptr(P["ln_w"]), hip.ptr(P["ln_b"]), hip.ptr(P["sc_w"]),
             hip.ptr(P["sc_b"]), hip.ptr(P["n1_w"]), hip.ptr(P["n1_b"]), EPS, hip.ptr(o["xn"]), hip.ptr(o["kvn"]), None, None,
             hip.ptr(o["score"]), hip.ptr(o["w"]), hip.ptr(o["dist"]), hip.ptr(o["smax"]), hip.stream_ptr())
    return o


def back(dist, smax, mask, noise, xn, w, k, cnum, P):
    """nr_ctm_back (first form, one problem) with NaN / pattern guards behind merged_pb and assign -> dict(assign, merged_pb, qn)."""
    B, N, C = xn.shape
    n = B * cnum * C
    mbuf = torch.full((n + 256,), float("nan"), device=DEV)
    abuf = torch.full((B * N + 64,), SENT, dtype=torch.int64, device=DEV)
    merged, qn = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    hip.call("nr_ctm_back", hip.ptr(dist), hip.ptr(smax), hip.ptr(mask, allow_none=True), hip.ptr(noise), hip.ptr(xn), hip.ptr(w), B, N, C, k,
             cnum, hip.ptr(P["n1_w"]), hip.ptr(P["n1_b"]), hip.ptr(P["proj_b"]), EPS, hip.ptr(merged), hip.ptr(mbuf), hip.ptr(qn),
             hip.ptr(abuf), hip.stream_ptr())
    torch.cuda.synchronize()
    assert bool(mbuf[n:].isnan().all()) and bool((abuf[B * N:] == SENT).all()) and not bool(mbuf[:n].isnan().any())
    return dict(assign=abuf[:B * N].view(B, N).clone(), merged_pb=mbuf[:n].clone(), qn=qn)


def agree(a, b, ref, xn, w, cnum, P, label):
    """3: two forms fed the same bits: the same assignment on every decided sample; where a sample's assignment is the same, its
    merged_pb inside the two bounds."""
    dec = ref.decided
    assert torch.equal(a["assign"].cpu()[dec], b["assign"].cpu()[dec]), label
    same = (a["assign"] == b["assign"]).all(-1).cpu()
    B, N, C = xn.shape
    _, want, A, _ = R.merge_ref(xn.cpu(), w.cpu(), a["assign"].cpu(), cnum, P["proj_b"].cpu())
    err = (a["merged_pb"].cpu().view(B, cnum, C).double() - b["merged_pb"].cpu().view(B, cnum, C).double()).abs()
    assert bool((err <= 2 * R.merge_bound(N, A, want))[same].all()), label


# ---- the stand-alone kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cnum", R.SHAPES)
def test_standalone_kernel(N, cnum):
    C = R.STANDALONE_C[(N, cnum)]
    worst = 0.0
    for n_, c_, k, masked in R.random_cases():
        if (n_, c_) != (N, cnum):
            continue
        x, mask, noise = (_g(t) for t in R.random_tokens(N, cnum, k, masked, C))
        label = f"stand-alone N{N} c{cnum} k{k} C{C} {'mask' if masked else 'nomask'}"
        assign, dist, smax = standalone(x, mask, noise, k, cnum)
        worst = max(worst, check_matrix(dist, smax, x, label))
        check_assign(dist, mask, noise, k, cnum, assign, label, edges=R.edge_samples(cnum) if masked else ())
        again = standalone(x, mask, noise, k, cnum)
        assert torch.equal(again[0], assign) and torch.equal(again[1], dist) and torch.equal(again[2], smax), label
    print(f"stand-alone N{N} C{C}: worst distance share {worst:.4f}")


# ---- nr_ctm_front + nr_ctm_back (first form, one problem) ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,cnum,C", R.FRONT_BACK)
def test_front_and_back_one_problem(N, cnum, C):
    P = params(C)
    for n_, c_, k, masked in R.random_cases():
        if (n_, c_) != (N, cnum):
            continue
        x, mask, noise = (_g(t) for t in R.random_tokens(N, cnum, k, masked, C))
        label = f"front+back N{N} c{cnum} k{k} C{C} {'mask' if masked else 'nomask'}"
        f = front(x, mask, P)
        check_matrix(f["dist"], f["smax"], f["xn"], label)
        b = back(f["dist"], f["smax"], mask, noise, f["xn"], f["w"], k, cnum, P)
        check_assign(f["dist"], mask, noise, k, cnum, b["assign"], label, edges=R.edge_samples(cnum) if masked else ())
        check_merge(f["xn"], f["w"], b["assign"], cnum, P, b["merged_pb"], label, qn=b["qn"])
        b2 = back(f["dist"], f["smax"], mask, noise, f["xn"], f["w"], k, cnum, P)
        assert torch.equal(b2["assign"], b["assign"]) and torch.equal(b2["merged_pb"], b["merged_pb"]), label
    # (b) the crafted matrices straight into nr_ctm_back, smax consistent with them; rows and weights of a front run on that mask
    for k in (3, 4, 5):
        dist, smax, mask, noise, names = (t if isinstance(t, tuple) else _g(t) for t in R.crafted(N, k, cnum))
        x = _g(torch.randn(len(names), N, C, generator=torch.Generator().manual_seed(R.SEED + k)))
        f = front(x, mask, P)
        label = f"back, crafted N{N} c{cnum} k{k} C{C}"
        b = back(dist, smax, mask, noise, f["xn"], f["w"], k, cnum, P)
        check_assign(dist, mask, noise, k, cnum, b["assign"], label, all_decided=True)
        check_merge(f["xn"], f["w"], b["assign"], cnum, P, b["merged_pb"], label, qn=b["qn"])


# ---- the grouped stage ------------------------------------------------------------------------------------------------------------
def modules(C, N, cnum, k, P):
    """Test-owned CTM + TCBlock: zero convolution (y = x exactly), the LayerNorm / score / bias parameters of `P`."""
    ctm = cluster.CTM(R.ratio_of(N, cnum), C, C, k=k)
    blk = cluster.TCBlock(C, C // 64)
    with torch.no_grad():
        ctm.conv.conv.weight.zero_()
        ctm.norm.weight.copy_(P["ln_w"]), ctm.norm.bias.copy_(P["ln_b"])
        ctm.score.weight.copy_(P["sc_w"]), ctm.score.bias.copy_(P["sc_b"])
        blk.norm1.weight.copy_(P["n1_w"]), blk.norm1.bias.copy_(P["n1_b"])
        blk.attn.proj.bias.copy_(P["proj_b"])
    return ctm.to(DEV).eval(), blk.to(DEV).eval()


def stage_views(view, B, N, C, cnum):
    """(dist [B,N,N], smax [B]) inside the stage workspace `view` is a view of: smax where nr_ctm_stage_workspace_layout2 says,
    dist in the block right before it (both 256-byte aligned: carve() of csrc/nr_ctm_group.hip)."""
    ws = torch.empty(0, dtype=torch.uint8, device=view.device).set_(view.untyped_storage())
    off = (ctypes.c_size_t * 14)()
    hip.call("nr_ctm_stage_workspace_layout2", B, N, C, cnum, off)
    so = int(off[7])
    span = (B * N * N * 4 + 255) // 256 * 256
    return ws[so - span: so - span + B * N * N * 4].view(torch.float32).view(B, N, N), ws[so: so + 4 * B].view(torch.float32)


def run_group(C, probs, inputs, P, overwrite=None):
    """One ctm_stage_group call of two problems -> per problem dict(saved..., dist, smax).  inputs: per problem (x, mask, noise).
    overwrite: per problem (dist, smax) written over the stage's own between its front and its back launch (masked stages)."""
    mods = [modules(C, N, cnum, k, P) for N, cnum, k in probs]
    plist = [(f"p{i}", x, mask, ctm, blk, noise) for i, ((x, mask, noise), (ctm, blk)) in enumerate(zip(inputs, mods))]
    seen = []

    def exchange(smax_list):
        seen.append(len(smax_list))
        for i, s in enumerate(smax_list):
            if overwrite is not None:
                B, N = inputs[i][0].shape[:2]
                d, _ = stage_views(s, B, N, C, probs[i][1])
                d.copy_(overwrite[i][0])
                s.copy_(overwrite[i][1])
    masked = inputs[0][1] is not None
    with torch.no_grad():
        outs, saved = ctm_stage_group(plist, {}, want_saved=True, exchange=exchange if masked else None)
    torch.cuda.synchronize()
    assert seen == ([2] if masked else [])
    res = []
    for i, sv in enumerate(saved):
        B, N = inputs[i][0].shape[:2]
        d, s = stage_views(sv["xn"], B, N, C, probs[i][1])
        assert not bool(outs[i].isnan().any())
        res.append(dict(sv, dist=d, smax=s))
    return res


def check_problem(r, mask, noise, N, cnum, k, P, label, own_matrix=True, edges=(), all_decided=False):
    if own_matrix:
        check_matrix(r["dist"], r["smax"], r["xn"], label)
    ref = check_assign(r["dist"], mask, noise, k, cnum, r["assign"], label, edges=edges, all_decided=all_decided)
    check_merge(r["xn"], r["w"], r["assign"], cnum, P, r["merged_pb"], label, qn_hi=r["qn_hi"], qn_lo=r["qn_lo"])
    # 3: the first form (one problem, a launch of its own) on the same bits
    b = back(r["dist"], r["smax"], mask, noise, r["xn"], r["w"], k, cnum, P)
    agree(dict(assign=r["assign"], merged_pb=r["merged_pb"]), b, ref, r["xn"], r["w"], cnum, P, label)


MASKED = [g for g in R.GROUPED if g[2]]
UNMASKED = [g for g in R.GROUPED if not g[2]]


@pytest.mark.parametrize("name,C,masked,probs", MASKED, ids=[g[0] for g in MASKED])
def test_grouped_masked_stage(name, C, masked, probs):
    """Back half as a launch of its own kind (beside the kv GEMM): on the stage's own matrix of random tokens, then on the crafted
    matrices written over it between the front and the back launch."""
    P = params(C)
    inputs = [tuple(_g(t) for t in R.random_tokens(N, cnum, k, True, C)) for N, cnum, k in probs]
    res = run_group(C, probs, inputs, P)
    for i, (N, cnum, k) in enumerate(probs):
        check_problem(res[i], inputs[i][1], inputs[i][2], N, cnum, k, P, f"{name}[{i}] N{N} c{cnum} k{k}", edges=R.edge_samples(cnum))
    craft = [R.crafted(N, k, cnum) for N, cnum, k in probs]
    g = torch.Generator().manual_seed(R.SEED)
    inputs = [(_g(torch.randn(16, N, C, generator=g)), _g(c[2]), _g(c[3])) for (N, cnum, k), c in zip(probs, craft)]
    over = [(_g(c[0]), _g(c[1])) for c in craft]
    res = run_group(C, probs, inputs, P, overwrite=over)
    res2 = run_group(C, probs, inputs, P, overwrite=over)
    for i, (N, cnum, k) in enumerate(probs):
        label = f"{name}[{i}] crafted N{N} c{cnum} k{k}"
        assert torch.equal(res[i]["dist"], over[i][0]) and torch.equal(res[i]["smax"], over[i][1]), label
        check_problem(res[i], inputs[i][1], inputs[i][2], N, cnum, k, P, label, own_matrix=False, all_decided=True)
        assert torch.equal(res[i]["assign"], res2[i]["assign"]) and torch.equal(res[i]["merged_pb"], res2[i]["merged_pb"]), label


@pytest.mark.parametrize("name,C,masked,probs", UNMASKED, ids=[g[0] for g in UNMASKED])
def test_grouped_fused_stage(name, C, masked, probs):
    """Front and back in one kernel: random tokens, then token sets with runs of bit-identical rows (the fused forms take no
    matrix: ties reach them through their own distances)."""
    P = params(C)
    inputs = [tuple(_g(t) for t in R.random_tokens(N, cnum, k, False, C)) for N, cnum, k in probs]
    res = run_group(C, probs, inputs, P)
    for i, (N, cnum, k) in enumerate(probs):
        check_problem(res[i], None, inputs[i][2], N, cnum, k, P, f"{name}[{i}] N{N} c{cnum} k{k}")
    rep = [R.repeated_rows(R.batch_of(N), N, C, 10 * N + k) for N, cnum, k in probs]
    inputs = [(_g(x), None, _g(nz)) for x, nz in rep]
    res = run_group(C, probs, inputs, P)
    res2 = run_group(C, probs, inputs, P)
    for i, (N, cnum, k) in enumerate(probs):
        label = f"{name}[{i}] repeated rows N{N} c{cnum} k{k}"
        ids_x, ids_xn = R.row_ids(rep[i][0]), R.row_ids(res[i]["xn"].cpu())
        assert torch.equal(ids_x[:, :, None] == ids_x[:, None, :], ids_xn[:, :, None] == ids_xn[:, None, :]), label
        check_problem(res[i], None, inputs[i][2], N, cnum, k, P, label)
        assert torch.equal(res[i]["assign"], res2[i]["assign"]) and torch.equal(res[i]["merged_pb"], res2[i]["merged_pb"]), label
        assert torch.equal(res[i]["dist"], res2[i]["dist"]), label
