"""The decision-exact DPC-KNN reference (tests/dpc_ref.py) held to the oracle, to an fp32 twin of the kernels' arithmetic and to
planted defects; the case list held to the planner.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import dpc_ref as R
import nr_oracle as O

CASES = R.all_random_inputs()                # (N, cnum, k, masked, C)
CRAFTED = R.crafted_cases()                  # (N, k, cnum)
_id = lambda c: "N%d-c%d-k%d-%s-C%d" % (c[0], c[1], c[2], "mask" if c[3] else "nomask", c[4])


@functools.lru_cache(maxsize=None)
def _case(case):
    N, cnum, k, masked, C = case
    x, mask, noise = R.random_tokens(*case)
    d = R.dist32_of(x)
    return x, mask, noise, d, R.assign_ref(d, mask, noise, k, cnum)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_assign_ref_agrees_with_the_oracle_on_decided_samples(case):
    N, cnum, k, masked, C = case
    x, mask, noise, d, ref = _case(case)
    want = O.dpc_knn(x.double(), cnum, k, None if mask is None else mask.double(), noise.double(), centre_ties="lowest_index")
    dec = ref.decided
    assert torch.equal(ref.assign[dec], want[dec])


def test_cap():
    """A condition on the reference alone: at most CAP of a random case's samples undecided, every named edge sample (one valid
    token, two, fewer than clusters, all) and every crafted sample decided."""
    worst = 0.0
    for case in CASES:
        N, cnum, k, masked, C = case
        ref = _case(case)[4]
        und = (~ref.decided).tolist()
        share = sum(und) / len(und)
        print(f"{_id(case):32s} undecided {sum(und)}/{len(und)}")
        worst = max(worst, share)
        assert share <= R.CAP, case
        if masked:
            assert all(not und[b] for b in R.edge_samples(cnum)), (case, und)
    print("largest undecided share", worst)
    for N, k, cnum in CRAFTED:
        dist, smax, mask, noise, names = R.crafted(N, k, cnum)          # (asserts that every sample is decided)
        assert torch.equal(smax, dist.flatten(1).max(-1)[0]) and torch.equal(dist, dist.transpose(1, 2))
        assert {"equal_row", "twin_rows", "same_bits", "equal_scores", "equidistant", "masked_nearest", "far", "all_zero",
                "far_in_knn"} <= set(names)


def test_the_fp32_twin_agrees_and_stays_inside_an_eighth_of_the_tolerances():
    """numpy float32 in the kernels' order of operations, with and without fused multiply-adds: the same assignment on decided
    samples; densities and scores within 1/8 of the sample's tolerance of the fp64 values (the pair tolerance: both sides)."""
    share_d = share_s = 0.0
    inputs = [(_case(c)[3], _case(c)[1], _case(c)[2], c[2], c[1], _case(c)[4]) for c in CASES]
    for N, k, cnum in CRAFTED:
        dist, _, mask, noise, _ = R.crafted(N, k, cnum)
        inputs.append((dist, mask, noise, k, cnum, R.assign_ref(dist, mask, noise, k, cnum)))
    for d, mask, noise, k, cnum, ref in inputs:
        for fma in (False, True):
            tw = R.twin32(d, mask, noise, k, cnum, fma=fma)
            dec = ref.decided
            assert torch.equal(tw.assign[dec], ref.assign[dec]), (k, cnum, fma)
            for got, want, tol in ((tw.density, ref.density, ref.tol_dens), (tw.score, ref.score, ref.tol_score)):
                want = want.numpy()
                rel = np.abs(got.astype(np.float64) - want) / np.where(want > 0, want, 1.0)
                assert (got[want == 0] == 0).all()
                if tol is ref.tol_score:
                    rel = rel[dec.numpy()]                  # (an undecided sample's parent entry may be another one)
                    tol = tol[dec]
                    if not len(rel):
                        continue
                sh = float((rel / tol.numpy()[:, None]).max())
                if got is tw.density:
                    share_d = max(share_d, sh)
                else:
                    share_s = max(share_s, sh)
    print(f"twin's largest share of the tolerance: density {share_d:.4f}, score {share_s:.4f}")
    assert share_d <= 1 / 8 and share_s <= 1 / 8


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_a_planted_defect_changes_a_decided_sample(defect):
    """The case list sees each defect: the twin with the defect assigns at least one decided sample differently -- in both of its
    forms, among the random cases or the crafted ones."""
    hits = {False: [], True: []}
    for fma in (False, True):
        for case in CASES:
            N, cnum, k, masked, C = case
            _, mask, noise, d, ref = _case(case)
            tw = R.twin32(d, mask, noise, k, cnum, fma=fma, defect=defect)
            bad = [b for b in range(d.shape[0]) if ref.decided[b] and not torch.equal(tw.assign[b], ref.assign[b])]
            if bad:
                hits[fma].append((_id(case), bad))
        for N, k, cnum in CRAFTED:
            dist, _, mask, noise, names = R.crafted(N, k, cnum)
            ref = R.assign_ref(dist, mask, noise, k, cnum)
            tw = R.twin32(dist, mask, noise, k, cnum, fma=fma, defect=defect)
            bad = [names[b] for b in range(len(names)) if not torch.equal(tw.assign[b], ref.assign[b])]
            if bad:
                hits[fma].append((f"crafted N{N} k{k} c{cnum}", bad))
    print(defect, "seen by", len(hits[False]), "/", len(hits[True]), "cases; first:", hits[False][:2])
    assert hits[False] and hits[True]


@pytest.mark.parametrize("C", sorted(R.DIST_FRAC))
def test_the_stored_share_of_the_distance_bound_is_the_twin_s(C):
    x = R.random_tokens(24, 4, 3, False, C)[0][:6]
    ref, rig, work = R.dist_ref(x)
    tw = R.dist_twin32(x)
    off = ~torch.eye(24, dtype=torch.bool)[None].expand_as(ref)
    frac = float(((tw.double() - ref).abs()[off] / rig[off]).max())
    print(f"C = {C}: the sequential twin uses {frac:.4f} of the rigorous bound (stored {R.DIST_FRAC[C]})")
    assert frac <= R.DIST_FRAC[C] <= 1.25 * frac
    assert ((tw.double() - ref).abs() <= work).all()


def test_merge_ref_of_an_all_padding_cluster_is_the_bias():
    g = torch.Generator().manual_seed(5)
    xn, pb = torch.randn(2, 6, 64, generator=g), torch.randn(64, generator=g)
    w = torch.tensor([[1.0, 2.0, 0.0, 0.0, 3.0, 0.0]] * 2)
    assign = torch.tensor([[0, 0, 1, 1, 2, 1]] * 2)
    share, mpb, A, merged = R.merge_ref(xn, w, assign, 4, pb)
    assert torch.equal(mpb[:, 1], pb.double().expand(2, 64)) and torch.equal(mpb[:, 3], pb.double().expand(2, 64))
    assert torch.allclose(share[0], torch.tensor([1 / 3, 2 / 3, 0, 0, 1, 0], dtype=torch.float64), atol=1e-6)
    want = O.merge_tokens(xn.double(), assign, 4, w.double())
    assert float((merged - want).abs().max()) < 1e-12


def test_planner_coverage():
    """What the grouped GPU cases reach, in the planner's own words: the first form with back_form 0, the second form with back
    forms 4 and 16 beside the kv GEMM, the fused kernel in its `few` and its 512-thread shape, the first form fused.  The second
    form's back half as a launch of its own (R.UNREACHABLE) is chosen for no shape: swept here, not forced."""
    from neighborretr_amd import hip
    P = hip.CTM_PLAN
    seen = set()
    for name, C, masked, probs in R.GROUPED:
        plan = hip.ctm_stage_plan([(R.batch_of(N), N, C, k, cnum, C // 64, masked, False) for N, cnum, k in probs])
        assert plan is not None, name
        word = (plan[P["form"]], plan[P["back"]], plan[P["back_form"]], plan[P["front_threads"]], plan[P["back_use_lds"]])
        print(f"{name:18s} form {word[0]}  back {('none', 'alone', 'beside kv')[word[1]]:9s}  back_form {word[2]:2d}  "
              f"front threads {word[3]:4d}  back rows in LDS {word[4]}")
        seen.add(word[:4])
        assert (plan[P["back"]] == hip.CTM_BACK_NONE) == (not masked)
    for want in ((1, hip.CTM_BACK_BESIDE_KV, 0, 1024), (2, hip.CTM_BACK_BESIDE_KV, 4, 512), (2, hip.CTM_BACK_BESIDE_KV, 16, 512),
                 (2, hip.CTM_BACK_NONE, 0, 256), (2, hip.CTM_BACK_NONE, 0, 512), (1, hip.CTM_BACK_NONE, 0, 256),
                 (1, hip.CTM_BACK_NONE, 0, 1024)):
        assert want in seen, (want, seen)
    for N in range(1, 65):
        for cnum in range(1, min(N, 16) + 1):
            plan = hip.ctm_stage_plan([(4, N, 512, 1, cnum, 8, True, False)])
            if plan is not None and plan[P["form"]] == 2:
                assert plan[P["back"]] == hip.CTM_BACK_BESIDE_KV, (N, cnum)
    print("never chosen:", ", ".join(R.UNREACHABLE))
