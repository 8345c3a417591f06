"""CPU: the similarity forward's fp64 restatement (tests/simfwd_ref.py) checked against itself, the launch-form table pinned
through nr_local_level_plan (host only: no GPU needed), nr_local_level_tiles held to the plan's tiling, every stored figure of
the operand bars recomputed, and every condition the GPU tests (tests/test_simfwd_gpu.py) put on their inputs asserted on the
reference alone."""
import functools

import pytest
import torch

import nr_oracle as O
import simfwd_ref as R
from neighborretr_amd import hip
from util import golden, params, problem

PREC = {"bf16": hip.PREC_BF16, "x3": hip.PREC_BF16X3}


def test_restatement_equals_a_pair_by_pair_loop_ties_included():
    """3 x 4 samples of 5 x 4 tokens, d = 64: `forward` on the exact inputs, on one and on three operand terms, and on the tie
    tier's operands, against the same sums pair by pair in Python doubles with a strict `>` scan for the first maximum.
    Values to 1e-12 (on the tie tier: equal), indices equal wherever the maximum is attained once -- and on the tie tier, whose
    sums are exact in any order, everywhere."""
    case = (5, 4, 3, 4, 64, "x3")
    x = R.make_inputs(case)
    Nt, Nv, A, Bv, d, _ = case
    sets = [R.exact_terms(x["t"], x["tm"], x["v"], x["vm"])]
    sets += [R.operand_terms(*x["planes"], A, Nt, Bv, Nv, three) for three in (False, True)]
    for terms in sets:
        got, ref = R.forward(terms, x["w_t"], x["w_v"]), R.naive(terms, x["w_t"], x["w_v"])
        for k in ("S", "pmax", "qmax"):
            assert (got[k] - ref[k]).abs().max() < 1e-12, k
        # masked tokens tie at an exact 0 in fp64 as well: the first index there, in both
        assert torch.equal(got["arg_v"], ref["arg_v"]) and torch.equal(got["arg_t"], ref["arg_t"])
    e = R.make_exact_inputs(case)
    terms = R.operand_terms(*e["planes"], A, Nt, Bv, Nv, True)
    got, ref = R.forward(terms, e["w_t"], e["w_v"]), R.naive(terms, e["w_t"], e["w_v"])
    for k in ("S", "pmax", "qmax", "arg_v", "arg_t"):
        assert torch.equal(got[k], ref[k]), k
    ties = (R.forward(terms, e["w_t"], e["w_v"], keep_R=True)["R"] == got["pmax"][..., None]).sum(-1)
    assert int((ties > 1).sum()) > 10                               # the scan's tie rule was exercised


def test_restatement_against_the_oracle_and_its_golden_S():
    """The golden case c1_b16 (16 x 16 samples, 24 x 12 tokens, d = 512).  With the oracle's own fp64 token weights the exact
    tier equals the oracle's fp64 S and pooled maxima to 1e-12; with the golden file's fp32 weights it is within 1e-6 of the
    reference model's fp32 S (half of the split-bf16 bar the kernels are held to against that file)."""
    gd = golden("c1_b16")
    x = problem(1001, 16, 24, 12, 128)
    terms = R.exact_terms(x["text_feat"], x["text_mask"], x["video_feat"], x["video_mask"])
    got = R.forward(terms, torch.from_numpy(gd["w_t"]), torch.from_numpy(gd["w_v"]))
    assert (got["S"] - torch.from_numpy(gd["S"]).double()).abs().max() < 1e-6
    P = {k: v.double() for k, v in params().items()}
    S, t2v, v2t, w_t, w_v, _, _ = O.local_level_parts(x["text_feat"].double(), x["video_feat"].double(), x["text_mask"],
                                                      x["video_mask"], P)
    got = R.forward(terms, w_t, w_v)
    assert (got["S"] - S).abs().max() < 1e-12
    assert ((got["pmax"] * w_t[:, None, :]).sum(-1) - t2v).abs().max() < 1e-12
    assert ((got["qmax"] * w_v[None]).sum(-1) - v2t).abs().max() < 1e-12
    assert (got["rowsum"] - S.sum(1)).abs().max() < 1e-12 and (got["colsum"] - S.sum(0)).abs().max() < 1e-12


def test_local_level_plan_no_gpu_needed():
    """nr_local_level_plan (host only): the plan of every row of simfwd_ref.FORMS.  Editing a row, or a picker, fails here."""
    for Nt, Nv, A, Bv, d, p, plan in R.FORMS:
        assert hip.local_level_plan(A, Nt, Bv, Nv, d, PREC[p]) == plan, (Nt, Nv, A, Bv, d, p)
    assert len({c[:6] for c in R.FORMS}) == len(R.FORMS)
    words = (hip.ctypes.c_int32 * hip.LLP_WORDS)(*([-7] * hip.LLP_WORDS))
    lib = hip.lib()
    for args in ((0, 24, 4, 12, 128, 0), (4, 24, 0, 12, 128, 0), (4, 0, 4, 12, 128, 0), (4, 24, 4, 0, 128, 0), (4, 24, 4, 12, 96, 0),
                 (4, 24, 4, 12, 0, 0), (4, 24, 4, 12, 128, 2)):
        assert lib.nr_local_level_plan(*args, words) == hip.NR_EINVAL, args
    assert lib.nr_local_level_plan(4, 24, 4, 12, 128, 0, None) == hip.NR_EINVAL
    assert lib.nr_local_level_plan(4, 256, 4, 12, 128, 0, words) == hip.NR_EUNSUPPORTED      # arg-max indices are u8
    assert lib.nr_local_level_plan(90, 1, 90, 1, 128, 0, words) == hip.NR_EUNSUPPORTED
    assert list(words) == [-7] * hip.LLP_WORDS                       # untouched by every refusal


def test_tiles_agree_with_the_plan_at_every_width():
    """nr_local_level_tiles takes no d; ops.local_level sizes the OUT_ROWSUM / OUT_COLSUM buffers by it.  For every row of the
    table at d = 64, 128 and 512 it reports exactly the plan's grid, and the grid is the plan's texts x videos per block -- so no
    launch writes partial sums in another tiling than the buffer was sized for."""
    for Nt, Nv, A, Bv, _, p, _ in R.FORMS:
        for d in (64, 128, 512):
            plan = hip.local_level_plan(A, Nt, Bv, Nv, d, PREC[p])
            if plan is None:
                continue
            texts, videos, cols, rows = plan[6:10]
            assert (rows, cols) == (-(-A // texts), -(-Bv // videos)), (Nt, Nv, A, Bv, d, p, plan)
            assert hip.local_level_tiles(A, Nt, Bv, Nv, PREC[p]) == (rows, cols), (Nt, Nv, A, Bv, d, p, plan)


def test_the_lds_kernel_never_runs_a_64_row_extent():
    """nr_pick_extent's tie rule (2 floor(64 / n) <= floor(128 / n): 128 rows waste no more than 64, and the larger extent wins a
    tie) never returns 64 rows, for any token count: of the nine (MI, NI) instances of nr_sim_kernel the five with MI = 2 or NI = 2
    are unreachable, and FORMS holds the other four."""
    seen = set()
    for n in range(1, 129):
        a, b = hip.local_level_plan(2, n, 2, 5, 64, 0), hip.local_level_plan(2, 5, 2, n, 64, 0)
        assert a[0] == b[0] == "lds" and a[1] in (96, 128) and b[2] in (96, 128), n
        seen |= {a[1], b[2]}
    assert seen == {96, 128}
    live = {c[6][1:3] for c in R.FORMS if c[6] is not None and c[6][0] == "lds"}
    assert live == {(96, 96), (96, 128), (128, 96), (128, 128)}


@functools.lru_cache(maxsize=None)
def _measured():
    twin = {p: [0.0, 0.0] for p in PREC}
    bound = {}
    for case in R.CASES:
        p, d = case[5], case[4]
        e_R, e_S, b_R, b_S = R.measure(case)
        twin[p] = [max(twin[p][0], e_R), max(twin[p][1], e_S)]
        old = bound.get((p, d), (0.0, 0.0))
        bound[(p, d)] = (max(old[0], b_R), max(old[1], b_S))
    return twin, bound


def test_every_stored_bar_recomputed():
    """The twin (plain fp32, sequential sums, CPU) against fp64 on the operand planes of EVERY GPU case: each stored figure is at
    least its measurement and at most twice it; no bar is looser than today's; every width of the table has its bound."""
    twin, bound = _measured()
    assert set(bound) == set(R.BOUND) and set(twin) == set(R.TWIN)
    for p in twin:
        for k in (0, 1):
            assert twin[p][k] <= R.TWIN[p][k] <= 2 * twin[p][k], (p, k, twin[p][k], R.TWIN[p][k])
    for key in bound:
        for k in (0, 1):
            assert bound[key][k] <= R.BOUND[key][k] <= 2 * bound[key][k], (key, k, bound[key][k], R.BOUND[key][k])
        bar_R, bar_S = R.bars(*key)
        assert 0 < bar_R <= R.TODAY[key[0]] and 0 < bar_S <= R.TODAY[key[0]]
        assert bar_R <= R.BAR_FACTOR * R.TWIN[key[0]][0] and bar_S <= R.BAR_FACTOR * R.TWIN[key[0]][1]
    # the one-pass bars are what this tier is for: three orders of magnitude under the 1e-3 of the exact tier
    assert max(R.bars("bf16", d)[1] for d in (64, 128, 192, 512)) < 1e-6


# shapes whose last block is full on an axis because the form's threshold leaves no choice (256 x 256 blocks need A % 4 == 0) or
# because the issue's shape fills the grid exactly: (Nt, Nv, A, Bv) -> axes that are NOT ragged
FULL = {(64, 64, 64, 61): "rows", (64, 64, 31, 64): "cols", (24, 12, 92, 184): "both", (64, 64, 46, 46): "both",
        (24, 64, 92, 46): "both", (64, 12, 46, 184): "both", (128, 128, 3, 3): "both",
        (9, 20, 9, 11): "rows", (1, 1, 5, 7): "both"}          # (one block of all 9 texts; one block of everything)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(map(str, c)))
def test_input_conditions_of_the_random_tier(case):
    """One fully masked text and video (an exact-zero row and column of S), every other sample with a live first token, the
    last sample (the ragged block's) live; ragged last blocks on both axes but for FULL; the operand
    products stay inside (-1, 1) with both signs, so an absolute bar means the same in every case."""
    Nt, Nv, A, Bv, d, p = case
    plan = dict((c[:6], c[6]) for c in R.FORMS)[case]
    texts, videos = plan[6:8]
    x = R.make_inputs(case)
    ma, mb = R.masked_samples(A, Bv)
    assert ma is not None and mb is not None and ma < A - 1 and mb < Bv - 1
    for m, blank, n in ((x["tm"], ma, A), (x["vm"], mb, Bv)):
        live = m.sum(-1)
        assert int(live[blank]) == 0 and int((live == 0).sum()) == 1
        assert bool((m[live > 0][:, 0] == 1).all()) and int(live[n - 1]) > 0
    full = FULL.get((Nt, Nv, A, Bv), "")
    assert (A % texts != 0) == (full not in ("rows", "both")), (A, texts)
    assert (Bv % videos != 0) == (full not in ("cols", "both")), (Bv, videos)
    hi_t, lo_t, hi_v, lo_v = x["planes"]
    assert float(R.bf16_bits(hi_t).float().view(A, Nt, d)[ma].abs().max()) == 0.0
    assert float(R.bf16_bits(lo_v).float().view(Bv, Nv, d)[mb].abs().max()) == 0.0
    sa, sb = R.subsample(A), R.subsample(Bv)
    terms = [(T[sa], V[sb]) for T, V in R.operand_terms(*x["planes"], A, Nt, Bv, Nv, p == "x3")]
    ref = R.forward(terms, x["w_t"][sa], x["w_v"][sb], keep_R=True)
    assert float(ref["R"].abs().max()) < 1.0 and float(ref["R"].min()) < -0.01 and float(ref["R"].max()) > 0.01
    assert float(ref["S"][sa.index(ma)].abs().max()) == 0.0 and float(ref["S"][:, sb.index(mb)].abs().max()) == 0.0
    assert (x["w_t"].sum(-1) - 1).abs().max() < 1e-6 and (x["w_v"].sum(-1) - 1).abs().max() < 1e-6


@pytest.mark.parametrize("case", R.one_case_per_form(), ids=lambda c: "-".join(map(str, c)))
def test_input_conditions_of_the_tie_tier(case):
    """The tie tier's claims: lo planes all zero, hi planes equal to the inputs; the fp32 twin equals fp64 bit for bit (products,
    maxima, S) -- the sums are exact in an order that is not the reference's; the fp32 sum of a whole row and column of S is
    exact too; and the all-negative pairs exist: text 0 against video 0 (and the last against the last) have every live product
    negative, two or more masked tokens on each side, every pooled maximum an exact 0 and its first index the first masked
    token."""
    Nt, Nv, A, Bv, d, p = case
    x = R.make_exact_inputs(case)
    hi_t, lo_t, hi_v, lo_v = x["planes"]
    assert int(lo_t.abs().max()) == 0 and int(lo_v.abs().max()) == 0
    assert torch.equal(R.bf16_bits(hi_t).float().view(A, Nt, d), x["t"] * x["tm"][..., None])
    assert torch.equal(R.bf16_bits(hi_v).float().view(Bv, Nv, d), x["v"] * x["vm"][..., None])
    assert int((x["t"] != 0).sum(-1).max()) <= 8 and int((x["v"] != 0).sum(-1).max()) <= 8
    assert torch.equal((x["w_t"] * 64).round() / 64, x["w_t"]) and float(x["w_t"].max()) <= 4 / 64
    sa, sb = R.subsample(A), R.subsample(Bv)
    terms = [(T[sa], V[sb]) for T, V in R.operand_terms(*x["planes"], A, Nt, Bv, Nv, p == "x3")]
    ref = R.forward(terms, x["w_t"][sa], x["w_v"][sb], keep_R=True)
    tw = R.twin(terms, x["w_t"][sa], x["w_v"][sb])
    for k in ("R", "pmax", "qmax", "S"):
        assert torch.equal(tw[k].double(), ref[k]), k
    assert float(ref["S"].abs().max()) <= (Nt + Nv) / 64 and max(A, Bv) * (Nt + Nv) / 64 * 2 ** 13 <= 2 ** 24
    if Nt > 2 and Nv > 2:
        for a, b in ((0, 0), (A - 1, Bv - 1)):
            lt, lv = int(x["tm"][a].sum()), int(x["vm"][b].sum())
            assert 1 <= lt <= Nt - 2 and 1 <= lv <= Nv - 2
            i, j = sa.index(a), sb.index(b)
            assert float(ref["R"][i, j, :lt, :lv].max()) < 0
            assert float(ref["pmax"][i, j].abs().max()) == 0.0 and float(ref["qmax"][i, j].abs().max()) == 0.0
            assert ref["arg_v"][i, j, :lt].tolist() == [lv] * lt and ref["arg_v"][i, j, lt:].tolist() == [0] * (Nt - lt)
            assert ref["arg_t"][i, j, :lv].tolist() == [lt] * lv and ref["arg_t"][i, j, lv:].tolist() == [0] * (Nv - lv)
