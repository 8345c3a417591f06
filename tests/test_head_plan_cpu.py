"""CPU: the host-side decisions of the step's orchestration (neighborretr_amd/head.py) -- the plan table, the refusals and the
order in which the clustering's and the local branch's launches are interleaved.  The expected values are written out from the
rules, not computed by the functions under test."""
import contextlib

import pytest

from neighborretr_amd import head, hip

BF16, X3, F16, MIXED = hip.PREC_BF16, hip.PREC_BF16X3, hip.PREC_F16, head.PREC_MIXED
NT, NV, D, H, M = 24, 12, 512, 1024, 64

# (prec, keep) -> (p_bb, p_mlp, p_bank, f16_b, lo_b without / with prepared_out, lo_k).  The rules: the mixed plan is one fp16 pass
# on the batch side and one bf16 pass on the bank side; `keep` turns fp16 into split-bf16; the batch gets an fp16 plane when a
# batch-side launch is fp16, a lo plane for the backward, for any split-bf16 launch and -- on the fp16 plan -- for the bank's
# shadow (prepared_out); the bank gets a lo plane for the backward or a split-bf16 bank path.
PLAN = {
    (BF16, False): (BF16, BF16, BF16, False, False, False, False),
    (BF16, True): (BF16, BF16, BF16, False, True, True, True),
    (X3, False): (X3, X3, X3, False, True, True, True),
    (X3, True): (X3, X3, X3, False, True, True, True),
    (MIXED, False): (F16, F16, BF16, True, False, True, False),
    (MIXED, True): (X3, X3, BF16, False, True, True, True),
}
# split tail = loss-only, both stream sets given, B <= 128 and B % 4 == 0
SPLIT_TAIL_B = {6: False, 8: True, 128: True, 132: False, 256: False}


@pytest.mark.parametrize("B", sorted(SPLIT_TAIL_B))
def test_plan_table(B):
    # the premise of PLAN's mixed rows: at these token counts every B has an fp16 form of the product and of both scorers
    assert hip.local_level_plan(B, NT, B, NV, D, F16) is not None
    assert hip.token_scorer_plan(B * NT, H, F16, 0) is not None and hip.token_scorer_plan(B * NV, H, F16, 0) is not None
    for (prec, keep), (p_bb, p_mlp, p_bank, f16_b, lo_plain, lo_out, lo_k) in PLAN.items():
        for prepared_out in (False, True):
            for streams in (False, True):
                p = head.head_plan((B, NT, D), NV, (M, M), H, 4, prec, keep, prepared_out, streams)
                tag = (B, prec, keep, prepared_out, streams)
                assert (p.B, p.Nt, p.Nv, p.d, p.M, p.K, p.b, p.r0) == (B, NT, NV, D, M, 4, B, 0), tag
                assert (p.p_bb, p.p_mlp, p.p_bank) == (p_bb, p_mlp, p_bank), tag
                assert (p.f16_b, p.lo_b, p.lo_k) == (f16_b, lo_out if prepared_out else lo_plain, lo_k), tag
                assert p.split_tail is (SPLIT_TAIL_B[B] and streams and not keep), tag
                assert p.keep is keep, tag


def test_plan_without_an_fp16_product_and_the_sharded_demotion():
    # B = 8 at 64 x 64 tokens: no fp16 form of the product (tests/test_f16_cpu.py), the scorers have one
    assert hip.local_level_plan(8, 64, 8, 64, D, F16) is None
    p = head.head_plan((8, 64, D), 64, (M, M), H, 4, MIXED, prepared_out=True, side_streams=True)
    assert (p.p_bb, p.p_mlp, p.p_bank, p.f16_b, p.lo_b, p.lo_k, p.split_tail) == (X3, F16, BF16, True, True, False, True)
    # sharded: rank 1 of 2 owns rows [64, 128); both slab products have an fp16 form at B = 128 ...
    assert hip.local_level_plan(64, NT, 128, NV, D, F16) is not None and hip.local_level_plan(128, NT, 64, NV, D, F16) is not None
    p = head.head_plan((128, NT, D), NV, (M, M), H, 20, MIXED, side_streams=True, shard=(1, 2))
    assert (p.b, p.r0, p.p_bb, p.p_mlp, p.p_bank, p.f16_b, p.lo_b, p.lo_k) == (64, 64, F16, F16, BF16, True, False, False)
    # ... and neither at B = 256, where the whole product has one: that form's own demotion
    assert hip.local_level_plan(256, NT, 256, NV, D, F16) is not None and hip.local_level_plan(128, NT, 256, NV, D, F16) is None
    p = head.head_plan((256, NT, D), NV, (M, M), H, 20, MIXED, shard=(0, 2))
    assert (p.b, p.r0, p.p_bb, p.p_mlp, p.p_bank, p.f16_b, p.lo_b, p.lo_k) == (128, 0, X3, F16, BF16, True, True, False)


def test_refusals_keep_their_messages():
    plan = lambda B=16, K=4, bank=(M, M), **kw: head.head_plan((B, NT, D), NV, bank, H, K, BF16, **kw)      # noqa: E731
    with pytest.raises(ValueError, match=r"num_neighbors=17 > batch=16: the reference raises IndexError here \(until_module.py:119-123\)"):
        plan(K=17)
    for bank in ((0, 0), (M, 0), (M - 1, M)):
        with pytest.raises(ValueError, match="^empty or inconsistent memory bank$"):
            plan(bank=bank)
    with pytest.raises(ValueError, match="^gt / gv missing and no join callable to produce them$"):
        plan(global_tokens=False)
    with pytest.raises(ValueError, match="^the gathered batch must divide over the ranks$"):
        plan(B=18, K=40, shard=(0, 4))                      # (checked first)
    with pytest.raises(ValueError, match="^num_neighbors=17 > batch=16$"):
        plan(K=17, shard=(0, 2))
    with pytest.raises(ValueError, match="^gt / gv missing and no join callable to produce them$"):
        plan(global_tokens=False, shard=(0, 2))
    assert plan(K=16).K == 16 and plan(bank=(0, 0), shard=(0, 2)).M == 0     # (the sharded forward has never checked the bank)


def _interleaved(capture_order, n_clu, n_loc):
    """_interleave over two generators that log one entry per launch: (side, index, inside the local context?)."""
    log, inside = [], [False]

    def launches(side, n):
        for i in range(n):
            log.append((side, i, inside[0]))
            yield
        return side + " done"

    @contextlib.contextmanager
    def on_local():
        inside[0] = True
        try:
            yield
        finally:
            inside[0] = False
    produced = head._interleave(launches("c", n_clu), launches("l", n_loc), capture_order, on_local)
    assert produced == "c done"
    assert all(inside_ == (side == "l") for side, _, inside_ in log), log
    return " ".join(f"{side}{i}" for side, i, _ in log)


def test_interleaving_order():
    # the shipped order, 24 clustering and 7 local launches: 7 | 5 | 7 | the local branch to its end | the clustering's rest
    assert _interleaved(((7, 5), (7, 1 << 30)), 24, 7) == (
        "c0 c1 c2 c3 c4 c5 c6 l0 l1 l2 l3 l4 c7 c8 c9 c10 c11 c12 c13 l5 l6 c14 c15 c16 c17 c18 c19 c20 c21 c22 c23")
    # the last pair repeats; the local branch runs out first (its generator ends on the turn after its last launch)
    assert _interleaved(((2, 1), (1, 3)), 4, 5) == "c0 c1 l0 c2 l1 l2 l3 c3 l4"
    # the clustering runs out first: the local branch runs to its end in one turn
    assert _interleaved(((2, 1), (1, 3)), 2, 5) == "c0 c1 l0 l1 l2 l3 l4"
    # a single pair, nothing to interleave on one side
    assert _interleaved(((3, 2),), 0, 3) == "l0 l1 l2"
    assert _interleaved(((3, 2),), 5, 0) == "c0 c1 c2 c3 c4"


def test_exhaust_returns_the_generators_value():
    def gen():
        yield
        yield
        return 7
    assert head.exhaust(gen()) == 7
