"""CPU: the host side of the one-pass fp16 precision (NR_PREC_F16 = 3; no GPU needed).

The fp16 forms are picked exactly as one bf16 pass is, so for every row of simfwd_ref.FORMS / scorer_ref.FORMS the plan call
for PREC_F16 must report the row's one-pass bf16 plan -- or refuse (None) where no fp16 kernel is built for that block: the
similarity builds fp16 only on the blocks the BASELINE configs' batch x batch products reach (96 x 96 at 24 x 12 tokens,
192 x 384, 256 x 256), never on the LDS kernel; the scorer builds it on every one-pass block."""
import ctypes
import importlib.util
import os

import pytest

import scorer_ref as SR
import simfwd_ref as FR
from neighborretr_amd import head, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_BLOCKS = {(24, 12, 96, 96), (24, 12, 192, 384), (64, 64, 256, 256)}      # (Nt, Nv, block rows, block columns)


def test_abi_and_constants():
    assert hip.version() == 5 and hip.PREC_F16 == 3 and head.PREC_MIXED == 2
    for name in ("nr_prepare_tokens_f16", "nr_prepare_tokens_pair_f16", "nr_split_f16"):
        assert name in hip.exported_symbols() and hasattr(hip.lib(), name)
    assert head.precision_plan(head.PREC_MIXED) == (hip.PREC_F16, hip.PREC_F16, hip.PREC_BF16)
    assert head.backward_plan(head.PREC_MIXED) == (hip.PREC_BF16X3, hip.PREC_BF16X3, hip.PREC_BF16)
    for p in (hip.PREC_BF16, hip.PREC_BF16X3):
        assert head.precision_plan(p) == (p, p, p) == head.backward_plan(p)


@pytest.mark.parametrize("row", [r for r in FR.FORMS if r[5] == "bf16"], ids=lambda r: "x".join(str(v) for v in r[:5]))
def test_similarity_plan_is_the_one_pass_bf16_plan_or_a_refusal(row):
    Nt, Nv, A, Bv, d, _, plan = row
    assert hip.local_level_plan(A, Nt, Bv, Nv, d, hip.PREC_BF16) == plan             # (the pinned table itself has not moved)
    built = plan is not None and plan[0] == "reg" and (Nt, Nv, plan[1], plan[2]) in F16_BLOCKS
    assert hip.local_level_plan(A, Nt, Bv, Nv, d, hip.PREC_F16) == (plan if built else None)
    if plan is not None:
        assert hip.local_level_tiles(A, Nt, Bv, Nv, hip.PREC_F16) == hip.local_level_tiles(A, Nt, Bv, Nv, hip.PREC_BF16)


def test_every_fp16_block_is_reached_by_a_row():
    seen = {(r[0], r[1], r[6][1], r[6][2]) for r in FR.FORMS if r[5] == "bf16" and r[6] is not None and r[6][0] == "reg"}
    assert F16_BLOCKS <= seen


@pytest.mark.parametrize("row", [r for r in SR.FORMS if "bf16" in r[1]], ids=lambda r: f"{r[0]}-{r[2]}x{r[3]}")
def test_scorer_plan_is_the_one_pass_bf16_plan(row):
    call, _, n, N, form = row
    fused = N if call == "fused" else 0
    assert hip.token_scorer_plan(n * N, 1024, hip.PREC_BF16, fused) == form
    assert hip.token_scorer_plan(n * N, 1024, hip.PREC_F16, fused) == form
    if call == "unfused":
        assert hip.token_scorer_plan(n * N, 1024, hip.PREC_F16, N) is None


def test_shape_aware_plan_follows_the_plan_calls():
    # BASELINE configs[1] / [2] / [3] batch sides and a small batch: fp16 everywhere
    for B, Nt, Nv in ((128, 24, 12), (1024, 24, 12), (128, 64, 64), (16, 24, 12)):
        assert head.precision_plan(head.PREC_MIXED, (B, Nt, Nv, 512, 1024)) == (hip.PREC_F16, hip.PREC_F16, hip.PREC_BF16)
    # shapes whose product has no fp16 kernel keep split-bf16 there (the scorer still has one)
    for B, Nt, Nv in ((8, 64, 64), (16, 24, 64), (16, 7, 5), (240, 24, 12)):
        assert hip.local_level_plan(B, Nt, B, Nv, 512, hip.PREC_F16) is None
        assert head.precision_plan(head.PREC_MIXED, (B, Nt, Nv, 512, 1024)) == (hip.PREC_BF16X3, hip.PREC_F16, hip.PREC_BF16)


def test_entry_points_refuse_on_the_host():
    """Argument checks that answer before any launch: nr_local_level_cand keeps refusing 2 and 3; the fp16 similarity refuses a
    shape that would run the LDS kernel; the grouped scorer refuses an fp16 set; the backward's hidden layer knows bf16 only."""
    lib = hip.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    for prec in (2, 3):
        assert lib.nr_local_level_cand(p, p, p, p, p, p, 2, 24, 3, 12, 512, prec, p, 4, p, None) == hip.NR_EINVAL
    assert lib.nr_local_level_fwd(p, None, p, None, p, p, 33, 3, 17, 6, 128, hip.PREC_F16, 0, p, None, None, None, None, None) == hip.NR_EUNSUPPORTED
    assert lib.nr_local_level_fwd(p, None, p, None, p, p, 121, 24, 241, 12, 128, hip.PREC_F16, 0, p, None, None, None, None, None) == hip.NR_EUNSUPPORTED
    assert lib.nr_local_level_fwd(p, None, p, None, p, p, 4, 24, 4, 12, 128, 2, 0, p, None, None, None, None, None) == hip.NR_EINVAL
    q = (hip.TokenWeightsProblem * 1)()
    for f in ("tok_hi", "norm", "w1_hi", "b1", "w2", "b2", "logit_part", "counters", "w"):
        setattr(q[0], f, p)
    q[0].n_samples, q[0].N, q[0].d, q[0].H, q[0].n_counters = 8, 24, 512, 1024, 64
    precs = (ctypes.c_int * 1)(hip.PREC_F16)
    assert lib.nr_token_weights_fwd_group(q, precs, 1, None) == hip.NR_EUNSUPPORTED
    assert lib.nr_token_mlp_bwd_hidden(p, p, p, 64, 512, p, p, p, p, 1024, hip.PREC_F16, p, p, p, 64, 0, None, None, p, p, p, None) == hip.NR_EINVAL
    assert lib.nr_prepare_tokens_f16(None, None, 4, 512, 1, p, None, p, None, None, None) == hip.NR_EINVAL
    assert lib.nr_split_f16(p, 0, p, None) == hip.NR_EINVAL


def test_probe_tool_on_c1_b16_stays_under_its_bar():
    spec = importlib.util.spec_from_file_location("prec_probe_f16", os.path.join(ROOT, "tools", "prec_probe_f16.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    shape, r = mod.probe_fixture("c1_b16")
    print(f"c1_b16 {shape}: max|dL| bf16 {r['dL_bf16']:.3g}, fp16 {r['dL_f16']:.3g}, fp16 flushed {r['dL_f16_ftz']:.3g}; operands {r['max_abs']}")
    assert r["finite"] == 5
    assert r["dL_f16"] <= mod.BAR == 5e-4 and r["dL_f16_ftz"] <= mod.BAR
    assert r["dL_bf16"] > mod.BAR                     # why one bf16 pass was never an option here
    assert max(r["max_abs"].values()) <= 1.0          # normalised tokens and scorer weights: far inside fp16's range
