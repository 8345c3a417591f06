"""The correction records of the evaluator and correction_from_args, which both eval_epoch callers read their flags through: what
a record holds, the one-correction rule, every refused value, and an empty querybank refused before anything is scored."""
from types import SimpleNamespace

import pytest
import torch

from neighborretr_amd import evaluator

NS = SimpleNamespace


def _stub(bank_items=0):
    """A model that cannot score: whatever reaches get_similarity_logits has gone past the checks."""
    def get_similarity_logits(self, *a, **kw):
        raise AssertionError("the slab was scored")
    feat, mask = torch.zeros((bank_items, 2, 8)), torch.zeros((bank_items, 2))
    return type("M", (), dict(mb_feat_t=feat, mb_feat_v=feat, mb_mask_t=mask, mb_mask_v=mask, precision="bf16",
                              get_similarity_logits=get_similarity_logits))()


def test_without_flags_there_is_no_correction_and_the_defaults_go_to_the_driver():
    for args in (NS(), NS(test_norm="none", local_scaling=None, mutual_proximity="none", hubness_k=None, bootstrap=None, ir_metrics=None)):
        correction, kw = evaluator.correction_from_args(args, None)
        assert correction is None
        assert kw == dict(bootstrap=0, bootstrap_seed=0, bootstrap_level=0.95, ir=False, hubness_k=0)
    _, kw = evaluator.correction_from_args(NS(hubness_k=5, bootstrap=200, bootstrap_seed=3, bootstrap_level=0.9, ir_metrics=1), None)
    assert kw == dict(bootstrap=200, bootstrap_seed=3, bootstrap_level=0.9, ir=True, hubness_k=5) and kw["ir"] is True


def test_a_test_norm_record_holds_the_label_and_the_entry():
    for mode in evaluator.TEST_NORM_MODES:
        c, _ = evaluator.correction_from_args(NS(test_norm=mode, test_norm_beta=12.5, qb_k=3, test_norm_iters=7), _stub(4))
        assert c.key == "test_norm" and c.needs_bank == (mode in ("qbnorm", "qbsinkhorn"))
        assert c.label == evaluator.test_norm_label(mode, 12.5, 7)
        assert c.entry == (dict(mode=mode, beta=12.5, qb_k=3) if mode == "qbnorm" else dict(mode=mode, beta=12.5))
        assert c == evaluator.test_norm_correction(mode, 12.5, 3, 7)._replace(apply=c.apply)
    c, _ = evaluator.correction_from_args(NS(test_norm="sinkhorn"), None)      # the defaults of the flags
    assert c.label == "[Sinkhorn b=20 it=50]" and c.entry == dict(mode="sinkhorn", beta=20.0)
    assert evaluator.correction_from_args(NS(test_norm="is"), None)[0].label == "[IS b=20]"


def test_a_local_scaling_record_holds_the_label_and_the_entry():
    for mode in evaluator.LOCAL_SCALING_MODES:
        for bank in (0, 1):
            c, _ = evaluator.correction_from_args(NS(local_scaling=mode, local_scaling_k=7, local_scaling_bank=bank), _stub(4))
            assert c.key == "local_scaling" and c.needs_bank is bool(bank)
            assert c.label == evaluator.local_scaling_label(mode, 7, bool(bank))
            assert c.entry == dict(mode=mode, k=7, bank=bool(bank)) and c.entry["bank"] is bool(bank)
    c, _ = evaluator.correction_from_args(NS(local_scaling="csls"), None)
    assert c.label == "[CSLS k=10]" and c.entry == dict(mode="csls", k=10, bank=False)


def test_a_mutual_proximity_record_holds_the_label_and_the_entry():
    for mode in evaluator.MUTUAL_PROXIMITY_MODES:
        for bank in (0, 1):
            c, _ = evaluator.correction_from_args(NS(mutual_proximity=mode, mutual_proximity_bank=bank), _stub(4))
            assert c.key == "mutual_proximity" and c.needs_bank is bool(bank)
            assert c.label == evaluator.mutual_proximity_label(mode, bool(bank))
            assert c.entry == dict(mode=mode, bank=bool(bank)) and c.entry["bank"] is bool(bank)


def test_two_corrections_at_once_are_refused():
    three = "mutual_proximity, local_scaling and test_norm are separate corrections: choose one of them"
    two = "local_scaling and test_norm are separate corrections: choose one of them"
    for args, text in ((NS(mutual_proximity="emp", test_norm="is"), three), (NS(mutual_proximity="gauss", local_scaling="csls"), three),
                       (NS(mutual_proximity="emp", test_norm="sinkhorn", local_scaling="ls"), three),
                       (NS(local_scaling="csls", test_norm="is"), two)):
        with pytest.raises(ValueError) as err:
            evaluator.correction_from_args(args, None)                          # no model: nothing may be touched
        assert str(err.value) == text


BAD = ([NS(test_norm="ISX"), NS(test_norm="is", qb_k=0), NS(test_norm="qbnorm", qb_k=129), NS(test_norm="dsl", hubness_k=129)]
       + [NS(test_norm="is", test_norm_beta=beta) for beta in (0.0, -2.0, float("inf"), float("nan"))]
       + [NS(test_norm="sinkhorn", test_norm_iters=it) for it in (0, -3, 2.5, True)]
       + [NS(local_scaling=mode) for mode in ("is", "mp")]
       + [NS(local_scaling="csls", local_scaling_k=k) for k in (0, 129, True, -1, 2.5)] + [NS(local_scaling="csls", hubness_k=129)]
       + [NS(mutual_proximity=mode) for mode in ("is", "csls", "mp")] + [NS(mutual_proximity="emp", hubness_k=129)]
       + [NS(hubness_k=129)]
       + [NS(bootstrap=b) for b in (-1, (1 << 20) + 1, 2.5, "10", True)]
       + [NS(bootstrap=10, bootstrap_seed=s) for s in (-1, (1 << 64) - 1, 0.5)]
       + [NS(bootstrap=10, bootstrap_level=level) for level in (0, 1, 0.0, 1.0, -0.1, 95, "0.9", None)]
       + [NS(ir_metrics=ir) for ir in (2, -1, 0.5, 1.0, "1", "yes", [1])])


@pytest.mark.parametrize("args", BAD, ids=lambda a: ",".join(f"{k}={v}" for k, v in vars(a).items()))
def test_every_value_the_checks_refuse_is_refused_from_the_flags_too(args):
    with pytest.raises(ValueError):
        evaluator.correction_from_args(args, None)                              # no model: nothing may be touched


def test_the_constructors_refuse_what_the_checks_refuse():
    for bad in (("ISX", 20.0, 1, 50), ("is", 0.0, 1, 50), ("is", 20.0, 0, 50), ("qbnorm", 20.0, 129, 50), ("sinkhorn", 20.0, 1, 0)):
        with pytest.raises(ValueError, match="test_norm|beta|k must"):
            evaluator.test_norm_correction(*bad)
    for bad in (("is", 10), ("csls", 0), ("csls", 129), ("csls", True)):
        with pytest.raises(ValueError):
            evaluator.local_scaling_correction(*bad)
    for bad in ("is", "csls", "", None):
        with pytest.raises(ValueError, match="mutual_proximity"):
            evaluator.mutual_proximity_correction(bad)


def test_an_empty_querybank_is_refused_before_anything_is_scored():
    z = torch.zeros((4, 2, 8))
    for args in (NS(test_norm="qbnorm"), NS(test_norm="qbsinkhorn"), NS(local_scaling="nicdm", local_scaling_bank=1),
                 NS(mutual_proximity="gauss", mutual_proximity_bank=1)):
        with pytest.raises(ValueError, match="load_memory_bank"):
            evaluator.correction_from_args(args, _stub(0))
        correction, kw = evaluator.correction_from_args(args, _stub(4))          # a filled bank: the record, nothing scored yet
        assert correction.needs_bank
        with pytest.raises(ValueError, match="load_memory_bank"):               # the driver itself: the bank's error, not the scorer's
            evaluator.sharded_evaluation(_stub(0), z, z, z[..., 0], z[..., 0], NS(world_size=1), correction, **kw)
    with pytest.raises(AssertionError, match="the slab was scored"):            # the stub does raise once the checks are passed
        evaluator.sharded_evaluation(_stub(0), z, z, z[..., 0], z[..., 0], NS(world_size=1))
