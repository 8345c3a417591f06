"""The non-finite step guard without a GPU: the restatement (tests/nonfinite_ref.py) against sequences worked by hand, the
argument checks of nr_bertadam_step_guarded on the host, and the flag / constructor validation."""
import ctypes
import math

import numpy as np
import pytest
import torch

import bertadam_ref as R
import nonfinite_ref as NF
from neighborretr_amd import hip, optim, training


def _state():
    groups = [dict(lr=1e-3, weight_decay=0.0, schedule="warmup_cosine", warmup=0.25, t_total=8, b2=0.98)]
    return R.State([np.array([1.0, 2.0, 3.0]), np.array([4.0])], [0, 0], groups)


GOOD = [np.array([3.0, 0.0, 4.0], np.float32), np.array([12.0], np.float32)]          # total 169: norm 13


def _bad(value, tensor=0):
    g = [x.copy() for x in GOOD]
    g[tensor][-1] = value
    return g


def test_good_bad_bad_good_by_hand():
    st, guard = _state(), NF.Guard(n_ring=2)
    before = None
    outcomes = []
    for k, grads in enumerate([GOOD, _bad(np.nan), _bad(np.inf, 1), GOOD]):
        if k == 1:
            before = ([x.copy() for x in st.p], [x.copy() for x in st.m], [x.copy() for x in st.v], list(st.step))
        outcomes.append(NF.guarded_step(st, guard, grads, global_max_norm=1.0, losses=(0.5 * k, 7.0)))
        if k in (1, 2):                                      # a bad step changes nothing
            for got, want in zip((st.p, st.m, st.v), before[:3]):
                assert all(np.array_equal(a, b) for a, b in zip(got, want))
            assert st.step == before[3] == [1, 1]
    assert outcomes == [False, True, True, False]
    assert guard.stats() == dict(attempts=4, skipped=2, consecutive=0, max_consecutive=2, last_skipped=2)
    assert st.step == [2, 2]
    # n_ring = 2: attempts 2 and 3 are left, oldest first, in slots 0 and 1
    recs = guard.records()
    assert [r["attempt"] for r in recs] == [2, 3] and [r["skipped"] for r in recs] == [1, 0]
    assert guard.ring[0] is recs[0] and guard.ring[1] is recs[1]
    assert math.isinf(recs[0]["grad_norm"]) and recs[0]["clip"] == 0.0          # 1 / (inf + 1e-6)
    assert recs[1]["grad_norm"] == np.float32(13.0) and recs[1]["clip"] == np.float32(1.0 / (13.0 + 1e-6))
    assert recs[1]["losses"] == [np.float32(1.5), np.float32(7.0)] + [np.float32(0)] * 6
    # the two good steps are exactly two steps of the plain restatement
    plain = _state()
    R.step(plain, GOOD, global_max_norm=1.0)
    R.step(plain, GOOD, global_max_norm=1.0)
    for got, want in zip((st.p, st.m, st.v), (plain.p, plain.m, plain.v)):
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_counters_while_a_run_is_open_and_nan_record():
    st, guard = _state(), NF.Guard(n_ring=4)
    NF.guarded_step(st, guard, _bad(np.nan))
    assert guard.stats() == dict(attempts=1, skipped=1, consecutive=1, max_consecutive=1, last_skipped=0)
    NF.guarded_step(st, guard, GOOD)
    NF.guarded_step(st, guard, _bad(-np.inf))
    NF.guarded_step(st, guard, _bad(1e20))
    assert guard.stats() == dict(attempts=4, skipped=3, consecutive=2, max_consecutive=2, last_skipped=3)
    recs = guard.records()
    assert [r["attempt"] for r in recs] == [0, 1, 2, 3]
    assert math.isnan(recs[0]["grad_norm"]) and recs[0]["clip"] == 1.0            # no global limit: c = 1
    assert recs[1]["grad_norm"] == np.float32(13.0)
    assert st.step == [1, 1]


def test_the_rule_counts_an_fp32_overflow_as_bad_and_nothing_below_it():
    assert math.isinf(NF.total_of_squares([np.array([1e20], np.float32)]))                 # 1e40 is finite in fp64, not in fp32
    assert math.isinf(NF.total_of_squares([np.full(4096, 1e19, np.float32)]))              # no single square overflows, the chunk does
    assert math.isfinite(NF.total_of_squares([np.full(4096, 1e17, np.float32)]))
    assert math.isfinite(NF.total_of_squares([np.array([1e19], np.float32), None, np.array([1e19], np.float32)]))
    assert math.isnan(NF.total_of_squares([np.array([np.inf, np.nan], np.float32)]))
    assert NF.total_of_squares([None, np.zeros(3, np.float32)]) == 0.0


def test_dyadic_gradients_sum_exactly_in_fp32():
    rs = np.random.RandomState(3)
    for g in NF.dyadic_gradients(rs, [4097, 7, 1], scale=0.25):
        sq = (g * g).astype(np.float32)
        forward, backward = np.float32(0), np.float32(0)
        for x in sq:
            forward = np.float32(forward + x)
        for x in sq[::-1]:
            backward = np.float32(backward + x)
        assert float(forward) == float(backward) == float(np.sum(g.astype(np.float64) ** 2))


def test_guarded_entry_point_refuses_bad_arguments_before_any_launch():
    """Every NR_EINVAL case of the header, on the host (no GPU needed: the checks come before the first launch)."""
    f = hip.lib().nr_bertadam_step_guarded
    buf = ctypes.create_string_buffer(8192)
    ok = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8

    def call(table=ok, T=1, n_chunks=1, groups=ok, G=1, gmn=1.0, ws=ok, guard=ok, losses=ok, n_losses=5, ring=ok, n_ring=4):
        return f(table, T, n_chunks, groups, G, gmn, ws, guard, losses, n_losses, ring, n_ring, None)

    E = hip.NR_EINVAL
    assert call(guard=None) == E and call(ring=None) == E
    assert call(guard=ok + 4) == E and call(ring=ok + 4) == E
    for n_ring in (0, -1, 3, 6, 4095, 8192, 1 << 20):
        assert call(n_ring=n_ring) == E, n_ring
    for n_losses in (-1, 9, 100):
        assert call(n_losses=n_losses) == E, n_losses
    assert call(losses=None, n_losses=1) == E
    # today's checks of nr_bertadam_step
    assert call(table=None) == E and call(groups=None) == E and call(ws=None) == E
    assert call(n_chunks=-1) == E and call(T=-1) == E and call(G=0) == E and call(G=-1) == E
    assert call(gmn=float("nan")) == E
    assert call(T=0, n_chunks=1) == E
    # nothing to update: NR_OK without a launch, whatever the optional losses are -- and still no null guard
    assert call(T=0, n_chunks=0) == 0 and call(T=0, n_chunks=0, losses=None, n_losses=0) == 0
    assert call(T=0, n_chunks=0, guard=None) == E
    assert not any(buf.raw)


def test_structs_have_the_stated_sizes():
    assert ctypes.sizeof(hip.StepGuard) == 48 and ctypes.sizeof(hip.StepRecord) == 56 == optim.RECORD_DTYPE.itemsize
    assert hip.GUARD_MAX_LOSSES == NF.MAX_LOSSES == 8 and hip.GUARD_MAX_RING == 4096
    for name in ("attempt", "grad_norm", "clip", "skipped", "n_losses", "losses"):
        assert optim.RECORD_DTYPE.fields[name][1] == getattr(hip.StepRecord, name).offset, name


@pytest.mark.parametrize("ring", [0, 3, 6, 1000, 8192, -4, 2.0, None])
def test_bertadam_refuses_a_bad_record_ring(ring):
    p = torch.nn.Parameter(torch.zeros(3))
    for on in (False, True):
        with pytest.raises(ValueError, match="record_ring"):
            optim.BertAdam([p], lr=1e-3, skip_nonfinite=on, record_ring=ring)


def test_bertadam_flag_values_and_readers_without_the_flag():
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (2, -1, "yes", None, 0.5):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            optim.BertAdam([p], lr=1e-3, skip_nonfinite=bad)
    for ring in (1, 2, 256, 4096):
        opt = optim.BertAdam([p], lr=1e-3, skip_nonfinite=True, record_ring=ring)
        assert opt.skip_nonfinite is True and opt.record_ring == ring
    off = optim.BertAdam([p], lr=1e-3)
    assert off.skip_nonfinite is False and off.record_ring == 256
    for reader in (off.guard_stats, off.records, lambda: off.watch_losses(None)):
        with pytest.raises(RuntimeError, match="skip_nonfinite=True"):
            reader()
    on = optim.BertAdam([p], lr=1e-3, skip_nonfinite=True)
    for bad in (torch.zeros(5), [1.0], torch.zeros(9)):              # not on the device / not a tensor / too long
        with pytest.raises(ValueError, match="watch_losses"):
            on.watch_losses(bad)


def test_prep_optimizer_passes_the_flag_on():
    from neighborretr_amd import modeling

    class Args:
        lr, coef_lr, weight_decay, warmup_proportion = 1e-4, 1e-3, 0.2, 0.1
    model = modeling.NeighborRetr(modeling.default_config(num_neighbors=4))
    assert optim.prep_optimizer(Args, model, 10, 0)[0].skip_nonfinite is False
    assert optim.prep_optimizer(Args, model, 10, 0, skip_nonfinite=True)[0].skip_nonfinite is True


@pytest.mark.parametrize("value", [2, -1, "1", 0.5, True, None])
def test_train_epoch_refuses_a_bad_flag_before_any_work(value):
    class Args:
        skip_nonfinite = value

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"train_epoch touched .{name} before checking the flag")

        def __iter__(self):
            raise AssertionError("train_epoch iterated the loader before checking the flag")
    with pytest.raises(ValueError, match="skip_nonfinite"):
        training.train_epoch(1, Args, Untouchable(), Untouchable(), "cpu", 1, Untouchable(), None, 0, 1, None)
