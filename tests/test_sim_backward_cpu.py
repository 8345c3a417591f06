"""CPU: the host-only mapping of the similarity backward (ops.sim_backward_launches) -- from a table of targets and products,
given as opaque identities, to the d_x launches, the weight-sum jobs and the transposing launches.  The compositions below are
the launches the three callers issued when they were written out by hand; the composition of a launch decides the kernel's
chunking and with it the bits of d_x, so the mapping has to reproduce them exactly."""
from collections import namedtuple

import pytest

from neighborretr_amd import ops

P = namedtuple("P", "name text video")            # a product: only its two operands matter to the mapping
T = ops.SimTarget
t, v, bt, bv, t_r, v_r = "t", "v", "bt", "bv", "t_r", "v_r"


def _replicated():
    P0, P1, P2 = P("P0", t, v), P("P1", t, bv), P("P2", bt, v)
    return (P0, P1, P2), [T(t, [P0, P1]), T(v, [P0, P2]), T(bv, [P1], False), T(bt, [P2], False)]


def _sharded():
    Pc, Pr, P1, P2 = P("Pc", t, v_r), P("Pr", t_r, v), P("P1", t_r, bv), P("P2", bt, v_r)
    return (Pc, Pr, P1, P2), [T(t, [Pc]), T(t_r, [Pr, P1]), T(v, [Pr]), T(v_r, [Pc, P2]), T(bv, [P1], False), T(bt, [P2], False)]


def test_replicated_table():
    (P0, P1, P2), table = _replicated()
    dx, jobs, tr = ops.sim_backward_launches(table)
    assert dx == [[(t, P0, 0), (t, P1, 0), (v, P0, 1), (v, P2, 1)]]
    assert jobs == [(t, [(P0, 0), (P1, 0)]), (v, [(P0, 1), (P2, 1)]), (bv, [(P1, 1)]), (bt, [(P2, 0)])]
    assert tr == [[v, bv, t, bt]]


def test_sharded_table():
    (Pc, Pr, P1, P2), table = _sharded()
    dx, jobs, tr = ops.sim_backward_launches(table)
    assert dx == [[(t, Pc, 0), (t_r, Pr, 0), (t_r, P1, 0), (v, Pr, 1)], [(v_r, Pc, 1), (v_r, P2, 1)]]
    assert jobs == [(t, [(Pc, 0)]), (t_r, [(Pr, 0), (P1, 0)]), (v, [(Pr, 1)]), (v_r, [(Pc, 1), (P2, 1)]), (bv, [(P1, 1)]),
                    (bt, [(P2, 0)])]
    assert tr == [[v_r, v, bv, t_r], [t, bt]]


def test_local_level_table():
    P0 = P("P", t, v)
    dx, jobs, tr = ops.sim_backward_launches([T(t, [P0]), T(v, [P0])])
    assert dx == [[(t, P0, 0), (v, P0, 1)]]
    assert jobs == [(t, [(P0, 0)]), (v, [(P0, 1)])]
    assert tr == [[v, t]]


def test_more_than_four_items_are_cut_into_launches_of_four():
    texts = ["t%d" % k for k in range(5)]
    prods = [P("P%d" % k, s, v) for k, s in enumerate(texts)]
    dx, jobs, tr = ops.sim_backward_launches([T(s, [p]) for s, p in zip(texts, prods)] + [T(v, prods[:2])])
    assert [len(launch) for launch in dx] == [4, 3]
    assert [it for launch in dx for it in launch] == [(s, p, 0) for s, p in zip(texts, prods)] + [(v, prods[0], 1), (v, prods[1], 1)]
    assert len(jobs) == 6
    assert tr == [[v] + texts[:2]]                      # a shared operand is transposed once
    dx, _, tr = ops.sim_backward_launches([T(v, prods[:2])] + [T(s, [p]) for s, p in zip(texts, prods)], group_max=2)
    assert [len(launch) for launch in dx] == [2, 2, 2, 1] and [len(c) for c in tr] == [2, 1]


def test_a_weights_only_target_gives_a_job_and_no_item():
    P0 = P("P", t, bv)
    dx, jobs, tr = ops.sim_backward_launches([T(bv, [P0], False)])
    assert dx == [] and tr == [] and jobs == [(bv, [(P0, 1)])]
    dx, jobs, tr = ops.sim_backward_launches([T(t, [P0]), T(bv, [P0], False)])
    assert dx == [[(t, P0, 0)]] and tr == [[bv]] and [s for s, _ in jobs] == [t, bv]


def test_tables_the_kernels_cannot_take_are_refused():
    P0, P1, P2 = P("P0", t, v), P("P1", t, bv), P("P2", t, v_r)
    with pytest.raises(ValueError):
        ops.sim_backward_launches([T(t, [P0, P1, P2])])              # PoolWJob has two sources
    with pytest.raises(ValueError):
        ops.sim_backward_launches([T(t, [])])
    with pytest.raises(ValueError):
        ops.sim_backward_launches([T(bt, [P0])])                     # not an operand of its product
    with pytest.raises(ValueError):
        ops.sim_backward_launches([T(t, [P0, P("Px", v, t)])])       # text operand of one, video operand of the other
    with pytest.raises(ValueError):
        ops.sim_backward_launches([T(t, [P0]), T(t, [P1])])          # one entry per set: its products are summed in ONE order


@pytest.mark.parametrize("table", [_replicated, _sharded])
def test_side_and_pooled_maxima_follow_the_operand(table):
    """Text operand -> side 0 and aux[2] (pmax); video operand -> side 1 and aux[3] (qmax) -- for every (target, product), in
    the d_x items and in the jobs alike; a job's source reads the pooled maxima of that side."""
    _, targets = table()
    dx, jobs, _ = ops.sim_backward_launches(targets)
    pairs = [(s, p, side) for launch in dx for s, p, side in launch] + [(s, p, side) for s, sides in jobs for p, side in sides]
    assert len(pairs) == sum(len(tg.products) * (1 + tg.want_dx) for tg in targets)
    Set = namedtuple("Set", "n")
    for s, p, side in pairs:
        assert (p.text, p.video)[side] == s and side == (0 if s == p.text else 1)
        full = ops.SimProduct(Set(3), Set(5), "dS", 1, 0.5, ("arg_v", "arg_t", "pmax", "qmax"))
        assert ops._pool_src(full, side) == ("dS", 1, 0.5, "pmax" if s == p.text else "qmax", 3, 5)
