"""CPU: the route a step takes through its token clustering (cluster_fused.cluster_route) as a table, the laziness of its two shape
gates, and the stage table every grouped call reads.  The expected values are written out from the rules, not computed by the
function under test."""
import itertools

import pytest
import torch

from neighborretr_amd import cluster_fused, modeling
from neighborretr_amd.cluster_fused import Route, cluster_route

TF = (False, True)


def _never(what):
    def gate():
        raise AssertionError(f"{what} was asked")
    return gate


def _route(gpu=True, grad=False, shard_now=False, side_streams=True, group=True, fuse=True, fused_training=None, cluster_stream=True,
           interleave=True, split_nodes=True, local_stream=True, shard_clustering=True, fusable=True, grouped_ok=True):
    """cluster_route with the shipped flags; a gate given as a bool answers that, anything else is the callable itself."""
    as_gate = lambda v: (lambda: v) if isinstance(v, bool) else v      # noqa: E731
    return cluster_route(gpu, grad, shard_now, side_streams, group, fuse, fused_training, cluster_stream, interleave, split_nodes,
                         as_gate(local_stream), shard_clustering, fusable=as_gate(fusable), grouped_ok=as_gate(grouped_ok))


def _expected(gpu, grad, shard_now, side_streams, group, fuse, fused_training, fusable, grouped_ok):
    """Today's precedence, with the training sub-flags as shipped (cluster stream, interleaved, split nodes, local stream)."""
    grouped_forward = gpu and fuse and fusable and grouped_ok           # the no-grad grouped forward takes these shapes
    if shard_now:
        if grad:
            return "sharded_training"
        if grouped_forward:
            return "sharded_loss_only"
        # (falls through: a sharded loss-only step whose shapes the fused clustering refuses clusters replicated)
    if not grad and gpu and side_streams and group and grouped_forward:
        return "grouped_steps"
    if grad and gpu and fuse and fused_training in (None, True) and grouped_ok:
        return "training_interleaved" if side_streams else "training_one_stream"       # (no side streams: no cluster stream)
    return "two_streams" if gpu and side_streams else "inline"


def test_route_table():
    seen = set()
    for gpu, grad, shard_now, side, group, fuse, fusable, ok in itertools.product(TF, repeat=8):
        for fused_training in (None, True, False):
            got = _route(gpu=gpu, grad=grad, shard_now=shard_now, side_streams=side, group=group, fuse=fuse,
                         fused_training=fused_training, fusable=fusable, grouped_ok=ok)
            want = _expected(gpu, grad, shard_now, side, group, fuse, fused_training, fusable, ok)
            assert got.name == want, (gpu, grad, shard_now, side, group, fuse, fused_training, fusable, ok, got)
            assert got.sharded_clustering is (True if want == "sharded_loss_only" else None)
            seen.add(want)
    assert seen == {"sharded_training", "sharded_loss_only", "grouped_steps", "training_interleaved", "training_one_stream",
                    "two_streams", "inline"}                              # (training_cluster_stream: the sub-flags below)


def test_rows_written_out():
    assert _route() == Route("grouped_steps")                               # the shipped loss-only step
    assert _route(grad=True) == Route("training_interleaved")              # the shipped training step
    assert _route(gpu=False) == _route(gpu=False, grad=True) == Route("inline")
    assert _route(side_streams=False) == Route("inline")                   # one hardware queue
    assert _route(group=False) == _route(fuse=False) == _route(fusable=False) == _route(grouped_ok=False) == Route("two_streams")
    assert _route(grad=True, fused_training=False) == _route(grad=True, fuse=False) == Route("two_streams")
    assert _route(grad=True, grouped_ok=False) == Route("two_streams")
    assert _route(grad=True, fused_training=True, fusable=False) == Route("training_interleaved")    # training never asks `fusable`
    # the sharded loss: the sub-choice is shard_clustering; refused shapes fall through to the replicated routes
    assert _route(shard_now=True) == Route("sharded_loss_only", True)
    assert _route(shard_now=True, shard_clustering=False) == Route("sharded_loss_only", False)
    assert _route(shard_now=True, grouped_ok=False) == _route(shard_now=True, fusable=False) == Route("two_streams")
    assert _route(shard_now=True, fuse=False, side_streams=False) == Route("inline")
    assert _route(shard_now=True, group=False, side_streams=False) == Route("sharded_loss_only", True)   # (reads neither flag)
    assert _route(shard_now=True, grad=True, fuse=False, grouped_ok=False) == Route("sharded_training")


@pytest.mark.parametrize("side,cluster_stream,interleave,split_nodes,local_stream",
                         list(itertools.product(TF, repeat=5)))
def test_training_sub_flags(side, cluster_stream, interleave, split_nodes, local_stream):
    got = _route(grad=True, side_streams=side, cluster_stream=cluster_stream, interleave=interleave, split_nodes=split_nodes,
                 local_stream=local_stream)
    if not (side and cluster_stream):
        want = "training_one_stream"                   # no stream of the clustering's own
    elif interleave and split_nodes and local_stream:
        want = "training_interleaved"
    else:
        want = "training_cluster_stream"
    assert got == Route(want)
    # the local stream is asked for only when everything else allows the interleaved route
    if not (side and cluster_stream and interleave and split_nodes):
        assert _route(grad=True, side_streams=side, cluster_stream=cluster_stream, interleave=interleave, split_nodes=split_nodes,
                      local_stream=_never("the local stream")) == Route(want)


def test_gates_are_asked_only_where_the_ladder_asked_them():
    fus, grp = _never("the one-problem gate"), _never("the library's planner")
    for grad, shard_now, side, group, fuse, fused_training in itertools.product(TF, TF, TF, TF, TF, (None, True, False)):
        # a CPU tensor asks neither, whatever the flags
        want = "sharded_training" if (shard_now and grad) else "inline"
        assert _route(gpu=False, grad=grad, shard_now=shard_now, side_streams=side, group=group, fuse=fuse,
                      fused_training=fused_training, fusable=fus, grouped_ok=grp).name == want
    for grad, shard_now, side, group, fused_training in itertools.product(TF, TF, TF, TF, (None, True, False)):
        # fuse_clustering = False asks neither
        want = "sharded_training" if (shard_now and grad) else ("two_streams" if side else "inline")
        assert _route(grad=grad, shard_now=shard_now, side_streams=side, group=group, fuse=False, fused_training=fused_training,
                      fusable=fus, grouped_ok=grp).name == want
    # the training routes never ask the one-problem gate; fused_training_clustering = False and the sharded training step ask nothing
    assert _route(grad=True, fusable=fus).name == "training_interleaved"
    assert _route(grad=True, fused_training=False, fusable=fus, grouped_ok=grp).name == "two_streams"
    assert _route(grad=True, shard_now=True, fusable=fus, grouped_ok=grp).name == "sharded_training"
    # loss-only: the planner only behind the one-problem gate; neither without side streams or group_clustering (unless sharded)
    assert _route(fusable=False, grouped_ok=grp).name == "two_streams"
    assert _route(side_streams=False, fusable=fus, grouped_ok=grp).name == "inline"
    assert _route(group=False, fusable=fus, grouped_ok=grp).name == "two_streams"
    assert _route(shard_now=True, fusable=False, grouped_ok=grp).name == "two_streams"

    def einval():
        raise ValueError("NR_EINVAL")
    # the planner's refusal of fewer tokens than k surfaces where it is asked ...
    for kw in (dict(), dict(grad=True), dict(shard_now=True)):
        with pytest.raises(ValueError, match="NR_EINVAL"):
            _route(grouped_ok=einval, **kw)
    # ... and nowhere else
    assert _route(group=False, side_streams=False, grouped_ok=einval).name == "inline"


def test_model_passes_its_gates_lazily(monkeypatch):
    m = modeling.NeighborRetr(modeling.default_config(), precision="bf16")
    monkeypatch.setattr(m, "_grouped_stages_supported", _never("the library's planner"))
    x = torch.zeros(2, 24, 512), torch.zeros(2, 12, 512)
    for grad in TF:
        with torch.set_grad_enabled(grad):
            assert m._cluster_route(*x, False) == Route("inline")


def test_stage_table():
    m = modeling.NeighborRetr(modeling.default_config(), precision="bf16")
    stages = m._stages()
    assert [s.key for s in stages] == ["text0", "video0", "text1", "video1"]
    assert [s.noise for s in stages] == ["t0", "v0", "t1", "v1"]
    for s, ctm, blk in zip(stages, ("text_ctm0", "video_ctm0", "text_ctm1", "video_ctm1"),
                           ("text_block0", "video_block0", "text_block1", "video_block1")):
        assert s.ctm is getattr(m, ctm) and s.block is getattr(m, blk)
    assert cluster_fused.stage_weight_list(stages) == [(s.key, s.ctm, s.block) for s in stages]
    assert [w[0] for w in cluster_fused.stage_weight_list(stages)] == ["text0", "video0", "text1", "video1"]
    tf, vf, tm, vm = (torch.zeros(2, 24, 8), torch.zeros(2, 12, 8), torch.ones(2, 24), torch.ones(2, 12))
    nz = {"t0": torch.zeros(2, 24), "v0": torch.zeros(2, 12), "t1": torch.zeros(2, 4)}            # (no "v1": the stage draws its own)
    p0 = cluster_fused.stage_problems(stages[:2], (tf, vf), (tm, vm), nz)
    assert [len(p) for p in p0] == [6, 6]
    for p, want in zip(p0, (("text0", tf, tm, m.text_ctm0, m.text_block0, nz["t0"]),
                            ("video0", vf, vm, m.video_ctm0, m.video_block0, nz["v0"]))):
        assert p[0] == want[0] and all(a is b for a, b in zip(p[1:], want[1:]))
    o_t, o_v = torch.zeros(2, 4, 8), torch.zeros(2, 3, 8)
    p1 = cluster_fused.stage_problems(stages[2:], (o_t, o_v), None, nz)
    for p, want in zip(p1, (("text1", o_t, None, m.text_ctm1, m.text_block1, nz["t1"]),
                            ("video1", o_v, None, m.video_ctm1, m.video_block1, None))):
        assert len(p) == 6 and p[0] == want[0] and all(a is b for a, b in zip(p[1:], want[1:]))
