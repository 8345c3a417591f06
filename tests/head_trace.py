"""Recorder of the step's launch schedule, and the step forms tests/test_head_schedule_gpu.py pins with it.

`Recorder` wraps, while active, hip.call, torch.cuda.Stream.wait_stream / wait_event, torch.cuda.Event.record and
torch.Tensor.record_stream, and appends to `trace`:

    ("call", entry name, s)          a C-ABI launch, s = the stream that was current (the fused scorer entries, which ops calls
                                     without hip.call, are wrapped on the library object and listed when they launched)
    ("wait", waiter, on)             waiter.wait_stream(on)   (the event torch records and waits for inside it is not listed again)
    ("record", e, s)                 event e recorded on stream s
    ("wait_event", waiter, e)
    ("record_stream", s, count)      at the end, per stream: how many tensor.record_stream(s) calls there were

Streams and events are numbered by first appearance, so no handle value enters a trace.  The schedule of a step does not depend
on whether it is captured (outside the split tail's exception path nothing in the head branches on capturing), so the forms run
eagerly; each is recorded on its SECOND run, after one unrecorded run that builds the weight splits, streams and caches.
"""
import numpy as np
import torch

from neighborretr_amd import hip, modeling
from util import golden, noise, params, problem

DEV = "cuda"
# the fused scorer entries: ops calls them on the loaded library itself (it reads their status), not through hip.call
DIRECT_ENTRIES = ("nr_token_weights_fwd", "nr_token_weights_fwd_pair", "nr_token_weights_fwd_group")


class Recorder:
    def __init__(self):
        self.trace, self._streams, self._events, self._kept, self._recorded, self._depth = [], {}, {}, [], {}, 0

    def _s(self, stream):
        return self._streams.setdefault(int(stream.cuda_stream), len(self._streams))

    def _e(self, event):
        if id(event) not in self._events:
            self._events[id(event)] = len(self._events)
            self._kept.append(event)                   # (alive, so that no later event takes its id)
        return self._events[id(event)]

    def _wrap(self, owner, name, entry):
        """owner.name -> a wrapper that appends entry(*args) (unless called from inside another wrapped call) and calls on."""
        inner, had = getattr(owner, name), name in vars(owner)

        def wrapper(*args, **kwargs):
            if self._depth == 0:
                made = entry(*args, **kwargs)
                if made is not None:
                    self.trace.append(made)
            self._depth += 1
            try:
                return inner(*args, **kwargs)
            finally:
                self._depth -= 1
        setattr(owner, name, wrapper)
        self._undo.append((owner, name, inner, had))

    def _count(self, tensor, stream):
        s = self._s(stream)
        self._recorded[s] = self._recorded.get(s, 0) + 1

    def __enter__(self):
        self._undo = []
        cur = torch.cuda.current_stream
        self._wrap(hip, "call", lambda name, *a: ("call", name, self._s(cur())))
        self._wrap(torch.cuda.Stream, "wait_stream", lambda waiter, on: ("wait", self._s(waiter), self._s(on)))
        self._wrap(torch.cuda.Stream, "wait_event", lambda waiter, ev: ("wait_event", self._s(waiter), self._e(ev)))
        self._wrap(torch.cuda.Event, "record", lambda ev, stream=None: ("record", self._e(ev), self._s(cur() if stream is None else stream)))
        self._wrap(torch.Tensor, "record_stream", self._count)
        for name in DIRECT_ENTRIES:
            self._wrap_direct(hip.lib(), name)
        return self

    def _wrap_direct(self, lib, name):
        inner = getattr(lib, name)

        def wrapper(*args):
            rc = inner(*args)
            if rc == 0:                                # (NR_EUNSUPPORTED: nothing was launched, ops falls back to other entries)
                self.trace.append(("call", name, self._s(torch.cuda.current_stream())))
            return rc
        setattr(lib, name, wrapper)
        self._undo.append((lib, name, inner, True))

    def __exit__(self, *exc):
        for owner, name, inner, had in reversed(self._undo):
            if had:
                setattr(owner, name, inner)
            else:
                delattr(owner, name)                   # (inherited: torch.Tensor.record_stream lives on the base class)
        self.trace += [("record_stream", s, n) for s, n in sorted(self._recorded.items())]
        return False


def _model(K, **cfg):
    """tests/test_head_gpu.py::_model, shipping precision plan."""
    m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K, **cfg), precision="bf16")
    _, unexpected = m.load_state_dict(params(), strict=False)
    assert not unexpected
    m = m.to(DEV)
    with torch.no_grad():
        m.clip.logit_scale.fill_(float(np.log(100.0)))
    return m.train()


def _loss_only(seed, B, Nt, Nv, M, K, frozen=False, side_streams=True, group=True, **cfg):
    """A model with its bank filled as test_a_failing_bank_push_does_not_poison_later_steps does -> step(): the five losses."""
    x = problem(seed, B, Nt, Nv, M, device=DEV)
    m = _model(K, **cfg)
    for k in ("mb_feat_t", "mb_feat_v", "mb_mask_t", "mb_mask_v"):
        setattr(m, k, x[k].clone().float() if "mask" in k else x[k].clone())
    m.mb_ind = torch.arange(M, device=DEV)
    m.bank_frozen, m.use_side_streams, m.group_clustering = frozen, side_streams, group

    def step():
        m._rng_state = None
        torch.manual_seed(5)
        with torch.no_grad():
            return [torch.stack(m(x["text_feat"], x["text_mask"], x["video_feat"], x["video_mask"], x["idx"], 0))]
    return m, step


def _pipelined(seed, B, Nt, Nv, M, K, U=2):
    """U overlapped steps as bench.py's unrolled(True) issues them (modeling.StepPipeline), outside a capture."""
    from neighborretr_amd.capture_guard import record_event, wait_event, wait_stream
    m, one = _loss_only(seed, B, Nt, Nv, M, K)
    m.prepare_pipeline(U, B)

    def steps():
        origin, prev, pending, pipes, out = torch.cuda.current_stream(), None, [], [], []
        try:
            for k in range(U):
                early = record_event(origin)
                if prev is not None and prev.push_done is not None:
                    wait_event(origin, prev.push_done)
                m._pipeline = prev = modeling.StepPipeline(k, prev)
                prev.early_fork = early
                pipes.append(prev)
                out += one()
                pending += prev.pending
        finally:
            m._pipeline = None
        for st_ in pending:
            wait_stream(origin, st_)
        torch.cuda.synchronize()                       # (the steps' buffers are owned by `pipes` until here)
        return out
    return m, steps


def _training(fused, **flags):
    """The forward of test_backward_matches_reference at c1_b16, shipping precision plan.  flags: model attributes to set."""
    g = golden("c1_b16")
    B, Nt, Nv, M, K = (int(g[k]) for k in ("B", "Nt", "Nv", "M", "K"))
    x = problem(int(g["seed"]), B, Nt, Nv, M, device=DEV)
    nz = noise(int(g["seed"]), B, Nt, Nv, device=DEV)
    m = _model(K)
    if not fused:
        m.fused_training_clustering = False
    for k, v in flags.items():
        setattr(m, k, v)
    x["text_feat"].requires_grad_(True)
    x["video_feat"].requires_grad_(True)
    c = m.config

    def step():
        losses = m._compute_losses(x["text_feat"], x["video_feat"], x["text_mask"], x["video_mask"], x["mb_feat_t"], x["mb_feat_v"],
                                   x["mb_mask_t"], x["mb_mask_v"], c.centrality_scale, c.beta, K, c.temperature,
                                   m.clip.logit_scale.exp(), noise=nz)
        return [torch.stack([l.detach() for l in losses])]
    return m, step


def _sharded_loss_only(seed, B, Nt, Nv, M, K, shard_clustering, W=2, rank=1):
    """Rank `rank` of a W-rank loss-only step with the loss sharded, in an emulated world without a process group (the peers'
    parts of every collective are device copies): the first step() settles the world over all ranks, every step() runs the
    rank.  The bank stays frozen, so that every rank of every sweep sees the same one."""
    from neighborretr_amd import comm
    x = problem(seed, B, Nt, Nv, M, device=DEV)
    m, _ = _loss_only(seed, B, Nt, Nv, M, K, frozen=True, world_size=W)
    m.shard_loss, m.shard_clustering = True, shard_clustering
    world, b = comm.EmulatedWorld(W, real_collectives=False), B // W

    def run(r):
        m.config.local_rank = r
        m._rng_state = None                            # (every rank of a real job draws the same batch-wide noise)
        torch.manual_seed(5)
        sl = slice(r * b, (r + 1) * b)
        with comm.use(world.comm(r)), torch.no_grad():
            return torch.stack(m(x["text_feat"][sl].contiguous(), x["text_mask"][sl].contiguous(), x["video_feat"][sl].contiguous(),
                                 x["video_mask"][sl].contiguous(), x["idx"][sl].contiguous(), 0))

    def step():
        if world.recording:
            world.settle(run)
        return [run(rank)]
    return m, step


FORMS = {
    "split_tail_push": lambda: _loss_only(1005, 32, 24, 12, 64, 8),
    "split_tail_frozen": lambda: _loss_only(1005, 32, 24, 12, 64, 8, frozen=True),
    "pipelined_x2": lambda: _pipelined(1005, 32, 24, 12, 64, 8),
    "joined_tail_b6": lambda: _loss_only(1005, 6, 20, 9, 16, 4),
    "single_stream": lambda: _loss_only(1005, 32, 24, 12, 64, 8, side_streams=False),
    "multi_token_split_tail": lambda: _loss_only(1005, 8, 64, 64, 16, 4, centrality_multi_token="mean"),
    # (64 tokens cluster to 3 / 6 global tokens per sample, as in the form above: the step runs under "mean" only)
    "paired_batch_scorers": lambda: _loss_only(1005, 128, 64, 64, 64, 20, centrality_multi_token="mean"),
    "training_interleaved": lambda: _training(True),
    "training_traced_clustering": lambda: _training(False),
    # the routes of cluster_fused.cluster_route that no form above reaches
    "training_cluster_stream": lambda: _training(True, interleave_training_forward=False),
    "training_one_stream": lambda: _training(True, cluster_side_stream=False),
    "loss_only_two_cluster_streams": lambda: _loss_only(1005, 32, 24, 12, 64, 8, group=False),
    "sharded_loss_only": lambda: _sharded_loss_only(1005, 32, 24, 12, 64, 8, shard_clustering=True),
    "sharded_loss_only_replicated_clustering": lambda: _sharded_loss_only(1005, 32, 24, 12, 64, 8, shard_clustering=False),
}


def run_form(name):
    """-> (trace, losses): the form's second run recorded; losses = per step of that run the five losses as float.hex()."""
    torch.manual_seed(20240607)                        # (conftest's seed: parameters outside the fixture's state dict are drawn from it)
    _, step = FORMS[name]()
    step()
    torch.cuda.synchronize()
    with Recorder() as rec:
        out = step()
    torch.cuda.synchronize()
    return rec.trace, [[float(v).hex() for v in o.cpu().tolist()] for o in out]
