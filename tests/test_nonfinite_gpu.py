"""GPU: the non-finite step guard (nr_bertadam_step_guarded, optim.BertAdam(skip_nonfinite=True), --skip_nonfinite 1) against
the unguarded kernels, bit for bit, and against the restatement (tests/nonfinite_ref.py).

Bit comparisons need no bar.  The one comparison of fp32 VALUES against the fp64 restatement -- the records' grad_norm and
clip -- is made on gradients whose squares add exactly in fp32 (nonfinite_ref.dyadic_gradients), so that both sides hold the same
total whatever their order of addition; sqrt and the division are correctly rounded on both sides, hence equality.  The whole
step is held to the bar of test_optim_gpu.test_graphed_step_with_the_update_inside: 4 x the distance of the same formulas in
fp32 torch ops from the restatement."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bertadam_ref as R
import nonfinite_ref as NF
import test_optim_gpu as T
from neighborretr_amd import hip, ops, optim

pytestmark = pytest.mark.gpu
ROOT = T.ROOT
DEV = "cuda"
BAD_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "1e20": 1e20}


# ---- the C ABI, guarded and not, on the same table ----------------------------------------------------------------------------
class GuardedAbi(T.AbiStepper):
    """AbiStepper through nr_bertadam_step_guarded; keeps the last launch's workspace like its parent."""

    def __init__(self, *args, n_ring=4, **kw):
        super().__init__(*args, **kw)
        self.n_ring = n_ring
        self.guard = torch.frombuffer(bytearray(bytes(hip.StepGuard(last_skipped=-1))), dtype=torch.uint8).to(DEV)
        self.ring = torch.zeros(n_ring * ctypes.sizeof(hip.StepRecord), dtype=torch.uint8, device=DEV)

    def step(self, grads, losses=None):
        call = ops.bertadam_step
        ops.bertadam_step = lambda dg, G, dt, n, nc, ws, gmn: ops.bertadam_step_guarded(dg, G, dt, n, nc, ws, self.guard, self.ring,
                                                                                      gmn, losses=losses)
        try:
            super().step(grads)                      # (same table, same upload, same workspace: only the entry point differs)
        finally:
            ops.bertadam_step = call

    def stats(self):
        g = hip.StepGuard.from_buffer_copy(self.guard.cpu().numpy().tobytes())
        return {k: int(getattr(g, k)) for k in ("attempts", "skipped", "consecutive", "max_consecutive", "last_skipped")}, int(g.skip)

    def records(self):
        return np.frombuffer(self.ring.cpu().numpy().tobytes(), dtype=optim.RECORD_DTYPE)


def _device_lr(stepper, n_live):
    """The fp32 learning rates and coefficients launch B left in the last workspace ([tensor_sq | scale | lr | part])."""
    ws = stepper.keep[2].cpu().numpy()
    r256 = lambda b: (b + 255) // 256 * 256                                          # noqa: E731
    off = r256(8 * n_live)
    scale = np.frombuffer(ws[off:off + 4 * n_live].tobytes(), dtype=np.float32)
    off += r256(4 * n_live)
    return scale, np.frombuffer(ws[off:off + 4 * n_live].tobytes(), dtype=np.float32)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for u, w in zip(a, b) for x, y in zip(u, w))


GROUPS = [dict(lr=1e-3, weight_decay=0.2, schedule="warmup_cosine", warmup=0.25, t_total=8, b2=0.98),
          dict(lr=1e-4, weight_decay=0.0, schedule="warmup_linear", warmup=0.25, t_total=6, b2=0.98, max_grad_norm=0.5)]
# (sizes, gradients and tensors as misaligned views, index of a tensor whose grad is None in step 1)
TABLES = {"one element": ([1], False, None),
          "sub-chunk tensors": ([3, 5, 7, 127, 255], False, None),
          "4096": ([4096], False, None),
          "4097": ([4097], False, None),
          "lengths 1, 2, 3 mod 4": ([4101, 4098, 4099, 5, 6, 7], False, None),
          "misaligned views": ([4099, 1, 8192, 513], True, None),
          "grad None": ([4097, 70, 9], False, 1)}


def _pair(sizes, misaligned, gmn, seed, n_ring=4):
    rs = np.random.RandomState(seed)
    init = [(0.05 * rs.standard_normal(n)).astype(np.float32) for n in sizes]
    group_of = [t % 2 for t in range(len(sizes))]
    steppers = []
    for cls, kw in ((T.AbiStepper, {}), (GuardedAbi, dict(n_ring=n_ring))):
        _, p = T._views(init, sizes, misaligned)
        s = cls(p, group_of, GROUPS, {0: 0.06}, gmn, **kw)
        if misaligned:
            _, s.m = T._views([np.zeros(n, np.float32) for n in sizes], sizes, True)
            _, s.v = T._views([np.zeros(n, np.float32) for n in sizes], sizes, True)
        steppers.append(s)
    return rs, init, group_of, steppers


def _on_device(grads, sizes, misaligned):
    _, views = T._views([g if g is not None else np.zeros(n, np.float32) for g, n in zip(grads, sizes)], sizes, misaligned)
    return [None if g is None else v for g, v in zip(grads, views)]


@pytest.mark.parametrize("clip", [True, False], ids=["global limit", "no global limit"])
@pytest.mark.parametrize("name", list(TABLES))
def test_finite_gradients_give_the_unguarded_bits_and_the_restated_record(name, clip):
    sizes, misaligned, none_at = TABLES[name]
    gmn = 1.0 if clip else None
    rs, init, group_of, (plain, guarded) = _pair(sizes, misaligned, gmn, seed=100 + len(sizes))
    ref, guard = R.State(init, group_of, GROUPS, clamp_max={0: 0.06}), NF.Guard(n_ring=4)
    for s in range(3):
        grads = NF.dyadic_gradients(rs, sizes, scale=[1.0, 2.0 ** -6, 4.0][s])
        if none_at is not None and s == 1:
            grads[none_at] = None
        losses = torch.tensor([0.25 * s, -1.0, 3.0], device=DEV) if s != 1 else None
        plain.step(_on_device(grads, sizes, misaligned))
        guarded.step(_on_device(grads, sizes, misaligned), losses=losses)
        assert not NF.guarded_step(ref, guard, grads, global_max_norm=gmn, losses=() if losses is None else losses.tolist())
        assert _same_bits(guarded.state(), plain.state()), (name, s)
        assert guarded.steps.cpu().tolist() == plain.steps.cpu().tolist() == ref.step
        n_live = sum(g is not None for g in grads)
        for a, b in zip(_device_lr(guarded, n_live), _device_lr(plain, n_live)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, s)
        stats, skip = guarded.stats()
        assert stats == guard.stats() and skip == 0
        rec, want = guarded.records()[s & 3], guard.ring[s & 3]
        print(f"{name} step {s}: grad_norm {rec['grad_norm']!r} (restated {want['grad_norm']!r})  clip {rec['clip']!r} "
              f"(restated {want['clip']!r})")
        assert rec["attempt"] == s and rec["skipped"] == 0
        assert rec["grad_norm"] == want["grad_norm"] and rec["clip"] == want["clip"]
        assert rec["n_losses"] == (0 if losses is None else 3) and rec["losses"].tolist() == [float(x) for x in want["losses"]]


# ---- one bad value -------------------------------------------------------------------------------------------------------------
PLANT_SIZES = [4099, 8192, 70, 5]                     # tensor 2 sits at an odd 4-byte offset: the dword path
POSITIONS = {"first of the first tensor": (0, 0), "last of the last tensor": (3, 4), "tail element 1 of 3": (0, 4096),
             "tail element 2 of 3": (0, 4097), "tail element 3 of 3": (0, 4098), "last of a full chunk": (1, 4095),
             "second full chunk": (1, 8191), "dword path": (2, 33)}


def _planted_table(values):
    """Device copies of `values`, tensor 2 as a view at a 4-byte offset that is not 16-byte aligned."""
    out = []
    for t, x in enumerate(values):
        if t == 2:
            buf = torch.zeros(len(x) + 8, dtype=torch.float32, device=DEV)
            view = buf[1:1 + len(x)]
            assert view.data_ptr() % 16 == 4
        else:
            view = torch.zeros(len(x), dtype=torch.float32, device=DEV)
            assert view.data_ptr() % 16 == 0
        view.copy_(torch.from_numpy(x))
        out.append(view)
    return out


@pytest.mark.parametrize("value", list(BAD_VALUES))
@pytest.mark.parametrize("where", list(POSITIONS))
def test_one_bad_value_leaves_everything_as_it_was(where, value):
    rs = np.random.RandomState(77)
    sizes = PLANT_SIZES
    init = [(0.05 * rs.standard_normal(n)).astype(np.float32) for n in sizes]
    g = GuardedAbi(_planted_table(init), [0, 1, 0, 1], GROUPS, {3: 0.06}, 1.0)
    g.m, g.v = (_planted_table([np.zeros(n, np.float32) for n in sizes]) for _ in range(2))
    g.step(_planted_table([rs.standard_normal(n).astype(np.float32) for n in sizes]))      # a good step: moments, counters move
    before, steps_before = g.state(), g.steps.cpu().tolist()
    assert steps_before == [1] * 4 and g.stats() == (dict(attempts=1, skipped=0, consecutive=0, max_consecutive=0, last_skipped=-1), 0)
    grads = [(0.01 * rs.standard_normal(n)).astype(np.float32) for n in sizes]
    t, e = POSITIONS[where]
    grads[t][e] = BAD_VALUES[value]
    assert not np.isfinite(NF.total_of_squares(grads))
    g_dev = _planted_table(grads)
    g.step(g_dev, losses=torch.tensor([float("nan"), 1.0], device=DEV))
    torch.cuda.synchronize()
    assert _same_bits(g.state(), before), (where, value)
    assert g.steps.cpu().tolist() == steps_before
    assert g.stats() == (dict(attempts=2, skipped=1, consecutive=1, max_consecutive=1, last_skipped=1), 1)
    rec = g.records()[1]
    assert rec["attempt"] == 1 and rec["skipped"] == 1 and not np.isfinite(rec["grad_norm"])
    assert np.isnan(rec["losses"][0]) and rec["losses"][1] == 1.0
    for x, want in zip(g_dev, grads):                                                        # gradients are read, never written
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- skipping leaves no trace ---------------------------------------------------------------------------------------------------
def test_good_bad_good_equals_good_good_of_the_unguarded_kernel():
    """Under warm-up + cosine (and warm-up + linear) a counter moved by the skipped step would change the next learning rate."""
    sizes = [4099, 1, 8192, 513]
    rs, init, group_of, (plain, guarded) = _pair(sizes, False, 1.0, seed=11)
    good = [[(rs.standard_normal(n) * 0.3).astype(np.float32) for n in sizes] for _ in range(3)]
    bad = [x.copy() for x in good[1]]
    bad[2][5000] = np.nan
    for grads in (good[0], good[1], good[2]):
        plain.step(_on_device(grads, sizes, False))
    for grads in (good[0], bad, good[1], bad, bad, good[2]):
        guarded.step(_on_device(grads, sizes, False))
    assert _same_bits(guarded.state(), plain.state())
    assert guarded.steps.cpu().tolist() == plain.steps.cpu().tolist() == [3] * 4
    for a, b in zip(_device_lr(guarded, 4), _device_lr(plain, 4)):
        assert np.array_equal(a, b) and (a != 0).all()               # step 3's rates: past the first warm-up step, not 0
    assert guarded.stats() == (dict(attempts=6, skipped=3, consecutive=0, max_consecutive=2, last_skipped=4), 0)
    recs = guarded.records()                                          # n_ring = 4: attempts 2 .. 5 in slots 2, 3, 0, 1
    assert [int(r["attempt"]) for r in recs] == [4, 5, 2, 3] and [int(r["skipped"]) for r in recs] == [1, 0, 0, 1]


# ---- the optimizer ----------------------------------------------------------------------------------------------------------------
def _guarded_optimizer(init, groups, group_of, ring=256):
    p = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in init]
    pg = [dict(params=[x for x, q in zip(p, group_of) if q == gi], **dict(R.GROUP_DEFAULTS, **g)) for gi, g in enumerate(groups)]
    return p, optim.BertAdam(pg, lr=1e-4, global_max_norm=1.0, clamp_max={p[1]: 0.06}, skip_nonfinite=True, record_ring=ring)


def _with_one_bad(grads, step=2):
    grads = [[g.copy() for g in row] for row in grads]
    grads[step][2][4097] = np.inf
    return grads


def _records_equal(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


def test_five_eager_guarded_steps_equal_five_replays_of_a_captured_guarded_step():
    init, grads, groups, group_of = T._small_problem()
    grads = _with_one_bad(grads)
    p_e, eager = _guarded_optimizer(init, groups, group_of)
    watched = torch.zeros(5, device=DEV)
    eager.watch_losses(watched)
    for s, row in enumerate(grads):
        watched.fill_(float(s))
        for x, g in zip(p_e, row):
            x.grad = torch.from_numpy(g).to(DEV)
        eager.step()
    p, opt = _guarded_optimizer(init, groups, group_of)
    static = [torch.zeros_like(x) for x in p]
    for x, g in zip(p, static):
        x.grad = g
    static_losses = torch.zeros(5, device=DEV)
    opt.prepare()
    opt.watch_losses(static_losses)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        live = opt.issue()
    torch.cuda.synchronize()
    assert opt.guard_stats() == dict(attempts=0, skipped=0, consecutive=0, max_consecutive=0, last_skipped=-1)   # capturing ran nothing
    for s, row in enumerate(grads):
        static_losses.fill_(float(s))
        for dst, g in zip(static, row):
            dst.copy_(torch.from_numpy(g))
        graph.replay()
        opt.advance(live)
    torch.cuda.synchronize()
    assert _same_bits(T._opt_state(opt, p), T._opt_state(eager, p_e))
    assert T._device_steps(opt, p) == T._device_steps(eager, p_e) == [4] * len(p)
    assert opt.guard_stats() == eager.guard_stats() == dict(attempts=5, skipped=1, consecutive=0, max_consecutive=1, last_skipped=2)
    assert _records_equal(opt.records(), eager.records())
    recs = opt.records()
    assert recs["attempt"].tolist() == [0, 1, 2, 3, 4] and recs["skipped"].tolist() == [0, 0, 1, 0, 0]
    assert recs["losses"][:, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and (recs["n_losses"] == 5).all()
    assert opt.get_lr() == eager.get_lr()
    assert [opt.state[x]["step"] for x in p] == [4] * len(p)


def test_the_host_mirror_follows_the_device_and_a_state_dict_continues_bit_for_bit():
    init, grads, groups, group_of = T._small_problem(seed=6)
    grads = _with_one_bad(grads, step=1)                              # good, bad, good | good, good
    ref, guard = R.State(init, group_of, groups, clamp_max={1: 0.06}), NF.Guard()
    p, opt = _guarded_optimizer(init, groups, group_of, ring=2)

    def run(o, params, rows):
        for row in rows:
            for x, g in zip(params, row):
                x.grad = torch.from_numpy(g).to(DEV)
            o.step()
    run(opt, p, grads[:3])
    for row in grads[:3]:
        NF.guarded_step(ref, guard, row, global_max_norm=1.0)
    assert [opt.state[x]["step"] for x in p] == [3] * len(p)         # the optimistic mirror, before anything has read it
    order = [t for gi in range(len(groups)) for t, q in enumerate(group_of) if q == gi]      # get_lr() lists group by group
    assert opt.get_lr() == [ref.lr()[t] for t in order]
    assert [opt.state[x]["step"] for x in p] == ref.step == [2] * len(p)
    assert opt.group_lr() == [R.scheduled_lr(dict(R.GROUP_DEFAULTS, **g), 2) for g in groups]
    assert opt.guard_stats() == guard.stats()
    recs = opt.records()                                              # a ring of two: attempts 1 and 2, in that order
    assert recs["attempt"].tolist() == [1, 2] and recs["skipped"].tolist() == [1, 0]
    assert opt.records(last=1)["attempt"].tolist() == [2] and len(opt.records(last=0)) == 0
    p3, three = _guarded_optimizer(init, groups, group_of)            # the default ring: three rows in order
    run(three, p3, grads[:3])
    assert three.records()["attempt"].tolist() == [0, 1, 2] and three.records()["skipped"].tolist() == [0, 1, 0]
    # the round trip: the counters a checkpoint carries are the device's, not the optimistic ones
    p4, again = _guarded_optimizer(init, groups, group_of)
    run(again, p4, grads[:3])                                         # (no reader called: state_dict() itself must synchronise)
    sd = again.state_dict()
    assert all(s["step"] == 2 for s in sd["state"].values())
    sd = {"state": {k: {"step": s["step"], "next_m": s["next_m"].cpu(), "next_v": s["next_v"].cpu()} for k, s in sd["state"].items()},
          "param_groups": sd["param_groups"]}
    pf = [torch.nn.Parameter(x.detach().clone()) for x in p4]
    pg = [dict(params=[x for x, q in zip(pf, group_of) if q == gi], **dict(R.GROUP_DEFAULTS, **g)) for gi, g in enumerate(groups)]
    fresh = optim.BertAdam(pg, lr=1e-4, global_max_norm=1.0, clamp_max={pf[1]: 0.06}, skip_nonfinite=True)
    fresh.load_state_dict(sd)
    run(fresh, pf, grads[3:])
    run(opt, p, grads[3:])
    assert _same_bits(T._opt_state(fresh, pf), T._opt_state(opt, p))
    assert T._device_steps(fresh, pf) == T._device_steps(opt, p) == [4] * len(p)
    assert fresh.guard_stats()["attempts"] == 2 and opt.guard_stats()["attempts"] == 5     # loading resets nothing, copies nothing


# ---- the whole step ------------------------------------------------------------------------------------------------------------
def test_graphed_step_skips_a_blank_batch_and_an_unguarded_one_does_not():
    sys.path.insert(0, ROOT)
    from main_retrieval import GraphedStep
    from util import problem
    B, Nt, Nv, M = 32, 24, 12, 64
    x = problem(1003, B, Nt, Nv, M, device=DEV)

    def batch(r, blank=False):
        vm = x["video_mask"].clone()
        if blank:
            vm[3] = 0                                                # one undecodable video: an all-zero mask
        return (x["text_feat"] + 0.01 * r, x["text_mask"], x["video_feat"] + 0.01 * r, vm, x["idx"] + 100 * r)
    feed = [batch(0), batch(1, blank=True), batch(2)]

    def fresh(guarded):
        m = T._model(K=8)
        m.mb_feat_t, m.mb_feat_v = x["mb_feat_t"].clone(), x["mb_feat_v"].clone()
        m.mb_mask_t, m.mb_mask_v = x["mb_mask_t"].clone(), x["mb_mask_v"].clone()
        m.mb_ind = torch.arange(5000, 5000 + M, device=DEV)
        opt, _, _ = optim.prep_optimizer(T._Args, m, 6, 0, global_max_norm=1.0, clamp_logit_scale=True, skip_nonfinite=guarded)
        return m, [p for _, p in m.named_parameters()], opt

    # the control, and first the precondition on its model: the blank batch does give a non-finite loss and gradient
    m, params, opt = fresh(False)
    m.bank_frozen = True
    losses = m(*feed[1], 0)
    grads = torch.autograd.grad(losses[0], params, allow_unused=True)
    m.bank_frozen = False
    assert not bool(torch.isfinite(losses[0]))
    assert any(g is not None and not bool(torch.isfinite(g).all()) for g in grads)
    del losses, grads
    step = GraphedStep(m, feed[0], params, optimizer=opt)
    for b in feed:
        step.run(b)
    torch.cuda.synchronize()
    assert not all(bool(torch.isfinite(p).all()) for p in params)    # a NaN result, not a fault: what the guard is for

    m, params, opt = fresh(True)
    init = [p.detach().cpu().numpy().copy() for p in params]
    index = {id(p): t for t, p in enumerate(params)}
    group_of = [None] * len(params)
    for gi, g in enumerate(opt.param_groups):
        for p in g["params"]:
            group_of[index[id(p)]] = gi
    groups = [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]
    clamp = {index[id(m.clip.logit_scale)]: T.LN100}
    ref, guard = R.State(init, group_of, groups, clamp_max=clamp), NF.Guard()
    eager = T.TorchEager([p.detach().reshape(-1) for p in params], group_of, groups, clamp, 1.0)
    step = GraphedStep(m, feed[0], params, optimizer=opt)
    for r, b in enumerate(feed):
        losses = step.run(b)
        torch.cuda.synchronize()
        grads = [None if g is None else g.detach() for g in step.grads]
        skipped = NF.guarded_step(ref, guard, [None if g is None else g.cpu().numpy() for g in grads], global_max_norm=1.0)
        assert skipped == (r == 1)
        assert all(bool(torch.isfinite(l)) for l in losses) == (r != 1)
        if not skipped:
            eager.step([None if g is None else g.reshape(-1) for g in grads])
        got = T._opt_state(opt, params)
        d_hip = R.state_distance(*[[a.reshape(-1) for a in part] for part in got], T._Flat(ref))
        d_torch = R.state_distance(*eager.state(), T._Flat(ref))
        print(f"guarded graphed step {r}: hip {d_hip:.3e}  fp32 torch {d_torch:.3e}")
        assert d_hip <= 4.0 * d_torch, (r, d_hip, d_torch)
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert all(bool(torch.isfinite(opt.state[p][k]).all()) for p in params if len(opt.state[p]) for k in ("next_m", "next_v"))
    assert opt.guard_stats() == guard.stats() == dict(attempts=3, skipped=1, consecutive=0, max_consecutive=1, last_skipped=1)
    recs = opt.records()
    assert recs["skipped"].tolist() == [0, 1, 0] and (recs["n_losses"] == 5).all()
    assert not np.isfinite(recs[1]["losses"][:5]).all() and not np.isfinite(recs[1]["grad_norm"])
    assert np.isfinite(recs[0]["losses"]).all() and np.isfinite(recs[2]["losses"]).all()
    live = [t for t, g in enumerate(step.grads) if g is not None]
    opt.get_lr()
    assert [opt.state[params[t]]["step"] for t in live] == [2] * len(live) == [T._device_steps(opt, params)[t] for t in live]


# ---- the entry point ------------------------------------------------------------------------------------------------------------
_COMMON = ["--do_train", "1", "--synthetic", "--batch_size", "32", "--num_neighbors", "8", "--mb_batch", "2", "--epochs", "1",
           "--synthetic_train", "256", "--synthetic_test", "100", "--n_display", "1", "--skip_nonfinite", "1"]
_TAIL = re.compile(r" ms/step\) skipped (\d+) longest run (\d+) grad norm median (\S+) max (\S+)$")
_RANK = re.compile(r"^rank (\d+) epoch 1 non-finite guard: skipped (\d+) parameters (finite|NOT FINITE) sha256 ([0-9a-f]{16})$", re.M)


def _child(cmd, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, timeout=limit + 30, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if " loss " in l]
    assert len(lines) == 8, r.stdout[-3000:]
    tails = [_TAIL.search(l) for l in lines]
    assert all(tails), lines
    losses = [float(l.split(" loss ")[1].split()[0]) for l in lines]
    skipped = [int(t.group(1)) for t in tails]
    print("\n".join(lines))
    assert "text->video R@1" in r.stdout
    return r.stdout, losses, skipped, tails


def test_main_retrieval_bertadam_graph_skips_the_blank_step(tmp_path):
    out, losses, skipped, tails = _child([sys.executable, os.path.join(ROOT, "main_retrieval.py")] + _COMMON + [
        "--output_dir", str(tmp_path), "--optimizer", "bertadam", "--hip_graph", "1", "--synthetic_blank", "3"], 540)
    assert "training step replayed as: whole" in out
    assert skipped == [0, 0, 1, 1, 1, 1, 1, 1] and [int(t.group(2)) for t in tails] == skipped
    assert [v == v for v in losses] == [True, True, False] + [True] * 5
    assert all(np.isfinite(float(t.group(3))) and np.isfinite(float(t.group(4))) for k, t in enumerate(tails) if k != 2)
    assert tails[2].group(3) == "nan"                                # a window of one step, and that step had no finite norm
    assert [(m.group(1), m.group(2), m.group(3)) for m in _RANK.finditer(out)] == [("0", "1", "finite")]
    lrs = [float(l.split(" lr ")[1].split()[0]) for l in out.splitlines() if " loss " in l]
    # the schedule stands still for the skipped step: steps 4 .. 8 use the rates of counters 2 .. 6
    want = [1e-4 * R.warmup_cosine(s / 8, 0.1) for s in (0, 1, 1, 2, 3, 4, 5, 6)]
    np.testing.assert_allclose(lrs, want, rtol=2e-3)


def test_main_retrieval_two_ranks_skip_together(tmp_path):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29653", os.path.join(ROOT, "main_retrieval.py")] + _COMMON + [
        "--output_dir", str(tmp_path), "--dist_backend", "gloo", "--optimizer", "bertadam", "--hip_graph", "1",
        "--synthetic_blank", "3:1"]
    out, losses, skipped, _ = _child(cmd, 840)
    assert skipped == [0, 0, 1, 1, 1, 1, 1, 1]
    ranks = sorted((m.group(1), m.group(2), m.group(3), m.group(4)) for m in _RANK.finditer(out))
    assert [r[:3] for r in ranks] == [("0", "1", "finite"), ("1", "1", "finite")], out[-3000:]
    assert ranks[0][3] == ranks[1][3]                                # the same parameter bits on both ranks


def test_main_retrieval_adamw_skips_on_the_host(tmp_path):
    out, losses, skipped, _ = _child([sys.executable, os.path.join(ROOT, "main_retrieval.py")] + _COMMON + [
        "--output_dir", str(tmp_path), "--optimizer", "adamw", "--synthetic_blank", "3"], 540)
    assert skipped == [0, 0, 1, 1, 1, 1, 1, 1]
    assert [v == v for v in losses] == [True, True, False] + [True] * 5
    assert [(m.group(1), m.group(2), m.group(3)) for m in _RANK.finditer(out)] == [("0", "1", "finite")]
