"""GPU: the weight EMA through the C ABI (nr_ema_update, nr_ema_swap, nr_bertadam_step_ema), through
neighborretr_amd.optim.WeightEma / BertAdam(ema=...) and through the entry point, against the fp64 restatement (tests/ema_ref.py)
and, bit for bit, against the un-fused forms.

The bar of the stand-alone form: max |got - ref| / A <= K 2^-21 after K updates, A the largest magnitude of any parameter or
shadow over the run.  Per update the rule rounds three times (the difference, 1 - d, the fused multiply-add), each rounding at
most 2^-24 of a quantity bounded by 4 A, and earlier errors shrink by d.  Measured on one MI355X, K = 40: 6.8e-8 to 4.3e-7, a
fortieth of the bar 1.907e-5 at worst; every mutant that changes the rule stands at 1.3e-4 or more
(test_standalone_form_against_the_restatement prints them)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_ref as E
import test_optim_gpu as O
from neighborretr_amd import hip, ops, optim

pytestmark = pytest.mark.gpu
ROOT = O.ROOT
DEV = "cuda"
SIZES = (4099, 1, 70000, 513, 0, 2049)         # _small_problem's, a tensor without elements, and the one whose shadow is NULL
NULL_AT = 5
GROUP_OF = [0, 1, 0, 1, 0, 1]
CLAMP = {1: 0.06}


def _views(values, misaligned):
    """Views into one zeroed flat device buffer (O._views, with room for a tensor without elements, whose data_ptr may be null)
    -> (flat, views, a mask of the flat elements no view owns)."""
    offs, off = [], 0
    for k, x in enumerate(values):
        if misaligned:
            off += (1 + k % 3 - off) % 4 or 4
        else:
            off = (off + 3) // 4 * 4
        offs.append(off)
        off += len(x)
    flat = torch.zeros(off + 4, dtype=torch.float32, device=DEV)
    free = np.ones(off + 4, dtype=bool)
    views = [flat[o:o + len(x)] for o, x in zip(offs, values)]
    for v, x, o in zip(views, values, offs):
        v.copy_(torch.from_numpy(np.ascontiguousarray(x)))
        free[o:o + len(x)] = False
        if len(x):
            assert v.data_ptr() % 4 == 0 and (v.data_ptr() % 16 != 0) == misaligned
    return flat, views, free


def _problem(seed=5, steps=5):
    rs = np.random.RandomState(seed)
    init = [(0.05 * rs.standard_normal(n)).astype(np.float32) for n in SIZES]
    shadows = [(x + 0.01 * rs.standard_normal(len(x))).astype(np.float32) for x in init]      # an average that has a past
    grads = [[(rs.standard_normal(n) * (3.0 if s % 2 else 0.01)).astype(np.float32) for n in SIZES] for s in range(steps)]
    _, _, groups, _ = O._small_problem()
    return init, shadows, grads, groups


def _ptr(t):
    return t.data_ptr() if t.numel() else 0


class Abi:
    """The C ABI directly.  mode "fused": nr_bertadam_step_ema (guarded=True: with a guard); "split": nr_bertadam_step, then
    nr_ema_update over the tensors that have a shadow."""

    def __init__(self, init, shadows, groups, decay=0.9, warmup=True, mis=(False, False), guarded=False, updates=0):
        self.flat_p, self.p, _ = _views(init, mis[0])
        self.flat_m, self.m, _ = _views([np.zeros_like(x) for x in init], mis[0])
        self.flat_v, self.v, _ = _views([np.zeros_like(x) for x in init], mis[0])
        self.flat_e, self.e, self.free_e = _views(shadows, mis[1])
        self.mis_g = mis[0]
        self.groups = [dict(O.R.GROUP_DEFAULTS, **g) for g in groups]
        self.steps = torch.zeros(len(init), dtype=torch.int32, device=DEV)
        state = hip.EmaState(decay=decay, updates=updates, warmup=int(warmup))
        self.host_state = state
        self.state = torch.frombuffer(bytearray(bytes(state)), dtype=torch.uint8).to(DEV)
        self.guard = self.ring = None
        if guarded:
            self.guard = torch.frombuffer(bytearray(bytes(hip.StepGuard(last_skipped=-1))), dtype=torch.uint8).to(DEV)
            self.ring = torch.zeros(8 * ctypes.sizeof(hip.StepRecord), dtype=torch.uint8, device=DEV)
        self.keep = []

    def step(self, grads, mode):
        T, G = len(self.p), len(self.groups)
        groups = (hip.OptimGroup * G)()
        for q, g in zip(groups, self.groups):
            q.lr, q.weight_decay, q.b1, q.b2, q.e, q.max_grad_norm, q.warmup = (g[k] for k in ("lr", "weight_decay", "b1", "b2", "e",
                                                                                           "max_grad_norm", "warmup"))
            q.t_total, q.schedule = g["t_total"], hip.SCHEDULE_IDS[g["schedule"]]
        _, g_dev, _ = _views(grads, self.mis_g)
        entries = (hip.OptimTensor * T)()
        for t, ent in enumerate(entries):
            ent.p, ent.g, ent.m, ent.v = _ptr(self.p[t]), _ptr(g_dev[t]), _ptr(self.m[t]), _ptr(self.v[t])
            ent.step, ent.n, ent.group = self.steps.data_ptr() + 4 * t, self.p[t].numel(), GROUP_OF[t]
            ent.has_clamp, ent.clamp_max = int(t in CLAMP), CLAMP.get(t, 0.0)
        n_chunks = ops.bertadam_plan(entries, groups)
        d_groups = torch.frombuffer(bytearray(bytes(groups)), dtype=torch.uint8).to(DEV)
        d_table = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(DEV)
        ws = torch.empty(max(256, ops.bertadam_workspace_bytes(T, n_chunks)), dtype=torch.uint8, device=DEV)
        self.keep = [d_groups, d_table, ws, g_dev]
        if mode == "fused":
            ptrs = (ctypes.c_uint64 * T)(*(0 if t == NULL_AT else _ptr(self.e[t]) for t in range(T)))
            d_ptrs = torch.frombuffer(bytearray(bytes(ptrs)), dtype=torch.uint8).to(DEV)
            self.keep.append(d_ptrs)
            ops.bertadam_step_ema(d_groups, G, d_table, T, n_chunks, ws, d_ptrs, self.state, guard=self.guard, ring=self.ring,
                                  global_max_norm=1.0)
        else:
            ops.bertadam_step(d_groups, G, d_table, T, n_chunks, ws, 1.0)
            averaged = [t for t in range(T) if t != NULL_AT]
            pairs = (hip.EmaTensor * len(averaged))()
            for ent, t in zip(pairs, averaged):
                ent.p, ent.ema, ent.n = _ptr(self.p[t]), _ptr(self.e[t]), self.p[t].numel()
            n_ema = ops.ema_plan(pairs, self.host_state)
            d_pairs = torch.frombuffer(bytearray(bytes(pairs)), dtype=torch.uint8).to(DEV)
            self.keep.append(d_pairs)
            ops.ema_update(d_pairs, len(averaged), n_ema, self.state)
        torch.cuda.synchronize()

    def ema_state(self):
        return hip.EmaState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def result(self):
        """Everything a step may write, as host arrays: p, m, v, shadows, the whole flat shadow buffer, counters, the state."""
        host = lambda xs: [x.cpu().numpy().copy() for x in xs]                # noqa: E731
        return dict(p=host(self.p), m=host(self.m), v=host(self.v), e=host(self.e), flat_e=self.flat_e.cpu().numpy().copy(),
                    steps=self.steps.cpu().numpy().copy(), state=self.state.cpu().numpy().copy())


def _assert_same(a, b, keys=("p", "m", "v", "e", "steps", "state")):
    for key in keys:
        if isinstance(a[key], list):
            for t, (x, y) in enumerate(zip(a[key], b[key])):
                assert np.array_equal(x, y), (key, t, int(np.sum(x != y)))
        else:
            assert np.array_equal(a[key], b[key]), key


# ---- 1. the stand-alone form against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("decay,warmup", [(0.999, True), (0.999, False), (0.5, True), (0.5, False)])
def test_standalone_form_against_the_restatement(decay, warmup):
    """40 updates of a random walk (0.05-scale values, 1e-3-scale moves), compared after every update; parameters at odd 4-byte
    offsets in half of the cases.  The mutants are held against the same device result: each must miss the bar wherever it
    changes the rule (no_warmup without warm-up, and swapped at decay 0.5 without warm-up, are the rule itself)."""
    K, sizes = 40, SIZES[:5]
    rows = E.random_walk(21, sizes, K)
    _, p, _ = _views(rows[0], misaligned=decay == 0.5)
    ema = optim.WeightEma(p, decay=decay, warmup=warmup)
    assert ema.updates() == 0 and ema.last_decay() is None
    ref = E.State(rows[0], decay, warmup)
    mutants = {m: E.State(rows[0], decay, warmup) for m in E.MUTANTS}
    err, err_m = 0.0, dict.fromkeys(E.MUTANTS, 0.0)
    for k in range(1, K + 1):
        for dst, x in zip(p, rows[k]):
            dst.copy_(torch.from_numpy(x))
        ema.update()
        E.update(ref, rows[k])
        got = [e.cpu().numpy() for e in ema.shadows]
        err = max(err, E.scaled_error(got, ref.e, rows)[0])
        for m, st in mutants.items():
            E.update(st, rows[k], before=rows[k - 1], mutate=(m,))
            err_m[m] = max(err_m[m], E.scaled_error(got, st.e, rows)[0])
    bar = K * 2.0 ** -21
    print(f"decay {decay} warmup {warmup}: max |got - ref| / A = {err:.3e} (bar {bar:.3e})")
    for m in E.MUTANTS:
        print(f"    mutant {m}: {err_m[m]:.3e}")
    assert err <= bar, (err, bar)
    for m in E.MUTANTS:
        same_rule = (m == "no_warmup" and not warmup) or (m == "swapped" and decay == 0.5 and not warmup)
        assert same_rule or err_m[m] > bar, (m, err_m[m], bar)
    assert ema.updates() == K == ref.updates and ema.last_decay() == ref.last_decay
    state = ema._read_state()
    assert state.omd == np.float32(1.0 - ref.last_decay) and state.decay == decay and state.warmup == int(warmup)
    for dst, x in zip(p, rows[K]):
        assert np.array_equal(dst.cpu().numpy(), x)                          # the parameters are only read


# ---- 2. fused = un-fused + stand-alone, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
def test_fused_form_is_the_unfused_form_plus_the_standalone_form(guarded):
    init, shadows, grads, groups = _problem()
    fused = Abi(init, shadows, groups, guarded=guarded, updates=3)
    split = Abi(init, shadows, groups, updates=3)
    for row in grads:
        fused.step(row, "fused")
        split.step(row, "split")
        _assert_same(fused.result(), split.result())
    got = fused.result()
    assert fused.ema_state().updates == 3 + len(grads) == split.ema_state().updates
    assert not np.array_equal(got["e"][0], shadows[0]) and not np.array_equal(got["p"][0], init[0])
    # the tensor with the NULL shadow: its p, m, v moved, the buffer that would have been its shadow and every element between
    # the shadows are as they were
    assert not np.array_equal(got["p"][NULL_AT], init[NULL_AT])
    assert np.array_equal(got["e"][NULL_AT], shadows[NULL_AT])
    assert not got["flat_e"][fused.free_e].any()
    if guarded:
        guard = hip.StepGuard.from_buffer_copy(fused.guard.cpu().numpy().tobytes())
        assert (guard.attempts, guard.skipped) == (len(grads), 0)


# ---- 3. alignment ------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_alignment():
    """p, m, v and shadows 16-byte aligned (the vector path), all at odd 4-byte offsets (the dword path), and p, m, v aligned
    with the shadows at odd offsets (the shadow as four dwords per lane): same values, same bits."""
    init, shadows, grads, groups = _problem(seed=8)
    results = []
    for mis in ((False, False), (True, True), (False, True)):
        for mode in ("fused", "split"):
            run = Abi(init, shadows, groups, mis=mis)
            for row in grads:
                run.step(row, mode)
            results.append(run.result())
    for other in results[1:]:
        _assert_same(results[0], other)


# ---- 4. the guard --------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_moves_no_shadow_and_is_no_update():
    init, shadows, grads, groups = _problem(seed=9, steps=6)
    grads[1][2][69999] = np.nan
    grads[3][0][17] = np.inf
    bad = (1, 3)
    run = Abi(init, shadows, groups, guarded=True)
    for s, row in enumerate(grads):
        before = run.result()
        run.step(row, "fused")
        after = run.result()
        if s in bad:
            _assert_same(before, after)                                       # shadows, state and p, m, v, counters too
            assert np.array_equal(before["flat_e"], after["flat_e"])
        else:
            assert run.ema_state().updates == hip.EmaState.from_buffer_copy(before["state"].tobytes()).updates + 1
            assert not np.array_equal(before["e"][2], after["e"][2])
    assert run.ema_state().updates == 4
    guard = hip.StepGuard.from_buffer_copy(run.guard.cpu().numpy().tobytes())
    assert (guard.attempts, guard.skipped) == (6, 2)
    good = Abi(init, shadows, groups)
    for s, row in enumerate(grads):
        if s not in bad:
            good.step(row, "fused")
    _assert_same(run.result(), good.result())


# ---- 5. graph ------------------------------------------------------------------------------------------------------------------
def _attached(init, groups, group_of, decay=0.9, names=False, skip=(3,)):
    """Parameters, a WeightEma over all of them but `skip` (NULL entries of the step's table) and the BertAdam that drives it."""
    p = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in init]
    known = [(f"w{t}", x) if names else x for t, x in enumerate(p) if t not in skip]
    ema = optim.WeightEma(known, decay=decay)
    pg = [dict(params=[x for x, q in zip(p, group_of) if q == gi], **dict(O.R.GROUP_DEFAULTS, **g)) for gi, g in enumerate(groups)]
    opt = optim.BertAdam(pg, lr=1e-4, global_max_norm=1.0, clamp_max={p[1]: 0.06}, ema=ema)
    return p, ema, opt


def _steps(p, opt, rows):
    for row in rows:
        for x, g in zip(p, row):
            x.grad = torch.from_numpy(g).to(DEV)
        opt.step()
    torch.cuda.synchronize()


def _full_state(p, ema, opt):
    return O._opt_state(opt, p) + ([e.cpu().numpy() for e in ema.shadows],)


def test_five_eager_steps_equal_five_replays_of_a_captured_step():
    init, grads, groups, group_of = O._small_problem()
    p, ema, opt = _attached(init, groups, group_of)
    with pytest.raises(RuntimeError, match="one driver"):
        ema.update()                                                          # attached: the optimizer's step is the driver
    _steps(p, opt, grads)
    want, want_updates = _full_state(p, ema, opt), ema.updates()
    assert want_updates == 5 and not np.array_equal(want[3][0], init[0])
    assert ema.shadow(p[3]) is None and len(ema.shadows) == 3

    p, ema, opt = _attached(init, groups, group_of)
    static = [torch.zeros_like(x) for x in p]
    for x, g in zip(p, static):
        x.grad = g
    opt.prepare()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        live = opt.issue()
    torch.cuda.synchronize()
    assert ema.updates() == 0 and all(np.array_equal(e.cpu().numpy(), x) for e, x in zip(ema.shadows, init))   # capturing ran nothing
    for row in grads:
        for dst, g in zip(static, row):
            dst.copy_(torch.from_numpy(g))
        graph.replay()
        opt.advance(live)
    torch.cuda.synchronize()
    got = _full_state(p, ema, opt)
    for x, y in zip(got, want):
        for u, w in zip(x, y):
            assert np.array_equal(u, w)
    assert ema.updates() == want_updates and ema.last_decay() == E.decay_at(0.9, True, 4)


# ---- 6. swap -------------------------------------------------------------------------------------------------------------------
def test_two_swaps_restore_every_bit_and_applied_restores_when_its_body_raises():
    rows = E.random_walk(31, SIZES[:5], 3)
    _, p, _ = _views(rows[0], misaligned=True)
    ema = optim.WeightEma(p, decay=0.5, warmup=False)
    for k in (1, 2, 3):
        for dst, x in zip(p, rows[k]):
            dst.copy_(torch.from_numpy(x))
        ema.update()
    params = [x.cpu().numpy() for x in p]
    shadows = [e.cpu().numpy() for e in ema.shadows]
    assert not np.array_equal(params[0], shadows[0])
    state = ema._state.cpu().numpy().copy()
    versions = [x._version for x in p]
    ema.swap()
    assert all(np.array_equal(x.cpu().numpy(), e) for x, e in zip(p, shadows))
    assert all(np.array_equal(e.cpu().numpy(), x) for e, x in zip(ema.shadows, params))
    assert all(x._version > v for x, v in zip(p, versions))
    ema.swap()
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(p, params))
    assert all(np.array_equal(e.cpu().numpy(), y) for e, y in zip(ema.shadows, shadows))
    assert np.array_equal(ema._state.cpu().numpy(), state)                    # a swap touches no state

    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with ema.applied():
            assert all(np.array_equal(x.cpu().numpy(), e) for x, e in zip(p, shadows))
            with pytest.raises(RuntimeError, match="nest"):
                with ema.applied():
                    pass
            with pytest.raises(RuntimeError, match="applied"):
                ema.update()
            raise Boom()
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(p, params))
    assert all(np.array_equal(e.cpu().numpy(), y) for e, y in zip(ema.shadows, shadows))
    with ema.applied():                                                       # and it can be entered again
        pass
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(p, params))


def test_swap_moves_the_version_counters_and_the_derived_weights():
    from neighborretr_amd import head
    m = O._model()
    ema = optim.WeightEma(m.named_parameters(), decay=0.9)
    with torch.no_grad():
        for k, e in enumerate(ema.shadows):
            e.mul_(1.0 + 0.01 * (1 + k % 3))                                  # an average that differs from the weights
    old_shadows = {n: e.clone() for n, e in zip(ema.names, ema.shadows)}
    before = m.scorer_weights("text_weight_fc")
    assert m.scorer_weights("text_weight_fc") is before
    versions = {n: p._version for n, p in m.named_parameters()}
    ema.swap()
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), old_shadows[n]) and p._version > versions[n], n
    after = m.scorer_weights("text_weight_fc")
    assert after is not before
    mlp = m.text_weight_fc
    fresh = head.ScorerWeights(mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)
    assert torch.equal(after.w1_hi, fresh.w1_hi) and torch.equal(after.w1_lo, fresh.w1_lo)
    assert not (torch.equal(after.w1_hi, before.w1_hi) and torch.equal(after.w1_lo, before.w1_lo))


def _graphed_run(with_block):
    """Six steps of GraphedStep(optimizer=BertAdam(ema=...)); with_block: between steps 3 and 4 the test set's similarity is
    computed with the average applied -> (parameters, moments, shadows) as host arrays, the number of updates."""
    sys.path.insert(0, ROOT)
    from main_retrieval import GraphedStep
    from util import problem
    B, Nt, Nv, M = 32, 24, 12, 64
    x = problem(1003, B, Nt, Nv, M, device=DEV)
    m = O._model(K=8)
    m.mb_feat_t, m.mb_feat_v = x["mb_feat_t"].clone(), x["mb_feat_v"].clone()
    m.mb_mask_t, m.mb_mask_v = x["mb_mask_t"].clone(), x["mb_mask_v"].clone()
    m.mb_ind = torch.arange(5000, 5000 + M, device=DEV)
    params = [p for _, p in m.named_parameters()]
    ema = optim.WeightEma(m.named_parameters(), decay=0.9)
    opt, _, _ = optim.prep_optimizer(O._Args, m, 6, 0, global_max_norm=1.0, clamp_logit_scale=True, ema=ema)
    assert opt.ema is ema

    def batch(r):
        return (x["text_feat"] + 0.01 * r, x["text_mask"], x["video_feat"] + 0.01 * r, x["video_mask"], x["idx"] + 100 * r)
    step = GraphedStep(m, batch(0), params, optimizer=opt)
    sims = None
    for r in range(6):
        if r == 3 and with_block:
            raw = [p.detach().clone() for p in params]
            with ema.applied():
                assert any(not torch.equal(p.detach(), q) for p, q in zip(params, raw))
                m.eval()
                with torch.no_grad():
                    sims = m.get_similarity_logits(x["text_feat"], x["video_feat"], x["text_mask"], x["video_mask"])
                m.train()
            assert all(torch.equal(p.detach(), q) for p, q in zip(params, raw))
        step.run(batch(r))
    torch.cuda.synchronize()
    assert sims is None or all(bool(torch.isfinite(s).all()) for s in (sims if isinstance(sims, (tuple, list)) else [sims])
                               if isinstance(s, torch.Tensor))
    return _full_state(params, ema, opt), ema.updates()


def test_an_applied_block_between_graphed_steps_changes_nothing():
    plain, n_plain = _graphed_run(False)
    block, n_block = _graphed_run(True)
    assert n_plain == n_block == 6
    for name, x, y in zip(("p", "m", "v", "shadow"), plain, block):
        for t, (u, w) in enumerate(zip(x, y)):
            assert np.array_equal(u, w), (name, t)
    assert any(not np.array_equal(e, p) for e, p in zip(plain[3], plain[0]))  # the average lags the weights


# ---- 7. state dict -------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_continues_bit_for_bit():
    init, grads, groups, group_of = O._small_problem(seed=6)
    p, ema, opt = _attached(init, groups, group_of, names=True)
    _steps(p, opt, grads)
    want = _full_state(p, ema, opt)

    p, ema, opt = _attached(init, groups, group_of, names=True)
    _steps(p, opt, grads[:3])
    sd_opt, sd_ema = opt.state_dict(), ema.state_dict()
    assert set(sd_ema) == {"decay", "warmup", "updates", "shadows"} and set(sd_ema["shadows"]) == {"w0", "w1", "w2"}
    assert (sd_ema["decay"], sd_ema["warmup"], sd_ema["updates"]) == (0.9, True, 3)
    assert all(set(s) == {"step", "next_m", "next_v"} for s in sd_opt["state"].values())      # the optimizer's keys are unchanged
    sd_opt = {"state": {k: {"step": s["step"], "next_m": s["next_m"].cpu(), "next_v": s["next_v"].cpu()}
                        for k, s in sd_opt["state"].items()}, "param_groups": sd_opt["param_groups"]}
    sd_ema = dict(sd_ema, shadows={k: v.cpu() for k, v in sd_ema["shadows"].items()})          # as read back from disk
    now = [x.detach().cpu().numpy() for x in p]
    p2, ema2, opt2 = _attached(now, groups, group_of, decay=0.5, names=True)
    where = [e.data_ptr() for e in ema2.shadows]
    state_at = ema2._state.data_ptr()
    opt2.load_state_dict(sd_opt)
    ema2.load_state_dict(sd_ema)
    assert where == [e.data_ptr() for e in ema2.shadows] and state_at == ema2._state.data_ptr()
    assert ema2.updates() == 3 and ema2.decay == 0.9 and ema2.last_decay() == E.decay_at(0.9, True, 2)
    _steps(p2, opt2, grads[3:])
    got = _full_state(p2, ema2, opt2)
    for x, y in zip(got, want):
        for u, w in zip(x, y):
            assert np.array_equal(u, w)
    assert ema2.updates() == 5
    with pytest.raises(KeyError):
        ema2.load_state_dict(dict(sd_ema, shadows={"w0": sd_ema["shadows"]["w0"]}))


# ---- training.train_epoch ----------------------------------------------------------------------------------------------------------
def test_train_epoch_honours_args_weight_ema(caplog):
    """The reference-signature loop with a torch optimizer: one stand-alone update per step, every validation a second time with
    the average applied (header tagged EMA), the parameters back in place afterwards."""
    import logging
    import test_training_gpu as TG
    from neighborretr_amd import synth, training
    N, B = 96, 16
    t, v, tm, vm = (torch.from_numpy(a) for a in synth.make_samples(94, "train", N, TG.Nt, TG.Nv))
    model = TG._model(mb_batch=3, batch_size=B, num_neighbors=6)
    loader = TG.Loader(TG._batches(t, v, tm, vm, torch.arange(N), B))
    training.MemoryBankManager(TG._args()).load_memory_bank(model, loader, torch.device(DEV), epoch=1)
    ema = optim.WeightEma(model.named_parameters(), decay=0.9)
    args = TG._args(weight_ema=ema)
    optimizer = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-2)
    val = TG.Loader(TG._batches(t[:40], v[:40], tm[:40], vm[:40], torch.arange(40), 20))
    with caplog.at_level(logging.INFO, logger="test_training"):
        training.train_epoch(1, args, model, loader, torch.device(DEV), 1, optimizer, None, 0, len(loader), val)
    assert ema.updates() == len(loader) == 6
    headers = [r.getMessage() for r in caplog.records if r.getMessage().startswith("EVALUATION RESULTS")]
    assert headers == ["EVALUATION RESULTS", "EVALUATION RESULTS [EMA]"] * 2, headers       # validation at steps 1 and 6
    moved = [n for (n, p), e in zip(model.named_parameters(), ema.shadows) if not torch.equal(p.detach(), e)]
    assert len(moved) > 10                                                   # the average lags the weights that train
    ref = E.State([np.zeros(1)], 0.9, True)
    for _ in range(6):
        E.update(ref, [np.zeros(1)])
    assert ema.last_decay() == ref.last_decay


# ---- 8. the entry point ----------------------------------------------------------------------------------------------------------
RK = re.compile(r"text->video R@1 .*$")


def _entry(out_dir, *extra, nan_at=()):
    """O._entry's run (B = 32, 16 steps, --synthetic_test 200) in a fresh child under its own time limit; nan_at: the 0-based
    steps whose loss is expected not to be a number (a blanked step under the guard)."""
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_train", "1", "--synthetic", "--batch_size", "32",
           "--num_neighbors", "8", "--mb_batch", "2", "--epochs", "1", "--synthetic_train", "512", "--synthetic_test", "200",
           "--n_display", "1", "--output_dir", str(out_dir)] + list(extra)
    r = subprocess.run(["timeout", "-k", "10", "540"] + cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in r.stdout.splitlines() if " loss " in l]
    assert len(losses) == 16 and [k for k, v in enumerate(losses) if not (v == v and v < 1e4)] == list(nan_at), losses
    return r.stdout


def _ema_lines(out):
    tagged = [l for l in out.splitlines() if " EMA text->video R@1 " in l]
    counts = [l for l in out.splitlines() if " ema updates " in l]
    assert len(tagged) == 1 and len(counts) == 1, out[-3000:]
    n, d = counts[0].split(" ema updates ")[1].split(" decay ")
    assert re.search(r"rank 0 epoch 1 ema sha256 [0-9a-f]{16}$", out, flags=re.M), out[-2000:]
    return RK.search(tagged[0]).group(0), int(n), float(d)


def _load_pair(tmp_path):
    raw = torch.load(os.path.join(str(tmp_path), "pytorch_model.bin.0"), map_location="cpu")
    avg = torch.load(os.path.join(str(tmp_path), "pytorch_model_ema.bin.0"), map_location="cpu")
    assert list(raw) == list(avg)
    assert any(not torch.equal(raw[k], avg[k]) for k in raw)
    return raw, avg


def test_main_retrieval_with_an_ema(tmp_path):
    """Fresh child processes, one after the other: bertadam eager and graphed (the average inside the optimizer's launches),
    adamw (the stand-alone update after the step, and with --permutation the "EMA - model" lines), bertadam with the guard and a blanked step (one update fewer); then the saved
    average evaluated through --init_model reproduces the run's EMA line."""
    for hip_graph in ("0", "1"):
        out_dir = tmp_path / f"g{hip_graph}"
        out = _entry(out_dir, "--optimizer", "bertadam", "--hip_graph", hip_graph, "--ema_decay", "0.9", "--save_model")
        line, n, d = _ema_lines(out)
        print(f"--hip_graph {hip_graph}: {line} | updates {n} decay {d}")
        assert n == 16 and d == round(E.decay_at(0.9, True, 15), 6)
        _load_pair(out_dir)
    # the saved average through --init_model: 0 missing / 0 unexpected keys and the same R@K line
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_eval", "1", "--synthetic", "--batch_size", "32",
           "--num_neighbors", "8", "--synthetic_test", "200", "--output_dir", str(out_dir), "--init_model",
           os.path.join(str(out_dir), "pytorch_model_ema.bin.0")]
    r = subprocess.run(["timeout", "-k", "10", "540"] + cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "init_model: 0 missing / 0 unexpected keys" in r.stdout, r.stdout[-2000:]
    again = RK.search([l for l in r.stdout.splitlines() if "text->video R@1" in l][0]).group(0)
    assert again == line, (again, line)

    out = _entry(tmp_path / "adamw", "--optimizer", "adamw", "--ema_decay", "0.9", "--permutation", "64")
    line, n, d = _ema_lines(out)
    print(f"adamw: {line} | updates {n} decay {d}")
    assert n == 16
    versus = [l for l in out.splitlines() if " EMA - model " in l]               # the average against the raw model, per direction
    assert len(versus) == 2 and all("paired permutation test vs model, 64 permutations" in l for l in versus), versus

    out = _entry(tmp_path / "guard", "--optimizer", "bertadam", "--ema_decay", "0.9", "--skip_nonfinite", "1",
                 "--synthetic_blank", "5", nan_at=(4,))
    line, n, d = _ema_lines(out)
    print(f"guarded, step 5 blanked: {line} | updates {n} decay {d}")
    assert n == 15 and "skipped 1" in out


def test_main_retrieval_two_ranks_agree_on_the_ema(tmp_path):
    """Two gloo ranks on one card, --hip_graph 1 (the form of test_main_retrieval_two_ranks_with_bertadam_in_the_graphed_step):
    the shadows' digests of the two ranks are the same."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29661", os.path.join(ROOT, "main_retrieval.py"), "--do_train", "1", "--synthetic",
           "--batch_size", "32", "--num_neighbors", "8", "--mb_batch", "2", "--epochs", "1", "--synthetic_train", "256",
           "--synthetic_test", "100", "--n_display", "1", "--output_dir", str(tmp_path), "--dist_backend", "gloo",
           "--hip_graph", "1", "--optimizer", "bertadam", "--ema_decay", "0.9"]
    r = subprocess.run(["timeout", "-k", "10", "840"] + cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    digests = dict(re.findall(r"rank (\d) epoch 1 ema sha256 ([0-9a-f]{16})", r.stdout))
    assert set(digests) == {"0", "1"} and digests["0"] == digests["1"], digests
    assert " ema updates 8 " in r.stdout and " EMA text->video R@1 " in r.stdout, r.stdout[-2000:]
