"""GPU: the multi-tensor BertAdam kernels (csrc/nr_optim.hip) through the C ABI and through neighborretr_amd.optim.BertAdam,
against the values captured from the unmodified reference (tests/golden/bertadam_small.npz) and the fp64 restatement
(tests/bertadam_ref.py); determinism, graph replay, version counters, the step graph with the update inside, state dicts and
the entry point.

Distance everywhere: max |a - b| / (|b| + 1e-3) over all elements of p, m and v.  Bars: 4 x d_ref (the reference's own distance
from the restatement, stored with the fixture) for the fixture; for generated cases 4 x the distance that the same formulas in
fp32 torch ops on the GPU have from the restatement ON THE SAME CASE, computed in the test.  Every generated case holds at
least 4096 elements: both sides' distance is a maximum over the elements, and only with enough of them is the fp32-torch
figure a measure of fp32 rounding rather than of one element's luck; smaller tables are held to the fixture's bar instead.
The fp32 learning rate the device computes is checked through the parameters it moves; the lr assertions read the host's
get_lr() / group_lr()."""
import ctypes
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bertadam_ref as R
from neighborretr_amd import hip, ops, optim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
LN100 = math.log(100.0)


def _capture_module():
    spec = importlib.util.spec_from_file_location("capture_bertadam_golden", os.path.join(ROOT, "tools", "capture_bertadam_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- three ways to take a step ------------------------------------------------------------------------------------------
class AbiStepper:
    """The C ABI directly: plan on the host, upload, nr_bertadam_step.  p / m / v: lists of device tensors (views allowed);
    grads per call."""

    def __init__(self, p, group_of, groups, clamp_max=None, global_max_norm=None):
        self.p, self.group_of = p, list(group_of)
        self.groups = [dict(R.GROUP_DEFAULTS, **g) for g in groups]
        self.m = [torch.zeros_like(x) for x in p]
        self.v = [torch.zeros_like(x) for x in p]
        self.steps = torch.zeros(len(p), dtype=torch.int32, device=DEV)
        self.clamp_max = dict(clamp_max or {})
        self.gmn = -1.0 if global_max_norm is None else float(global_max_norm)
        self.keep = []

    def step(self, grads):
        live = [t for t, g in enumerate(grads) if g is not None]
        G = len(self.groups)
        groups = (hip.OptimGroup * G)()
        for q, g in zip(groups, self.groups):
            q.lr, q.weight_decay, q.b1, q.b2, q.e, q.max_grad_norm, q.warmup = (g[k] for k in ("lr", "weight_decay", "b1", "b2", "e",
                                                                                           "max_grad_norm", "warmup"))
            q.t_total, q.schedule = g["t_total"], hip.SCHEDULE_IDS[g["schedule"]]
        entries = (hip.OptimTensor * len(live))()
        for ent, t in zip(entries, live):
            ent.p, ent.g, ent.m, ent.v = self.p[t].data_ptr(), grads[t].data_ptr(), self.m[t].data_ptr(), self.v[t].data_ptr()
            ent.step = self.steps.data_ptr() + 4 * t
            ent.n, ent.group = self.p[t].numel(), self.group_of[t]
            ent.has_clamp, ent.clamp_max = int(t in self.clamp_max), self.clamp_max.get(t, 0.0)
        n_chunks = ops.bertadam_plan(entries, groups)
        d_groups = torch.frombuffer(bytearray(bytes(groups)), dtype=torch.uint8).to(DEV)
        d_table = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(DEV)
        ws = torch.empty(max(256, ops.bertadam_workspace_bytes(len(live), n_chunks)), dtype=torch.uint8, device=DEV)
        self.keep = [d_groups, d_table, ws]
        ops.bertadam_step(d_groups, G, d_table, len(live), n_chunks, ws, self.gmn)

    def state(self):
        return ([x.cpu().numpy() for x in self.p], [x.cpu().numpy() for x in self.m], [x.cpu().numpy() for x in self.v])


class TorchEager:
    """The same formulas in fp32 torch ops on the GPU: the yardstick of the generated cases."""

    def __init__(self, p, group_of, groups, clamp_max=None, global_max_norm=None):
        self.p = [x.clone() for x in p]
        self.m = [torch.zeros_like(x) for x in p]
        self.v = [torch.zeros_like(x) for x in p]
        self.step_of = [0] * len(p)
        self.group_of, self.groups = list(group_of), [dict(R.GROUP_DEFAULTS, **g) for g in groups]
        self.clamp_max, self.gmn = dict(clamp_max or {}), global_max_norm

    def step(self, grads):
        live = [t for t, g in enumerate(grads) if g is not None]
        gs = {t: grads[t].clone() for t in live}
        if self.gmn is not None and self.gmn > 0:
            total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(gs[t]) for t in live]))
            c = torch.clamp(self.gmn / (total + 1e-6), max=1.0)
            for t in live:
                gs[t].mul_(c)
        for t in live:
            grp = self.groups[self.group_of[t]]
            g = gs[t]
            if grp["max_grad_norm"] > 0:
                g.mul_(torch.clamp(grp["max_grad_norm"] / (torch.linalg.vector_norm(g) + 1e-6), max=1.0))
            self.m[t].mul_(grp["b1"]).add_(g, alpha=1 - grp["b1"])
            self.v[t].mul_(grp["b2"]).addcmul_(g, g, value=1 - grp["b2"])
            u = self.m[t] / (self.v[t].sqrt() + grp["e"])
            if grp["weight_decay"] > 0:
                u += grp["weight_decay"] * self.p[t]
            self.p[t].add_(-(R.scheduled_lr(grp, self.step_of[t]) * u))
            if t in self.clamp_max:
                self.p[t].clamp_(max=self.clamp_max[t])
            self.step_of[t] += 1

    def state(self):
        return ([x.cpu().numpy() for x in self.p], [x.cpu().numpy() for x in self.m], [x.cpu().numpy() for x in self.v])


def _make_optimizer(p, group_of, groups, clamp_max=None, global_max_norm=None):
    """optim.BertAdam over the parameters p (torch.nn.Parameter list) with the per-group settings of `groups`."""
    pg = []
    for gi, g in enumerate(groups):
        g = dict(R.GROUP_DEFAULTS, **g)
        pg.append(dict(params=[x for x, q in zip(p, group_of) if q == gi], **g))
    pg = [g for g in pg if g["params"]]
    return optim.BertAdam(pg, lr=1e-4, global_max_norm=global_max_norm,
                          clamp_max={p[t]: bound for t, bound in (clamp_max or {}).items()})


def _device_steps(opt, p):
    """The device step counters in the order of p (the optimizer keeps them in the order of its groups)."""
    steps = opt._dev["steps"].cpu().tolist()
    return [steps[opt._index[id(x)]] for x in p]


def _opt_state(opt, p):
    m = [opt.state[x]["next_m"].cpu().numpy() if len(opt.state[x]) else np.zeros(tuple(x.shape), np.float32) for x in p]
    v = [opt.state[x]["next_v"].cpu().numpy() if len(opt.state[x]) else np.zeros(tuple(x.shape), np.float32) for x in p]
    return [x.detach().cpu().numpy() for x in p], m, v


# ---- the fixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["A", "B"])
@pytest.mark.parametrize("via", ["abi", "optimizer"])
def test_fixture_step_by_step(run, via):
    C = _capture_module()
    z = np.load(os.path.join(ROOT, "tests", "golden", "bertadam_small.npz"))
    seed = int(z["seed"])
    init, grads = C.initial_params(seed), C.gradients(seed)
    groups = [dict(g, **C.COMMON) for g in C.GROUPS]
    clamp = {C.CLAMP_INDEX: C.CLAMP_MAX}
    gmn = 1.0 if run == "A" else None
    bar = 4.0 * float(z[f"d_ref_{run}"])
    ref = R.State(init, C.GROUP_OF, groups, clamp_max=clamp)
    p = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in init]
    if via == "abi":
        stepper = AbiStepper([x.data for x in p], C.GROUP_OF, groups, clamp, gmn)
    else:
        opt = _make_optimizer(p, C.GROUP_OF, groups, clamp, gmn)
    for s in range(C.N_STEPS):
        g_dev = [None if g is None else torch.from_numpy(g).to(DEV) for g in grads[s]]
        lr_before = ref.lr()
        R.step(ref, grads[s], global_max_norm=gmn)
        if via == "abi":
            stepper.step(g_dev)
            got = stepper.state()
            steps = stepper.steps.cpu().tolist()
        else:
            for x, g in zip(p, g_dev):
                x.grad = g
            opt.step()
            got = _opt_state(opt, p)
            steps = _device_steps(opt, p)
            lr = opt.get_lr()
            if s + 1 in C.RECORD:
                np.testing.assert_allclose(lr, z[f"{run}_lr_{s + 1}"], rtol=1e-12)
        assert steps == ref.step, (s, steps, ref.step)
        for x, g in zip(g_dev, grads[s]):
            assert x is None or np.array_equal(x.cpu().numpy(), g)              # gradients are read, never written
        d = R.state_distance(*got, ref)
        print(f"run {run} via {via} step {s + 1}: vs restatement {d:.3e} (bar {bar:.3e})")
        assert d <= bar, (s, d, bar)
        if s == 0:                                # the first step under warm-up has learning rate 0: no parameter moves
            assert lr_before == [0.0] * len(init)
            assert all(np.array_equal(a, b) for a, b in zip(got[0], init))
        if s + 1 in C.RECORD:
            class Stored:
                p = [z[f"{run}_p_{s + 1}_{t}"] for t in range(len(init))]
                m = [z[f"{run}_m_{s + 1}_{t}"] for t in range(len(init))]
                v = [z[f"{run}_v_{s + 1}_{t}"] for t in range(len(init))]
            d = R.state_distance(*got, Stored)
            print(f"run {run} via {via} step {s + 1}: vs stored reference {d:.3e} (bar {bar:.3e})")
            assert d <= bar, (s, d, bar)
    assert float(got[0][C.CLAMP_INDEX][0]) <= np.float32(LN100)


# ---- seeded sweep -------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 5, 7, 64, 127, 255, 256, 1021, 4093, 4096, 4097, 8191, 8209, 65537, 131071, 2 ** 20, 2 ** 20 + 3]
N_CASES = 44


def _sweep_case(i):
    rs = np.random.RandomState(9000 + i)
    n_tensors = [1, 2, 3, 17, 85, 300][i % 6] if i < 36 else int(rs.randint(1, 301))
    big = [4099, 8209, 65537, 131071, 2 ** 20, 2 ** 20 + 3][(i // 2) % 6]
    sizes = [big] + [int(SIZES[rs.randint(0, 15 if n_tensors > 20 else 17)]) for _ in range(n_tensors - 1)]
    order = rs.permutation(n_tensors)
    sizes = [sizes[k] for k in order]                              # the large tensor anywhere in the table
    schedules = ["warmup_cosine", "warmup_constant", "warmup_linear"]
    n_groups = 1 + i % 4
    groups = []
    for q in range(n_groups):
        groups.append(dict(lr=[1e-4, 1e-7, 3e-3][(i + q) % 3], weight_decay=[0.2, 0.0][(i + q) % 2],
                           schedule=schedules[(i + q) % 3], warmup=[0.1, 0.25, 0.0][(i // 3 + q) % 3],
                           t_total=-1 if (i + q) % 5 == 4 else 5 + (i + q) % 4, b1=0.9, b2=[0.98, 0.999][q % 2], e=1e-6,
                           max_grad_norm=-1 if (i + q) % 4 == 3 else [1.0, 0.05][(i + q) % 2]))
    group_of = [int(rs.randint(0, n_groups)) for _ in range(n_tensors)]
    gmn = [None, 1.0, 0.3][i % 3]
    clamp = {0: 0.01} if i % 4 == 1 else {}
    misaligned = i % 2 == 0                                        # views at 4-byte-aligned, non-16-byte-aligned offsets
    return dict(rs=rs, sizes=sizes, groups=groups, group_of=group_of, gmn=gmn, clamp=clamp, misaligned=misaligned,
                none_at=(1, n_tensors - 1) if n_tensors > 1 else None, zero_at=(2, 0), scale=[10.0, 0.01, 1.0][i % 3])


def _views(flat_values, sizes, misaligned):
    """Views into one flat device buffer; `misaligned`: every view starts at an element offset that is odd modulo 4."""
    offs, off = [], 0
    for k, n in enumerate(sizes):
        if misaligned:
            off += (1 + k % 3 - off) % 4 or 4
        offs.append(off)
        off += n
    flat = torch.zeros(off + 4, dtype=torch.float32, device=DEV)
    views = [flat[o:o + n] for o, n in zip(offs, sizes)]
    for v, x in zip(views, flat_values):
        v.copy_(torch.from_numpy(x))
    if misaligned:
        assert all(v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0 for v in views)
    return flat, views


@pytest.mark.parametrize("i", range(N_CASES))
def test_sweep_against_the_restatement(i):
    case = _sweep_case(i)
    rs, sizes = case["rs"], case["sizes"]
    assert sum(sizes) >= 4096
    init = [(0.05 * rs.standard_normal(n)).astype(np.float32) for n in sizes]
    ref = R.State(init, case["group_of"], case["groups"], clamp_max=case["clamp"])
    _, p = _views(init, sizes, case["misaligned"])
    abi = AbiStepper(p, case["group_of"], case["groups"], case["clamp"], case["gmn"])
    if case["misaligned"]:                                         # the moments as misaligned views too
        _, abi.m = _views([np.zeros(n, np.float32) for n in sizes], sizes, True)
        _, abi.v = _views([np.zeros(n, np.float32) for n in sizes], sizes, True)
    eager = TorchEager(p, case["group_of"], case["groups"], case["clamp"], case["gmn"])
    for s in range(3):
        grads = [(rs.standard_normal(n) * case["scale"] * (1.0 if s != 1 else 0.02)).astype(np.float32) for n in sizes]
        if case["zero_at"][0] == s:
            grads[case["zero_at"][1]][:] = 0
        if case["none_at"] is not None and case["none_at"][0] == s:
            grads[case["none_at"][1]] = None
        _, g_views = _views([g if g is not None else np.zeros(n, np.float32) for g, n in zip(grads, sizes)], sizes, case["misaligned"])
        g_dev = [None if g is None else v for g, v in zip(grads, g_views)]
        before = [None if g is None else g.clone() for g in g_dev]
        R.step(ref, grads, global_max_norm=case["gmn"])
        abi.step(g_dev)
        eager.step(g_dev)
        assert all(a is None or torch.equal(a, b) for a, b in zip(g_dev, before))
        assert abi.steps.cpu().tolist() == ref.step
        d_hip, d_torch = R.state_distance(*abi.state(), ref), R.state_distance(*eager.state(), ref)
        print(f"case {i} step {s}: hip {d_hip:.3e}  fp32 torch {d_torch:.3e}")
        assert d_hip <= 4.0 * d_torch, (i, s, d_hip, d_torch)


# Tables too small for the fp32-torch yardstick (its maximum runs over a handful of elements): one tensor of one element, tables
# made only of tensors below one chunk (every chunk a tail, as many chunks as tensors), a tensor of exactly one chunk less / plus
# one element.  Bar: the fixture's, 4 x d_ref of the run with the same clipping (A: global clip on, B: off).
SMALL_TABLES = [[1], [1, 1, 1], [2], [3, 5, 7, 127, 255], [4095], [4096], [4097], [1, 4095, 1, 2, 1021, 64] * 7, [5] * 300]


@pytest.mark.parametrize("k", range(2 * len(SMALL_TABLES)))
def test_small_tables_against_the_restatement(k):
    sizes, clip = SMALL_TABLES[k // 2], k % 2 == 0
    z = np.load(os.path.join(ROOT, "tests", "golden", "bertadam_small.npz"))
    bar = 4.0 * float(z["d_ref_A" if clip else "d_ref_B"])
    rs = np.random.RandomState(7000 + k)
    groups = [dict(lr=1e-4, weight_decay=0.2, schedule="warmup_cosine", warmup=0.1, t_total=12, b2=0.98),
              dict(lr=1e-4, weight_decay=0.0, schedule="warmup_linear", warmup=0.25, t_total=6, b2=0.98, max_grad_norm=0.5)]
    group_of = [t % 2 for t in range(len(sizes))]
    init = [(0.05 * rs.standard_normal(n)).astype(np.float32) for n in sizes]
    ref = R.State(init, group_of, groups)
    misaligned = k % 4 < 2
    _, p = _views(init, sizes, misaligned)
    abi = AbiStepper(p, group_of, groups, None, 1.0 if clip else None)
    for s in range(4):
        grads = [(rs.standard_normal(n) * (10.0 if s % 2 == 0 else 0.01)).astype(np.float32) for n in sizes]
        if s == 2 and len(sizes) > 1:
            grads[-1] = None
        _, g_views = _views([g if g is not None else np.zeros(n, np.float32) for g, n in zip(grads, sizes)], sizes, misaligned)
        R.step(ref, grads, global_max_norm=1.0 if clip else None)
        abi.step([None if g is None else v for g, v in zip(grads, g_views)])
        assert abi.steps.cpu().tolist() == ref.step
        d = R.state_distance(*abi.state(), ref)
        print(f"small table {sizes[:6]}{'...' if len(sizes) > 6 else ''} clip {clip} step {s}: {d:.3e} (bar {bar:.3e})")
        assert d <= bar, (sizes, s, d, bar)


# ---- bits ---------------------------------------------------------------------------------------------------------------------
def _small_problem(seed=5, sizes=(4099, 1, 70000, 513), misaligned=False):
    rs = np.random.RandomState(seed)
    init = [(0.05 * rs.standard_normal(n)).astype(np.float32) for n in sizes]
    grads = [[(rs.standard_normal(n) * (3.0 if s % 2 else 0.01)).astype(np.float32) for n in sizes] for s in range(5)]
    groups = [dict(lr=1e-3, weight_decay=0.2, schedule="warmup_cosine", warmup=0.2, t_total=9, b2=0.98),
              dict(lr=1e-4, weight_decay=0.0, schedule="warmup_linear", warmup=0.1, t_total=7, max_grad_norm=0.5)]
    return init, grads, groups, [0, 1, 0, 1]


def _eager_run(init, grads, groups, group_of, gmn=1.0):
    p = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in init]
    opt = _make_optimizer(p, group_of, groups, {1: 0.06}, gmn)
    for row in grads:
        for x, g in zip(p, row):
            x.grad = torch.from_numpy(g).to(DEV)
        opt.step()
    torch.cuda.synchronize()
    return _opt_state(opt, p), opt


def test_same_inputs_same_bits():
    init, grads, groups, group_of = _small_problem()
    a, _ = _eager_run(init, grads, groups, group_of)
    b, _ = _eager_run(init, grads, groups, group_of)
    for x, y in zip(a, b):
        for u, w in zip(x, y):
            assert np.array_equal(u, w)


def test_bits_do_not_depend_on_alignment():
    """16-byte aligned tensors take the vector path, views at odd 4-byte offsets the dword path: same values, same bits."""
    init, grads, groups, group_of = _small_problem(seed=8, sizes=(4099, 1, 70000, 513, 8192))
    group_of = group_of + [0]
    results = []
    for misaligned in (False, True):
        _, p = _views(init, [len(x) for x in init], misaligned)
        abi = AbiStepper(p, group_of, groups, {1: 0.06}, 1.0)
        if misaligned:
            _, abi.m = _views([np.zeros_like(x) for x in init], [len(x) for x in init], True)
            _, abi.v = _views([np.zeros_like(x) for x in init], [len(x) for x in init], True)
        for row in grads:
            _, g = _views(row, [len(x) for x in row], misaligned)
            abi.step(g)
        results.append(abi.state())
    for x, y in zip(*results):
        for u, w in zip(x, y):
            assert np.array_equal(u, w)


def test_five_eager_steps_equal_five_replays_of_a_captured_step():
    init, grads, groups, group_of = _small_problem()
    want, eager_opt = _eager_run(init, grads, groups, group_of)
    p = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in init]
    opt = _make_optimizer(p, group_of, groups, {1: 0.06}, 1.0)
    static = [torch.zeros_like(x) for x in p]
    for x, g in zip(p, static):
        x.grad = g
    opt.prepare()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        live = opt.issue()
    torch.cuda.synchronize()
    assert all(np.array_equal(x.detach().cpu().numpy(), y) for x, y in zip(p, init))      # capturing applied nothing
    assert _device_steps(opt, p) == [0] * len(p)
    versions = [x._version for x in p]
    for row in grads:
        for dst, g in zip(static, row):
            dst.copy_(torch.from_numpy(g))
        graph.replay()
        opt.advance(live)
    torch.cuda.synchronize()
    got = _opt_state(opt, p)
    for x, y in zip(got, want):
        for u, w in zip(x, y):
            assert np.array_equal(u, w)
    assert all(x._version >= v + 5 for x, v in zip(p, versions))
    assert _device_steps(opt, p) == [5] * len(p) == [opt.state[x]["step"] for x in p]
    assert opt.get_lr() == eager_opt.get_lr()
    for dst, g in zip(static, grads[-1]):
        assert np.array_equal(dst.cpu().numpy(), g)                                       # gradient buffers unchanged


def test_state_dict_round_trip_continues_bit_for_bit():
    init, grads, groups, group_of = _small_problem(seed=6)
    want, _ = _eager_run(init, grads, groups, group_of)
    first, opt = _eager_run(init, grads[:3], groups, group_of)
    sd = opt.state_dict()
    assert all(set(s) == {"step", "next_m", "next_v"} and s["step"] == 3 for s in sd["state"].values())
    sd = {"state": {k: {"step": s["step"], "next_m": s["next_m"].cpu(), "next_v": s["next_v"].cpu()} for k, s in sd["state"].items()},
          "param_groups": sd["param_groups"]}                      # as a checkpoint read back from disk would be
    p = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in first[0]]
    fresh = _make_optimizer(p, group_of, groups, {1: 0.06}, 1.0)
    fresh.load_state_dict(sd)
    for row in grads[3:]:
        for x, g in zip(p, row):
            x.grad = torch.from_numpy(g).to(DEV)
        fresh.step()
    got = _opt_state(fresh, p)
    for x, y in zip(got, want):
        for u, w in zip(x, y):
            assert np.array_equal(u, w)
    assert _device_steps(fresh, p) == [5] * len(p)


def test_load_state_dict_keeps_the_moments_where_a_captured_step_expects_them():
    """Loading a state replaces values, not storage: a table that a captured step holds keeps pointing at the live moments."""
    import copy
    init, grads, groups, group_of = _small_problem(seed=9)
    p = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in init]
    opt = _make_optimizer(p, group_of, groups, {1: 0.06}, 1.0)

    def steps(rows):
        for row in rows:
            for x, g in zip(p, row):
                x.grad = torch.from_numpy(g).to(DEV)
            opt.step()
    steps(grads[:3])
    sd = copy.deepcopy(opt.state_dict())
    steps(grads[3:])
    where = [(opt.state[x]["next_m"].data_ptr(), opt.state[x]["next_v"].data_ptr()) for x in p]
    opt.load_state_dict(sd)
    assert where == [(opt.state[x]["next_m"].data_ptr(), opt.state[x]["next_v"].data_ptr()) for x in p]
    for i, x in enumerate(x for g in opt.param_groups for x in g["params"]):      # a state dict numbers tensors group by group
        assert torch.equal(opt.state[x]["next_m"], sd["state"][i]["next_m"]) and opt.state[x]["step"] == 3
    assert _device_steps(opt, p) == [3] * len(p)


def test_launcher_rejects_bad_arguments_before_any_launch():
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    ok = ctypes.c_void_p(ws.data_ptr())
    f = hip.lib().nr_bertadam_step
    assert f(None, 1, 1, ok, 1, 1.0, ok, None) == hip.NR_EINVAL
    assert f(ok, 1, 1, None, 1, 1.0, ok, None) == hip.NR_EINVAL
    assert f(ok, 1, 1, ok, 1, 1.0, None, None) == hip.NR_EINVAL
    assert f(ok, 1, -1, ok, 1, 1.0, ok, None) == hip.NR_EINVAL
    assert f(ok, 1, 1, ok, 0, 1.0, ok, None) == hip.NR_EINVAL
    assert f(ok, 1, 1, ok, 1, float("nan"), ok, None) == hip.NR_EINVAL
    torch.cuda.synchronize()
    assert not ws.any()


# ---- the model ----------------------------------------------------------------------------------------------------------------
class _Args:
    lr, coef_lr, weight_decay, warmup_proportion = 1e-4, 1e-3, 0.2, 0.1


def _model(K=4):
    from neighborretr_amd import modeling
    from util import params
    m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K))
    m.load_state_dict(params(), strict=False)
    m = m.to(DEV).train()
    with torch.no_grad():
        m.clip.logit_scale.fill_(float(np.log(100.0)))
    return m


def test_step_moves_the_version_counters_and_the_derived_weights():
    m = _model()
    opt, _, _ = optim.prep_optimizer(_Args, m, 10, 0, global_max_norm=1.0, clamp_logit_scale=True)
    before = m.scorer_weights("text_weight_fc")
    assert m.scorer_weights("text_weight_fc") is before              # cached per parameter version
    w_before = m.text_weight_fc[0].weight.detach().clone()
    g = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(2):                                               # the first step under warm-up has learning rate 0
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g, device=DEV)
        versions = {n: p._version for n, p in m.named_parameters()}
        opt.step()
        assert all(p._version > versions[n] for n, p in m.named_parameters())
    after = m.scorer_weights("text_weight_fc")
    assert after is not before
    # the splits follow the updated fp32 weights
    assert not (torch.equal(after.w1_hi, before.w1_hi) and torch.equal(after.w1_lo, before.w1_lo))
    assert not torch.equal(m.text_weight_fc[0].weight.detach(), w_before)
    from neighborretr_amd import head
    mlp = m.text_weight_fc
    fresh = head.ScorerWeights(mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)
    assert torch.equal(after.w1_hi, fresh.w1_hi) and torch.equal(after.w1_lo, fresh.w1_lo)
    assert float(m.clip.logit_scale.detach()) <= np.float32(LN100)


def test_graphed_step_with_the_update_inside():
    sys.path.insert(0, ROOT)
    from main_retrieval import GraphedStep
    from util import problem
    B, Nt, Nv, M = 32, 24, 12, 64
    x = problem(1003, B, Nt, Nv, M, device=DEV)

    def batch(r):
        return (x["text_feat"] + 0.01 * r, x["text_mask"], x["video_feat"] + 0.01 * r, x["video_mask"], x["idx"] + 100 * r)

    def load_bank(m, shift):
        m.mb_feat_t, m.mb_feat_v = x["mb_feat_t"].clone() + shift, x["mb_feat_v"].clone() + shift
        m.mb_mask_t, m.mb_mask_v = x["mb_mask_t"].clone(), x["mb_mask_v"].clone()
        m.mb_ind = torch.arange(5000 + shift, 5000 + shift + M, device=DEV)

    m = _model(K=8)
    named = list(m.named_parameters())
    params = [p for _, p in named]
    opt, _, _ = optim.prep_optimizer(_Args, m, 6, 0, global_max_norm=1.0, clamp_logit_scale=True)
    load_bank(m, 0)
    init = [p.detach().cpu().numpy().copy() for p in params]
    index = {id(p): t for t, p in enumerate(params)}
    group_of = [None] * len(params)
    for gi, g in enumerate(opt.param_groups):
        for p in g["params"]:
            group_of[index[id(p)]] = gi
    groups = [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]
    clamp = {index[id(m.clip.logit_scale)]: LN100}
    ref = R.State(init, group_of, groups, clamp_max=clamp)
    eager = TorchEager([p.detach().reshape(-1) for p in params], group_of, groups, clamp, 1.0)
    step = GraphedStep(m, batch(0), params, optimizer=opt)
    torch.cuda.synchronize()
    assert all(np.array_equal(p.detach().cpu().numpy(), q) for p, q in zip(params, init))  # warm-up and capture: no update
    for r in range(6):
        if r == 3:
            load_bank(m, 1)                                          # a new bank generation: run() re-captures
            gen = step.generation
        losses = step.run(batch(r))
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(l)) for l in losses)
        if r == 3:
            assert step.generation != gen
        grads = [None if g is None else g.detach() for g in step.grads]
        assert all((p.grad is None) == (g is None) for p, g in zip(params, grads))
        R.step(ref, [None if g is None else g.cpu().numpy() for g in grads], global_max_norm=1.0)
        eager.step([None if g is None else g.reshape(-1) for g in grads])
        got = _opt_state(opt, params)
        d_hip = R.state_distance(*[[a.reshape(-1) for a in part] for part in got], _Flat(ref))
        d_torch = R.state_distance(*eager.state(), _Flat(ref))
        print(f"graphed step {r}: hip {d_hip:.3e}  fp32 torch {d_torch:.3e}")
        assert d_hip <= 4.0 * d_torch, (r, d_hip, d_torch)
        assert float(m.clip.logit_scale.detach()) <= np.float32(LN100)
        live = [t for t, g in enumerate(grads) if g is not None]
        assert [opt.state[params[t]]["step"] for t in live] == [r + 1] * len(live)        # one update per run(), re-capture included
        assert [_device_steps(opt, params)[t] for t in live] == [r + 1] * len(live)
    # a batch of another shape: an eager step that ends in the same update
    short = tuple(t[:B - 1] for t in batch(7))
    step.run(short)
    torch.cuda.synchronize()
    assert opt.state[params[live[0]]]["step"] == 7 and _device_steps(opt, params)[live[0]] == 7


class _Flat:
    def __init__(self, ref):
        self.p, self.m, self.v = ([a.reshape(-1) for a in part] for part in (ref.p, ref.m, ref.v))


# ---- the entry point ------------------------------------------------------------------------------------------------------------
def _entry(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--do_train", "1", "--synthetic", "--batch_size", "32",
           "--num_neighbors", "8", "--mb_batch", "2", "--epochs", "1", "--synthetic_train", "512", "--synthetic_test", "200",
           "--n_display", "1", "--output_dir", str(tmp_path)] + list(extra)
    r = subprocess.run(["timeout", "-k", "10", "540"] + cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if " loss " in l]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in lines]
    assert len(losses) == 16 and all(v == v and v < 1e4 for v in losses), losses
    assert "text->video R@1" in r.stdout
    return lines, r.stdout


def test_main_retrieval_with_bertadam(tmp_path):
    """16 steps, warm-up 0.1: the head's learning rate starts at 0, rises for two steps, then follows the cosine down.  Eager
    first, then with the step (update included) replayed from a graph: each a fresh child, one after the other."""
    for hip_graph in ("0", "1"):
        lines, out = _entry(tmp_path, "--optimizer", "bertadam", "--hip_graph", hip_graph)
        lrs = [float(l.split(" lr ")[1].split()[0]) for l in lines]
        print(f"--hip_graph {hip_graph}: lr {lrs}")
        peak = int(np.argmax(lrs))
        assert lrs[0] == 0.0 and 0 < peak < len(lrs) - 1
        assert all(a < b for a, b in zip(lrs[:peak], lrs[1:peak + 1]))
        assert all(a > b for a, b in zip(lrs[peak:], lrs[peak + 1:]))
        want = [1e-4 * R.warmup_cosine(s / 16, 0.1) for s in range(16)]
        np.testing.assert_allclose(lrs, want, rtol=2e-3)             # (the log prints four digits)
        if hip_graph == "1":
            assert "training step replayed as: whole" in out


def test_main_retrieval_two_ranks_with_bertadam_in_the_graphed_step(tmp_path):
    """Two gloo ranks on one card, --hip_graph 1: the update follows the step's replay (after the gradient average) on the flat
    buffer's views, eight steps; the logged learning rate is the schedule's and the losses stay finite."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29647", os.path.join(ROOT, "main_retrieval.py"), "--do_train", "1", "--synthetic",
           "--batch_size", "32", "--num_neighbors", "8", "--mb_batch", "2", "--epochs", "1", "--synthetic_train", "256",
           "--synthetic_test", "100", "--n_display", "1", "--output_dir", str(tmp_path), "--dist_backend", "gloo",
           "--hip_graph", "1", "--optimizer", "bertadam"]
    r = subprocess.run(["timeout", "-k", "10", "840"] + cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "training step replayed as: segmented" in r.stdout, r.stdout[-2000:]
    lines = [l for l in r.stdout.splitlines() if " loss " in l]
    losses = [float(l.split(" loss ")[1].split()[0]) for l in lines]
    assert len(losses) == 8 and all(v == v and v < 1e4 for v in losses), r.stdout[-2000:]
    lrs = [float(l.split(" lr ")[1].split()[0]) for l in lines]
    np.testing.assert_allclose(lrs, [1e-4 * R.warmup_cosine(s / 8, 0.1) for s in range(8)], rtol=2e-3)
    assert "text->video R@1" in r.stdout


def test_main_retrieval_default_optimizer_log_is_unchanged_in_form(tmp_path):
    lines, _ = _entry(tmp_path)
    import re
    form = re.compile(r"^\d\d:\d\d:\d\d epoch 1 step \d+/16 loss \S+ centrality \S+ uniform \S+ neighbor \S+ kl \S+ \(\S+ ms/step\)$")
    assert all(form.match(l) for l in lines), lines[:2]
