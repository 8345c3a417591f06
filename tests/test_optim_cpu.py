"""BertAdam without a GPU: the fp64 restatement (tests/bertadam_ref.py) against the values captured from the unmodified reference
optimizer (tests/golden/bertadam_small.npz), the schedules, prep_optimizer's grouping, the constructor's checks and the state
layout.  The kernels themselves are tested in test_optim_gpu.py."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import bertadam_ref as R
from neighborretr_amd import hip, modeling, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bertadam_small.npz")


def _capture_module():
    """The fixture's description (shapes, groups, gradient stream) lives in the capture tool: one statement of it."""
    spec = importlib.util.spec_from_file_location("capture_bertadam_golden", os.path.join(ROOT, "tools", "capture_bertadam_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden_distance(C, z, run, rec):
    d = 0.0
    for k in (int(x) for x in z["record"]):
        for key in ("p", "m", "v"):
            for t in range(len(C.SHAPES)):
                d = max(d, R.distance(rec[k][key][t], z[f"{run}_{key}_{k}_{t}"]))
    return d


def test_restatement_matches_the_reference_fixture_and_the_bar_rejects_wrong_formulas():
    C = _capture_module()
    z = np.load(GOLDEN)
    seed = int(z["seed"])
    init, grads = C.initial_params(seed), C.gradients(seed)
    for t, x in enumerate(init):
        assert np.array_equal(x, z[f"init_{t}"])
    assert np.array_equal(C.scales(), z["scales"])
    for run, clip in (("A", True), ("B", False)):
        bar = 4.0 * float(z[f"d_ref_{run}"])
        assert 0.0 < bar < 1e-4, bar
        d = _golden_distance(C, z, run, C.run_restatement(init, grads, clip))
        print(f"run {run}: restatement vs reference {d:.3e}, bar {bar:.3e}")
        assert d <= bar, (run, d, bar)
    # each wrong formula misses the bar by a factor of 1000 or more on the run named
    for mutation, run, clip in (("no_tensor_clip", "B", False), ("no_global_clip", "A", True), ("bias_correction", "A", True),
                                ("bias_correction", "B", False), ("schedule_after_increment", "A", True),
                                ("schedule_after_increment", "B", False)):
        bar = 4.0 * float(z[f"d_ref_{run}"])
        d = _golden_distance(C, z, run, C.run_restatement(init, grads, clip, mutate=(mutation,)))
        print(f"{mutation} on run {run}: {d:.3e} = {d / bar:.0f} x bar")
        assert d >= 1000.0 * bar, (mutation, run, d, bar)
    # run A does not see the per-tensor clip at all (after the global clip no tensor's norm exceeds 1): why run B exists
    a = C.run_restatement(init, grads, True)
    b = C.run_restatement(init, grads, True, mutate=("no_tensor_clip",))
    assert all(np.array_equal(x, y) for k in a for key in ("p", "m", "v") for x, y in zip(a[k][key], b[k][key]))


def test_learning_rates_of_the_fixture():
    """get_lr() of the reference after steps 1, 2, 8, 12 (one entry per tensor that had a gradient in that step)."""
    C = _capture_module()
    z = np.load(GOLDEN)
    for k in (int(x) for x in z["record"]):
        steps = [k - 1 if (t == C.NO_GRAD[1] and k > C.NO_GRAD[0]) else k for t in range(len(C.SHAPES))]
        order = [t for q in range(len(C.GROUPS)) for t in range(len(C.SHAPES)) if C.GROUP_OF[t] == q]
        if k - 1 == C.NO_GRAD[0]:
            order = [t for t in order if t != C.NO_GRAD[1]]
        want = [R.scheduled_lr(dict(C.GROUPS[C.GROUP_OF[t]], **C.COMMON), steps[t]) for t in order]
        for run in ("A", "B"):
            np.testing.assert_allclose(z[f"{run}_lr_{k}"], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["warmup_cosine", "warmup_constant", "warmup_linear"])
def test_schedules(name):
    w = 0.1
    after = {"warmup_cosine": lambda x: 0.5 * (1 + math.cos(math.pi * x)), "warmup_constant": lambda x: 1.0,
             "warmup_linear": lambda x: max((x - 1.0) / (w - 1.0), 0.0)}[name]
    below, above = math.nextafter(w, 0.0), math.nextafter(w, 1.0)
    for fn in (optim.SCHEDULES[name], R.SCHEDULES[name]):
        assert fn(0.0, w) == 0.0
        assert fn(below, w) == below / w
        assert fn(w, w) == after(w)                        # at x == warmup the warm-up branch has ended
        assert fn(above, w) == after(above)
        assert fn(1.0, w) == after(1.0)
    assert optim.SCHEDULES["warmup_cosine"](1.0, w) == 0.0
    assert optim.SCHEDULES["warmup_linear"](1.0, w) == 0.0 and optim.SCHEDULES["warmup_linear"](1.5, w) == 0.0
    assert set(hip.SCHEDULE_IDS) == set(optim.SCHEDULES)


class _Args:
    lr, coef_lr, weight_decay, warmup_proportion = 1e-4, 1e-3, 0.2, 0.1


def test_prep_optimizer_groups_like_the_reference():
    model = modeling.NeighborRetr(modeling.default_config())
    opt, scheduler, out = optim.prep_optimizer(_Args, model, 120, 0)
    assert scheduler is None and out is model and isinstance(opt, optim.BertAdam)
    assert [len(g["params"]) for g in opt.param_groups] == [1, 44, 0, 40]
    assert sum(len(g["params"]) for g in opt.param_groups) == len(list(model.parameters())) == 85
    names = {id(p): n for n, p in model.named_parameters()}
    assert [names[id(p)] for p in opt.param_groups[0]["params"]] == ["clip.logit_scale"]
    for gi, (lr, wd) in enumerate(((1e-4 * 1e-3, 0.2), (1e-4, 0.2), (1e-4 * 1e-3, 0.0), (1e-4, 0.0))):
        g = opt.param_groups[gi]
        assert g["lr"] == lr and g["weight_decay"] == wd
        assert (g["schedule"], g["warmup"], g["t_total"], g["b1"], g["b2"], g["e"], g["max_grad_norm"]) == \
            ("warmup_cosine", 0.1, 120, 0.9, 0.98, 1e-6, 1.0)
    for n, p in model.named_parameters():
        decayed = not any(s in n for s in ("bias", "LayerNorm.bias", "LayerNorm.weight"))
        gi = (0 if "clip." in n else 1) + (0 if decayed else 2)
        assert any(p is q for q in opt.param_groups[gi]["params"]), n
    assert opt.global_max_norm is None and opt.clamp_max == {}           # the trainer clips and clamps around step()
    fused, _, _ = optim.prep_optimizer(_Args, model, 120, 0, global_max_norm=1.0, clamp_logit_scale=True)
    assert fused.global_max_norm == 1.0
    assert fused.clamp_max == {id(model.clip.logit_scale): math.log(100.0)}


def test_shims_re_export():
    from NeighborRetr.models.optimization import BertAdam, warmup_cosine
    from NeighborRetr.training.optimizer import prep_optimizer
    assert BertAdam is optim.BertAdam and prep_optimizer is optim.prep_optimizer and warmup_cosine is optim.warmup_cosine


def test_constructor_checks():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (dict(lr=-1.0), dict(lr=1e-3, schedule="cosine"), dict(lr=1e-3, warmup=1.0), dict(lr=1e-3, warmup=-0.5),
                dict(lr=1e-3, b1=1.0), dict(lr=1e-3, b2=-0.1), dict(lr=1e-3, e=-1e-6), dict(lr=1e-3, e=float("nan")),
                dict(lr=1e-3, global_max_norm=float("nan")), dict()):
        with pytest.raises(ValueError):
            optim.BertAdam(p, **bad)
    with pytest.raises(ValueError):
        optim.BertAdam(p, lr=1e-3, clamp_max={torch.nn.Parameter(torch.zeros(1)): 1.0})
    opt = optim.BertAdam(p, lr=1e-3)
    assert opt.defaults == dict(lr=1e-3, schedule="warmup_linear", warmup=-1, t_total=-1, b1=0.9, b2=0.999, e=1e-6,
                                weight_decay=0.01, max_grad_norm=1.0)
    assert opt.get_lr() == []
    p[0].grad = torch.zeros(3)
    assert opt.get_lr() == [0]


def test_cpu_parameters_raise_the_device_error():
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.BertAdam([p], lr=1e-3)
    p.grad = torch.ones(3)
    with pytest.raises(hip.NrHipError, match="cpu"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(3))


def test_state_dict_layout_is_the_references():
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))
    opt = optim.BertAdam([{"params": [a], "lr": 1e-7}, {"params": [b], "weight_decay": 0.0}], lr=1e-4, warmup=0.1, t_total=10,
                         schedule="warmup_cosine", b2=0.98)
    sd = {"state": {0: {"step": 3, "next_m": torch.full((3,), 0.5), "next_v": torch.full((3,), 0.25)},
                    1: {"step": 2, "next_m": torch.ones(2, 2), "next_v": torch.ones(2, 2)}},
          "param_groups": [dict(opt.defaults, lr=1e-7, params=[0]), dict(opt.defaults, weight_decay=0.0, params=[1])]}
    opt.load_state_dict(sd)                                  # a state dict in the reference's layout loads as it is
    assert set(opt.state[a]) == {"step", "next_m", "next_v"} and opt.state[a]["step"] == 3 and opt.state[b]["step"] == 2
    out = opt.state_dict()
    assert set(out) == {"state", "param_groups"} and set(out["state"][0]) == {"step", "next_m", "next_v"}
    assert torch.equal(out["state"][0]["next_v"], torch.full((3,), 0.25))
    assert set(out["param_groups"][0]) == {"lr", "schedule", "warmup", "t_total", "b1", "b2", "e", "weight_decay",
                                           "max_grad_norm", "params"}
    a.grad, b.grad = torch.zeros(3), torch.zeros(2, 2)
    assert opt.get_lr() == [1e-7 * R.warmup_cosine(0.3, 0.1), 1e-4 * R.warmup_cosine(0.2, 0.1)]
    assert opt.group_lr() == opt.get_lr()


def test_table_plan_rejects_bad_entries_before_any_launch():
    """nr_bertadam_plan is host-only: null pointers, negative counts, group indices out of range, bad schedule ids."""
    lib = hip.lib()
    n = hip._I(0)

    def plan(entries, groups):
        return lib.nr_bertadam_plan(entries, len(entries), groups, len(groups), n)

    def entry(**kw):
        e = hip.OptimTensor()
        e.p, e.g, e.m, e.v, e.step, e.n, e.group = 4096, 8192, 12288, 16384, 64, 5000, 0
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    def group(**kw):
        g = hip.OptimGroup()
        g.lr, g.b1, g.b2, g.e, g.max_grad_norm, g.warmup, g.t_total, g.schedule = 1e-4, 0.9, 0.98, 1e-6, 1.0, 0.1, 10, 0
        for k, v in kw.items():
            setattr(g, k, v)
        return g
    ok = (hip.OptimTensor * 3)(entry(), entry(n=0), entry(n=4096))
    assert plan(ok, (hip.OptimGroup * 1)(group())) == 0
    assert n.value == 3 and [e.chunk0 for e in ok] == [0, 2, 2]
    for bad in (entry(p=None), entry(g=None), entry(m=None), entry(v=None), entry(step=None), entry(n=-1), entry(group=1),
                entry(group=-1), entry(g=8194)):
        assert plan((hip.OptimTensor * 1)(bad), (hip.OptimGroup * 1)(group())) == hip.NR_EINVAL
    for bad in (group(schedule=3), group(schedule=-1), group(t_total=0), group(t_total=-2)):
        assert plan((hip.OptimTensor * 1)(entry()), (hip.OptimGroup * 1)(bad)) == hip.NR_EINVAL
    assert lib.nr_bertadam_plan(ok, -1, (hip.OptimGroup * 1)(group()), 1, n) == hip.NR_EINVAL
    assert lib.nr_bertadam_plan(ok, 3, None, 1, n) == hip.NR_EINVAL
    assert lib.nr_bertadam_workspace_bytes(0, 0) == 0
    assert lib.nr_bertadam_workspace_bytes(3, 3) == 256 * 4
    # the launcher's own checks come before any launch, so they can be exercised without a device
    assert lib.nr_bertadam_step(None, 3, 3, None, 1, 1.0, None, None) == hip.NR_EINVAL
    assert lib.nr_bertadam_step(None, -1, 0, None, 1, 1.0, None, None) == hip.NR_EINVAL
    assert lib.nr_bertadam_step(None, 0, 0, None, 0, 1.0, None, None) == 0
