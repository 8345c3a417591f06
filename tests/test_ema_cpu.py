"""No GPU: the weight EMA's decay warm-up, the restatement (tests/ema_ref.py) and its mutants against an fp32 emulation of the
kernels' roundings, the two structs' sizes, the host-side argument checks of nr_ema_plan and of the four entry points (they
return before any launch), constructor and flag validation, and the keys of model_state_dict."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import bertadam_ref as R
import ema_ref as E
from neighborretr_amd import hip, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_decay_warm_up_values():
    for f in (E.decay_at, optim.ema_decay_at):
        assert f(0.999, True, 0) == 0.1                                     # (1 + 0) / (10 + 0)
        assert f(0.999, True, 90) == 0.91                                   # 91 / 100
        assert f(0.999, True, 8989) == 8990.0 / 8999.0 < 0.999              # the last update under the ramp ...
        assert f(0.999, True, 8992) == 0.999 and f(0.999, True, 10 ** 9) == 0.999          # ... then capped (8991 / 9000 = 0.999)
        assert f(0.5, True, 8) == 0.5 and f(0.5, True, 7) == 8.0 / 17.0
        assert f(0.999, False, 0) == 0.999 and f(0.0, True, 5) == 0.0


def test_restatement_by_hand():
    st = E.State([np.array([1.0, -2.0])], decay=0.5, warmup=True)
    E.update(st, [np.array([2.0, -2.0])])                                    # d = 0.1: e += 0.9 (p - e)
    assert np.allclose(st.e[0], [1.9, -2.0], rtol=0, atol=1e-15) and st.updates == 1 and st.last_decay == 0.1
    E.update(st, [np.array([2.0, 0.0])])                                     # d = 2 / 11
    assert np.allclose(st.e[0], [1.9 + (9 / 11) * 0.1, -2.0 + (9 / 11) * 2.0], rtol=0, atol=1e-15) and st.updates == 2
    E.update(st, [None])                                                     # not averaged in this step: the count still moves
    assert st.updates == 3


@pytest.mark.parametrize("decay,warmup", [(0.999, True), (0.999, False), (0.5, True), (0.5, False)])
def test_fp32_emulation_meets_the_bar_and_the_mutants_miss_it(decay, warmup):
    """The GPU test's bar, K 2^-21 of the largest magnitude A after K updates: per update the rule rounds three times (the
    difference, 1 - d, the fused multiply-add), each rounding at most 2^-24 of a quantity bounded by 4 A, and earlier errors
    shrink by d.  The fp32 emulation of the rule stays far inside it; every mutant that changes the rule at these settings
    is far outside."""
    K, sizes = 40, (4099, 1, 513)
    rows = E.random_walk(11, sizes, K)
    ref, emu = E.State(rows[0], decay, warmup), E.State(rows[0], decay, warmup)
    mutants = {m: E.State(rows[0], decay, warmup) for m in E.MUTANTS}
    err, d, err_m, abs_m = 0.0, 0.0, dict.fromkeys(E.MUTANTS, 0.0), dict.fromkeys(E.MUTANTS, 0.0)
    for k in range(1, K + 1):                        # compared after every update: a wrong warm-up shows in the first ones only
        E.update(ref, rows[k])
        E.update_fp32(emu, rows[k])
        err = max(err, E.scaled_error(emu.e, ref.e, rows)[0])
        d = max([d] + [R.distance(a, b) for a, b in zip(emu.e, ref.e)])
        for m, st in mutants.items():
            E.update(st, rows[k], before=rows[k - 1], mutate=(m,))
            err_m[m] = max(err_m[m], E.scaled_error(emu.e, st.e, rows)[0])
            abs_m[m] = max([abs_m[m]] + [float(np.max(np.abs(a - b))) for a, b in zip(emu.e, st.e)])
    bar = K * 2.0 ** -21
    print(f"decay {decay} warmup {warmup}: fp32 emulation {err:.3e} (bar {bar:.3e}), distance {d:.3e}")
    assert err <= bar and d < 1e-5
    for m in E.MUTANTS:
        same_rule = (m == "no_warmup" and not warmup) or (m == "swapped" and decay == 0.5 and not warmup)
        print(f"    mutant {m}: {err_m[m]:.3e} ({abs_m[m]:.3e} absolute)")
        assert same_rule or err_m[m] > 4 * bar, (m, err_m[m], bar)
        if decay == 0.999 and warmup:                # the setting the GPU test shows the mutants at
            assert abs_m[m] > 1e-3, (m, abs_m[m])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_are_the_headers():
    header = open(os.path.join(ROOT, "include", "nr_hip.h")).read()
    lib = hip.lib()
    for name, cls, size in (("NrEmaState", hip.EmaState, 24), ("NrEmaTensor", hip.EmaTensor, 32)):
        stated = re.search(r"\}\s*" + name + r";\s*/\*\s*(\d+) bytes", header)
        assert stated and int(stated.group(1)) == size == ctypes.sizeof(cls) == int(lib.nr_struct_size(name.encode()))
        assert size % 8 == 0 and hip.STRUCTS[name] is cls
    assert [f[0] for f in hip.EmaState._fields_] == ["decay", "updates", "warmup", "omd"]
    assert [f[0] for f in hip.EmaTensor._fields_] == ["p", "ema", "n", "chunk0", "pad_"]
    for name in ("nr_bertadam_step_ema", "nr_ema_plan", "nr_ema_update", "nr_ema_swap"):
        assert f"int {name}(" in header and name in hip.exported_symbols() and hasattr(lib, name), name
    assert lib.nr_version() == 5


def _entries(sizes, base=0x10000):
    entries = (hip.EmaTensor * len(sizes))()
    for ent, n in zip(entries, sizes):
        ent.p, ent.ema, ent.n = base, base + 0x100000, n
        base += 0x200000
    return entries


def test_ema_plan_chunks_and_checks():
    lib = hip.lib()
    n = ctypes.c_int(-1)
    state = hip.EmaState(decay=0.999, updates=0, warmup=1)
    entries = _entries([4099, 1, 0, 70000, 4096])
    assert lib.nr_ema_plan(entries, 5, ctypes.byref(state), ctypes.byref(n)) == 0
    assert [e.chunk0 for e in entries] == [0, 2, 3, 3, 21] and n.value == 22
    assert lib.nr_ema_plan(None, 0, ctypes.byref(state), ctypes.byref(n)) == 0 and n.value == 0
    bad = hip.NR_EINVAL
    assert lib.nr_ema_plan(entries, 5, ctypes.byref(state), None) == bad
    assert lib.nr_ema_plan(entries, 5, None, ctypes.byref(n)) == bad
    assert lib.nr_ema_plan(None, 5, ctypes.byref(state), ctypes.byref(n)) == bad
    assert lib.nr_ema_plan(entries, -1, ctypes.byref(state), ctypes.byref(n)) == bad
    for decay in (1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert lib.nr_ema_plan(entries, 5, ctypes.byref(hip.EmaState(decay=decay)), ctypes.byref(n)) == bad, decay
    assert lib.nr_ema_plan(entries, 5, ctypes.byref(hip.EmaState(decay=0.0)), ctypes.byref(n)) == 0
    assert lib.nr_ema_plan(entries, 5, ctypes.byref(hip.EmaState(decay=0.5, updates=-1)), ctypes.byref(n)) == bad
    for field, value in (("p", 0), ("ema", 0), ("p", 0x10002), ("ema", 0x10001), ("n", -1)):
        entries = _entries([4099, 5])
        setattr(entries[1], field, value)
        assert lib.nr_ema_plan(entries, 2, ctypes.byref(state), ctypes.byref(n)) == bad, (field, value)
    entries = _entries([4099, 0])
    entries[1].p = entries[1].ema = 0                                        # a tensor without elements needs no storage
    assert lib.nr_ema_plan(entries, 2, ctypes.byref(state), ctypes.byref(n)) == 0 and n.value == 2
    with pytest.raises(hip.NrHipError):
        from neighborretr_amd import ops
        ops.ema_plan(_entries([5]), hip.EmaState(decay=1.0))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call here returns NR_EINVAL (or NR_OK for T = 0) from the host-side checks: no launch is made, so no GPU is needed
    and the made-up addresses are never touched."""
    lib = hip.lib()
    ok, odd, bad = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004), hip.NR_EINVAL
    up, swap, fused = lib.nr_ema_update, lib.nr_ema_swap, lib.nr_bertadam_step_ema
    assert up(None, 0, 0, ok, None) == 0 and swap(None, 0, 0, None) == 0                 # T = 0: nothing to do
    assert up(None, 0, 1, ok, None) == bad and swap(None, 0, 1, None) == bad
    assert up(ok, 1, 1, None, None) == bad and up(ok, 1, 1, odd, None) == bad            # state: null, misaligned
    assert up(None, 1, 1, ok, None) == bad and up(odd, 1, 1, ok, None) == bad            # table
    assert up(ok, -1, 1, ok, None) == bad and up(ok, 1, -1, ok, None) == bad
    assert up(None, 0, 0, None, None) == bad
    assert swap(None, 1, 1, None) == bad and swap(odd, 1, 1, None) == bad
    assert swap(ok, -1, 1, None) == bad and swap(ok, 1, -1, None) == bad

    def f(table=ok, T=1, n_chunks=1, groups=ok, G=1, gmn=1.0, ws=ok, guard=None, losses=None, n_losses=0, ring=None, n_ring=0,
          ema=ok, state=ok):
        return fused(table, T, n_chunks, groups, G, gmn, ws, guard, losses, n_losses, ring, n_ring, ema, state, None)
    assert f(T=0, n_chunks=0) == 0 and f(T=0, n_chunks=0, guard=ok, ring=ok, n_ring=4) == 0
    assert f(T=0, n_chunks=1) == bad
    for kw in (dict(table=None), dict(groups=None), dict(ws=None), dict(ws=odd), dict(G=0), dict(T=-1), dict(n_chunks=-1), dict(G=-1),
               dict(gmn=float("nan")), dict(ema=None), dict(ema=odd), dict(state=None), dict(state=odd)):
        assert f(**kw) == bad, kw
        assert f(guard=ok, ring=ok, n_ring=4, **kw) == bad, kw
    for kw in (dict(guard=odd, ring=ok, n_ring=4), dict(guard=ok, ring=None, n_ring=4), dict(guard=ok, ring=odd, n_ring=4),
               dict(guard=ok, ring=ok, n_ring=3), dict(guard=ok, ring=ok, n_ring=0), dict(guard=ok, ring=ok, n_ring=8192),
               dict(guard=ok, ring=ok, n_ring=4, n_losses=9, losses=ok), dict(guard=ok, ring=ok, n_ring=4, n_losses=-1),
               dict(guard=ok, ring=ok, n_ring=4, n_losses=2, losses=None),
               dict(guard=ok, ring=ok, n_ring=4, n_losses=2, losses=ctypes.c_void_p(0x10002))):
        assert f(T=0, n_chunks=0, **kw) == bad, kw


# ---- the host side ----------------------------------------------------------------------------------------------------------------
def test_constructor_validation():
    p = torch.nn.Parameter(torch.zeros(4))
    for kw in (dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(decay="0.9"), dict(warmup=2), dict(warmup=None)):
        with pytest.raises(ValueError, match="WeightEma"):
            optim.WeightEma([p], **kw)
    with pytest.raises(ValueError, match="no parameters"):
        optim.WeightEma([])
    with pytest.raises(ValueError, match="twice"):
        optim.WeightEma([p, p])
    with pytest.raises(hip.NrHipError, match="not on a GPU"):              # no CPU fallback: a parameter off the GPU is an error
        optim.WeightEma([p])
    with pytest.raises(hip.NrHipError, match="not on a GPU"):
        optim.WeightEma([("w", p)], decay=0.9, warmup=False)
    with pytest.raises(TypeError, match="WeightEma"):
        optim.BertAdam([p], lr=1e-3, ema="average")
    opt = optim.BertAdam([p], lr=1e-3)                                       # without ema: nothing new
    assert opt.ema is None and "ema" not in opt.state_dict() and all("ema" not in g for g in opt.state_dict()["param_groups"])


def _main():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import main_retrieval
    return main_retrieval


def _parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py"] + argv)
    return _main().get_args()


def test_main_retrieval_accepts_the_ema_flags(monkeypatch, capsys):
    a = _parse([], monkeypatch)
    assert (a.ema_decay, a.ema_warmup) == (0.0, 1)
    a = _parse(["--do_train", "1", "--ema_decay", "0.99", "--ema_warmup", "0"], monkeypatch)
    assert (a.ema_decay, a.ema_warmup) == (0.99, 0)
    a = _parse(["--do_train", "1", "--ema_decay", "0.9", "--permutation", "64"], monkeypatch)      # EMA against the raw model
    assert a.permutation == 64
    for argv, word in ((["--do_train", "1", "--ema_decay", "1.0"], "--ema_decay must"),
                       (["--do_train", "1", "--ema_decay", "-0.5"], "--ema_decay must"),
                       (["--do_train", "1", "--ema_decay", "nan"], "--ema_decay must"),
                       (["--do_eval", "1", "--ema_decay", "0.9"], "--ema_decay belongs to training"),
                       (["--do_train", "1", "--ema_decay", "0.9", "--ema_warmup", "2"], "--ema_warmup"),
                       (["--do_train", "1", "--permutation", "64"], "--permutation needs")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            _parse(argv, monkeypatch)
        assert word in capsys.readouterr().err


def test_evaluation_flags_accept_a_permutation_test_of_the_ema():
    """--ema_decay gives --permutation something to compare: the evaluation then carries its units without a correction."""
    from types import SimpleNamespace
    from neighborretr_amd import evaluator
    correction, kw = evaluator.correction_from_args(SimpleNamespace(permutation=64, permutation_seed=3, ema_decay=0.9), None)
    assert correction is None and (kw["permutation"], kw["permutation_seed"]) == (64, 3)
    with pytest.raises(ValueError, match="permutation needs a correction"):
        evaluator.correction_from_args(SimpleNamespace(permutation=64, ema_decay=0.0), None)


def test_model_state_dict_has_the_models_keys():
    """model_state_dict needs only the map from parameters to shadows, so it is exercised here on the CPU with that map filled
    by hand (a WeightEma proper cannot be built without a GPU); tests/test_ema_gpu.py loads the real thing through --init_model."""
    from neighborretr_amd import modeling
    m = modeling.NeighborRetr(modeling.default_config())
    ema = optim.WeightEma.__new__(optim.WeightEma)
    named = dict(m.named_parameters())
    left_out = "clip.logit_scale"
    ema._shadow_of = {id(p): torch.full_like(p, 7.0) for n, p in named.items() if n != left_out}
    sd, own = ema.model_state_dict(m), m.state_dict()
    assert list(sd) == list(own)
    for k, v in sd.items():
        if k in named and k != left_out:
            assert bool((v == 7.0).all()) and v.shape == own[k].shape and v.data_ptr() != ema._shadow_of[id(named[k])].data_ptr()
        else:                                                                # buffers and parameters the average does not know
            assert torch.equal(v, own[k])
    missing, unexpected = modeling.NeighborRetr(modeling.default_config()).load_state_dict(sd, strict=False)
    assert not missing and not unexpected
