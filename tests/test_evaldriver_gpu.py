"""GPU: evaluator.sharded_evaluation called with a correction record against the legacy-named entry points that wrap it, for every
mode of every correction, with and without a querybank, on one rank and on three emulated ranks: the same trees, bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from neighborretr_amd import evaluator, synth
from test_irmetrics_gpu import DEV, Nt, Nv, _emulated, _model, _same_tree, _without

pytestmark = pytest.mark.gpu

# (constructor, the entry point with the raw dictionaries around it, the entry point of the corrected dictionaries alone)
FAMILIES = {"test_norm": (evaluator.test_norm_correction, evaluator.sharded_metrics_with_test_norm, evaluator.sharded_normalised_metrics),
            "local_scaling": (evaluator.local_scaling_correction, evaluator.sharded_metrics_with_local_scaling,
                              evaluator.sharded_local_scaled_metrics),
            "mutual_proximity": (evaluator.mutual_proximity_correction, evaluator.sharded_metrics_with_mutual_proximity,
                                 evaluator.sharded_mutual_proximity_metrics)}
CASES = ([("test_norm", dict(mode=mode, beta=12.5, qb_k=2, n_iter=2)) for mode in evaluator.TEST_NORM_MODES]
         + [("local_scaling", dict(mode=mode, k=3, bank=bank)) for mode in evaluator.LOCAL_SCALING_MODES for bank in (False, True)]
         + [("mutual_proximity", dict(mode=mode, bank=bank)) for mode in evaluator.MUTUAL_PROXIMITY_MODES for bank in (False, True)])
EXTRAS = dict(hubness_k=3, bootstrap=8, bootstrap_seed=11, ir=True)


def _dev(*arrays):
    return tuple(torch.from_numpy(np.asarray(a, dtype=np.float32)).to(DEV) for a in arrays)


@functools.lru_cache(maxsize=None)
def _sets():
    """24 x 24 single-sentence; 31 sentences over 9 videos (two of them with one sentence): uneven slabs on three ranks."""
    t, v, tm, vm = synth.make_samples(4242, "test", 24, Nt, Nv)
    sizes = np.asarray([1, 5, 3, 4, 2, 6, 1, 7, 2])
    ends = np.cumsum(sizes)
    mt, _, mtm, _ = synth.make_samples(92, "test", 31, Nt, Nv)
    _, mv, _, mvm = synth.make_samples(93, "test", 9, Nt, Nv)
    mt = mt + 0.4 * mv[np.searchsorted(ends, np.arange(31), side="right")].mean(1, keepdims=True)
    return {"single": _dev(t, v, tm, vm) + (None,), "multi": _dev(mt, mv, mtm, mvm) + ((ends - 1).tolist(),)}


@functools.lru_cache(maxsize=None)
def _bank():
    t, v, tm, vm = synth.make_samples(77, "train", 13, Nt, Nv)
    return _dev(t, tm, v, vm)


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("kind", ["single", "multi"])
@pytest.mark.parametrize("key,params", CASES, ids=lambda p: p if isinstance(p, str) else "-".join(str(x) for x in p.values()))
def test_the_driver_with_a_record_equals_the_legacy_entry_points(key, params, kind, W):
    m = _model()
    t, v, tm, vm, cut = _sets()[kind]
    make, with_raw, alone = FAMILIES[key]
    record = make(**params)
    assert record.key == key and record.needs_bank == (params.get("bank", False) or params["mode"] in evaluator.BANK_MODES)
    where = dict(querybank=_bank(), cut_off_points=cut)

    def fn(a, r):
        return (evaluator.sharded_evaluation(m, t, v, tm, vm, a, record, **where, **EXTRAS),
                with_raw(m, t, v, tm, vm, a, **params, **where, **EXTRAS),
                alone(m, t, v, tm, vm, a, **params, **where, hubness_k=EXTRAS["hubness_k"]))
    outs = [fn(SimpleNamespace(world_size=1), 0)] if W == 1 else _emulated(W, fn)
    for driver, legacy, corrected in outs:
        for d in range(2):
            assert {"hubness", "bootstrap", "ir", key} <= set(driver[d]) and {"bootstrap_vs_raw", "ir"} <= set(driver[d][key])
            assert _same_tree(driver[d], legacy[d])
            assert _same_tree(_without(driver[d][key], "bootstrap", "bootstrap_vs_raw", "ir"), corrected[d])
            assert _same_tree(driver[d], outs[0][0][d])                          # every rank holds the same tree
