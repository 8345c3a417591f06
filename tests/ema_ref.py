"""fp64 NumPy restatement of the weight EMA: per averaged element, after the parameter's update of the step,

    d = min(decay, (1 + n) / (10 + n)) under warm-up, else decay        (n: the updates that have happened before this one)
    e = e + (1 - d) (p_new - e);   n += 1

Plain formulas, no cleverness; the `mutate` switches exist so that a test can show its bar tells a wrong rule from the right
one.  `update_fp32` is the same rule with the three fp32 roundings of the kernels (the difference, 1 - d, the fused multiply-add),
for checks that need no GPU."""
import numpy as np

MUTANTS = ("no_warmup", "swapped", "stale")


def decay_at(decay, warmup, n):
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


class State:
    """Shadows (float64 copies of the parameters at construction), the decay, the warm-up switch and the count of updates."""

    def __init__(self, params, decay=0.999, warmup=True):
        self.e = [np.array(x, dtype=np.float64) for x in params]
        self.decay, self.warmup, self.updates = float(decay), bool(warmup), 0
        self.last_decay = None


def _decay(state, mutate):
    d = decay_at(state.decay, state.warmup and "no_warmup" not in mutate, state.updates)
    state.last_decay = d
    return 1.0 - d if "swapped" in mutate else d


def update(state, params, before=None, mutate=()):
    """One update in place.  params[t]: the parameter AFTER the step's update (None: tensor t is not averaged in this step);
    before[t]: the parameter before it, which only the mutant "stale" averages.  mutate: any of MUTANTS -- "no_warmup" (the
    decay without its ramp), "swapped" (d and 1 - d exchanged), "stale" -- deliberately wrong variants."""
    d = _decay(state, mutate)
    source = before if "stale" in mutate else params
    for t, p in enumerate(source):
        if params[t] is None:
            continue
        state.e[t] = state.e[t] + (1.0 - d) * (np.asarray(p, dtype=np.float64) - state.e[t])
    state.updates += 1
    return state


def update_fp32(state, params):
    """The rule as the kernels round it, on float32 shadows: omd = fl(1 - d); e = fl(omd * fl(p - e) + e).  (The product of two
    floats is exact in double; the sum is rounded to double and then to float, which differs from a fused multiply-add only in
    rare double-rounding cases, far below any bar here.)"""
    d = _decay(state, ())
    omd = np.float32(1.0 - d)
    for t, p in enumerate(params):
        if p is None:
            continue
        e = np.asarray(state.e[t], dtype=np.float32)
        diff = (np.asarray(p, dtype=np.float32) - e).astype(np.float32)
        state.e[t] = (np.float64(omd) * diff.astype(np.float64) + e.astype(np.float64)).astype(np.float32)
    state.updates += 1
    return state


def random_walk(seed, sizes, steps, scale=0.05, move=1e-3):
    """steps + 1 float32 parameter lists: values of `scale`, then `steps` moves of `move` each (the test's input)."""
    rs = np.random.RandomState(seed)
    rows = [[(scale * rs.standard_normal(n)).astype(np.float32) for n in sizes]]
    for _ in range(steps):
        rows.append([(x + move * rs.standard_normal(len(x))).astype(np.float32) for x in rows[-1]])
    return rows


def scaled_error(got, ref, rows):
    """max |got - ref| / A over all shadows; A: the largest magnitude of any parameter (rows) or reference shadow."""
    A = max([float(np.max(np.abs(x))) for row in rows for x in row if len(x)] + [float(np.max(np.abs(x))) for x in ref if len(x)])
    err = max([float(np.max(np.abs(np.asarray(g, dtype=np.float64) - r))) for g, r in zip(got, ref) if len(r)] + [0.0])
    return err / A, A
