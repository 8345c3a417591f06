"""fp64 NumPy restatement of the BertAdam step (DESIGN.md "BertAdam in the captured step"): the trainer's global clip, the
optimizer's per-tensor clip, moments without bias correction, weight decay on the parameter before the update, the warm-up
schedules read at the step counter BEFORE its increment, the upper clamp.  Plain formulas, no cleverness; the `mutate`
switches exist so that a test can show its bar tells a wrong formula from the right one."""
import math

import numpy as np


def warmup_cosine(x, warmup):
    return x / warmup if x < warmup else 0.5 * (1.0 + math.cos(math.pi * x))


def warmup_constant(x, warmup):
    return x / warmup if x < warmup else 1.0


def warmup_linear(x, warmup):
    return x / warmup if x < warmup else max((x - 1.0) / (warmup - 1.0), 0.0)


SCHEDULES = {"warmup_cosine": warmup_cosine, "warmup_constant": warmup_constant, "warmup_linear": warmup_linear}
GROUP_DEFAULTS = dict(lr=1e-4, warmup=-1, t_total=-1, schedule="warmup_linear", b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01,
                      max_grad_norm=1.0)


def scheduled_lr(group, step):
    if group["t_total"] == -1:
        return float(group["lr"])
    return float(group["lr"]) * SCHEDULES[group["schedule"]](step / group["t_total"], group["warmup"])


class State:
    """Parameters, moments and step counters of a list of tensors (float64 copies)."""

    def __init__(self, params, group_of, groups, clamp_max=None):
        self.p = [np.array(x, dtype=np.float64) for x in params]
        self.m = [np.zeros_like(x) for x in self.p]
        self.v = [np.zeros_like(x) for x in self.p]
        self.step = [0] * len(self.p)
        self.group_of = list(group_of)
        self.groups = [dict(GROUP_DEFAULTS, **g) for g in groups]
        self.clamp_max = dict(clamp_max or {})              # tensor index -> upper bound

    def lr(self):
        return [scheduled_lr(self.groups[self.group_of[t]], self.step[t]) for t in range(len(self.p))]


def step(state, grads, global_max_norm=None, mutate=()):
    """One step in place.  grads[t] is None for a tensor that takes no part (it keeps its step counter).  mutate: any of
    "no_tensor_clip", "no_global_clip", "bias_correction", "schedule_after_increment" -- deliberately wrong variants."""
    g64 = [None if g is None else np.asarray(g, dtype=np.float64) for g in grads]
    live = [t for t, g in enumerate(g64) if g is not None]
    c = 1.0
    if global_max_norm is not None and global_max_norm > 0 and "no_global_clip" not in mutate:
        total = math.sqrt(sum(float(np.sum(g64[t] * g64[t])) for t in live))
        c = min(1.0, global_max_norm / (total + 1e-6))
    for t in live:
        grp = state.groups[state.group_of[t]]
        ct = 1.0
        if grp["max_grad_norm"] > 0 and "no_tensor_clip" not in mutate:
            n_t = c * math.sqrt(float(np.sum(g64[t] * g64[t])))
            ct = min(1.0, grp["max_grad_norm"] / (n_t + 1e-6))
        gh = g64[t] * (c * ct)
        b1, b2 = grp["b1"], grp["b2"]
        state.m[t] = b1 * state.m[t] + (1.0 - b1) * gh
        state.v[t] = b2 * state.v[t] + (1.0 - b2) * gh * gh
        m, v = state.m[t], state.v[t]
        if "bias_correction" in mutate:
            k = state.step[t] + 1
            m, v = m / (1.0 - b1 ** k), v / (1.0 - b2 ** k)
        u = m / (np.sqrt(v) + grp["e"])
        if grp["weight_decay"] > 0:
            u = u + grp["weight_decay"] * state.p[t]
        lr = scheduled_lr(grp, state.step[t] + (1 if "schedule_after_increment" in mutate else 0))
        state.p[t] = state.p[t] - lr * u
        if t in state.clamp_max:
            state.p[t] = np.minimum(state.p[t], state.clamp_max[t])
        state.step[t] += 1
    return state


def distance(a, b):
    """max |a - b| / (|b| + 1e-3) over the elements; b is the side that is trusted more."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-3)))


def state_distance(got_p, got_m, got_v, ref):
    """Distance over all elements of p, m and v; ref is a State (or anything with .p/.m/.v lists)."""
    d = 0.0
    for got, want in ((got_p, ref.p), (got_m, ref.m), (got_v, ref.v)):
        for a, b in zip(got, want):
            d = max(d, distance(a, b))
    return d
