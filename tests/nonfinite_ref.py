"""fp64 restatement of the non-finite step guard around the BertAdam step, on top of tests/bertadam_ref.py: the
rule that calls a step bad, the guard's counters, the record ring.  Plain Python, no cleverness.

The rule.  total = sum over the tensors that take part of sum(g^2); the step is bad when total is not finite IN THE KERNELS'
ARITHMETIC, where the squares of one 4096-element chunk of one tensor are added in fp32: a NaN or an infinite entry, or a chunk
whose sum of squares reaches the value at which fp32 rounds to infinity (2^128 - 2^103).  The kernels add a chunk's squares in
an order of their own with one rounding per addition, so a chunk sum within a few 2^-24 of that value is not decided here; no
test goes near it (1e20 squared is 1e40).  A bad step changes nothing in p, m, v and the step counters.  For finite gradients
total is the plain fp64 sum: the kernels' total differs from it by the fp32 roundings of their chunk sums unless every partial
sum is exact in fp32 (gradients that are small multiples of a power of two: dyadic_gradients below), which is what a test that
wants the SAME fp32 grad_norm and clip from both sides feeds."""
import math

import numpy as np

import bertadam_ref as R

CHUNK = 4096
FP32_ROUNDS_TO_INF = 2.0 ** 128 - 2.0 ** 103
MAX_LOSSES = 8


def total_of_squares(grads):
    """The sum the decision is made from: fp64, tensors in table order, with the fp32 overflow of a chunk sum carried as inf."""
    total = 0.0
    for g in grads:
        if g is None:
            continue
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        for e0 in range(0, g.size, CHUNK):
            with np.errstate(over="ignore", invalid="ignore"):
                s = float(np.sum(g[e0:e0 + CHUNK] * g[e0:e0 + CHUNK]))
            if s >= FP32_ROUNDS_TO_INF:
                s = math.inf
            total += s
    return total


def coefficient(global_max_norm, total):
    """c as launch B forms it, NaN kept (bertadam_ref.step has no use for a NaN c: it never sees a bad step)."""
    if global_max_norm is None or not global_max_norm > 0:
        return 1.0
    c = global_max_norm / (math.sqrt(total) + 1e-6) if total == total else math.nan
    return 1.0 if c > 1.0 else c


class Guard:
    """NrStepGuard and the ring of NrStepRecord, as Python values."""

    def __init__(self, n_ring=256):
        assert n_ring >= 1 and n_ring & (n_ring - 1) == 0
        self.attempts = self.skipped = self.consecutive = self.max_consecutive = 0
        self.last_skipped = -1
        self.n_ring = n_ring
        self.ring = [None] * n_ring

    def stats(self):
        return {k: getattr(self, k) for k in ("attempts", "skipped", "consecutive", "max_consecutive", "last_skipped")}

    def records(self):
        """The records still held, oldest first."""
        n = min(self.attempts, self.n_ring)
        return [self.ring[a & (self.n_ring - 1)] for a in range(self.attempts - n, self.attempts)]


def guarded_step(state, guard, grads, global_max_norm=None, losses=()):
    """One guarded step in place -> True when it was skipped."""
    assert len(losses) <= MAX_LOSSES
    total = total_of_squares(grads)
    bad = not math.isfinite(total)
    attempt = guard.attempts
    guard.attempts += 1
    if bad:
        guard.skipped += 1
        guard.consecutive += 1
        guard.max_consecutive = max(guard.max_consecutive, guard.consecutive)
        guard.last_skipped = attempt
    else:
        guard.consecutive = 0
    with np.errstate(over="ignore", invalid="ignore"):
        record = dict(attempt=attempt, grad_norm=np.float32(math.sqrt(total) if total == total else math.nan),
                      clip=np.float32(coefficient(global_max_norm, total)), skipped=int(bad),
                      losses=[np.float32(x) for x in losses] + [np.float32(0)] * (MAX_LOSSES - len(losses)))
    guard.ring[attempt & (guard.n_ring - 1)] = record
    if not bad:
        R.step(state, grads, global_max_norm=global_max_norm)
    return bad


def dyadic_gradients(rs, sizes, scale=1.0):
    """Gradients k / 8 * scale, k an integer in [-16, 16], scale a power of two: every square is a multiple of scale^2 / 64 and
    at most 256 of them, so every partial sum over up to 2^16 elements stays below 2^24 units and is exact in fp32: any order of
    addition gives the fp64 sum."""
    assert math.log2(scale) == int(math.log2(scale)) and sum(sizes) <= 2 ** 16
    return [(rs.randint(-16, 17, size=n) / 8.0 * scale).astype(np.float32) for n in sizes]
