#!/usr/bin/env python
"""Captures tests/golden/bertadam_small.npz from the UNMODIFIED reference optimizer (models/optimization.py:76-211) on the CPU
and appends a line to tests/golden/CAPTURE_LOG_bertadam.txt.  Data only: parameters, moments and learning rates.

    python tools/capture_bertadam_golden.py [--reference /root/reference]

Six fp32 tensors in four groups (lr 1e-4 / 1e-7, weight decay 0.2 / 0), warmup_cosine with warmup 0.1 over t_total = 12, twelve
steps.  Run A wraps every step() in the trainer's global clip (1.0) and logit-scale clamp (trainer.py:104-119); run B calls
step() and the clamp alone, so that the optimizer's own per-tensor clip engages.  Gradients: RandomState(seed).standard_normal
in tensor order, step after step, times 10 on steps 0, 3, 6, 9 and times 0.01 otherwise; tensor 1 gets an all-zero gradient
on step 5 and tensor 3 gets none at all on step 7 (the draw is made and dropped, so the stream does not depend on it).
The log line carries d_ref: the distance of the reference's fp32 result from the fp64 restatement (tests/bertadam_ref.py)."""
import argparse
import datetime
import importlib.util
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bertadam_ref as R  # noqa: E402

SHAPES = [(96, 64), (512,), (1,), (4099,), (7, 3, 5), (1,)]
GROUP_OF = [0, 2, 3, 1, 1, 3]
GROUPS = [dict(lr=1e-7, weight_decay=0.2), dict(lr=1e-4, weight_decay=0.2), dict(lr=1e-7, weight_decay=0.0),
          dict(lr=1e-4, weight_decay=0.0)]
COMMON = dict(warmup=0.1, t_total=12, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6, max_grad_norm=1.0)
N_STEPS = 12
RECORD = (1, 2, 8, 12)
CLAMP_INDEX, CLAMP_MAX = 5, math.log(100.0)
ZERO_GRAD = (5, 1)          # (step, tensor)
NO_GRAD = (7, 3)
SEED = 20241026


def scales():
    return np.array([10.0 if s % 3 == 0 and s < 12 else 0.01 for s in range(N_STEPS)], dtype=np.float64)


def initial_params(seed):
    rs = np.random.RandomState(seed + 1)
    out = [(0.05 * rs.standard_normal(s)).astype(np.float32) for s in SHAPES]
    out[CLAMP_INDEX] = np.array([CLAMP_MAX - 1e-4], dtype=np.float32)
    return out


def gradients(seed):
    """grads[step][tensor]: fp32 array or None."""
    rs = np.random.RandomState(seed)
    sc = scales()
    out = []
    for s in range(N_STEPS):
        row = []
        for t, shp in enumerate(SHAPES):
            g = (rs.standard_normal(shp) * sc[s]).astype(np.float32)
            if (s, t) == ZERO_GRAD:
                g = np.zeros(shp, dtype=np.float32)
            row.append(None if (s, t) == NO_GRAD else g)
        out.append(row)
    return out


def run_reference(BertAdam, init, grads, global_clip):
    params = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in init]
    groups = [dict(params=[p for p, q in zip(params, GROUP_OF) if q == gi], **g) for gi, g in enumerate(GROUPS)]
    opt = BertAdam(groups, lr=1e-4, weight_decay=0.2, **COMMON)
    rec = {}
    engaged = 0
    for s in range(N_STEPS):
        for p, g in zip(params, grads[s]):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        if global_clip:
            torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        engaged += int(float(params[CLAMP_INDEX].data) > CLAMP_MAX)
        torch.clamp_(params[CLAMP_INDEX].data, max=CLAMP_MAX)
        if s + 1 in RECORD:
            zero = [np.zeros(shp, dtype=np.float32) for shp in SHAPES]
            rec[s + 1] = dict(
                p=[p.detach().numpy().copy() for p in params],
                m=[opt.state[p]["next_m"].numpy().copy() if "next_m" in opt.state[p] else z for p, z in zip(params, zero)],
                v=[opt.state[p]["next_v"].numpy().copy() if "next_v" in opt.state[p] else z for p, z in zip(params, zero)],
                lr=np.array(opt.get_lr(), dtype=np.float64))
    return rec, engaged


def run_restatement(init, grads, global_clip, record=RECORD, mutate=()):
    st = R.State(init, GROUP_OF, [dict(g, **COMMON) for g in GROUPS], clamp_max={CLAMP_INDEX: CLAMP_MAX})
    rec = {}
    for s in range(N_STEPS):
        R.step(st, grads[s], global_max_norm=1.0 if global_clip else None, mutate=mutate)
        if s + 1 in record:
            rec[s + 1] = dict(p=[x.copy() for x in st.p], m=[x.copy() for x in st.m], v=[x.copy() for x in st.v])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--seed", type=int, default=SEED)
    args = ap.parse_args()
    path = os.path.join(args.reference, "NeighborRetr", "models", "optimization.py")
    if not os.path.exists(path):
        print("reference checkout not present; nothing to capture")
        return 1
    spec = importlib.util.spec_from_file_location("reference_optimization", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_num_threads(1)
    init, grads = initial_params(args.seed), gradients(args.seed)
    out = dict(seed=np.int64(args.seed), scales=scales(), record=np.array(RECORD, dtype=np.int64))
    for t, x in enumerate(init):
        out[f"init_{t}"] = x
    d_ref = {}
    notes = []
    for run, clip in (("A", True), ("B", False)):
        rec, engaged = run_reference(mod.BertAdam, init, grads, clip)
        want = run_restatement(init, grads, clip)
        d = 0.0
        for k in RECORD:
            for key in ("p", "m", "v"):
                for t in range(len(SHAPES)):
                    out[f"{run}_{key}_{k}_{t}"] = rec[k][key][t]
                    d = max(d, R.distance(rec[k][key][t], want[k][key][t]))
            out[f"{run}_lr_{k}"] = rec[k]["lr"]
        d_ref[run] = d
        out[f"d_ref_{run}"] = np.float64(d)
        notes.append(f"run {run}: d_ref {d:.3e}, clamp engaged on {engaged} of {N_STEPS} steps")
    dst = os.path.join(ROOT, "tests", "golden", "bertadam_small.npz")
    np.savez_compressed(dst, **out)
    size = os.path.getsize(dst)
    line = (f"{datetime.date.today().isoformat()} capture_bertadam_golden.py seed {args.seed} torch {torch.__version__}: "
            + "; ".join(notes) + f"  ({size} bytes)")
    with open(os.path.join(ROOT, "tests", "golden", "CAPTURE_LOG_bertadam.txt"), "a") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
