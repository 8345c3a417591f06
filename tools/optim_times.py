#!/usr/bin/env python
"""What the optimizer tail of a training step costs, before and after the update moved into the step's graph (DESIGN.md
"BertAdam in the captured step").  configs[1] (B = 128, Nt = 24, Nv = 12, M = 512, K = 20), one GPU, profiler off:

  (a) GraphedStep replay (forward + backward) followed by the eager tail
      clip_grad_norm_(1.0) + AdamW.step + zero_grad + logit-scale clamp        -- the entry point's default step
  (b) GraphedStep(optimizer=BertAdam) replay: forward + backward + update in ONE graph (global clip and clamp inside)

alternating blocks of (a) and (b) in one process, 200 steps each after warm-up, host clock around a final synchronise per
block; the spread over the blocks is printed next to the mean.  Then the update alone (three launches, device events), and
the same for the parameter set of `--encoders 1` (ViT-B/32 towers + head, synthetic gradients: the tail only, no forward).

    python tools/optim_times.py [--out profiles/optim_step_times.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/optim_times.py --kernels-only     # per-kernel times, a run of its own
    python tools/optim_times.py --summary DIR                                                 # ... read from its trace database
    python tools/optim_times.py --guard [--out profiles/optim_guard_times.txt]                # the non-finite guard's cost (6.9)
    python tools/optim_times.py --ema [--out profiles/optim_ema_times.txt]                    # the weight EMA's cost (6.11)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from main_retrieval import GraphedStep  # noqa: E402
from neighborretr_amd import modeling, optim, synth  # noqa: E402

DEV = "cuda"
B, Nt, Nv, M, K = 128, 24, 12, 512, 20
HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E peak
BYTES_PER_ELEMENT = 28     # read p, g, m, v; write p, m, v


class Args:
    lr, coef_lr, weight_decay, warmup_proportion = 1e-4, 1e-3, 0.2, 0.1


def head_model(problem):
    m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(7).items()}, strict=False)
    m = m.to(DEV).train()
    m.mb_feat_t, m.mb_feat_v = problem["mb_feat_t"].clone(), problem["mb_feat_v"].clone()
    m.mb_mask_t, m.mb_mask_v = problem["mb_mask_t"].clone(), problem["mb_mask_v"].clone()
    m.mb_ind = torch.arange(M, device=DEV)
    return m


def step_times(out):
    problem = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_problem(1002, B, Nt, Nv, M).items()}
    batch = tuple(problem[k] for k in ("text_feat", "text_mask", "video_feat", "video_mask", "idx"))
    ma, mb = head_model(problem), head_model(problem)
    pa = [p for p in ma.parameters() if p.requires_grad]
    pb = [p for p in mb.parameters() if p.requires_grad]
    adamw = torch.optim.AdamW(ma.parameters(), lr=Args.lr, weight_decay=Args.weight_decay)
    bert = optim.prep_optimizer(Args, mb, 10 ** 6, 0, global_max_norm=1.0, clamp_logit_scale=True, wrap=False)[0]
    ga = GraphedStep(ma, batch, pa)
    gb = GraphedStep(mb, batch, pb, optimizer=bert)
    ln100 = float(np.log(100))

    def a():
        ga.run(batch)
        torch.nn.utils.clip_grad_norm_(ma.parameters(), 1.0)
        adamw.step()
        adamw.zero_grad(set_to_none=True)
        torch.clamp_(ma.clip.logit_scale.data, max=ln100)

    def b():
        gb.run(batch)
        bert.zero_grad(set_to_none=True)

    def bare():
        ga.run(batch)

    def block(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for fn in (a, b, bare):
        block(fn, 20)
    ta, tb, t0 = [], [], []
    for _ in range(4):                                # 4 x 50 = 200 steps each, alternating
        ta.append(block(a, 50))
        tb.append(block(b, 50))
        t0.append(block(bare, 50))
    n_elem = sum(p.numel() for p in pb)
    out(f"configs[1] head only: {len(pb)} parameter tensors, {n_elem} elements")
    out(f"  forward + backward graph alone                          : {np.mean(t0):.3f} ms/step   blocks {np.round(t0, 3).tolist()}")
    out(f"  (a) graph + eager clip / AdamW / zero_grad / clamp      : {np.mean(ta):.3f} ms/step   blocks {np.round(ta, 3).tolist()}")
    out(f"  (b) graph with the BertAdam update inside               : {np.mean(tb):.3f} ms/step   blocks {np.round(tb, 3).tolist()}")
    out(f"  tail of (a): {np.mean(ta) - np.mean(t0):.3f} ms; tail of (b): {np.mean(tb) - np.mean(t0):.3f} ms; spread of (a) over its "
        f"blocks {max(ta) - min(ta):.3f} ms")
    return bert, pb


def update_alone(out, name, params, opt, n=100):
    """The three launches by themselves on static gradients: device time between two events, eager and replayed."""
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
    opt.prepare(params)
    for _ in range(5):
        opt.step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        opt.step()
    e1.record()
    host = (time.perf_counter() - t0) / n * 1e6
    torch.cuda.synchronize()
    eager = e0.elapsed_time(e1) / n * 1e3
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        live = opt.issue()
    g.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    opt.advance(live)
    replay = e0.elapsed_time(e1) / n * 1e3
    n_elem = sum(p.numel() for p in params)
    rate = n_elem * BYTES_PER_ELEMENT / (replay * 1e-6)
    # the multi-rank step's layout: gradients as views of ONE flat buffer at odd 4-byte offsets (p, m, v stay aligned)
    flat = torch.randn(n_elem + 4 * len(params) + 8, device=DEV) * 0.01
    off = 1
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel() + (1 if (off + p.numel()) % 4 == 0 else 0)
    assert all(p.grad.data_ptr() % 16 for p in params if p.numel() > 3)
    for _ in range(5):
        opt.step()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    views = e0.elapsed_time(e1) / n * 1e3
    out(f"{name}: {len(params)} tensors, {n_elem} elements, {n_elem * BYTES_PER_ELEMENT / 1e6:.1f} MB per step in the update launch")
    out(f"  three launches, eager: {eager:.1f} us device, {host:.1f} us host to issue; replayed from a graph of their own: {replay:.1f} us")
    out(f"  gradients as misaligned views of one flat buffer (dword gradient loads, 16-byte p / m / v): {views:.1f} us eager")
    out(f"  all three launches together move the update launch's bytes at {rate / 1e12:.2f} TB/s (a lower bound for the update "
        "launch alone; its own time and share of the HBM peak come from the kernel trace: --summary)")


def guard_cost(out, blocks=6, n=50):
    """the three launches with the non-finite guard against the three without, head-only table, each replayed
    from a graph of its own on static finite gradients; alternating blocks, device events around each block."""
    graphs = {}
    for name, guarded in (("unguarded", False), ("guarded", True)):
        m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K)).to(DEV).train()
        params = list(m.parameters())
        opt = optim.prep_optimizer(Args, m, 10 ** 6, 0, global_max_norm=1.0, clamp_logit_scale=True, wrap=False,
                                   skip_nonfinite=guarded)[0]
        gen = torch.Generator(device=DEV).manual_seed(1)
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen, device=DEV) * 0.01
        opt.prepare(params)
        if guarded:
            opt.watch_losses(torch.zeros(5, device=DEV))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.issue()
        for _ in range(10):
            g.replay()
        graphs[name] = (g, opt, m)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in graphs}
    for _ in range(blocks):
        for name, (g, _, _) in graphs.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / n * 1e3)
    stats = graphs["guarded"][1].guard_stats()
    assert stats["skipped"] == 0 and stats["attempts"] == 10 + blocks * n, stats
    out(f"non-finite guard, head only, three launches replayed from a graph of their own, {blocks} alternating blocks of {n}:")
    for name, t in times.items():
        out(f"  {name:9s}: median {np.median(t):.2f} us per step   blocks {np.round(t, 2).tolist()}   spread {max(t) - min(t):.2f} us")
    out(f"  guarded median - unguarded median: {np.median(times['guarded']) - np.median(times['unguarded']):+.2f} us")


def ema_cost(out, encoders, blocks=6, n=50):
    """the three launches with the weight EMA attached against the three without, and the stand-alone
    update() (two launches), each replayed from a graph of its own on static finite gradients; alternating blocks, device
    events around each block.  By bytes the update launch moves 36 instead of 28 per element, update() 12."""
    graphs = {}
    for name in ("without", "with ema", "update()"):
        if encoders:
            m, params = encoder_params()
        else:
            m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K)).to(DEV).train()
            params = list(m.parameters())
        ema = optim.WeightEma(m.named_parameters(), decay=0.999) if name != "without" else None
        g = torch.cuda.CUDAGraph()
        if name == "update()":
            ema.update()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                ema.update()
            opt = None
        else:
            opt = optim.prep_optimizer(Args, m, 10 ** 6, 0, global_max_norm=1.0, clamp_logit_scale=True, wrap=False, ema=ema)[0]
            gen = torch.Generator(device=DEV).manual_seed(1)
            for p in params:
                p.grad = torch.randn(p.shape, generator=gen, device=DEV) * 0.01
            opt.prepare(params)
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                opt.issue()
        for _ in range(10):
            g.replay()
        graphs[name] = (g, opt, ema, m)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in graphs}
    for _ in range(blocks):
        for name, (g, _, _, _) in graphs.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / n * 1e3)
    assert graphs["with ema"][2].updates() == 10 + blocks * n and graphs["update()"][2].updates() == 11 + blocks * n
    n_elem = sum(p.numel() for p in graphs["without"][3].parameters())
    out(f"weight EMA, {'--encoders 1 parameter set' if encoders else 'head only'} ({n_elem} elements), each form replayed from a "
        f"graph of its own, {blocks} alternating blocks of {n}:")
    for name, t in times.items():
        out(f"  {name:9s}: median {np.median(t):.2f} us per step   blocks {np.round(t, 2).tolist()}   spread {max(t) - min(t):.2f} us")
    med = {name: float(np.median(t)) for name, t in times.items()}
    out(f"  with ema / without: {med['with ema'] / med['without']:.3f} of the three launches (by the update launch's bytes at most "
        f"36 / 28 = {36 / 28:.3f}); update() / without: {med['update()'] / med['without']:.3f} (12 / 28 = {12 / 28:.3f} of the update "
        "launch alone)")
    del graphs
    torch.cuda.empty_cache()


def adamw_tail_alone(out, name, params, n=50):
    opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.2)
    grads = [torch.randn_like(p) * 0.01 for p in params]

    def tail():
        for p, g in zip(params, grads):
            p.grad = g
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    for _ in range(5):
        tail()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tail()
    torch.cuda.synchronize()
    out(f"{name}: eager clip_grad_norm_ + AdamW.step + zero_grad alone: {(time.perf_counter() - t0) / n * 1e3:.3f} ms/step (host clock, synchronised)")


def encoder_params():
    m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K), with_encoders=True).to(DEV).train()
    return m, [p for p in m.parameters() if p.requires_grad]


def summary(d, out=print):
    """Per-launch times of the three kernels from the trace database rocprofv3 wrote under d (its `top_kernels` view; run with
    --kernels-only: the head's parameters), and the update launch's bytes per second against the HBM peak."""
    import glob
    import sqlite3
    path = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))[0]
    rows = list(sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"))
    m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K))
    n_elem = sum(p.numel() for p in m.parameters())
    out(f"rocprofv3 --kernel-trace --stats of {os.path.basename(__file__)} --kernels-only (head only, {n_elem} elements):")
    for name, calls, total in rows:
        if "nr_bertadam" not in name:
            continue
        per = total / calls                                       # the view's durations are microseconds
        line = f"  {name.split('(')[0]:30s} {calls:4d} launches  {per:8.2f} us per launch"
        if "update" in name:
            rate = n_elem * BYTES_PER_ELEMENT / (per * 1e-6)
            line += (f"  = {rate / 1e12:.2f} TB/s for {BYTES_PER_ELEMENT} B x {n_elem} elements = {rate / HBM_PEAK:.2f} of the "
                     f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak (memory-bound)")
        out(line)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        return summary(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="50 eager updates of the head's parameters and nothing else")
    ap.add_argument("--skip-encoders", action="store_true")
    ap.add_argument("--guard", action="store_true", help="only: the three launches with the non-finite guard against without")
    ap.add_argument("--ema", action="store_true", help="only: the three launches with the weight EMA against without, and update()")
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    if args.guard:
        out(f"tools/optim_times.py --guard on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
        guard_cost(out)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if args.ema:
        out(f"tools/optim_times.py --ema on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
        ema_cost(out, encoders=False)
        if not args.skip_encoders:
            ema_cost(out, encoders=True, n=20)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if args.kernels_only:
        m = modeling.NeighborRetr(modeling.default_config(num_neighbors=K)).to(DEV).train()
        params = list(m.parameters())
        opt = optim.prep_optimizer(Args, m, 10 ** 6, 0, global_max_norm=1.0, clamp_logit_scale=True, wrap=False)[0]
        for p in params:
            p.grad = torch.randn_like(p) * 0.01
        for _ in range(50):
            opt.step()
        torch.cuda.synchronize()
        return
    out(f"tools/optim_times.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    bert, pb = step_times(out)
    update_alone(out, "head only", pb, bert)
    if not args.skip_encoders:
        m, params = encoder_params()
        opt = optim.prep_optimizer(Args, m, 10 ** 6, 0, global_max_norm=1.0, clamp_logit_scale=True, wrap=False)[0]
        update_alone(out, "--encoders 1 parameter set", params, opt, n=30)
        adamw_tail_alone(out, "--encoders 1 parameter set", params)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
