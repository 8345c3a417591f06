"""GPU: a training run cut at a step boundary and resumed from the training-state file (neighborretr_amd.checkpoint, DESIGN.md
6.12) continues with the BITS of the run that was not cut.  Every comparison is bitwise (bytes); there is no tolerance here.

"Straight": N steps in a row.  "Cut": k steps, capture_state -> save -> fresh model, optimizer and EMA objects built from other
initial weights -> load -> restore_state, then N - k steps.  Shapes: the entry point's at --batch_size 32 --synthetic_train 192
(6 steps an epoch) --mb_batch 2 (a bank of 64: the ring wraps at the third step), default token counts, K = 20."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from neighborretr_amd import checkpoint, optim, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
B, N_TRAIN, NT, NV, BANK, STEPS, CUT = 32, 192, 24, 12, 64, 6, 4


class _Args:
    lr, coef_lr, weight_decay, warmup_proportion = 1e-4, 1e-3, 0.2, 0.1


@functools.lru_cache(maxsize=None)
def _data():
    t, v, tm, vm = (torch.from_numpy(a).to(DEV) for a in synth.make_samples(42, "train", N_TRAIN, NT, NV))
    return t, tm, v, vm, torch.arange(N_TRAIN, device=DEV)


def _batch(i, blanks=()):
    """Step i (0-based) of the epoch; blanks: the 1-based steps whose first video comes back undecodable (--synthetic_blank)."""
    t, tm, v, vm, idx = (x[i * B:(i + 1) * B] for x in _data())
    if i + 1 in blanks:
        v, vm = v.clone(), vm.clone()
        v[0] = 0
        vm[0] = 0
    return t, tm, v, vm, idx


def _model(seed):
    from neighborretr_amd import modeling
    from util import params
    m = modeling.NeighborRetr(modeling.default_config())
    m.load_state_dict(params(seed=seed), strict=False)
    m = m.to(DEV).train()
    with torch.no_grad():
        m.clip.logit_scale.fill_(float(np.log(100.0)))
    return m


def _load_bank(m):
    """What main_retrieval.load_memory_bank hands over in feature mode: the first mb_batch batches."""
    t, tm, v, vm, idx = (x[:BANK] for x in _data())
    m.mb_ind, m.mb_feat_t, m.mb_feat_v = idx.clone(), t.clone(), v.clone()
    m.mb_mask_t, m.mb_mask_v, m.mb_batch = tm.clone(), vm.clone(), BANK


class Run:
    """A model with its optimizer and EMA, stepping the way main_retrieval.train_epoch does.
    kind: bertadam (device guard, attached EMA) or adamw (host guard, stand-alone EMA); graph: through GraphedStep."""

    def __init__(self, kind, graph, seed=7, bank=True, blanks=()):
        self.kind, self.graph, self.blanks = kind, graph, tuple(blanks)
        self.m = _model(seed)
        if bank:
            _load_bank(self.m)
        self.ema = optim.WeightEma(self.m.named_parameters(), decay=0.99)
        self.host_skips = None
        if kind == "bertadam":
            self.opt = optim.prep_optimizer(_Args, self.m, 2 * STEPS, 0, global_max_norm=1.0, clamp_logit_scale=True, wrap=False,
                                            skip_nonfinite=True, ema=self.ema)[0]
        else:
            self.opt = torch.optim.AdamW(self.m.parameters(), lr=_Args.lr, weight_decay=_Args.weight_decay)
            self.host_skips = dict(skipped=0, consecutive=0, max_consecutive=0, norms=[])
        self.step = None
        self.resumed = False

    def take(self, i):
        """Step i -> its five losses on the host."""
        m, opt = self.m, self.opt
        batch = _batch(i, self.blanks)
        if self.graph:
            if self.step is None:
                sys.path.insert(0, ROOT)
                from main_retrieval import GraphedStep
                # (a resumed run captures where the straight run replays: main_retrieval.train_epoch's way around it)
                kept = checkpoint.volatile_words(m) if self.resumed else None
                self.step = GraphedStep(m, batch, [p for p in m.parameters() if p.requires_grad], optimizer=opt)
                if kept is not None:
                    checkpoint.reapply_volatile(m, kept)
            losses = self.step.run(batch)
            opt.zero_grad(set_to_none=True)
        elif self.kind == "bertadam":
            losses = m(*batch, 0)
            losses[0].backward()
            opt.watch_losses(torch.stack([l.detach().float() for l in losses]))
            opt.step()
            opt.zero_grad(set_to_none=True)
        else:
            losses = m(*batch, 0)
            losses[0].backward()
            norm, hs = float(torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)), self.host_skips
            hs["norms"].append(norm)
            if np.isfinite(norm):
                hs["consecutive"] = 0
                opt.step()
                self.ema.update()
            else:
                hs["skipped"] += 1
                hs["consecutive"] += 1
                hs["max_consecutive"] = max(hs["max_consecutive"], hs["consecutive"])
            opt.zero_grad(set_to_none=True)
            torch.clamp_(m.clip.logit_scale.data, max=float(np.log(100)))
        return torch.stack([l.detach().float() for l in losses]).cpu()

    def capture(self, next_step):
        return checkpoint.capture_state(self.m, self.opt, self.ema, position=dict(epoch=0, next_step=next_step, global_step=next_step),
                                        config=dict(batch_size=B), host_guard=self.host_skips)

    def snapshot(self):
        """Everything a later step depends on, as host values."""
        m, opt = self.m, self.opt
        torch.cuda.synchronize()
        out = dict(params=[p.detach().cpu() for p in m.parameters()], shadows=[e.cpu() for e in self.ema.shadows],
                   ema_state=self.ema._state.cpu(), ema_updates=self.ema.updates(),
                   bank={k: v.cpu() for k, v in m._mb.items()}, mb_batch=int(m.mb_batch),
                   head=int(m._mb_head_dev.item()) if m._mb_head_dev is not None else int(m._mb_head),
                   rng=None if m._rng_state is None else m._rng_state.cpu())
        if self.kind == "bertadam":
            stats = opt.guard_stats()
            out.update(m=[opt.state[p]["next_m"].cpu() for p in opt._all if len(opt.state[p])],
                       v=[opt.state[p]["next_v"].cpu() for p in opt._all if len(opt.state[p])],
                       steps=opt._dev["steps"].cpu(), host_steps=[opt.state[p]["step"] for p in opt._all if len(opt.state[p])],
                       guard=stats, records=torch.frombuffer(bytearray(opt.records().tobytes()), dtype=torch.uint8),
                       lr=opt.group_lr())
        else:
            out.update(adamw=checkpoint._plain(opt.state_dict()["state"]), host_skips=checkpoint._plain(dict(self.host_skips)))
        return out


def bits(a, b, where=""):
    """None when a and b are the same structure of the same bits, else where they first differ."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        ok = (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
              and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))
        return None if ok else where
    if isinstance(a, dict):
        if not isinstance(b, dict) or list(a) != list(b):
            return where + " (keys)"
        return next((d for d in (bits(a[k], b[k], f"{where}/{k}") for k in a) if d), None)
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return where + " (length)"
        return next((d for d in (bits(x, y, f"{where}/{i}") for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if isinstance(a, float):
        return None if isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes() else where
    return None if type(a) is type(b) and a == b else where


@functools.lru_cache(maxsize=None)
def _straight(kind, graph, blanks=()):
    """The uninterrupted run, computed once per form -> (the losses of every step, the final snapshot, the final `_mb_gen`)."""
    torch.manual_seed(20240607)
    run = Run(kind, graph, blanks=blanks)
    losses = [run.take(i) for i in range(STEPS)]
    return losses, run.snapshot(), run.m._mb_gen


def _cut(kind, graph, tmp_path, blanks=()):
    torch.manual_seed(20240607)
    first = Run(kind, graph, blanks=blanks)
    losses = [first.take(i) for i in range(CUT)]
    path = str(tmp_path / "training_state.pt")
    checkpoint.save(path, first.capture(CUT))
    del first
    second = Run(kind, graph, seed=8, bank=False, blanks=blanks)        # other initial weights, no bank, new optimizer and EMA
    state = checkpoint.load(path, config=dict(batch_size=B))
    where = [p.data_ptr() for p in second.m.parameters()] + [e.data_ptr() for e in second.ema.shadows] + [second.ema._state.data_ptr()]
    pos = checkpoint.restore_state(state, second.m, second.opt, second.ema, host_guard=second.host_skips)
    assert pos == dict(epoch=0, next_step=CUT, global_step=CUT)
    assert where == [p.data_ptr() for p in second.m.parameters()] + [e.data_ptr() for e in second.ema.shadows] + [second.ema._state.data_ptr()]
    second.resumed = True
    losses += [second.take(i) for i in range(CUT, STEPS)]
    return losses, second.snapshot(), second


def _assert_equal_runs(got, want):
    for i, (x, y) in enumerate(zip(got[0], want[0])):
        assert bits(x, y) is None, f"the losses of step {i + 1} differ: {x.tolist()} / {y.tolist()}"
    assert len(got[0]) == len(want[0]) == STEPS
    diff = bits(got[1], want[1], "state")
    assert diff is None, f"first difference at {diff}"


# ---- 1, 2: bertadam with the device guard and an attached EMA, eager and through GraphedStep -------------------------------------
def test_eager_bertadam_resumes_bit_for_bit(tmp_path):
    want = _straight("bertadam", False)
    assert want[1]["head"] != 0 or want[1]["bank"]["mb_ind"][0] >= BANK          # the ring has wrapped
    assert want[1]["guard"]["attempts"] == STEPS and want[1]["ema_updates"] == STEPS
    _assert_equal_runs(_cut("bertadam", False, tmp_path), want)


def test_graphed_bertadam_resumes_bit_for_bit(tmp_path):
    """The cut run captures its graph at its first step after the restore, in the middle of the epoch, where the straight run
    replays: the capture's warm-up passes advance the noise counter (the capture hazard of DESIGN.md 6.12).  Without
    checkpoint.reapply_volatile after that capture this test fails: the noise words of the final state differ, the counter
    standing three prologues ahead (seen on an MI355X; at these shapes the draws only break ties between equal densities, and
    the losses of steps 5 and 6 came out the same bits all the same -- the state comparison is what catches it)."""
    want = _straight("bertadam", True)
    got = _cut("bertadam", True, tmp_path)
    assert got[2].step.form == "whole"
    _assert_equal_runs(got, want)


# ---- 3: a skipped step on each side of the cut -----------------------------------------------------------------------------------
def test_skipped_steps_on_both_sides_of_the_cut(tmp_path):
    blanks = (2, 5)
    want = _straight("bertadam", True, blanks)
    assert want[1]["guard"]["skipped"] == 2 and want[1]["guard"]["last_skipped"] == 4 and want[1]["guard"]["max_consecutive"] == 1
    got = _cut("bertadam", True, tmp_path, blanks)
    stats = got[2].opt.guard_stats()
    assert stats["skipped"] == 2
    assert (stats["last_skipped"], stats["max_consecutive"]) == (want[1]["guard"]["last_skipped"], want[1]["guard"]["max_consecutive"])
    assert bits(got[1]["steps"], want[1]["steps"]) is None and int(want[1]["steps"].max()) == STEPS - 2      # the schedule's place
    assert bits(got[1]["lr"], want[1]["lr"]) is None
    assert got[1]["ema_updates"] == STEPS - 2
    _assert_equal_runs(got, want)


# ---- 4: saving perturbs nothing ----------------------------------------------------------------------------------------------------
def test_saving_after_every_step_perturbs_nothing():
    want = _straight("bertadam", True)
    torch.manual_seed(20240607)
    run = Run("bertadam", True)
    losses = []
    for i in range(STEPS):
        losses.append(run.take(i))
        gen, captured_at = run.m._mb_gen, run.step.generation
        state = run.capture(i + 1)
        assert run.m._mb_gen == gen == captured_at and run.step.generation == captured_at        # no re-capture follows
        assert state["bank"]["head"] == int(run.m._mb_head_dev.item())
    _assert_equal_runs((losses, run.snapshot()), want)
    assert run.m._mb_gen == want[2]


# ---- 5: adamw, the host guard, a stand-alone EMA -------------------------------------------------------------------------------------
def test_adamw_with_the_host_guard_resumes_bit_for_bit(tmp_path):
    blanks = (2,)
    want = _straight("adamw", False, blanks)
    assert want[1]["host_skips"]["skipped"] == 1 and want[1]["ema_updates"] == STEPS - 1
    _assert_equal_runs(_cut("adamw", False, tmp_path, blanks), want)


# ---- 6: the loss-only step after a bank restore ------------------------------------------------------------------------------------
def test_loss_only_step_after_a_bank_restore(tmp_path):
    """no_grad steps keep the bank's prepared bf16 shadow in step with the ring incrementally; a restore drops it and the next
    step rebuilds it from the fp32 ring.  Both give the same losses, bit for bit: the shadow need not be in the state."""
    def steps(m, lo, hi):
        with torch.no_grad():
            return [torch.stack([l.float() for l in m(*_batch(i), 0)]).cpu() for i in range(lo, hi)]
    torch.manual_seed(20240607)
    never_saved = _model(7)
    _load_bank(never_saved)
    want = steps(never_saved, 0, 5)
    assert never_saved._mb_shadow is not None                 # kept incrementally

    saved = _model(7)
    _load_bank(saved)
    steps(saved, 0, 4)
    state = checkpoint.capture_state(saved, torch.optim.SGD(saved.parameters(), lr=0.0), position=dict(epoch=0, next_step=4, global_step=4))
    path = str(tmp_path / "training_state.pt")
    checkpoint.save(path, state)
    fresh = _model(8)
    checkpoint.restore_state(checkpoint.load(path), fresh, torch.optim.SGD(fresh.parameters(), lr=0.0))
    assert fresh._mb_shadow is None
    got = steps(fresh, 4, 5)[0]
    assert fresh._mb_shadow is not None                       # rebuilt from the fp32 ring
    assert bits(got, want[4]) is None, (got.tolist(), want[4].tolist())
    for a, b in zip(fresh._mb_shadow, never_saved._mb_shadow):
        assert torch.equal(a.hi, b.hi) and torch.equal(a.lo, b.lo) and torch.equal(a.norm, b.norm)


# ---- 7, 8: fresh processes, the user's route -----------------------------------------------------------------------------------------
ENTRY = ["--do_train", "1", "--synthetic", "--batch_size", "32", "--synthetic_train", "192", "--mb_batch", "2", "--synthetic_test", "64",
         "--epochs", "2", "--hip_graph", "1", "--optimizer", "bertadam", "--skip_nonfinite", "1", "--ema_decay", "0.99"]
DIGEST = re.compile(r"^rank (\d+) epoch (\d+) training state sha256 ([0-9a-f]{16})$", flags=re.M)
RK = re.compile(r"text->video R@1 .*$")


def _entry(launch, out_dir, *extra, ok=True):
    cmd = launch + [os.path.join(ROOT, "main_retrieval.py")] + ENTRY + ["--output_dir", str(out_dir)] + list(extra)
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, capture_output=True, text=True, timeout=330, cwd=ROOT)
    assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _final(out, ranks):
    """The last digest of every rank and the last raw and EMA evaluation lines."""
    seen = {}
    for rank, epoch, hexd in DIGEST.findall(out):
        seen[int(rank)] = (int(epoch), hexd)
    assert sorted(seen) == list(range(ranks)), out[-3000:]
    raw = [RK.search(l).group(0) for l in out.splitlines() if "text->video R@1" in l and " EMA " not in l]
    avg = [RK.search(l).group(0) for l in out.splitlines() if " EMA text->video R@1" in l]
    return seen, raw[-1], avg[-1]


def _straight_cut_resumed(launch, tmp_path, ranks, common=()):
    a = _entry(launch(0), tmp_path / "a", "--resume", "auto", *common)              # straight; nothing to resume from, the flag prints the digests
    assert "--resume auto: no " in a.stdout and not os.path.exists(tmp_path / "a" / "training_state.pt")
    b = _entry(launch(1), tmp_path / "b", "--save_state_every", "2", "--max_steps", "9", *common)
    assert "--max_steps 9: stopped after global step 9" in b.stdout and os.path.exists(tmp_path / "b" / "training_state.pt")
    c = _entry(launch(2), tmp_path / "b", "--resume", "auto", *common)
    assert "resumed at epoch 2, step 4 (global step 9)" in c.stdout, c.stdout[-3000:]
    assert "memory bank:" not in c.stdout                               # the saved bank, no load_memory_bank inside the epoch
    want, got, cut = _final(a.stdout, ranks), _final(c.stdout, ranks), _final(b.stdout, ranks)
    assert all(v[0] == 2 for v in want[0].values())
    assert got[0] == want[0], (got[0], want[0])                         # every rank's final digest
    assert got[1:] == want[1:], (got[1:], want[1:])                     # the final evaluation lines, raw and EMA
    assert cut[0] != want[0]
    assert len(set(v[1] for v in want[0].values())) == 1                # the ranks agree
    return a, b, c


def test_fresh_processes_resume_the_straight_run(tmp_path):
    _straight_cut_resumed(lambda n: [sys.executable], tmp_path, 1)
    d = _entry([sys.executable], tmp_path / "b", "--resume", "auto", "--batch_size", "64", ok=False)
    assert "batch_size: saved 32, this run 64" in d.stderr, d.stderr[-2000:]


def test_two_ranks_resume_the_straight_run(tmp_path):
    def launch(n):
        return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(29671 + n)]
    _straight_cut_resumed(launch, tmp_path, 2, common=("--dist_backend", "gloo"))
