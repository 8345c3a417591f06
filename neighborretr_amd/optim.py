"""BertAdam and prep_optimizer with the reference's interfaces (models/optimization.py:76-211, training/optimizer.py:12-86),
the update itself done by the multi-tensor HIP kernels of csrc/nr_optim.hip (DESIGN.md "BertAdam in the captured step").

What a step computes, in this order (trainer.py:104-119 around BertAdam.step):

  1. optional global clip (`global_max_norm`, the trainer's 1.0):  c = min(1, global_max_norm / (sqrt(sum_t ||g_t||^2) + 1e-6));
  2. per tensor, if the group's max_grad_norm > 0:                 c_t = min(1, max_grad_norm / (c ||g_t|| + 1e-6));
     the gradient that enters the moments is g c c_t -- the gradient tensors themselves are never written;
  3. m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  u = m / (sqrt(v) + e) (+ weight_decay * p when > 0); no bias correction;
  4. lr_t = lr * schedule(step / t_total, warmup) with the tensor's step counter BEFORE this step (lr when t_total == -1);
  5. p -= lr_t u;  p = min(p, clamp_max[p]) where given (`clip.logit_scale`: ln 100);  step += 1.

`step()` issues three launches on the current stream and nothing else -- no `.item()`, no device synchronisation, no allocation
once the moments exist (the one host wait it can take: a table upload finding all four staging buffers still unread by the device)
-- so it can be captured into a HIP graph; the step counters and the schedule live on the device.  The table of
pointers the kernels read is uploaded again only when one of its pointers (or a group's hyper-parameter) has changed.  There is
no CPU or eager path behind it: parameters that are not on the GPU raise.

`skip_nonfinite=True` takes the same three launches through nr_bertadam_step_guarded: a step whose sum of squared
gradients is not finite -- a NaN, an infinity, or an entry whose square overflows fp32 -- changes no parameter, no moment and no
step counter, decided on the device, so it works inside a replayed graph too.  The host cannot know the outcome without a
synchronisation: its step mirror keeps counting every step and is corrected from the device counters (one small blocking copy)
whenever something reads it -- get_lr(), group_lr(), state_dict(), guard_stats(), records().

`WeightEma` keeps an exponential moving average of the weights in fp32 shadows with its decay, warm-up and
count of updates in a device-resident state.  It has two drivers, one per average: attached to a BertAdam (`ema=`), launch C of
the step averages every tensor it updates, under the guard and inside a captured step included; on its own, `update()` averages
every tensor in two launches.  A tensor that never receives a gradient equals its shadow either way.
"""
import contextlib
import ctypes
import math

import numpy as np
import torch
from torch.optim import Optimizer

from . import hip, ops


# What a schedule returns once the warm-up ramp (x / warmup while x < warmup) is over; x = step / t_total.
_PAST_WARMUP = {
    "warmup_cosine": lambda x, warmup: (1.0 + math.cos(math.pi * x)) / 2.0,
    "warmup_constant": lambda x, warmup: 1.0,
    "warmup_linear": lambda x, warmup: max((x - 1.0) / (warmup - 1.0), 0.0),
}


def _make_schedule(name):
    past = _PAST_WARMUP[name]

    def schedule(x, warmup=0.002):
        return x / warmup if x < warmup else past(x, warmup)
    schedule.__name__ = schedule.__qualname__ = name
    schedule.__doc__ = f"Learning-rate multiplier of `{name}` at x = step / t_total (DESIGN.md 6.3)."
    return schedule


SCHEDULES = {name: _make_schedule(name) for name in _PAST_WARMUP}
warmup_cosine, warmup_constant, warmup_linear = (SCHEDULES[k] for k in ("warmup_cosine", "warmup_constant", "warmup_linear"))
_REQUIRED = object()
_RING = 4                     # pinned staging buffers of the eager path (a buffer is reused only after its copy has completed)
_ENTRY = ctypes.sizeof(hip.OptimTensor)
_GROUP = ctypes.sizeof(hip.OptimGroup)
# one row of records(): NrStepRecord of include/nr_hip.h, field by field
RECORD_DTYPE = np.dtype([("attempt", "<i8"), ("grad_norm", "<f4"), ("clip", "<f4"), ("skipped", "<i4"), ("n_losses", "<i4"),
                         ("losses", "<f4", (hip.GUARD_MAX_LOSSES,))])
assert RECORD_DTYPE.itemsize == ctypes.sizeof(hip.StepRecord)
_GUARD_FIELDS = ("attempts", "skipped", "consecutive", "max_consecutive", "last_skipped")


def ema_decay_at(decay, warmup, n):
    """The decay update number n (0-based) uses: min(decay, (1 + n) / (10 + n)) under warm-up, else decay."""
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


class WeightEma:
    """Exponential moving average of parameters: e += (1 - d) (p - e) after every update, d = ema_decay_at(decay, warmup, n)
    with n the updates so far (counted on the device: a step the non-finite guard skipped is no update).

    params: an iterable of parameters or of (name, parameter) pairs as from named_parameters().  Every parameter gets one
    contiguous fp32 shadow, a copy of it at construction.  The kernels are HIP: parameters that are not on the GPU, not fp32 or
    not contiguous raise NrHipError.

    Attached to a BertAdam (BertAdam(..., ema=this)) a tensor is averaged in the steps that update it; stand-alone every tensor
    is averaged on every update()."""

    def __init__(self, params, decay=0.999, warmup=True):
        for name, value, ok, wanted in (("decay", decay, lambda x: isinstance(x, (int, float)) and 0.0 <= x < 1.0, "in [0, 1)"),
                                        ("warmup", warmup, lambda x: isinstance(x, (bool, int)) and x in (0, 1),
                                         "False / True (or 0 / 1)")):
            if not ok(value):
                raise ValueError(f"WeightEma: {name} = {value!r} is not accepted, it must be {wanted}")
        items = list(params)
        if items and isinstance(items[0], (tuple, list)):
            self.names, self.params = [str(n) for n, _ in items], [p for _, p in items]
        else:
            self.names, self.params = list(range(len(items))), items
        if not self.params:
            raise ValueError("WeightEma has no parameters")
        if len({id(p) for p in self.params}) != len(self.params) or len(set(self.names)) != len(self.names):
            raise ValueError("WeightEma: a parameter or a name is given twice")
        for p in self.params:
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"WeightEma takes parameters or (name, parameter) pairs, got {type(p).__name__}")
            if not p.is_cuda:
                raise hip.NrHipError(f"WeightEma: a parameter of shape {tuple(p.shape)} lives on '{p.device}', not on a GPU; the "
                                     "average runs in HIP kernels and has no CPU fallback")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise hip.NrHipError(f"WeightEma: parameters must be contiguous float32 tensors, got {p.dtype} "
                                     f"{'contiguous' if p.is_contiguous() else 'non-contiguous'} of shape {tuple(p.shape)}")
        self.device = self.params[0].device
        if any(p.device != self.device for p in self.params):
            raise hip.NrHipError("WeightEma: all parameters must live on one device")
        hip.lib()
        self.decay, self.warmup = float(decay), bool(warmup)
        with torch.no_grad():
            self.shadows = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        self._shadow_of = {id(p): e for p, e in zip(self.params, self.shadows)}
        self._state = torch.zeros(ctypes.sizeof(hip.EmaState), dtype=torch.uint8, device=self.device)
        self._table = torch.empty(len(self.params) * ctypes.sizeof(hip.EmaTensor), dtype=torch.uint8, device=self.device)
        self._key = None
        self._driver = None       # the BertAdam this average is attached to
        self._applied = False
        self._write_state(0)
        self._upload()

    # ---- internals ----------------------------------------------------------------------------------------------------------
    def _write_state(self, updates):
        state = hip.EmaState(decay=self.decay, updates=int(updates), warmup=int(self.warmup), omd=0.0)
        if updates > 0:
            state.omd = 1.0 - ema_decay_at(self.decay, self.warmup, updates - 1)
        self._state.copy_(torch.frombuffer(bytearray(bytes(state)), dtype=torch.uint8))

    def _read_state(self):
        return hip.EmaState.from_buffer_copy(self._state.cpu().numpy().tobytes())

    def _upload(self):
        """The (parameter, shadow) table on the device, checked by nr_ema_plan; again only when a parameter has moved."""
        key = tuple(p.data_ptr() for p in self.params)
        if key == self._key:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightEma: a parameter's storage has moved since the table was uploaded; call update() or swap() "
                               "once outside the graph capture first")
        entries = (hip.EmaTensor * len(self.params))()
        for ent, p, e in zip(entries, self.params, self.shadows):
            ent.p, ent.ema, ent.n = p.data_ptr(), e.data_ptr(), p.numel()
        self._n_chunks = ops.ema_plan(entries, hip.EmaState(decay=self.decay, updates=0, warmup=int(self.warmup)))
        self._table.copy_(torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8))
        self._key = key

    def shadow(self, p):
        """The shadow of parameter p, None when p is not averaged."""
        return self._shadow_of.get(id(p))

    # ---- the interface --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self):
        """The stand-alone form: every shadow takes one update, two launches on the current stream, no allocation: capturable."""
        if self._driver is not None:
            raise RuntimeError("WeightEma.update(): this average is attached to an optimizer, whose step updates it -- there is "
                               "one driver per average")
        if self._applied:
            raise RuntimeError("WeightEma.update() inside applied(): the parameters hold the average now")
        self._upload()
        ops.ema_update(self._table, len(self.params), self._n_chunks, self._state)

    @torch.no_grad()
    def swap(self):
        """Exchanges the contents of parameters and shadows in place (a captured step has the addresses baked in) and moves the
        parameters' version counters: modeling.scorer_weights / cluster_fused.build_stage_weights key their bf16 splits on
        them and would serve the splits of the other weights otherwise."""
        self._upload()
        ops.ema_swap(self._table, len(self.params), self._n_chunks)
        torch.autograd.graph.increment_version(self.params)

    @contextlib.contextmanager
    def applied(self):
        """with ema.applied(): the parameters hold the average (evaluate here); swapped back on exit, also when the body raises."""
        if self._applied:
            raise RuntimeError("WeightEma.applied() does not nest")
        self.swap()
        self._applied = True
        try:
            yield self
        finally:
            self._applied = False
            self.swap()

    def updates(self):
        """The number of updates so far, from the device (a blocking copy)."""
        return int(self._read_state().updates)

    def last_decay(self):
        """The decay the last update used (None before the first), from the device's count (a blocking copy)."""
        n = self.updates()
        return ema_decay_at(self.decay, self.warmup, n - 1) if n > 0 else None

    def state_dict(self):
        return dict(decay=self.decay, warmup=self.warmup, updates=self.updates(),
                    shadows={name: e.detach().clone() for name, e in zip(self.names, self.shadows)})

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Values go into the existing shadows and device state: a captured step holds their addresses."""
        shadows = state_dict["shadows"]
        if set(shadows) != set(self.names):
            raise KeyError(f"WeightEma.load_state_dict: the shadows' names differ: {sorted(map(str, set(shadows) ^ set(self.names)))[:8]}")
        decay, warmup, updates = float(state_dict["decay"]), state_dict["warmup"], int(state_dict["updates"])
        if not 0.0 <= decay < 1.0 or warmup not in (0, 1) or updates < 0:
            raise ValueError("WeightEma.load_state_dict: decay must lie in [0, 1), warmup be False / True and updates be >= 0")
        for name, e in zip(self.names, self.shadows):
            src = shadows[name]
            if tuple(src.shape) != tuple(e.shape):
                raise ValueError(f"WeightEma.load_state_dict: shadow {name!r} has shape {tuple(src.shape)}, not {tuple(e.shape)}")
            e.copy_(src)
        self.decay, self.warmup = decay, bool(warmup)
        self._write_state(updates)

    def model_state_dict(self, model):
        """model.state_dict() with every averaged parameter replaced by a clone of its shadow; buffers and the parameters the
        average does not know stay as the model has them.  The keys are the model's: --init_model loads it unchanged."""
        sd = model.state_dict()
        for name, p in model.named_parameters():
            e = self._shadow_of.get(id(p))
            if e is not None and name in sd:
                sd[name] = e.detach().clone()
        return sd

    def sha256(self):
        """Digest over the shadows' bytes in order (a blocking copy): ranks that agree print the same one."""
        import hashlib
        digest = hashlib.sha256()
        for e in self.shadows:
            digest.update(e.detach().cpu().numpy().tobytes())
        return digest.hexdigest()


class BertAdam(Optimizer):
    """Adam without bias correction, with decoupled weight decay, a per-tensor gradient clip and a built-in warm-up schedule.

    The reference's constructor and argument checks, plus
      global_max_norm  None / <= 0: off; else the trainer's clip_grad_norm_(parameters, global_max_norm) fused into the step;
      clamp_max        {parameter: upper bound} applied after the update (the trainer's logit-scale clamp);
      skip_nonfinite   True: a step whose gradients are not all finite is skipped on the device (module docstring);
      record_ring      with skip_nonfinite, the number of per-step records kept for records(): a power of two in [1, 4096];
      ema              a WeightEma: launch C averages every tensor it updates into its shadow (nr_bertadam_step_ema), guarded
                       or not; a parameter the average does not know is left out.  The optimizer is then the average's driver.
    `state[p] = {'step', 'next_m', 'next_v'}` as in the reference, so state dicts move between the two implementations; 'step'
    is the host's mirror of the device counter."""

    def __init__(self, params, lr=_REQUIRED, warmup=-1, t_total=-1, schedule="warmup_linear", b1=0.9, b2=0.999, e=1e-6,
                 weight_decay=0.01, max_grad_norm=1.0, global_max_norm=None, clamp_max=None, skip_nonfinite=False, record_ring=256,
                 ema=None):
        if lr is _REQUIRED:
            raise ValueError("BertAdam needs a learning rate")
        unit = lambda x: 0.0 <= x < 1.0                                           # noqa: E731
        for name, value, ok, wanted in (("lr", lr, lambda x: x >= 0.0, "a number >= 0"),
                                        ("schedule", schedule, lambda x: x in SCHEDULES, "one of " + ", ".join(SCHEDULES)),
                                        ("warmup", warmup, lambda x: x == -1 or unit(x), "-1 (none) or a fraction in [0, 1)"),
                                        ("b1", b1, unit, "in [0, 1)"), ("b2", b2, unit, "in [0, 1)"),
                                        ("e", e, lambda x: x >= 0.0, "a number >= 0"),
                                        ("global_max_norm", global_max_norm, lambda x: x is None or float(x) == float(x),
                                         "None or a number"),
                                        ("skip_nonfinite", skip_nonfinite, lambda x: isinstance(x, (bool, int)) and x in (0, 1),
                                         "False / True (or 0 / 1)"),
                                        ("record_ring", record_ring,
                                         lambda x: isinstance(x, int) and not isinstance(x, bool) and 1 <= x <= hip.GUARD_MAX_RING
                                         and x & (x - 1) == 0, f"a power of two in [1, {hip.GUARD_MAX_RING}]")):
            if not ok(value):
                raise ValueError(f"BertAdam: {name} = {value!r} is not accepted, it must be {wanted}")
        if ema is not None:
            if not isinstance(ema, WeightEma):
                raise TypeError(f"BertAdam: ema takes a WeightEma, got {type(ema).__name__}")
            if ema._driver is not None:
                raise ValueError("BertAdam: this WeightEma is attached to another optimizer already")
        defaults = dict(lr=lr, schedule=schedule, warmup=warmup, t_total=t_total, b1=b1, b2=b2, e=e, weight_decay=weight_decay,
                        max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        self.global_max_norm = None if global_max_norm is None else float(global_max_norm)
        self.clamp_max = {}
        known = {id(p) for g in self.param_groups for p in g["params"]}
        for p, bound in (clamp_max or {}).items():
            if id(p) not in known:
                raise ValueError("clamp_max names a tensor that is not one of the optimizer's parameters")
            self.clamp_max[id(p)] = float(bound)
        self.skip_nonfinite, self.record_ring = bool(skip_nonfinite), int(record_ring)
        self.ema = ema
        if ema is not None:
            ema._driver = self
        self._watched = None      # watch_losses(): the device tensor whose values go into every step's record
        self._dirty = False       # skip_nonfinite: the step mirror has counted steps the device may have skipped
        self._dev = None          # device-side state: created by the first step() / prepare()
        self._key = None          # what the device table currently holds
        self._held = {}           # tables of captured steps, per owner: alive (and untouched) as long as that capture is in use

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def get_lr(self):
        """The scheduled learning rate of every parameter that has a gradient, from the host's mirror of the step counters
        ([0] before the first step, as in the reference)."""
        self._sync_steps()
        live = [(group, self.state[p]) for group in self.param_groups for p in group["params"] if p.grad is not None]
        if any(len(state) == 0 for _, state in live):
            return [0]
        return [_scheduled(group, state["step"]) for group, state in live]

    def group_lr(self, applied=False):
        """One scheduled learning rate per parameter group, read at its most advanced tensor: the rate the NEXT step will use
        (what get_lr() reports), or with `applied=True` the rate the last step used (0 steps: the first step's)."""
        self._sync_steps()
        out = []
        for group in self.param_groups:
            steps = [self.state[p]["step"] for p in group["params"] if len(self.state[p])]
            step = max(steps) if steps else 0
            out.append(_scheduled(group, max(step - 1, 0) if applied else step))
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.advance(self.issue())
        return loss

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    # ---- the non-finite guard (skip_nonfinite=True) ----------------------------------------------------------------------
    def watch_losses(self, losses):
        """Registers a float32 device tensor of at most 8 values (None: none) whose contents every later issue() / step() copies
        into its step's record WHEN THE LAUNCHES EXECUTE: the address is baked into the launch, so inside a graph capture pass
        a tensor of the capture (static across replays).  The optimizer keeps the tensor alive."""
        self._need_guard("watch_losses")
        if losses is not None:
            if not (isinstance(losses, torch.Tensor) and losses.is_cuda and losses.dtype == torch.float32 and losses.is_contiguous()
                    and losses.numel() <= hip.GUARD_MAX_LOSSES):
                raise ValueError(f"watch_losses takes a contiguous float32 device tensor of at most {hip.GUARD_MAX_LOSSES} values")
        self._watched = losses

    def guard_stats(self):
        """{attempts, skipped, consecutive, max_consecutive, last_skipped} as the device holds them now (a blocking copy)."""
        self._need_guard("guard_stats")
        self._sync_steps()
        guard = hip.StepGuard.from_buffer_copy(self._device_state()["guard"].cpu().numpy().tobytes())
        return {k: int(getattr(guard, k)) for k in _GUARD_FIELDS}

    def records(self, last=None):
        """The per-step records still in the ring, oldest first, as a NumPy structured array (RECORD_DTYPE): min(attempts,
        record_ring) rows, every attempt index once; `last`: only the newest `last` of them.  A blocking copy."""
        self._need_guard("records")
        attempts = self.guard_stats()["attempts"]
        ring = np.frombuffer(self._dev["ring_records"].cpu().numpy().tobytes(), dtype=RECORD_DTYPE)
        n = min(attempts, self.record_ring)
        if last is not None:
            n = min(n, max(int(last), 0))
        rows = ring[[a & (self.record_ring - 1) for a in range(attempts - n, attempts)]] if n else ring[:0]
        return rows.copy()

    def guard_state_dict(self):
        """The guard as the device holds it now, raw: {guard: the 48 bytes of NrStepGuard, records: the record ring's bytes,
        record_ring} with uint8 host tensors (a blocking copy).  state_dict() does not carry them."""
        self._need_guard("guard_state_dict")
        dev = self._device_state()
        return dict(guard=dev["guard"].cpu(), records=dev["ring_records"].cpu(), record_ring=self.record_ring)

    @torch.no_grad()
    def load_guard_state_dict(self, state_dict):
        """guard_state_dict()'s value into the existing device guard and record ring (a captured step holds their addresses).
        The only call that sets them: load_state_dict() leaves them alone."""
        self._need_guard("load_guard_state_dict")
        dev = self._device_state()
        guard, records = state_dict["guard"], state_dict["records"]
        if int(state_dict["record_ring"]) != self.record_ring:
            raise ValueError(f"BertAdam.load_guard_state_dict: the records come from a ring of {state_dict['record_ring']}, this "
                             f"optimizer's has {self.record_ring}")
        for name, src, dst in (("guard", guard, dev["guard"]), ("records", records, dev["ring_records"])):
            if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.numel() != dst.numel():
                raise ValueError(f"BertAdam.load_guard_state_dict: {name} must be a uint8 tensor of {dst.numel()} bytes")
        dev["guard"].copy_(guard.reshape(-1))
        dev["ring_records"].copy_(records.reshape(-1))

    def _need_guard(self, what):
        if not self.skip_nonfinite:
            raise RuntimeError(f"BertAdam.{what}() belongs to the non-finite guard: build the optimizer with skip_nonfinite=True")

    def _sync_steps(self):
        """skip_nonfinite: the device counters are the truth (a skipped step does not move them) -> the host's mirror."""
        if not self._dirty or self._dev is None:
            return
        steps = self._dev["steps"].cpu().tolist()
        for i, p in enumerate(self._all):
            if len(self.state[p]):
                self.state[p]["step"] = int(steps[i])
        self._dirty = False

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Moments that already exist keep their storage and take the loaded values (a captured step has their addresses in its
        table); the device counters are set from the loaded step counts.  The guard's counters and records are left alone."""
        mine = {p: (st["next_m"], st["next_v"]) for p, st in self.state.items() if "next_m" in st}
        super().load_state_dict(state_dict)
        for p, (m, v) in mine.items():
            st = self.state[p]
            if "next_m" in st and st["next_m"].shape == m.shape and st["next_v"].shape == v.shape:
                m.copy_(st["next_m"])
                v.copy_(st["next_v"])
            else:                                    # the loaded state has nothing for this tensor: it starts over
                m.zero_()
                v.zero_()
                st.setdefault("step", 0)
            st["next_m"], st["next_v"] = m, v
        self._key = None
        self._dirty = False                          # the loaded counts are the mirror now, and the device's below
        if self._dev is not None:
            self._upload_steps()

    # ---- the two halves of step(), for a caller that captures the launches into a graph ----------------------------------
    @torch.no_grad()
    def prepare(self, params=None, owner=None):
        """Ahead of ONE graph capture of issue(): allocates the moments (for `params`, default: every parameter), the counters,
        the workspace, and the pair of buffers -- pinned host, device -- the captured table copy will use.  Nothing is
        allocated inside the capture.  `owner`: whoever holds the graph; the pair of its previous capture, which that graph
        replaces, is dropped (a step that is re-captured every epoch keeps one pair, not one per epoch)."""
        dev = self._device_state()
        for p in (params if params is not None else self._all):
            self._moments(p)
        if owner is not None:
            self._held.pop(id(owner), None)
        dev["spare"] = (owner, torch.empty(dev["bytes"], dtype=torch.uint8, pin_memory=True),
                        torch.empty(dev["bytes"], dtype=torch.uint8, device=dev["device"]))

    @torch.no_grad()
    def issue(self):
        """The three launches for the parameters that have a gradient now -> those parameters.  Host state (the step mirror,
        the tensors' version counters) is NOT touched: advance() does that, once per execution of the launches."""
        dev = self._device_state()
        live = [p for p in self._all if p.grad is not None]
        if not live:
            return live
        capturing = torch.cuda.is_current_stream_capturing()
        key = self._table_key(live)
        if capturing or key != self._key:
            if capturing and (dev["spare"] is None or any(len(self.state[p]) == 0 for p in live)):
                raise RuntimeError("BertAdam.issue() inside a graph capture: call prepare() before the capture begins (moments "
                                   "and the table's buffers must not be allocated inside it)")
            table, n_chunks = self._build(live)
            if capturing:
                # the copy below becomes a memcpy node that reads the pinned buffer on every replay: both buffers belong to
                # this capture alone and stay alive, untouched, as long as the optimizer
                owner, pinned, buf = dev["spare"]
                dev["spare"] = None
                self._held[id(owner) if owner is not None else id(pinned)] = (pinned, buf)
            else:
                slot = dev["ring"][dev["next"]]
                dev["next"] = (dev["next"] + 1) % _RING
                pinned, event = slot
                # the copy that last read this buffer: done long ago as a rule; a host wait only when the host has run _RING
                # table uploads ahead of the device
                event.synchronize()
                buf = dev["table"]
            ctypes.memmove(pinned.data_ptr(), table, len(table))
            buf.copy_(pinned, non_blocking=True)
            if capturing:
                launch = (buf, len(live), n_chunks)
            else:
                event.record()
                self._key, dev["launch"] = key, (buf, len(live), n_chunks)
                launch = dev["launch"]
        else:
            launch = dev["launch"]
        buf, T, n_chunks = launch
        if self.ema is not None:
            guarded = self.skip_nonfinite
            ops.bertadam_step_ema(buf, len(self.param_groups), buf, T, n_chunks, dev["workspace"], buf, self.ema._state,
                                  guard=dev["guard"] if guarded else None, ring=dev["ring_records"] if guarded else None,
                                  global_max_norm=self.global_max_norm, table_offset=dev["table_off"],
                                  shadows_offset=dev["ema_off"], losses=self._watched if guarded else None)
        elif self.skip_nonfinite:
            ops.bertadam_step_guarded(buf, len(self.param_groups), buf, T, n_chunks, dev["workspace"], dev["guard"],
                                      dev["ring_records"], self.global_max_norm, table_offset=dev["table_off"],
                                      losses=self._watched)
        else:
            ops.bertadam_step(buf, len(self.param_groups), buf, T, n_chunks, dev["workspace"], self.global_max_norm,
                              table_offset=dev["table_off"])
        return live

    def advance(self, live):
        """After one execution of issue()'s launches: the parameters have changed outside autograd, so their version counters
        move (modeling.scorer_weights / cluster_fused.build_stage_weights key their bf16 splits on them), and so does the
        host's mirror of the step counters.  With skip_nonfinite the device may have skipped the step: the mirror counts it
        all the same (finding out would synchronise) and is marked for correction at the next read; the version bump of a
        skipped step only makes the derived weights be re-derived, equal."""
        if not live:
            return
        torch.autograd.graph.increment_version(live)
        for p in live:
            self.state[p]["step"] += 1
        self._dirty = self.skip_nonfinite

    # ---- internals ----------------------------------------------------------------------------------------------------------
    def _device_state(self):
        if self._dev is not None:
            return self._dev
        self._all = [p for g in self.param_groups for p in g["params"]]
        if not self._all:
            raise ValueError("BertAdam has no parameters")
        for p in self._all:
            if not p.is_cuda:
                raise hip.NrHipError(f"BertAdam: a parameter of shape {tuple(p.shape)} lives on '{p.device}', not on a GPU; the "
                                     "update runs in HIP kernels and has no CPU fallback (move the model to the device before "
                                     "building the optimizer)")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise hip.NrHipError(f"BertAdam: parameters must be contiguous float32 tensors, got {p.dtype} "
                                     f"{'contiguous' if p.is_contiguous() else 'non-contiguous'} of shape {tuple(p.shape)}")
        device = self._all[0].device
        if any(p.device != device for p in self._all):
            raise hip.NrHipError("BertAdam: all parameters must live on one device")
        if self.ema is not None and self.ema.device != device:
            raise hip.NrHipError("BertAdam: the WeightEma lives on another device than the parameters")
        hip.lib()
        N, G = len(self._all), len(self.param_groups)
        self._index = {id(p): i for i, p in enumerate(self._all)}
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        table_off = (G * _GROUP + 63) // 64 * 64
        nbytes = table_off + N * _ENTRY
        ema_off = 0
        if self.ema is not None:                                   # third section: one shadow pointer per table entry
            ema_off = (nbytes + 63) // 64 * 64
            nbytes = ema_off + N * 8
        max_chunks = sum((p.numel() + 4095) // 4096 for p in self._all)
        ws = ops.bertadam_workspace_bytes(N, max_chunks)
        with torch.cuda.device(device):
            self._dev = dict(
                device=device, bytes=nbytes, table_off=table_off, ema_off=ema_off,
                steps=torch.zeros(N, dtype=torch.int32, device=device),
                table=torch.empty(nbytes, dtype=torch.uint8, device=device),
                workspace=torch.empty(max(ws, 256), dtype=torch.uint8, device=device),
                ring=[(torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()) for _ in range(_RING)],
                next=0, launch=None, spare=None)
            if self.skip_nonfinite:
                guard = hip.StepGuard(last_skipped=-1)
                self._dev["guard"] = torch.frombuffer(bytearray(bytes(guard)), dtype=torch.uint8).to(device)
                self._dev["ring_records"] = torch.zeros(self.record_ring * RECORD_DTYPE.itemsize, dtype=torch.uint8, device=device)
        self._upload_steps()
        return self._dev

    def _upload_steps(self):
        host = torch.tensor([int(self.state[p]["step"]) if len(self.state[p]) else 0 for p in self._all], dtype=torch.int32)
        self._dev["steps"].copy_(host)

    def _moments(self, p):
        state = self.state[p]
        if len(state) == 0:
            state["step"] = 0
            state["next_m"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state["next_v"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return state

    def _group_values(self):
        return tuple((float(g["lr"]), float(g["weight_decay"]), float(g["b1"]), float(g["b2"]), float(g["e"]),
                      float(g["max_grad_norm"]), float(g["warmup"]), int(g["t_total"]), g["schedule"])
                     for g in self.param_groups)

    def _table_key(self, live):
        shadows = None
        if self.ema is not None:
            shadows = tuple(0 if e is None else e.data_ptr() for e in map(self.ema.shadow, live))
        return (tuple((id(p), p.data_ptr(), p.grad.data_ptr()) for p in live), self._group_values(), self.global_max_norm, shadows)

    def _build(self, live):
        """Host image of [groups | table] for the tensors in `live`, checked and chunked by nr_bertadam_plan."""
        dev = self._dev
        G = len(self.param_groups)
        groups = (hip.OptimGroup * G)()
        for q, vals in zip(groups, self._group_values()):
            q.lr, q.weight_decay, q.b1, q.b2, q.e, q.max_grad_norm, q.warmup, q.t_total = vals[:8]
            if vals[8] not in hip.SCHEDULE_IDS:
                raise ValueError("Invalid schedule parameter: {}".format(vals[8]))
            q.schedule = hip.SCHEDULE_IDS[vals[8]]
        entries = (hip.OptimTensor * len(live))()
        steps = dev["steps"].data_ptr()
        for ent, p in zip(entries, live):
            g = p.grad
            if g.is_sparse:
                raise RuntimeError("BertAdam does not support sparse gradients")
            if g.device != p.device or g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != p.numel():
                raise hip.NrHipError(f"BertAdam: the gradient of a parameter of shape {tuple(p.shape)} must be a contiguous float32 "
                                     f"tensor of that size on {p.device} (got {g.dtype}, {tuple(g.shape)}, {g.device})")
            state = self._moments(p)
            m, v = state["next_m"], state["next_v"]
            if (m.device != p.device or v.device != p.device or m.dtype != torch.float32 or v.dtype != torch.float32
                    or not m.is_contiguous() or not v.is_contiguous() or m.numel() != p.numel() or v.numel() != p.numel()):
                raise hip.NrHipError("BertAdam: next_m / next_v must be contiguous float32 tensors of the parameter's size on its device")
            i = self._index[id(p)]
            ent.p, ent.g, ent.m, ent.v = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            ent.step = steps + 4 * i
            ent.n = p.numel()
            ent.group = self._group_of[i]
            bound = self.clamp_max.get(id(p))
            ent.has_clamp = int(bound is not None)
            ent.clamp_max = bound if bound is not None else 0.0
        n_chunks = ops.bertadam_plan(entries, groups)
        image = bytearray(dev["bytes"])
        image[:G * _GROUP] = bytes(groups)
        image[dev["table_off"]:dev["table_off"] + len(live) * _ENTRY] = bytes(entries)
        if self.ema is not None:
            shadows = (ctypes.c_uint64 * len(live))(*(0 if e is None else e.data_ptr() for e in map(self.ema.shadow, live)))
            image[dev["ema_off"]:dev["ema_off"] + 8 * len(live)] = bytes(shadows)
        return (ctypes.c_char * len(image)).from_buffer(image), n_chunks


def _scheduled(group, step):
    if group["t_total"] != -1:
        return group["lr"] * SCHEDULES[group["schedule"]](step / group["t_total"], group["warmup"])
    return group["lr"]


_UNDECAYED = ("bias", "LayerNorm.bias", "LayerNorm.weight")     # substrings of parameter names that take no weight decay


def _group_index(name):
    """0: CLIP, decayed; 1: head, decayed; 2: CLIP, no decay; 3: head, no decay (the order of the reference's four groups)."""
    return (0 if "clip." in name else 1) + (2 if any(mark in name for mark in _UNDECAYED) else 0)


def prep_optimizer(args, model, num_train_optimization_steps, local_rank, global_max_norm=None, clamp_logit_scale=False,
                   wrap=True, skip_nonfinite=False, ema=None):
    """training/optimizer.py:12-86 -> (optimizer, None, model).  Four groups: names with `clip.` train at lr * coef_lr, names
    containing `bias`, `LayerNorm.bias` or `LayerNorm.weight` take no weight decay; warmup_cosine over
    `num_train_optimization_steps`, b1 0.9, b2 0.98, e 1e-6, per-tensor max_grad_norm 1.0.

    By default the trainer's global clip and logit-scale clamp stay with the caller (training.train_epoch does both around
    step(), like the reference's trainer); `global_max_norm=1.0` / `clamp_logit_scale=True` move them into the step;
    `skip_nonfinite=True` builds the optimizer with the device-side non-finite guard (BertAdam); `ema`: a WeightEma the
    optimizer's step drives (BertAdam).  The model
    comes back wrapped in DistributedDataParallel when a process group is up (the reference wraps whenever CUDA is there, which
    needs one; `wrap=False`: never), else as it came."""
    if hasattr(model, "module"):
        model = model.module
    named = list(model.named_parameters())
    members = [[], [], [], []]
    for name, p in named:
        members[_group_index(name)].append(p)
    clip_lr = args.lr * args.coef_lr
    groups = [dict(params=members[0], weight_decay=args.weight_decay, lr=clip_lr),
              dict(params=members[1], weight_decay=args.weight_decay),
              dict(params=members[2], weight_decay=0.0, lr=clip_lr),
              dict(params=members[3], weight_decay=0.0)]
    clamp = {}
    if clamp_logit_scale:
        clamp = {p: math.log(100.0) for n, p in named if n.endswith("clip.logit_scale") or n == "logit_scale"}
        if not clamp:
            raise ValueError("clamp_logit_scale: the model has no clip.logit_scale parameter")
    optimizer = BertAdam(groups, lr=args.lr, warmup=args.warmup_proportion, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6,
                         t_total=num_train_optimization_steps, weight_decay=args.weight_decay, max_grad_norm=1.0,
                         global_max_norm=global_max_norm, clamp_max=clamp, skip_nonfinite=skip_nonfinite, ema=ema)
    import torch.distributed as dist
    if wrap and torch.cuda.is_available() and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local_rank], output_device=local_rank,
                                                          find_unused_parameters=True)
    return optimizer, None, model
