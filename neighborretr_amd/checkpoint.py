"""The whole training state as one value: what a run that was cut off needs to continue with the bits of the
run that was not.

    state = capture_state(model, optimizer, ema, position=..., config=...)     # device -> host copies, nothing is changed
    save(path, state)                                                          # path.tmp, fsync, os.replace
    state = load(path, config=...)                                             # CheckpointError on anything that does not fit
    position = restore_state(state, model, optimizer, ema)                     # values into the EXISTING storage

The dict holds tensors, ints, floats, strs, lists and dicts only (and None / bool where a torch optimizer's own state dict has
them), so the file loads with torch.load(..., weights_only=True).

    format, abi      FORMAT; hip.version()
    position         {epoch, next_step, global_step}: the step the run takes next (epoch and next_step count from 0)
    config           the arguments that fix the trajectory (config_from_args)
    model            model.state_dict()
    bank             the RAW ring: the five `_mb` tensors as they lie, the head, mb_batch -- never through the mb_* properties,
                     which roll the live bank into FIFO order (another summation order of the means over bank samples, a dropped
                     shadow, a re-capture in the run that only wanted to save)
    rng              the {seed, counter} words of the DPC-KNN noise stream, None when the stream was never used
    optimizer        kind; its state_dict(); BertAdam: guard_state_dict() (the device guard and its record ring as raw bytes);
                     any other optimizer: the host guard's counts
    ema              WeightEma.state_dict()
    host_rng         torch's CPU generator state and the current device's

Not in it: the bank's prepared bf16 shadow (dropped on restore, rebuilt lazily from the fp32 ring), the derived weight caches
(keyed on the parameters' version counters, which restore moves), graphs, data-loader state.
"""
import hashlib
import os

import torch

from . import hip

FORMAT = 1
LOSS_KEYS = ("centrality_scale", "kl_weight", "uniform_weight", "beta", "num_neighbors", "temperature", "neighbor_weight")
CONFIG_KEYS = ("batch_size", "world_size", "epochs", "lr", "coef_lr", "warmup_proportion", "weight_decay", "optimizer", "precision",
               "seed", "synthetic_train", "max_words", "max_frames", "mb_batch", "encoders", "skip_nonfinite", "ema_decay",
               "ema_warmup", "centrality_multi_token") + LOSS_KEYS
_TOP = ("format", "abi", "position", "config", "model", "bank", "rng", "optimizer", "ema", "host_rng")
_BANK = ("mb_ind", "mb_feat_t", "mb_feat_v", "mb_mask_t", "mb_mask_v")


class CheckpointError(RuntimeError):
    """A training-state file that cannot be used: unreadable, of another format or ABI, or of a run with other arguments."""


def config_from_args(args):
    """The arguments that fix the trajectory, as plain values (CONFIG_KEYS; an argument the caller does not have is left out)."""
    return {k: getattr(args, k) for k in CONFIG_KEYS if hasattr(args, k)}


def _host(t):
    return t.detach().to("cpu", copy=True).contiguous()


def _plain(v):
    """v with every tensor as a host copy and every tuple as a list."""
    if isinstance(v, torch.Tensor):
        return _host(v)
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def capture_state(model, optimizer, ema=None, position=None, config=None, host_guard=None):
    """The training state as host values.  Reads only: device-to-host copies on the current stream and one .item() for the ring
    head; the live bank, its shadow and `_mb_gen` stay as they are, so a captured step goes on replaying.

    position: {epoch, next_step, global_step}; config: config_from_args(args); host_guard: the counts of the host's form of the
    non-finite guard (main_retrieval's args._host_skips) when the optimizer is not a BertAdam."""
    from .optim import BertAdam
    model = _unwrap(model)
    if ema is not None and ema._applied:
        raise RuntimeError("capture_state inside WeightEma.applied(): the parameters hold the average and the shadows the weights")
    position = dict(position or {})
    state = dict(format=FORMAT, abi=int(hip.version()),
                 position={k: int(position.get(k, 0)) for k in ("epoch", "next_step", "global_step")},
                 config=_plain(dict(config or {})))
    state["model"] = {k: _host(v) for k, v in model.state_dict().items()}
    on_device = model._mb_head_dev is not None
    state["bank"] = dict(ring={k: _host(v) for k, v in model._mb.items()},          # (in the live dict's order)
                         head=int(model._mb_head_dev.item()) if on_device else int(model._mb_head),
                         head_on_device=int(on_device), mb_batch=int(model.mb_batch))
    state["rng"] = None if model._rng_state is None else _host(model._rng_state)
    if isinstance(optimizer, BertAdam):
        opt = dict(kind="bertadam", state=_plain(optimizer.state_dict()),
                   guard=optimizer.guard_state_dict() if optimizer.skip_nonfinite else None, host_guard=None)
    else:
        opt = dict(kind=type(optimizer).__name__.lower(), state=_plain(optimizer.state_dict()), guard=None,
                   host_guard=None if host_guard is None else _plain(dict(host_guard)))
    state["optimizer"] = opt
    state["ema"] = None if ema is None else _plain(ema.state_dict())
    host_rng = dict(cpu=torch.get_rng_state().clone(), device=None)
    device = next(model.parameters()).device
    if device.type == "cuda":
        host_rng["device"] = torch.cuda.get_rng_state(device).clone()
    state["host_rng"] = host_rng
    return state


@torch.no_grad()
def restore_state(state, model, optimizer, ema=None, host_guard=None):
    """Puts `state` back -> its position.  Values go into the storage that exists -- parameters (through copy_: their version
    counters move and the cached bf16 splits are re-derived), moments, step counters, guard, record ring, shadows, the EMA's
    device state, the noise stream's words -- because a captured step holds those addresses.  The bank is ASSIGNED (ring, head,
    mb_batch) and `_mb_gen` moves once: a step captured earlier re-captures, as after a bank loaded from outside.

    host_guard: the dict that takes the saved counts of the host's guard (main_retrieval's args._host_skips)."""
    from .optim import BertAdam
    model = _unwrap(model)
    kind = "bertadam" if isinstance(optimizer, BertAdam) else type(optimizer).__name__.lower()
    saved = state["optimizer"]
    if saved["kind"] != kind:
        raise CheckpointError(f"the state was saved from a {saved['kind']} optimizer, this run has a {kind}")
    if (state["ema"] is None) != (ema is None):
        raise CheckpointError("the state was saved " + ("without" if state["ema"] is None else "with") + " a weight EMA, this run has "
                              + ("one" if ema is not None else "none"))
    if ema is not None and ema._applied:
        raise RuntimeError("restore_state inside WeightEma.applied()")
    model.load_state_dict(state["model"], strict=True)
    device = next(model.parameters()).device
    # the bank: fresh tensors on the parameters' device (an empty bank stays the host's empty tensors), raw order kept
    bank = state["bank"]
    if set(bank["ring"]) != set(_BANK):
        raise CheckpointError(f"the state's bank has the tensors {sorted(bank['ring'])}, not {sorted(_BANK)}")
    model._mb = {k: (v.to(device, copy=True) if v.numel() else v.clone()) for k, v in bank["ring"].items()}
    if bank["head_on_device"] and device.type == "cuda":
        model._mb_head, model._mb_head_dev = 0, torch.tensor([int(bank["head"])], dtype=torch.int32, device=device)
    else:
        model._mb_head, model._mb_head_dev = int(bank["head"]), None
    model.mb_batch = int(bank["mb_batch"])
    model._mb_shadow, model._last_prepared, model._ring_advanced = None, {}, False
    model._mb_gen += 1
    if state["rng"] is None:
        model._rng_state = None
    else:
        model._rng_state_on(device).copy_(state["rng"])
    optimizer.load_state_dict(saved["state"])
    if kind == "bertadam":
        if (saved["guard"] is not None) != bool(optimizer.skip_nonfinite):
            raise CheckpointError("the state and this run differ in skip_nonfinite")
        if saved["guard"] is not None:
            optimizer.load_guard_state_dict(saved["guard"])
    elif saved["host_guard"] is not None and host_guard is not None:
        host_guard.clear()
        host_guard.update(_plain(saved["host_guard"]))
    if ema is not None:
        ema.load_state_dict(state["ema"])
    torch.set_rng_state(state["host_rng"]["cpu"])
    if state["host_rng"]["device"] is not None and device.type == "cuda":
        torch.cuda.set_rng_state(state["host_rng"]["device"], device)
    return dict(state["position"])


def volatile_words(model):
    """What a graph capture moves although no step is taken: its warm-up passes run the step prologue, which advances the
    counter of the DPC-KNN noise stream (the bank is frozen meanwhile, and the optimizer's prepare() only allocates what does
    not exist yet).  A run resumed inside an epoch captures where the uninterrupted run replays: it takes these words before
    the capture and puts them back after it (reapply_volatile)."""
    model = _unwrap(model)
    return dict(rng=None if model._rng_state is None else model._rng_state.clone())


@torch.no_grad()
def reapply_volatile(model, kept):
    """volatile_words()'s value back into the existing storage (the captured step holds the address)."""
    model = _unwrap(model)
    if kept["rng"] is not None:
        model._rng_state.copy_(kept["rng"])


def save(path, state):
    """Atomic: the file at `path` is the previous state or this one, never a part of either."""
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def load(path, config=None):
    """The state in the file at `path`.  CheckpointError: a file that cannot be read (missing, truncated, not a state), an
    unknown format, another ABI, or -- with `config`, the run's config_from_args -- a config that differs; the message lists
    every differing key with both values."""
    try:
        state = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as err:                         # whatever the unpickler makes of a damaged file
        raise CheckpointError(f"{path}: unreadable or truncated ({type(err).__name__}: {err})") from err
    if not isinstance(state, dict) or any(k not in state for k in _TOP):
        raise CheckpointError(f"{path}: not a training state (keys missing)")
    if state["format"] != FORMAT:
        raise CheckpointError(f"{path}: format {state['format']!r}, this build reads format {FORMAT}")
    if state["abi"] != int(hip.version()):
        raise CheckpointError(f"{path}: written under C ABI version {state['abi']!r}, this build has {int(hip.version())}")
    if config is not None:
        mine, theirs = _plain(dict(config)), state["config"]
        missing = object()
        differ = [(k, theirs.get(k, missing), mine.get(k, missing)) for k in sorted(set(mine) | set(theirs))
                  if theirs.get(k, missing) != mine.get(k, missing)]
        if differ:
            show = lambda v: "(absent)" if v is missing else repr(v)        # noqa: E731
            raise CheckpointError(f"{path}: the state belongs to a run with other arguments: "
                                  + ", ".join(f"{k}: saved {show(a)}, this run {show(b)}" for k, a, b in differ))
    return state


def digest(state):
    """sha256 (hex) over every tensor's bytes and every scalar of the state in a fixed key order, and the position; `format`,
    `abi` and `config` stay out."""
    h = hashlib.sha256()

    def walk(name, v):
        if isinstance(v, dict):
            for k in sorted(v, key=str):
                walk(f"{name}/{k}", v[k])
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{name}/{i}", x)
        elif isinstance(v, torch.Tensor):
            t = v.detach().cpu().contiguous()
            h.update(f"{name}:{t.dtype}:{tuple(t.shape)}:".encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        else:
            h.update(f"{name}={v!r};".encode())
    for key in _TOP:
        if key not in ("format", "abi", "config", "position"):
            walk(key, state[key])
    walk("position", state["position"])
    return h.hexdigest()
