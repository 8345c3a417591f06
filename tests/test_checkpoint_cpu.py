"""CPU: the training-state file (neighborretr_amd.checkpoint) -- round trip through save / load under
weights_only=True, the atomic write, every refusal of load(), the raw memory-bank ring of a CPU model, and the entry point's
flag errors.  All comparisons are bitwise."""
import os
import sys

import pytest
import torch

from neighborretr_amd import checkpoint, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    """Equal in structure, types and bits."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
                and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


CONFIG = dict(batch_size=32, world_size=1, epochs=2, lr=1e-4, coef_lr=1e-3, warmup_proportion=0.1, weight_decay=0.2,
              optimizer="bertadam", precision="bf16", seed=42, synthetic_train=192, max_words=24, max_frames=12, mb_batch=2,
              encoders=0, skip_nonfinite=1, ema_decay=0.99, ema_warmup=1, centrality_multi_token="raise", beta=0.7,
              num_neighbors=20, temperature=3.0)


def hand_made(seed=0, **over):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)          # noqa: E731
    nan = torch.tensor([float("nan"), float("inf"), -0.0, 1e-42])           # bits that == would not tell apart
    state = dict(
        format=checkpoint.FORMAT, abi=int(hip.version()), position=dict(epoch=1, next_step=3, global_step=9), config=dict(CONFIG),
        model={"a.weight": r(3, 4), "a.bias": nan, "clip.logit_scale": r(())},
        bank=dict(ring=dict(mb_ind=torch.arange(6), mb_feat_t=r(6, 2, 4), mb_feat_v=r(6, 3, 4), mb_mask_t=torch.ones(6, 2),
                            mb_mask_v=torch.ones(6, 3)), head=4, head_on_device=1, mb_batch=6),
        rng=torch.tensor([42, 27], dtype=torch.int64),
        optimizer=dict(kind="bertadam", state=dict(state={0: dict(step=9, next_m=r(3, 4), next_v=r(3, 4))},
                                                   param_groups=[dict(lr=1e-4, schedule="warmup_cosine", params=[0])]),
                       guard=dict(guard=torch.arange(48, dtype=torch.uint8), records=torch.zeros(96, dtype=torch.uint8), record_ring=2),
                       host_guard=None),
        ema=dict(decay=0.99, warmup=True, updates=9, shadows={"a.weight": r(3, 4)}),
        host_rng=dict(cpu=torch.get_rng_state(), device=None))
    state.update(over)
    return state


def test_a_hand_made_state_round_trips_under_weights_only(tmp_path):
    state = hand_made()
    path = str(tmp_path / "training_state.pt")
    checkpoint.save(path, state)
    assert not os.path.exists(path + ".tmp")
    assert same(torch.load(path, map_location="cpu", weights_only=True), state)      # nothing but plain values in the file
    got = checkpoint.load(path, config=CONFIG)
    assert same(got, state)
    assert checkpoint.digest(got) == checkpoint.digest(state)
    assert len(checkpoint.digest(state)) == 64


def test_the_digest_sees_every_tensor_and_the_position_and_not_the_config():
    base = checkpoint.digest(hand_made())
    assert base == checkpoint.digest(hand_made())
    assert base == checkpoint.digest(hand_made(config=dict(CONFIG, lr=3.0)))
    moved = hand_made()
    moved["position"]["next_step"] = 4
    assert checkpoint.digest(moved) != base
    for where in (("model", "a.bias"), ("rng",), ("optimizer", "state", "state", 0, "next_v"), ("optimizer", "guard", "records"),
                  ("ema", "shadows", "a.weight"), ("bank", "ring", "mb_mask_v"), ("host_rng", "cpu")):
        state = hand_made()
        t = state
        for k in where:
            t = t[k]
        flat = t.reshape(-1).view(torch.uint8)
        flat[-1] ^= 1                                        # one bit
        assert checkpoint.digest(state) != base, where


def test_a_failed_replace_leaves_the_previous_file(tmp_path, monkeypatch):
    path = str(tmp_path / "training_state.pt")
    old = hand_made(seed=1)
    checkpoint.save(path, old)

    def refuse(src, dst):
        raise OSError("no replace today")
    monkeypatch.setattr(os, "replace", refuse)
    with pytest.raises(OSError, match="no replace today"):
        checkpoint.save(path, hand_made(seed=2))
    monkeypatch.undo()
    assert same(checkpoint.load(path, config=CONFIG), old)
    assert not os.path.exists(path + ".tmp")


def test_load_refuses_what_does_not_fit(tmp_path):
    path = str(tmp_path / "training_state.pt")
    checkpoint.save(path, hand_made())
    whole = open(path, "rb").read()
    for keep in (0, 10, len(whole) // 2, len(whole) - 7):
        cut = str(tmp_path / f"cut{keep}.pt")
        with open(cut, "wb") as f:
            f.write(whole[:keep])
        with pytest.raises(checkpoint.CheckpointError, match="unreadable or truncated"):
            checkpoint.load(cut)
    with pytest.raises(checkpoint.CheckpointError, match="unreadable or truncated"):
        checkpoint.load(str(tmp_path / "absent.pt"))
    torch.save({"format": 1}, path)
    with pytest.raises(checkpoint.CheckpointError, match="not a training state"):
        checkpoint.load(path)
    checkpoint.save(path, hand_made(format=checkpoint.FORMAT + 1))
    with pytest.raises(checkpoint.CheckpointError, match=f"format {checkpoint.FORMAT + 1}"):
        checkpoint.load(path)
    checkpoint.save(path, hand_made(abi=int(hip.version()) + 1))
    with pytest.raises(checkpoint.CheckpointError, match=f"ABI version {int(hip.version()) + 1}"):
        checkpoint.load(path)


def test_a_differing_config_names_every_key_with_both_values(tmp_path):
    path = str(tmp_path / "training_state.pt")
    checkpoint.save(path, hand_made())
    assert checkpoint.load(path)["config"] == CONFIG         # without the run's config nothing is compared
    mine = dict(CONFIG, batch_size=64, lr=2e-4, optimizer="adamw", kl_weight=1.0)
    del mine["beta"]
    with pytest.raises(checkpoint.CheckpointError) as err:
        checkpoint.load(path, config=mine)
    msg = str(err.value)
    for part in ("batch_size: saved 32, this run 64", "lr: saved 0.0001, this run 0.0002", "optimizer: saved 'bertadam', this run 'adamw'",
                 "kl_weight: saved (absent), this run 1.0", "beta: saved 0.7, this run (absent)"):
        assert part in msg, (part, msg)
    for same_key in ("epochs", "seed", "mb_batch"):
        assert same_key + ":" not in msg


def test_config_from_args_takes_the_trajectory_arguments():
    from types import SimpleNamespace
    args = SimpleNamespace(**{k: i for i, k in enumerate(checkpoint.CONFIG_KEYS)}, output_dir="x", n_display=3, hip_graph=1)
    assert checkpoint.config_from_args(args) == {k: i for i, k in enumerate(checkpoint.CONFIG_KEYS)}
    for key in ("batch_size", "world_size", "epochs", "lr", "coef_lr", "warmup_proportion", "weight_decay", "optimizer", "precision",
                "seed", "synthetic_train", "max_words", "max_frames", "mb_batch", "encoders", "skip_nonfinite", "ema_decay",
                "ema_warmup", "centrality_multi_token", "centrality_scale", "kl_weight", "uniform_weight", "beta", "num_neighbors",
                "temperature", "neighbor_weight"):
        assert key in checkpoint.CONFIG_KEYS, key


def _cpu_model(seed):
    from neighborretr_amd import modeling
    torch.manual_seed(seed)
    return modeling.NeighborRetr(modeling.default_config(num_neighbors=4))


def test_a_cpu_bank_round_trips_raw(tmp_path):
    """Three pushes, the last two wrapping a bank of six; the raw order, the (host) head and mb_batch come back as they were,
    `_mb_gen` moves exactly once on restore and not at all on capture."""
    m = _cpu_model(1)
    g = torch.Generator().manual_seed(3)
    for r, b in enumerate((6, 4, 4)):
        m.update_memory_bank(torch.arange(100 * r, 100 * r + b), torch.randn(b, 5, 8, generator=g), torch.randn(b, 3, 8, generator=g),
                             torch.ones(b, 5), torch.ones(b, 3))
    assert m._mb["mb_ind"].tolist() == [200, 201, 202, 203, 100, 101]
    m._mb_head = 2                                           # a host head that is not 0: the ring as it lies, not the FIFO order
    opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)
    gen = m._mb_gen
    raw = {k: v.clone() for k, v in m._mb.items()}
    state = checkpoint.capture_state(m, opt, position=dict(epoch=0, next_step=3, global_step=3), config=CONFIG)
    assert m._mb_gen == gen and m._mb_head == 2 and all(torch.equal(m._mb[k], raw[k]) for k in raw)
    assert state["rng"] is None and state["ema"] is None and state["bank"]["head"] == 2 and state["bank"]["head_on_device"] == 0
    path = str(tmp_path / "training_state.pt")
    checkpoint.save(path, state)

    m2 = _cpu_model(2)
    assert any(not torch.equal(p, q) for p, q in zip(m.parameters(), m2.parameters()))
    opt2 = torch.optim.SGD(m2.parameters(), lr=0.1, momentum=0.9)
    gen2, versions = m2._mb_gen, [p._version for p in m2.parameters()]
    where = [p.data_ptr() for p in m2.parameters()]
    pos = checkpoint.restore_state(checkpoint.load(path, config=CONFIG), m2, opt2)
    assert pos == dict(epoch=0, next_step=3, global_step=3)
    assert m2._mb_gen == gen2 + 1
    assert m2._mb_head == 2 and m2._mb_head_dev is None and m2.mb_batch == m.mb_batch == 6 and m2._mb_shadow is None
    assert list(m2._mb) == list(raw) and all(same(m2._mb[k], raw[k]) for k in raw)
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), m2.parameters()))
    assert where == [p.data_ptr() for p in m2.parameters()]                  # into the existing storage ...
    assert all(p._version > v for p, v in zip(m2.parameters(), versions))    # ... through copy_: the derived caches re-derive
    # what the reference-named attributes show is the same FIFO on both sides
    assert torch.equal(m2.mb_ind, m.mb_ind) and m.mb_ind.tolist() == [202, 203, 100, 101, 200, 201]


def test_capture_inside_an_applied_average_raises():
    class Applied:
        _applied = True
    m = _cpu_model(1)
    with pytest.raises(RuntimeError, match="applied"):
        checkpoint.capture_state(m, torch.optim.SGD(m.parameters(), lr=0.1), ema=Applied())


@pytest.mark.parametrize("argv, message", [
    (["--do_train", "1", "--save_state_every", "-1"], "must be >= 0"),
    (["--do_train", "1", "--max_steps", "-3"], "must be >= 0"),
    (["--do_eval", "1", "--resume", "auto"], "needs --do_train 1"),
    (["--do_train", "1", "--resume", "auto", "--init_model", "x.bin"], "not together with --init_model"),
])
def test_flag_errors_go_through_the_parser(monkeypatch, capsys, argv, message):
    sys.path.insert(0, ROOT)
    import main_retrieval
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py", "--synthetic"] + argv)
    with pytest.raises(SystemExit) as err:
        main_retrieval.get_args()
    assert err.value.code == 2
    assert message in capsys.readouterr().err


def test_the_flags_default_to_off(monkeypatch):
    sys.path.insert(0, ROOT)
    import main_retrieval
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py", "--synthetic", "--do_train", "1"])
    args = main_retrieval.get_args()
    assert (args.save_state_every, args.resume, args.max_steps) == (0, None, 0)
