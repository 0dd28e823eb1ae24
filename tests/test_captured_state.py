"""What the plugin captured belongs to the module prepare() built: the inference graph tables' rule on the CPU, a second
prepare() on one plugin object, and a training-step capture that raises."""
import importlib
import types

import numpy as np
import pytest
import torch

from test_model_parity import FakeValLoader

NETWORKS = [("LarvaNet", ["--num_modules=2", "--num_blocks=2,1"]), ("LarvaNetV2", ["--num_modules=2", "--num_blocks=1,2"])]
ARGS = types.SimpleNamespace(train_path="/tmp")


def test_graph_table_rule_with_fake_callables():
    from larvanet_amd.infer_graphs import GraphTable
    calls = {"run": 0, "capture": 0, "replay": 0}

    def run(x):
        calls["run"] += 1
        return ("ran", x)

    def capture(x):
        calls["capture"] += 1

        def replay(y):
            calls["replay"] += 1
            return ("replayed", y)
        return replay

    t = GraphTable()
    assert t.forward("a", 1, capture, run) == ("ran", 1) and calls == {"run": 1, "capture": 0, "replay": 0} and not t
    assert t.forward("a", 2, capture, run) == ("replayed", 2) and calls == {"run": 1, "capture": 1, "replay": 1}
    assert t.forward("a", 3, capture, run) == ("replayed", 3) and calls == {"run": 1, "capture": 1, "replay": 2}
    assert len(t) == 1 and "a" in t and list(t) == ["a"] and t.get("a") is t["a"] and list(t.values()) == [t["a"]]
    for key in "bcd":
        for x in range(2):
            t.forward(key, x, capture, run)
    assert len(t) == 4 and calls == {"run": 4, "capture": 4, "replay": 5}
    for x in range(5):   # four entries held: a fifth key runs however often it is seen
        assert t.forward("e", x, capture, run) == ("ran", x)
    assert len(t) == 4 and "e" not in t and calls == {"run": 9, "capture": 4, "replay": 5}

    failed = {"n": 0}

    def fails(x):
        failed["n"] += 1
        return False

    t = GraphTable()
    got = [t.forward("k", x, fails, run) for x in range(5)]
    assert got == [("ran", x) for x in range(5)] and failed["n"] == 1 and t["k"] is False

    t = GraphTable()
    for x in range(2):
        t.forward("held", x, capture, run)
    for i in range(512):
        t.forward(("once", i), 0, capture, run)
    assert len(t.seen) == 513 and ("once", 0) in t.seen   # ("held" and 512 more: not yet more than 512 when last looked at)
    t.forward(("once", 512), 0, capture, run)             # finds more than 512 counts: they are cleared, the entry is not
    assert set(t.seen) == {("once", 512)} and list(t) == ["held"]
    before = calls["replay"]
    assert t.forward("held", 7, capture, run) == ("replayed", 7) and calls["replay"] == before + 1


def _plugin(name, flags, seed, training, extra=()):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(list(flags) + list(extra))
    m.strict_graph = True
    torch.manual_seed(seed)
    m.prepare(is_training=training, scales=[4])
    return m


def _again(m, seed, training):
    torch.manual_seed(seed)
    m.prepare(is_training=training, scales=[4])
    return m


def _weights(m):
    return {k: v.cpu().numpy().copy() for k, v in m.model.state_dict().items()}


def _same_weights(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _batches(hip_device, n, w=16, seed=23):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(4, 3, 12, w, generator=g) * 255).to(hip_device), (torch.rand(4, 3, 48, 4 * w, generator=g) * 255).to(hip_device))
            for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,flags", NETWORKS, ids=[n for n, _ in NETWORKS])
def test_second_prepare_trains_like_a_fresh_plugin(hip_device, name, flags):
    """A captured step reads the module, the gradient bucket and the optimizer of the prepare() before it: a second
    prepare() on the same plugin must forget it."""
    warm, fixed = _batches(hip_device, 2, seed=3), _batches(hip_device, 3)
    m = _plugin(name, flags, 5, True)
    for x, t in warm:
        m.train_step_larva(ARGS, FakeValLoader(7), x, t)
    assert m._step is not None and m.hip_graph_fell_back is None
    results = []
    for p in (_again(m, 11, True), _plugin(name, flags, 11, True)):
        results.append(([p.train_step_larva(ARGS, FakeValLoader(7), x, t) for x, t in fixed], _weights(p)))
        assert p._step is not None and p.use_hip_graph
    assert results[0][0] == results[1][0] and all(isinstance(v, float) for v in results[0][0])
    _same_weights(results[0][1], results[1][1])


def _u8_images(n, h, w, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["float", "u8", "ensemble"])
@pytest.mark.parametrize("name,flags", NETWORKS, ids=[n for n, _ in NETWORKS])
def test_second_prepare_upscales_like_a_fresh_plugin(hip_device, name, flags, form):
    if form == "float":
        rng = np.random.RandomState(5)
        batch = [rng.randint(0, 256, size=(3, 16, 20)).astype(np.float32) for _ in range(4)]
    else:
        batch = _u8_images(4, 16, 20, 5) if form == "u8" else _u8_images(1, 9, 14, 5)
    extra = ["--self_ensemble"] if form == "ensemble" else []
    call = (lambda p: p.upscale(batch, 4)) if form == "float" else (lambda p: p.upscale_u8(batch, 4))
    table = {"float": "_infer_graphs", "u8": "_infer_graphs_u8", "ensemble": "_infer_graphs_se"}[form]
    m = _plugin(name, flags, 5, False, extra)
    for _ in range(3):
        call(m)
    old = dict(getattr(m, table))
    assert len(old) == 1 and all(v is not False for v in old.values())
    _again(m, 11, False)
    got = [call(m) for _ in range(3)]
    want = call(_plugin(name, flags, 11, False, extra))   # first sight: eager
    for i, g in enumerate(got):
        assert np.array_equal(g, want), i
    now = getattr(m, table)
    assert len(now) == 1 and set(now) == set(old) and all(now[k] is not old[k] and now[k] is not False for k in now)
    assert sum(len(t) for t in (m._infer_graphs, m._infer_graphs_u8, m._infer_graphs_se)) == 1


def _raise_once_in_exit_losses(m):
    def once(*a):
        del m._exit_losses   # (the class's method again)
        raise RuntimeError("injected into the capture's first warm-up run")
    m._exit_losses = once


@pytest.mark.gpu
def test_capture_that_raises_falls_back_whole(hip_device):
    """strict_graph off: a capture of a new shape that raises (on the host, before anything was launched) switches the
    plugin to eager launches with nothing half-made left, and the eager step is the step of a plugin that never captured."""
    from larvanet_amd.autograd import DualChain
    name, flags = NETWORKS[0]
    (xa, ta), = _batches(hip_device, 1)
    (xb, tb), = _batches(hip_device, 1, w=20, seed=29)
    m = _plugin(name, flags, 5, True)
    m.strict_graph = False
    first = m.train_step_larva(ARGS, FakeValLoader(7), xa, ta)
    assert m.input_buffers(xa.shape, ta.shape) is not None
    _raise_once_in_exit_losses(m)
    second = m.train_step_larva(ARGS, FakeValLoader(7), xb, tb)
    assert "_exit_losses" not in vars(m)
    assert "RuntimeError" in m.hip_graph_fell_back and "injected" in m.hip_graph_fell_back
    assert m.use_hip_graph is False
    assert m.input_buffers(xa.shape, ta.shape) is None and m.input_buffers(xb.shape, tb.shape) is None
    assert not DualChain._forked and not DualChain._keep
    ref = _plugin(name, flags, 5, True)
    ref.use_hip_graph = False
    assert isinstance(first, float) and [ref.train_step_larva(ARGS, FakeValLoader(7), x, t) for x, t in ((xa, ta), (xb, tb))][1] == second
    _same_weights(_weights(m), _weights(ref))


@pytest.mark.gpu
def test_capture_that_raises_under_strict_graph_keeps_the_previous_capture(hip_device):
    name, flags = NETWORKS[0]
    (xa, ta), (xa2, ta2) = _batches(hip_device, 2)
    (xb, tb), = _batches(hip_device, 1, w=20, seed=29)
    m, ref = _plugin(name, flags, 5, True), _plugin(name, flags, 5, True)
    losses = [m.train_step_larva(ARGS, FakeValLoader(7), xa, ta)]
    held = m._step
    _raise_once_in_exit_losses(m)
    with pytest.raises(RuntimeError, match="injected"):
        m.train_step_larva(ARGS, FakeValLoader(7), xb, tb)
    assert m._step is held and m.use_hip_graph and m.hip_graph_fell_back is None
    bufs = m.input_buffers((4, 3, 12, 16), (4, 3, 48, 64))
    assert bufs is not None and bufs[0].shape == xa.shape and bufs[1].shape == ta.shape
    assert m.input_buffers(xb.shape, tb.shape) is None
    losses.append(m.train_step_larva(ARGS, FakeValLoader(7), xa2, ta2))
    assert m._step is held
    assert losses == [ref.train_step_larva(ARGS, FakeValLoader(7), x, t) for x, t in ((xa, ta), (xa2, ta2))]
    _same_weights(_weights(m), _weights(ref))
