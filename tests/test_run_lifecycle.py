"""The run around the training step: resumed, lr-dropped and handed-over runs, end to end.

Every other file enters through train_step_larva on batches it builds itself.  Here the DRIVER runs (train_larva.main /
train_larvaV2.main: loader -> input_buffers -> sampler launch -> captured step -> validation -> plateau scheduler ->
checkpoint and training state), and three things a 300 000-step run depends on are held to a value:

  C1  a run interrupted at step k and resumed from its training state continues bit for bit: losses, learning rates,
      counters, scheduler, weights, moments, the loader's sampler state and every file both runs wrote;
  C2  the driver's run follows oracle/larva_torch.train_trajectory in float64 on batches rebuilt on the host from the
      same seed: the same learning rates, validation steps and checkpoint names, losses within 2e-3 relative, PSNRs
      within 0.02 dB, final weights within four times the distance of torch's own fp32
      CPU run from float64 (measured in the test);
  C3  the flat optimizer's hand-over to torch's per-tensor AdamW in the middle of a run, and a per-tensor state loaded
      back into a flat optimizer, against float64 torch.optim.AdamW: losses within 2e-5 relative, weights as in C2;
  C4  on the CPU: the loaders' sampler states, the optimizer state across both paths, atomic saves, the conditions C2's
      inputs must meet (the lr really moves, no plateau decision near zero), and two float64 mutants (moments dropped
      at the hand-over, an lr drop ignored) that land outside the weight bar by more than ten times.

All networks are two bodies of one block; every run is 12 steps of batch 4 on 12 x 12 patches (tests/run_ref.py).

Measured on the MI355X (weights: largest distance from float64 / share of elements further than 2e-5):
see DESIGN.md section 7q."""
import copy
import gc
import glob
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

import run_ref as R
from larvanet_amd.models import LarvaNet as V1
from larvanet_amd.optim import FlatAdamW, flatten_parameters

gpu = pytest.mark.gpu


# The file builds many plugins with captured graphs, which live in reference cycles: a graph freed by the collector while
# another is being captured aborts the process (tests/test_interleaved_shapes.py).  The collector runs between tests only.
@pytest.fixture(scope="module", autouse=True)
def _nothing_dropped_earlier_is_left():
    gc.collect()
    yield


@pytest.fixture(autouse=True)
def _the_collector_runs_between_tests_only(_nothing_dropped_earlier_is_left):
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        gc.collect()
        if was:
            gc.enable()


def _same(a, b, where=""):
    """Bitwise / exact equality of two nested python objects; returns the first place that differs, or None."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        ok = (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
              and torch.equal(a.cpu(), b.cpu()))
        return None if ok else where + ": tensors differ"
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return None if np.array_equal(np.asarray(a), np.asarray(b)) else where + ": arrays differ"
    if isinstance(a, dict) and isinstance(b, dict):
        if sorted(map(str, a)) != sorted(map(str, b)):
            return "%s: keys %s against %s" % (where, sorted(map(str, a)), sorted(map(str, b)))
        for k in a:
            bad = _same(a[k], b[k], "%s[%r]" % (where, k))
            if bad:
                return bad
        return None
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return "%s: lengths %d against %d" % (where, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            bad = _same(x, y, "%s[%d]" % (where, i))
            if bad:
                return bad
        return None
    return None if a == b else "%s: %r against %r" % (where, a, b)


# ================================================================ C4: CPU
def _write_div2k(tmp_path, n=3):
    from PIL import Image
    hr_dir, lr_dir = tmp_path / "HR", tmp_path / "LR" / "X4"
    hr_dir.mkdir(parents=True)
    lr_dir.mkdir(parents=True)
    for i in range(n):
        lr, hr = R.SL.make_pair(i, 20 + i, 24, 4, False)
        Image.fromarray(hr.transpose(1, 2, 0)).save(hr_dir / ("%04d.png" % i))
        Image.fromarray(lr.transpose(1, 2, 0)).save(lr_dir / ("%04dx4.png" % i))
    return str(tmp_path / "LR"), str(hr_dir)


def _loader(kind, tmp_path, seed="--data_seed=5"):
    """-> (a prepared loader of `kind`, draw: loader -> one batch as nested arrays)."""
    mod = importlib.import_module("larvanet_amd.dataloaders." + kind)
    ld = mod.create_loader()
    if kind == "synthetic_loader":
        ld.parse_args(["--synthetic_images=3", "--synthetic_lr_size=20", seed])
        ld.prepare([4])
    elif kind == "div2k_train_loader":
        if not (tmp_path / "HR").exists():
            _write_div2k(tmp_path)
        ld.parse_args(["--data_input_path", str(tmp_path / "LR"), "--data_truth_path", str(tmp_path / "HR")] + [seed] * bool(seed))
        ld.prepare([4])
    else:
        # prepare() makes the dataset resident on a device; the draw stream needs the generator and the shapes only
        ld.parse_args(["--device_source=synthetic_loader"] + [seed] * bool(seed))
        ld.rng = np.random.RandomState(5)
        ld.shapes = [(20, 20), (20, 28), (20, 36)]
        return ld, lambda l: R.DPL.draw_batch(l.rng, l.shapes, 4, 12)
    return ld, lambda l: [np.stack(part) for part in l.get_patch_batch(batch_size=4, scale=4, input_patch_size=12)]


@pytest.mark.parametrize("kind", ["synthetic_loader", "div2k_train_loader", "device_patch_loader"])
def test_sampler_state_round_trip(kind, tmp_path):
    """Three batches, the state, two more; a new loader given the state draws the same two."""
    a, draw = _loader(kind, tmp_path)
    for _ in range(3):
        draw(a)
    state = copy.deepcopy(a.sampler_state())
    assert state is not None
    want = [draw(a), draw(a)]
    b, _ = _loader(kind, tmp_path)
    fresh = draw(b)
    assert _same(fresh, want[0]) is not None          # (a new loader starts the stream again: the defect)
    b.load_sampler_state(state)
    got = [draw(b), draw(b)]
    assert _same(got, want) is None
    assert _same(b.sampler_state(), a.sampler_state()) is None


def test_loaders_that_cannot_be_continued_say_so(tmp_path):
    """combined_loader prefetches on threads; a stream without --data_seed is entropy per process: None, both."""
    from larvanet_amd.dataloaders import combined_loader
    lr_root, hr_root = _write_div2k(tmp_path)
    c = combined_loader.create_loader()
    c.parse_args(["--data_input_path", lr_root, "--data_truth_path", hr_root, "--data_seed=5"])
    c.prepare([4])
    assert c.is_threaded and c.sampler_state() is None
    with pytest.raises(NotImplementedError):
        c.load_sampler_state(("MT19937",))
    for kind in ("div2k_train_loader", "device_patch_loader"):
        assert _loader(kind, tmp_path, seed="")[0].sampler_state() is None


def test_device_loader_leaves_the_models_lr_flag_alone():
    """--lr is a prefix of the device loader's --lr_from_hr: argparse's prefix matching took the model's flag for it and
    ended the driver ("argument --lr_from_hr: ignored explicit argument '0.002'")."""
    ld = R.DPL.create_loader()
    parsed, rest = ld.parse_args(["--device_source=synthetic_loader", "--lr=0.002", "--data_seed=1", "--threshold=0.1"])
    assert rest == ["--lr=0.002", "--threshold=0.1"] and parsed.lr_from_hr is False and ld.args.data_seed == 1


def _flat_optimizer(seed, lr=1e-3):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.Conv2d(5, 2, 3))
    params = [p for p in net.parameters()]
    flat = flatten_parameters(net)
    return net, params, FlatAdamW(params, flat, None, lr=lr)


def test_optimizer_state_across_paths_on_the_cpu():
    """A per-tensor state loaded into a flat optimizer fills _m / _v / _t in _plist order and restores the param-group
    scalars (before: torch's load_state_dict filled `state`, which the flat launch never reads, and the next step ran
    with zero moments and t = 0); flat -> flat round-trips; flat -> per-tensor stays a RuntimeError.  No step is taken by
    the flat optimizer (its launch needs the device)."""
    net, params, flat_opt = _flat_optimizer(0)
    # torch's own AdamW on copies of the parameters: three CPU steps on random gradients
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.AdamW(twins, lr=1e-3)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        for p in twins:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    ref.param_groups[0]["lr"] = 2.5e-4
    flat_opt.load_training_state({"flat": False, "torch": ref.state_dict()})
    assert flat_opt._t == 3 and flat_opt._flat_p is not None and not flat_opt.state
    assert flat_opt.param_groups[0]["lr"] == 2.5e-4 and all(a is b for a, b in zip(flat_opt.param_groups[0]["params"], params))
    off = 0
    for p, twin in zip(params, twins):
        n = p.numel()
        assert torch.equal(flat_opt._m[off:off + n].view_as(p), ref.state[twin]["exp_avg"])
        assert torch.equal(flat_opt._v[off:off + n].view_as(p), ref.state[twin]["exp_avg_sq"])
        off += n
    assert off == flat_opt._m.numel() and float(flat_opt._v.min()) >= 0 and float(flat_opt._v.max()) > 0
    # flat -> flat
    st = copy.deepcopy(flat_opt.training_state())
    assert st["flat"] is True
    _, _, other = _flat_optimizer(7, lr=9.0)
    other.load_training_state(st)
    assert other._t == 3 and torch.equal(other._m, flat_opt._m) and torch.equal(other._v, flat_opt._v)
    assert other.param_groups[0]["lr"] == 2.5e-4
    # flat -> per-tensor: refused
    _, _, handed = _flat_optimizer(8)
    handed._flat_p = None   # (what _fallback_step leaves behind)
    with pytest.raises(RuntimeError, match="flat optimizer state"):
        handed.load_training_state(st)
    # per-tensor -> per-tensor: torch's own
    handed.load_training_state({"flat": False, "torch": ref.state_dict()})
    assert len(handed.state) == len(params) and handed.param_groups[0]["lr"] == 2.5e-4


def _host_plugin(seed=0, extra=()):
    m = V1.create_model()
    m.parse_args(R.TINY + list(extra))
    torch.manual_seed(seed)
    m.prepare(is_training=True, scales=[4])
    return m


def test_training_state_carries_the_sampler_and_old_files_still_load(tmp_path, capsys):
    """save_training_state stores the attached loader's sampler state and restore_training_state hands it back; a file
    from before the entry, a state without one and a plugin without a loader load with ONE warning line that says the
    patch stream restarts.  (No step is taken: this runs wherever the plugin can be built.)"""
    a = _host_plugin()
    a.train_loader, draw = _loader("synthetic_loader", tmp_path)
    for _ in range(3):
        draw(a.train_loader)
    a.global_step, a.total_volume, a.temp_volume = 6, 3456.0 * 3, 1728
    path = a.save_training_state(str(tmp_path))
    assert os.path.basename(path) == "train_state_step6.pth"
    want = [draw(a.train_loader), draw(a.train_loader)]
    capsys.readouterr()

    b = _host_plugin(seed=1)
    b.train_loader, _ = _loader("synthetic_loader", tmp_path)
    assert b.restore_training_state(path) is True
    assert "WARNING" not in capsys.readouterr().out
    assert (b.global_step, b.total_volume, b.temp_volume) == (6, 3456.0 * 3, 1728)
    assert _same([draw(b.train_loader), draw(b.train_loader)], want) is None

    st = torch.load(path, map_location="cpu", weights_only=False)
    old = {k: v for k, v in st.items() if k != "train_loader"}
    none = dict(st, train_loader=None)
    for name, content, loader in (("old.pth", old, True), ("none.pth", none, True), ("noloader.pth", st, False)):
        torch.save(content, str(tmp_path / name))
        c = _host_plugin(seed=2)
        if loader:
            c.train_loader, _ = _loader("synthetic_loader", tmp_path)
        assert c.restore_training_state(str(tmp_path / name)) is False
        out = capsys.readouterr().out
        assert out.count("WARNING") == 1 and "patch stream restarts" in out, out
        assert c.global_step == 6
        if loader:   # the stream is where a new loader's is
            assert _same(draw(c.train_loader), draw(_loader("synthetic_loader", tmp_path)[0])) is None


def test_an_interrupted_save_leaves_the_previous_file_and_nothing_partial(tmp_path, monkeypatch):
    m = _host_plugin()
    m.global_step = 4
    paths = [m.save(str(tmp_path)), m.save_training_state(str(tmp_path))]
    before = [open(p, "rb").read() for p in paths]
    names = sorted(os.listdir(str(tmp_path)))
    assert names == ["model_step4_vol0G.pth", "train_state_step4.pth"]

    real = torch.save

    def interrupted(obj, f, *a, **k):
        real(obj, f, *a, **k)
        raise KeyboardInterrupt   # (what ends a run: raised after the bytes are out, as late as a save can be cut)

    with torch.no_grad():
        for p in m.model.parameters():
            p.add_(1.0)
    monkeypatch.setattr(torch, "save", interrupted)
    for call in (m.save, m.save_training_state):
        with pytest.raises(KeyboardInterrupt):
            call(str(tmp_path))
    monkeypatch.setattr(torch, "save", real)
    assert sorted(os.listdir(str(tmp_path))) == names
    assert [open(p, "rb").read() for p in paths] == before
    assert m.save(str(tmp_path)) == paths[0] and open(paths[0], "rb").read() != before[0]


def _used_lrs(model, rec):
    return [R.PLATEAU[model]["lr"]] + rec["lrs"][:-1]


@pytest.mark.parametrize("model", ["LarvaNet", "LarvaNetV2"])
def test_the_oracle_runs_move_the_lr_with_margin(model):
    """What C2's inputs must meet, on the float64 oracle alone: the lr drops at least twice, at least one validation
    after the first leaves it alone, and every plateau decision (PSNR - best - threshold) is at least 0.05 dB from zero,
    2.5 times the PSNR bar the device run is held to -- so the device cannot legitimately decide otherwise."""
    p = R.PLATEAU[model]
    rec, _ = R.oracle_run(model, torch.float64)
    drops = R.lr_drops(p["lr"], rec["lrs"])
    decisions = R.plateau_decisions(rec["psnrs"], p["threshold"])
    print(model, "psnrs", rec["psnrs"], "decisions", decisions, "drops after steps", drops)
    assert len(drops) >= 2
    assert any(d > 0 for d in decisions)                 # a validation that improves and drops nothing
    assert min(abs(d) for d in decisions) >= R.MARGIN
    assert rec["lrs"][-1] < p["lr"] / 3 and len(set(rec["lrs"])) >= 3
    if model == "LarvaNet":   # C1 resumes where a cooldown runs: the first save after a drop is not the last step
        assert drops[0] in rec["val_steps"] and 1 < drops[0] < R.STEPS - 2
    # torch's fp32 run of the same trajectory decides the same
    rec32, _ = R.oracle_run(model, torch.float32)
    assert rec32["lrs"] == rec["lrs"] and rec32["val_steps"] == rec["val_steps"]


def test_the_weight_bars_see_a_dropped_moment_and_an_ignored_lr_drop():
    """Two float64 mutants against the float64 runs, measured with the bar of C2 / C3 (four times the fp32 CPU run's
    distance): each must be outside by more than ten times."""
    # the hand-over forgets the moments (C3: after step 3 of 6), and the cross-path load forgets them (after 6 of 8)
    fb = R.fixed_batch()
    for steps, at in ((6, 3), (8, 6)):
        _, w64 = R.adamw_run("LarvaNet", torch.float64, fb, [4e-4] * steps)
        _, w32 = R.adamw_run("LarvaNet", torch.float32, fb, [4e-4] * steps)
        _, mut = R.adamw_run("LarvaNet", torch.float64, fb, [4e-4] * steps, reset_at=at)
        d32, f32 = R.weight_distance(w32, w64)
        dm, fm = R.weight_distance(mut, w64)
        print("moments dropped after %d of %d: d32 %.3e f32 %.2e, mutant %.3e %.2e" % (at, steps, d32, f32, dm, fm))
        assert dm >= 10 * 4 * d32 and fm >= 10 * (4 * f32 + 1e-3)
    # an lr drop that never reaches the AdamW launch: from that step on the lr is twice what it should be
    for model, which in (("LarvaNet", 0), ("LarvaNet", 1), ("LarvaNetV2", 0)):
        rec, w64 = R.oracle_run(model, torch.float64)
        _, w32 = R.oracle_run(model, torch.float32)
        used = _used_lrs(model, rec)
        batches = R.host_batches(R.STEPS, torch.float64)
        _, replay = R.adamw_run(model, torch.float64, batches, used)
        assert R.weight_distance(replay, w64) == (0.0, 0.0)   # (the replay IS the trajectory)
        drop = R.lr_drops(R.PLATEAU[model]["lr"], rec["lrs"])[which]
        assert R.STEPS - drop <= 12
        _, mut = R.adamw_run(model, torch.float64, batches, used[:drop] + [2 * v for v in used[drop:]])
        d32, f32 = R.weight_distance(w32, w64)
        dm, fm = R.weight_distance(mut, w64)
        print("%s, drop after step %d ignored: d32 %.3e f32 %.2e, mutant %.3e %.2e" % (model, drop, d32, f32, dm, fm))
        assert dm >= 10 * 4 * d32 and fm >= 10 * (4 * f32 + 1e-3)


# ================================================================ GPU: the driver's runs
def _driver_run(monkeypatch, model, argv, seed):
    """One train_larva(V2).main call -> everything the tests compare, on the host.  Losses are recorded by wrapping
    train_step_larva on the class, PSNRs by wrapping validate_for_train."""
    steps, vals = [], []
    step, validate = V1.LarvaNet.train_step_larva, V1.LarvaNet.validate_for_train

    def recording_step(self, *a, **k):
        loss = step(self, *a, **k)
        steps.append({"loss": loss, "lr": self.get_lr(), "global_step": self.global_step,
                      "total_volume": self.total_volume, "temp_volume": self.temp_volume})
        return loss

    def recording_validate(self, *a, **k):
        psnr = validate(self, *a, **k)
        vals.append((self.global_step, float(psnr)))
        return psnr

    with monkeypatch.context() as mp:
        mp.setattr(V1.LarvaNet, "train_step_larva", recording_step)
        mp.setattr(V1.LarvaNet, "validate_for_train", recording_validate)
        R.register_val_loader(mp)
        torch.manual_seed(seed)
        main = importlib.import_module("larvanet_amd.train_larvaV2" if model == "LarvaNetV2" else "larvanet_amd.train_larva").main
        m = main(argv)
    torch.cuda.synchronize()
    for s in steps:   # (--async_loss hands back 0-d device tensors)
        s["loss"] = float(s["loss"])
    opt = m.optim
    shape = (R.BATCH, 3, R.PATCH, R.PATCH)
    run = {"steps": steps, "vals": vals, "scheduler": copy.deepcopy(m.scheduler.state_dict()),
           "weights": {k: v.detach().cpu().clone() for k, v in m.model.state_dict().items()},
           "flat": isinstance(opt, FlatAdamW) and opt._flat_p is not None,
           "m": opt._m.cpu().clone(), "v": opt._v.cpu().clone(), "t": opt._t,
           "sampler": copy.deepcopy(m.train_loader.sampler_state()),
           "captured": m._step is not None,
           "buffers": m.input_buffers(shape, (R.BATCH, 3, R.PATCH * m.scale, R.PATCH * m.scale)) is not None,
           "counters": (m.global_step, m.total_volume, m.temp_volume)}
    del m
    return run


# case -> (model, loader, extra flags, k or None = the first save after an lr drop, env)
CASES = {
    "1-sync": ("LarvaNet", "device", [], None, {}),
    "2-async": ("LarvaNet", "device", ["--async_loss"], None, {}),
    "3-host-loader": ("LarvaNet", "host", [], 2, {}),
    "4-v2-every-step": ("LarvaNetV2", "device", [], 3, {}),
    "5-x2-lr-from-hr": ("LarvaNet", "device", ["--scales=2", "--lr_from_hr"], 4, {}),
    "6-no-graph": ("LarvaNet", "device", [], None, {"LARVA_HIP_GRAPH": "0"}),
}
_STRAIGHT = {}


def _straight(case, monkeypatch, tmp_path_factory):
    """The straight run of a case, made once (C2 reads the runs of cases 1 and 4 again)."""
    if case not in _STRAIGHT:
        model, loader, extra, _, env = CASES[case]
        path = tmp_path_factory.mktemp("straight")
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            run = _driver_run(mp, model, R.driver_argv(model, path, loader, extra=extra), R.INIT_SEED)
        run["dir"] = str(path)
        _STRAIGHT[case] = run
    return _STRAIGHT[case]


def _files(path):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(path, "*.pth")))


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_resumed_run_equals_the_straight_run_bit_for_bit(hip_device, case, monkeypatch, tmp_path_factory):
    model, loader, extra, k, env = CASES[case]
    a = _straight(case, monkeypatch, tmp_path_factory)
    assert len(a["steps"]) == R.STEPS and a["flat"]
    assert a["captured"] == (not env) and a["buffers"] == a["captured"]
    lrs = [s["lr"] for s in a["steps"]]
    if k is None:
        k = R.lr_drops(R.PLATEAU[model]["lr"], lrs)[0]
        st = torch.load(os.path.join(a["dir"], "train_state_step%d.pth" % k), map_location="cpu", weights_only=False)
        assert st["scheduler"]["cooldown_counter"] == 1 and st["train_loader"] is not None   # saved with a cooldown running
    if case in ("1-sync", "4-v2-every-step"):
        assert len(set(lrs)) >= 3   # the lr really moved
    weights = [f for f in _files(a["dir"]) if f.startswith("model_step%d_" % k)]
    assert len(weights) == 1
    path = tmp_path_factory.mktemp("resumed")
    argv = R.driver_argv(model, path, loader, extra=extra) + [
        "--restore_path", os.path.join(a["dir"], weights[0]),
        "--resume_state", os.path.join(a["dir"], "train_state_step%d.pth" % k)]
    with monkeypatch.context() as mp:
        for name, v in env.items():
            mp.setenv(name, v)
        b = _driver_run(mp, model, argv, seed=99)   # (other initial weights and torch stream: both are restored)
    assert len(b["steps"]) == R.STEPS - k
    for i, (x, y) in enumerate(zip(a["steps"][k:], b["steps"])):
        assert x == y, "step %d: straight %r, resumed %r" % (k + 1 + i, x, y)
    assert a["vals"][-len(b["vals"]):] == b["vals"] and b["vals"]
    assert a["counters"] == b["counters"]
    assert _same(a["scheduler"], b["scheduler"], "scheduler") is None
    assert _same(a["weights"], b["weights"], "state_dict") is None
    assert b["flat"] and a["t"] == b["t"] and torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"])
    assert _same(a["sampler"], b["sampler"], "sampler_state") is None and a["sampler"] is not None
    assert b["captured"] == a["captured"] and b["buffers"] == a["buffers"]
    # every file the resumed run wrote, the straight run wrote too, with the same content
    later = [f for f in _files(a["dir"]) if int(re.search(r"step(\d+)", f).group(1)) > k]
    assert _files(str(path)) == later and later
    for f in later:
        fa = torch.load(os.path.join(a["dir"], f), map_location="cpu", weights_only=False)
        fb = torch.load(os.path.join(str(path), f), map_location="cpu", weights_only=False)
        assert _same(fa, fb, f) is None


@gpu
def test_an_unseeded_stream_is_not_stored_and_the_driver_says_so_once(hip_device, monkeypatch, tmp_path, capsys):
    """Without --data_seed there is no stream to continue: the state holds None, the saving run says so in one line when
    it starts, the resumed run in one line when it loads the state, and both go on as they did before."""
    argv = [a for a in R.driver_argv("LarvaNet", tmp_path, "device", steps=2) if not a.startswith("--data_seed")]
    a = _driver_run(monkeypatch, "LarvaNet", argv, R.INIT_SEED)
    out = capsys.readouterr().out
    assert out.count("WARNING") == 1 and "restarts the patch stream" in out
    assert a["counters"][0] == 2 and a["sampler"] is None
    state = os.path.join(str(tmp_path), "train_state_step2.pth")
    assert torch.load(state, map_location="cpu", weights_only=False)["train_loader"] is None
    argv[argv.index("--max_steps=2")] = "--max_steps=3"
    b = _driver_run(monkeypatch, "LarvaNet", argv + ["--restore_path", os.path.join(str(tmp_path), "model_step2_vol0G.pth"),
                                                     "--resume_state", state], seed=99)
    out = capsys.readouterr().out
    assert out.count("WARNING") == 1 and "The patch stream restarts" in out
    assert b["counters"][0] == 3 and len(b["steps"]) == 1 and np.isfinite(b["steps"][0]["loss"])


@gpu
@pytest.mark.parametrize("case", ["1-sync", "4-v2-every-step"])
def test_driver_run_follows_the_float64_oracle(hip_device, case, monkeypatch, tmp_path_factory):
    model = CASES[case][0]
    a = _straight(case, monkeypatch, tmp_path_factory)
    rec, w64 = R.oracle_run(model, torch.float64)
    _, w32 = R.oracle_run(model, torch.float32)
    assert a["captured"] and a["buffers"]   # the sampler wrote the batches in place into the captured step's inputs
    assert [s["lr"] for s in a["steps"]] == rec["lrs"]
    assert [s["global_step"] for s in a["steps"]] == list(range(1, R.STEPS + 1))
    assert [s["total_volume"] for s in a["steps"]] == rec["total_volume"]
    assert [s["temp_volume"] for s in a["steps"]] == rec["temp_volume"]
    assert [v[0] for v in a["vals"]] == rec["val_steps"]
    names = sorted((f for f in _files(a["dir"]) if f.startswith("model_step")), key=lambda f: int(re.search(r"step(\d+)", f).group(1)))
    assert names == list(dict.fromkeys(rec["ckpt_names"]))   # (V2 saves step 1 once under one name)
    assert [f for f in _files(a["dir"]) if f.startswith("train_state")] == \
        sorted("train_state_step%d.pth" % s for s in set(rec["val_steps"][1:]))
    loss_err = max(abs(s["loss"] - r) / abs(r) for s, r in zip(a["steps"], rec["losses"]))
    psnr_err = max(abs(v[1] - r) for v, r in zip(a["vals"], rec["psnrs"]))
    d32, f32 = R.weight_distance(w32, w64)
    d, f = R.weight_distance(a["weights"], w64)
    print("%s: loss %.3e rel, psnr %.3e dB; weights: fp32 CPU d32 %.3e f32 %.3e, device %.3e %.3e (bars %.3e %.3e)"
          % (model, loss_err, psnr_err, d32, f32, d, f, 4 * d32, 4 * f32 + 1e-3))
    assert loss_err <= R.LOSS_BAR and psnr_err <= R.PSNR_BAR
    # the last checkpoint holds the final weights (both runs save at step 12)
    last = torch.load(os.path.join(a["dir"], names[-1]), map_location="cpu")
    assert _same(last, a["weights"], names[-1]) is None
    assert d <= 4 * d32 and f <= 4 * f32 + 1e-3


# ================================================================ GPU: hand-over and cross-path resume (eager, plugin level)
class _Val:
    def get_num_images(self):
        return R.VAL_IMAGES

    def get_image_pair(self, image_index, scale):
        lr, hr = R.val_pairs(scale)[image_index]
        return lr, hr, "val%d" % image_index


def _eager_plugin(seed):
    m = V1.create_model()
    m.parse_args(R.TINY)
    torch.manual_seed(seed)
    m.prepare(is_training=True, scales=[4])
    m.use_hip_graph = False
    return m


def _check_against_float64(what, losses, weights, steps):
    fb = R.fixed_batch()
    l64, w64 = R.adamw_run("LarvaNet", torch.float64, fb, [4e-4] * steps)
    _, w32 = R.adamw_run("LarvaNet", torch.float32, fb, [4e-4] * steps)
    d32, f32 = R.weight_distance(w32, w64)
    d, f = R.weight_distance(weights, w64)
    loss_err = max(abs(a - b) / abs(b) for a, b in zip(losses, l64[-len(losses):]))
    print("%s: loss %.3e rel; weights: fp32 CPU d32 %.3e f32 %.3e, device %.3e %.3e (bars %.3e %.3e)"
          % (what, loss_err, d32, f32, d, f, 4 * d32, 4 * f32 + 1e-3))
    assert loss_err <= R.STEP_LOSS_BAR
    assert d <= 4 * d32 and f <= 4 * f32 + 1e-3


@gpu
def test_flat_to_torch_handover_mid_run_and_cross_path_resume(hip_device, tmp_path):
    """Three flat steps, one parameter's .grad replaced by a fresh tensor (how a bucket ends), three steps on torch's
    path with the moments handed over: six float64 AdamW steps.  Then that run's per-tensor state loaded into a fresh
    flat plugin and two flat steps: eight."""
    x, t = (v.to(hip_device) for v in R.fixed_batch()[0])
    args = types.SimpleNamespace(train_path=str(tmp_path))
    m = _eager_plugin(R.INIT_SEED)
    n_params = len(list(m.model.parameters()))
    losses = [m.train_step_larva(args, _Val(), x, t) for _ in range(3)]
    assert m.grad_bucket is not None and not m.optim.state and m.optim._t == 3 and m.optim._flat_p is not None
    p = m.model.body_1.res_blocks[0].body[2].weight
    p.grad = p.grad.clone()
    losses += [m.train_step_larva(args, _Val(), x, t) for _ in range(3)]
    assert m.grad_bucket is None and len(m.optim.state) == n_params and m.optim._flat_p is None
    assert all(float(s["step"]) == 6.0 for s in m.optim.state.values())
    _check_against_float64("hand-over after 3 of 6", losses, m.model.state_dict(), 6)

    wpath, spath = m.save(str(tmp_path)), m.save_training_state(str(tmp_path))
    assert torch.load(spath, map_location="cpu", weights_only=False)["optimizer"]["flat"] is False
    c = _eager_plugin(99)
    c.restore(wpath)
    c.restore_training_state(spath)
    assert c.global_step == 6 and c.optim._t == 6 and c.optim._flat_p is not None and not c.optim.state
    assert float(c.optim._v.max()) > 0
    more = [c.train_step_larva(args, _Val(), x, t) for _ in range(2)]
    assert c.grad_bucket is not None and not c.optim.state and c.optim._t == 8   # the two steps were flat launches
    _check_against_float64("per-tensor state into a flat optimizer, 2 more of 8", more, c.model.state_dict(), 8)
