"""Benchmark metrics on the device (csrc/larva_metrics.hip, kernels.u8_metrics, evaluate_u8_tensor on the plugins,
pipeline.evaluate_stream): exact squared error / PSNR and the Gaussian-window SSIM on the Y channel or on RGB, over a
shaved window of two uint8 HWC images.  Host definitions run anywhere; kernels and networks are marked gpu.

The SSIM oracle is tests/metrics_ref.py (float64, scipy's gaussian_filter as skimage calls it).  Bar: |device - float64|
<= 2e-5 per image -- the driver prints four decimals, so the error must stay well below 5e-5, and an fp32 evaluation of
the same arithmetic sits at 3e-6 .. 4e-6.  The kernel as built sums the moments in double (a numpy statement of the same
valid-window sums is within 1e-15 of the oracle); the bar stays where the protocol puts it.  The GPU tests print each
figure before they assert; their measured maximum is not recorded yet.  Squared errors are compared as
integers."""
import importlib
import os

import numpy as np
import pytest
import torch

import metrics_ref

SSIM_BAR = 2e-5
BLOCKS = (2, 2, 2, 2)


def _model(name="LarvaNet", extra=(), precision="fp32", blocks=BLOCKS, scale=4):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks)),
                  "--precision=" + precision] + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[scale])
    m.strict_graph = True
    return m


def _blocks_image(seed, h, w):
    """uint8 (h, w, 3): hard-edged 8 x 8 blocks, every block and colour drawn from {0, 64, 200, 255}."""
    rng = np.random.default_rng(seed)
    levels = np.array([0, 64, 200, 255], np.uint8)
    grid = levels[rng.integers(0, 4, ((h + 7) // 8, (w + 7) // 8, 3))]
    return np.ascontiguousarray(np.repeat(np.repeat(grid, 8, 0), 8, 1)[:h, :w])


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _smooth_saturated(seed, h, w, jitter):
    """Smooth waves stretched past both ends of the range and clipped: flat 0 and 255 areas (where E[x^2] - E[x]^2
    cancels to nothing) between smooth slopes; `jitter` levels of seeded noise on top before the clip."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        fy, fx, ph = rng.uniform(0.01, 0.06), rng.uniform(0.01, 0.06), rng.uniform(0, 6.28)
        img[:, :, c] = 127.5 + 230.0 * np.sin(fy * yy + ph) * np.cos(fx * xx - ph)
    img += rng.uniform(-jitter, jitter, img.shape)
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- host
def test_metrics_source_is_built_and_the_workspace_helper_sizes_and_refuses():
    from larvanet_amd import build, hip_lib
    assert "larva_metrics.hip" in build.SOURCES
    if not os.path.exists(hip_lib.LIB_PATH):
        build.build_extension(verbose=False)
    lib = hip_lib.load()
    # the size helper is host code: 16 bytes per workgroup, refusals as -1
    assert lib.larva_u8_metrics_workspace_bytes(11, 11, 1) == 16
    assert lib.larva_u8_metrics_workspace_bytes(11, 11, 0) == 48
    assert lib.larva_u8_metrics_workspace_bytes(1356, 2040, 0) >= 16 * 3 * (1346 // 22) * (2030 // 32)
    for bad in ((0, 11, 0), (11, 0, 0), (11, 11, 2), (1 << 20, 11, 0)):
        assert lib.larva_u8_metrics_workspace_bytes(*bad) == -1


def test_rgb_to_y_u8_is_the_integer_rule_on_all_triples():
    """All 2^24 colour triples: the integer rule against an independent int64 statement of it, and against the float64
    formula of the float protocol (rgb / 255 @ [65.481, 128.553, 24.966] + 16, np.round), which lands on the other side of
    an exact tie at no more than 35 triples, one level each."""
    from larvanet_amd.metrics import rgb_to_y_u8
    differ = 0
    ties = 0
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], -1)
        got = rgb_to_y_u8(rgb)
        assert got.dtype == np.uint8 and got.shape == (256, 256)
        n = 65481 * np.int64(r) + 128553 * g.astype(np.int64) + 24966 * b.astype(np.int64)
        twice = 2 * n + 255000                       # floor((2 n + d) / 2 d) rounds half up ...
        up = twice // 510000
        tie = twice % 510000 == 0
        want = 16 + np.where(tie & (up % 2 == 1), up - 1, up)   # ... and an exact tie goes to the even neighbour
        assert np.array_equal(got.astype(np.int64), want), r
        ties += int(tie.sum())
        f = np.round((rgb.astype(np.float64) / 255.0) @ np.array([65.481, 128.553, 24.966]) + 16.0)
        d = f.astype(np.int64) - got.astype(np.int64)
        assert np.abs(d).max() <= 1
        assert not (d != 0)[~tie].any(), r           # (they differ at exact ties only)
        differ += int((d != 0).sum())
    assert ties == 194
    assert differ <= 35
    assert rgb_to_y_u8(np.array([[0, 0, 0], [255, 255, 255]], np.uint8)).tolist() == [16, 235]


def test_shave_and_psnr_from_sse():
    from larvanet_amd.metrics import psnr_from_sse, shave
    a = np.arange(7 * 9 * 3).reshape(7, 9, 3)
    assert shave(a, 0) is a and np.array_equal(shave(a, 2), a[2:5, 2:7]) and shave(a[:, :, 0], 3).shape == (1, 3)
    with pytest.raises(ValueError):
        shave(a, -1)
    assert psnr_from_sse(0, 10) == float("inf")
    assert abs(psnr_from_sse(65025 * 10, 10)) < 1e-12 and abs(psnr_from_sse(10, 10) - 20 * np.log10(255.0)) < 1e-12
    assert abs(psnr_from_sse(540_000_000_000, 1356 * 2040 * 3) - 10 * np.log10(65025 * 1356 * 2040 * 3 / 5.4e11)) < 1e-12
    with pytest.raises(ValueError):
        psnr_from_sse(1, 0)


def test_metric_window_refuses_on_the_host():
    from larvanet_amd import kernels as K
    assert K.metric_window((40, 50), (40, 50), 0, True) == (0, 0, 40, 50)
    assert K.metric_window((40, 50), (43, 57), 4, True) == (4, 4, 32, 42)
    assert K.metric_window((19, 19), (19, 19), 4, True) == (4, 4, 11, 11)
    assert K.metric_window((12, 12), (12, 12), 4, False) == (4, 4, 4, 4)
    for out, truth, shave, ssim in (((40, 50), (39, 50), 0, True), ((40, 50), (40, 49), 0, False), ((40, 50), (40, 50), -1, True),
                                    ((18, 40), (18, 40), 4, True), ((40, 10), (40, 10), 0, True), ((8, 8), (8, 8), 4, False)):
        with pytest.raises(ValueError):
            K.metric_window(out, truth, shave, ssim)


@pytest.mark.parametrize("name", ["LarvaNet", "LarvaNetV2", "LarvaLeg", "LarvaLegV2"])
def test_plugins_refuse_bad_evaluate_arguments_before_device_work(name):
    """Without a GPU nothing below may reach a kernel: every bad argument is refused on the host."""
    from larvanet_amd import kernels as K, pipeline
    extra = ("--leg=2",) if name.startswith("LarvaLeg") else ()
    m = _model(name, extra, blocks=(1, 1))
    x = torch.zeros(1, 8, 12, 3, dtype=torch.uint8)
    t = torch.zeros(1, 32, 48, 3, dtype=torch.uint8)
    with pytest.raises(TypeError):
        m.evaluate_u8_tensor(x.float(), t)
    with pytest.raises(TypeError):
        m.evaluate_u8_tensor(x, t.float())
    with pytest.raises(ValueError):
        m.evaluate_u8_tensor(x, t[0])
    with pytest.raises(RuntimeError):
        m.evaluate_u8_tensor(x, t)                       # CPU tensors
    with pytest.raises(TypeError):
        K.u8_metrics(t[0].float(), t[0], 4, "y")
    with pytest.raises(RuntimeError):
        K.u8_metrics(t[0], t[0], 4, "y")                 # CPU tensors
    with pytest.raises(ValueError):
        K.u8_metrics(t[0], t[0], 4, "luma")
    lr = np.zeros((8, 12, 3), np.uint8)
    for kwargs in ({"depth": 0}, {"shave": -1}, {"channel": "ycbcr"}):
        with pytest.raises(ValueError):
            pipeline.evaluate_stream(m, [(lr, t[0].numpy())], 4, **kwargs)
    with pytest.raises(ValueError):
        pipeline.evaluate_stream(m, [(lr, t[0].numpy())], 2)


# ---------------------------------------------------------------- kernels (GPU)
def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _device_metrics(out, truth, shave, channel, device, ssim=True):
    from larvanet_amd import kernels as K
    return K.metrics_from_record(K.u8_metrics(_dev(out, device), _dev(truth, device), shave, channel, ssim).cpu())


@pytest.mark.gpu
def test_y_conversion_and_squared_error_are_exact_on_every_colour_triple(hip_device):
    """4096 x 4096: every colour triple once, against a seeded permutation of the same image."""
    from larvanet_amd.metrics import rgb_to_y_u8
    v = np.arange(1 << 24, dtype=np.uint32)
    a = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    b = np.ascontiguousarray(a.reshape(-1, 3)[np.random.default_rng(5).permutation(1 << 24)].reshape(4096, 4096, 3))
    d_rgb = int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    d_y = int(((rgb_to_y_u8(a).astype(np.int64) - rgb_to_y_u8(b).astype(np.int64)) ** 2).sum())
    assert d_rgb > 1 << 32
    for shave in (0, 3):
        want_rgb, want_y = d_rgb, d_y
        if shave:
            wa, wb = a[3:-3, 3:-3], b[3:-3, 3:-3]
            want_rgb = int(((wa.astype(np.int64) - wb.astype(np.int64)) ** 2).sum())
            want_y = int(((rgb_to_y_u8(wa).astype(np.int64) - rgb_to_y_u8(wb).astype(np.int64)) ** 2).sum())
        for ssim in (False, True):   # (both tilings of the squared error)
            got = _device_metrics(a, b, shave, "rgb", hip_device, ssim=ssim)
            print("rgb shave %d ssim %s: sse %d (want %d)" % (shave, ssim, got["sse"], want_rgb))
            assert got["sse"] == want_rgb and got["n"] == 3 * (4096 - 2 * shave) ** 2
            got = _device_metrics(a, b, shave, "y", hip_device, ssim=ssim)
            print("y   shave %d ssim %s: sse %d (want %d)" % (shave, ssim, got["sse"], want_y))
            assert got["sse"] == want_y and got["n"] == (4096 - 2 * shave) ** 2
    same = _device_metrics(a, a, 0, "rgb", hip_device, ssim=False)
    assert same["sse"] == 0 and same["psnr"] == float("inf") and same["ssim"] is None


# (out h, out w, truth h, truth w, shave): windows of 11 x 11 (one sample), 11 x 40, 37 x 12, odd sizes, x0 / y0 / pitches
# that are not multiples of 4, a truth larger than the output, tile edges of the kernel (22 x 32 samples per workgroup)
SHAPES = [(11, 11, 11, 11, 0), (19, 19, 19, 19, 4), (11, 40, 11, 40, 0), (37, 12, 37, 12, 0), (17, 46, 20, 49, 3),
          (43, 53, 43, 53, 0), (43, 53, 45, 54, 2), (64, 64, 64, 64, 4), (32, 42, 32, 42, 0), (33, 43, 33, 43, 0),
          (54, 74, 54, 74, 0), (55, 75, 61, 80, 0), (131, 97, 140, 101, 3), (97, 203, 97, 203, 4), (97, 203, 97, 203, 2)]


def _pair(kind, seed, oh, ow, th, tw):
    if kind == "noise":
        return _noise(seed, oh, ow), _noise(seed + 1, th, tw)
    if kind == "saturated":
        truth = _smooth_saturated(seed, th, tw, 0.0)
        out = _smooth_saturated(seed, th, tw, 6.0)[:oh, :ow]
        return np.ascontiguousarray(out), truth
    truth = _smooth_saturated(seed, th, tw, 3.0)
    return np.ascontiguousarray(truth[:oh, :ow]), truth


@pytest.mark.gpu
@pytest.mark.parametrize("channel", ["y", "rgb"])
@pytest.mark.parametrize("kind", ["noise", "saturated", "self"])
def test_ssim_and_psnr_equal_the_float64_oracle(hip_device, kind, channel):
    worst = 0.0
    for i, (oh, ow, th, tw, shave) in enumerate(SHAPES):
        out, truth = _pair(kind, 100 + i, oh, ow, th, tw)
        want = metrics_ref.evaluate(out, truth, shave, channel)
        got = _device_metrics(out, truth, shave, channel, hip_device)
        err = abs(got["ssim"] - want["ssim"])
        worst = max(worst, err)
        print("%s %s %s shave %d: ssim %.15f (float64 %.15f, |d| %.3g), sse %d" %
              (kind, channel, (oh, ow, th, tw), shave, got["ssim"], want["ssim"], err, got["sse"]))
        assert got["sse"] == want["sse"] and got["n"] == want["n"]
        assert got["psnr"] == want["psnr"]
        assert err <= SSIM_BAR
        if kind == "self":
            assert got["ssim"] == 1.0 and got["psnr"] == float("inf")   # (IEEE division of equal roundings)
        no_ssim = _device_metrics(out, truth, shave, channel, hip_device, ssim=False)
        assert no_ssim["sse"] == want["sse"] and no_ssim["ssim"] is None
    print("max |device - float64| over %s / %s: %.3g" % (kind, channel, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("channel,shave", [("rgb", 0), ("y", 4)])
def test_one_div2k_sized_pair(hip_device, channel, shave):
    truth = _smooth_saturated(7, 1356, 2040, 2.0)
    out = np.clip(_smooth_saturated(7, 1356, 2040, 0.0).astype(np.int16) + _noise(8, 1356, 2040) % 7 - 3, 0, 255).astype(np.uint8)
    want = metrics_ref.evaluate(out, truth, shave, channel)
    got = _device_metrics(out, truth, shave, channel, hip_device)
    print("1356 x 2040 %s: ssim %.15f (float64 %.15f, |d| %.3g), psnr %.9f" %
          (channel, got["ssim"], want["ssim"], abs(got["ssim"] - want["ssim"]), got["psnr"]))
    assert got["sse"] == want["sse"] and abs(got["ssim"] - want["ssim"]) <= SSIM_BAR


@pytest.mark.gpu
def test_results_are_bitwise_reproducible_across_calls_and_streams(hip_device):
    from larvanet_amd import kernels as K
    out, truth = _pair("saturated", 3, 211, 317, 215, 320)
    o, t = _dev(out, hip_device), _dev(truth, hip_device)
    for channel in ("y", "rgb"):
        first = K.u8_metrics(o, t, 3, channel).cpu()
        again = K.u8_metrics(o, t, 3, channel).cpu()
        assert torch.equal(first, again)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            other = K.u8_metrics(o, t, 3, channel)
        side.synchronize()
        assert torch.equal(first, other.cpu())


@pytest.mark.gpu
def test_refusals_come_before_any_launch(hip_device):
    from larvanet_amd import kernels as K
    t = _dev(_noise(1, 40, 50), hip_device)
    for args in ((t, t[:39].contiguous(), 0, "y"), (t, t, -1, "y"), (t[:18].contiguous(), t[:18].contiguous(), 4, "y"),
                 (t, t, 0, "cmyk")):
        with pytest.raises(ValueError):
            K.u8_metrics(*args)
    with pytest.raises(TypeError):
        K.u8_metrics(t.float(), t, 0, "y")
    with pytest.raises(RuntimeError):
        K.u8_metrics(t.cpu(), t, 0, "y")
    with pytest.raises(RuntimeError):
        K.u8_metrics(t[:, ::2], t, 0, "y")               # not contiguous
    assert K.metrics_from_record(K.u8_metrics(t[:12].contiguous(), t, 4, "y", ssim=False).cpu())["n"] == 4 * 42


# ---------------------------------------------------------------- networks (GPU)
def _truth_for(lr, scale, seed, extra=(0, 0)):
    """A truth for the upscaled `lr`: its pixels repeated, seeded noise on top, `extra` more rows / columns."""
    h, w = lr.shape[0] * scale + extra[0], lr.shape[1] * scale + extra[1]
    big = np.repeat(np.repeat(lr, scale, 0), scale, 1).astype(np.int16)
    big = np.pad(big, ((0, extra[0]), (0, extra[1]), (0, 0)), mode="edge")
    jitter = np.random.default_rng(seed).integers(-20, 21, (h, w, 3))
    return np.clip(big + jitter, 0, 255).astype(np.uint8)


def _eval_pairs(scale):
    sizes = [(40, 56), (33, 47), (40, 56), (21, 90), (33, 47), (40, 56), (64, 64), (33, 47)]
    lrs = [_blocks_image(900 + i, h, w) for i, (h, w) in enumerate(sizes)]
    return [(a, _truth_for(a, scale, 50 + i, extra=(i % 3, (2 * i) % 5))) for i, a in enumerate(lrs)]


NETWORKS = [("LarvaNet", ()), ("LarvaNetV2", ()), ("LarvaLeg", ("--leg=2",))]
CASES = [(name, extra, precision, 4) for name, extra in NETWORKS for precision in ("fp32", "fp16")]
CASES += [(name, extra, "fp32", scale) for name, extra in NETWORKS for scale in (2, 3)]


def _same(a, b):
    return a["sse"] == b["sse"] and a["n"] == b["n"] and a["psnr"] == b["psnr"] and a["ssim"] == b["ssim"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra,precision,scale", CASES, ids=lambda v: "".join(v) if isinstance(v, tuple) else str(v))
def test_evaluate_equals_metrics_of_upscale_u8_and_the_host_oracle(hip_device, name, extra, precision, scale):
    from larvanet_amd import kernels as K, pipeline
    pairs = _eval_pairs(scale)
    one = _model(name, extra, precision, scale=scale)
    for channel, shave in (("y", None), ("rgb", 0)):
        eff = scale if shave is None else shave
        images = [one.upscale_u8([lr], scale)[0] for lr, _ in pairs]
        want = []
        for (lr, truth), image in zip(pairs, images):
            sr = one.upscale_u8_tensor(_dev(lr[None], hip_device))
            assert np.array_equal(sr[0].cpu().numpy(), image)
            direct = K.metrics_from_record(K.u8_metrics(sr[0], _dev(truth, hip_device), eff, channel).cpu())
            host = metrics_ref.evaluate(image, truth, eff, channel)
            assert direct["sse"] == host["sse"] and abs(direct["psnr"] - host["psnr"]) <= 1e-9
            assert abs(direct["ssim"] - host["ssim"]) <= SSIM_BAR
            want.append(direct)
        m = _model(name, extra, precision, scale=scale)
        for (lr, truth), w in zip(pairs, want):
            got = m.evaluate_u8_tensor(_dev(lr[None], hip_device), _dev(truth[None], hip_device), shave=shave, channel=channel)
            assert len(got) == 1 and _same(got[0], w)
        for depth in (1, 2):
            m = _model(name, extra, precision, scale=scale)
            got = list(pipeline.evaluate_stream(m, iter(pairs), scale, shave=shave, channel=channel, depth=depth))
            assert len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want)), depth
            kept = list(pipeline.evaluate_stream(m, pairs, scale, shave=shave, channel=channel, depth=depth, keep_images=True))
            streamed = list(pipeline.upscale_stream(_model(name, extra, precision, scale=scale), [lr for lr, _ in pairs],
                                                    scale, depth=depth))
            for (g, image), w, s in zip(kept, want, streamed):
                assert _same(g, w) and image.dtype == np.uint8 and np.array_equal(image, s)
        psnr_only = list(pipeline.evaluate_stream(m, pairs, scale, shave=shave, channel=channel, ssim=False))
        assert all(p["ssim"] is None and p["sse"] == w["sse"] for p, w in zip(psnr_only, want))


@pytest.mark.gpu
def test_evaluate_takes_batches(hip_device):
    m = _model("LarvaNet")
    lrs = [_blocks_image(40 + i, 24, 36) for i in range(3)]
    truths = [_truth_for(a, 4, i) for i, a in enumerate(lrs)]
    got = m.evaluate_u8_tensor(_dev(np.stack(lrs), hip_device), _dev(np.stack(truths), hip_device))
    images = m.upscale_u8(lrs, 4)
    for g, image, truth in zip(got, images, truths):
        want = metrics_ref.evaluate(image, truth, 4, "y")
        assert g["sse"] == want["sse"] and abs(g["ssim"] - want["ssim"]) <= SSIM_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_graph_tables_are_unchanged_by_evaluate_calls(hip_device, precision):
    from larvanet_amd import pipeline
    m = _model("LarvaNet", precision=precision)
    fresh = _model("LarvaNet", precision=precision)
    for h, w in ((64, 64), (37, 127)):
        a = _blocks_image(7 + h, h, w)
        truth = _truth_for(a, 4, 1)
        chw = np.ascontiguousarray(a.transpose(2, 0, 1))
        for _ in range(3):
            m.evaluate_u8_tensor(_dev(a[None], hip_device), _dev(truth[None], hip_device))
            fresh.upscale_u8_tensor(_dev(a[None], hip_device))
        assert len(list(pipeline.evaluate_stream(m, [(a, truth)] * 2, 4))) == 2
        assert len(list(pipeline.upscale_stream(fresh, [a] * 2, 4))) == 2
        for call in range(3):
            assert np.array_equal(m.upscale([chw], 4), fresh.upscale([chw], 4)), (h, w, call)
        assert np.array_equal(m.upscale_u8([a], 4), fresh.upscale_u8([a], 4))
    assert set(m._infer_graphs) == set(fresh._infer_graphs)
    assert set(m._infer_graphs_u8) == set(fresh._infer_graphs_u8) and m._infer_graphs_u8


@pytest.mark.gpu
def test_evaluate_stream_is_bitwise_reproducible(hip_device):
    from larvanet_amd import pipeline
    pairs = _eval_pairs(4)
    m = _model("LarvaNet")
    first = list(pipeline.evaluate_stream(m, pairs, 4, channel="rgb", shave=0))
    again = list(pipeline.evaluate_stream(m, pairs, 4, channel="rgb", shave=0, depth=1))
    assert all(_same(a, b) for a, b in zip(first, again))


@pytest.mark.gpu
def test_evaluate_stream_refuses_a_small_truth_and_raises_fp16_overflow_at_the_right_image(hip_device):
    from larvanet_amd import pipeline
    pairs = _eval_pairs(4)[:6]
    m = _model("LarvaNet", precision="fp16")
    want = list(pipeline.evaluate_stream(m, pairs, 4))
    bad_at = 3

    def feed():
        for i, pair in enumerate(pairs):
            if i == bad_at:
                with torch.no_grad():
                    m.model.head.feature_extraction.weight.mul_(1e4)   # head output >> 65504
                m.model.invalidate_packed_weights()
            yield pair

    for depth in (1, 2):
        m = _model("LarvaNet", precision="fp16")
        got = []
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            for g in pipeline.evaluate_stream(m, feed(), 4, depth=depth):
                got.append(g)
        assert len(got) == bad_at and all(_same(g, w) for g, w in zip(got, want)), depth
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            m.evaluate_u8_tensor(_dev(pairs[0][0][None], hip_device), _dev(pairs[0][1][None], hip_device))
    m = _model("LarvaNet")
    small = [(pairs[0][0], pairs[0][1][:-8])]
    with pytest.raises(ValueError, match="smaller than the output"):
        list(pipeline.evaluate_stream(m, small, 4))
    with pytest.raises(ValueError, match="at least 11"):
        list(pipeline.evaluate_stream(m, [(pairs[0][0][:4, :4], pairs[0][1])], 4))
