"""The 8-bit image path: uint8 HWC images in, uint8 HWC images out (kernels.u8_hwc_to_f32_chw / f32_chw_to_u8_hwc, the
fp16 leg end's uint8 epilogue, upscale_u8 / upscale_u8_tensor on the four plugins, pipeline.upscale_stream,
larvanet_amd.upscale_images).  Host logic runs anywhere; kernels and networks are marked gpu.

Every GPU comparison is exact (np.array_equal).  The contract:
    upscale_u8([a], s)[0] == image_to_uint8(upscale([a.transpose(2, 0, 1)], s)[0]).transpose(1, 2, 0)
at the same --precision: uint8 -> fp32 is exact, the same kernels run on the same fp32 image, and the device rounds
(half to even) and clamps as numpy does.

Network inputs are seeded images of hard-edged 8 x 8 blocks drawn from {0, 64, 200, 255}.  With the seed-0 initial
weights a float64 CPU forward (torch operators, the plugins' own state_dict) puts 5 - 13 % of the HR values below -0.5
and 4 - 13 % above 255.5 for every case below that has a network or a bicubic base (V1, V2, --leg=2, --num_filters 32,
bilinear base with a network, bicubic --leg=0; x2 / x3 / x4; 64 x 64, 37 x 127, 339 x 510), so both clamps act; the tests
assert a share of at least 1 % each on the float output as a condition on the input."""
import importlib

import numpy as np
import pytest
import torch

PLUGINS = ("LarvaNet", "LarvaNetV2", "LarvaLeg", "LarvaLegV2")
BLOCKS = (4, 4, 4, 4)


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


# ---------------------------------------------------------------- host
@pytest.mark.parametrize("name", PLUGINS)
def test_plugins_have_the_u8_entry_points_and_check_arguments_before_device_work(name):
    """On a machine without a GPU nothing below may reach a kernel: every bad argument is refused on the host."""
    extra = ("--leg=2",) if name.startswith("LarvaLeg") else ()
    m = _model(name, extra, blocks=(1, 1))
    assert callable(m.upscale_u8) and callable(m.upscale_u8_tensor)
    good = _blocks_image(1, 8, 12)
    with pytest.raises(TypeError):
        m.upscale_u8([good.astype(np.float32)], 4)
    with pytest.raises(ValueError):
        m.upscale_u8([np.ascontiguousarray(good.transpose(2, 0, 1))], 4)   # CHW
    with pytest.raises(ValueError):
        m.upscale_u8([good, _blocks_image(2, 8, 16)], 4)                   # mixed shapes
    for bad_scale in (2, 3, 8):
        with pytest.raises(ValueError):
            m.upscale_u8([good], bad_scale)
    with pytest.raises(ValueError):
        m.upscale_u8([], 4)
    with pytest.raises(TypeError):
        m.upscale_u8_tensor(torch.zeros(1, 8, 12, 3))                      # float tensor
    with pytest.raises(ValueError):
        m.upscale_u8_tensor(torch.zeros(1, 3, 8, 12, dtype=torch.uint8))   # CHW
    from larvanet_amd import pipeline
    with pytest.raises(ValueError):
        pipeline.upscale_stream(m, [good], 2)
    with pytest.raises(ValueError):
        pipeline.upscale_stream(m, [good], 4, depth=0)


# ---------------------------------------------------------------- kernels (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 4), (2, 48, 48), (1, 37, 127), (1, 339, 510), (1, 1, 1)])
def test_u8_hwc_to_f32_chw_is_exact(hip_device, shape):
    from larvanet_amd import kernels as K
    n, h, w = shape
    x = np.random.default_rng(h * 1000 + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    x.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)[:x.size]   # (every byte value, where the image is large enough)
    got = K.u8_hwc_to_f32_chw(torch.from_numpy(x).to(hip_device)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, x.transpose(0, 3, 1, 2).astype(np.float32))


def _crafted(n_values, seed):
    """Float values that decide a rounding or a clamp, then seeded noise on -64 .. 320, n_values in all."""
    ties = [k + 0.5 for k in range(-2, 257)]
    special = [0.0, -0.0, -0.49999997, 254.5, 255.49998, 255.5, 1e9, -1e9, float("inf"), float("-inf")]
    head = np.array(ties + special, np.float32)
    rng = np.random.default_rng(seed)
    out = (rng.random(n_values) * 384 - 64).astype(np.float32)
    reps = max(1, min(3, n_values // head.size))   # (at several offsets: every lane position of the 12-byte store)
    for r in range(reps):
        at = r * (head.size + 1)
        out[at:at + head.size] = head[:max(0, n_values - at)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("width", [1, 3, 5, 127, 510])
def test_f32_chw_to_u8_hwc_equals_image_to_uint8(hip_device, width, scale):
    from larvanet_amd import kernels as K
    from larvanet_amd.metrics import image_to_uint8
    ww = width * scale
    for n, hh in ((1, 7 * scale), (2, 5 * scale), (1, 1)):
        x = _crafted(n * 3 * hh * ww, ww * 100 + hh).reshape(n, 3, hh, ww)
        got = K.f32_chw_to_u8_hwc(torch.from_numpy(x).to(hip_device)).cpu().numpy()
        ref = image_to_uint8(x).transpose(0, 2, 3, 1)
        assert got.dtype == np.uint8 and np.array_equal(got, ref), (n, hh, ww)


@pytest.mark.gpu
def test_f32_chw_to_u8_hwc_tie_table(hip_device):
    """The crafted values on their own, against the answers written out: half to even, then the clamps."""
    from larvanet_amd import kernels as K
    vals = np.array([-2.5, -0.5, 0.5, 1.5, 2.5, 3.5, 254.5, 255.49998, 255.5, 256.5, -0.49999997, 0.0, -0.0, 1e9, -1e9,
                     float("inf"), float("-inf"), 127.5, 128.5, 64.4999], np.float32)
    want = np.array([0, 0, 0, 2, 2, 4, 254, 255, 255, 255, 0, 0, 0, 255, 0, 255, 0, 128, 128, 64], np.uint8)
    x = np.zeros((1, 3, 1, vals.size), np.float32)
    x[0, 1, 0] = vals
    got = K.f32_chw_to_u8_hwc(torch.from_numpy(x).to(hip_device)).cpu().numpy()
    assert np.array_equal(got[0, 0, :, 1], want) and not got[0, 0, :, 0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 4), (2, 48, 48), (1, 339, 510), (1, 37, 127)])
def test_fused_u8_leg_end_equals_the_pointwise_pass(hip_device, shape):
    from larvanet_amd import kernels as K
    n, h, w = shape
    rng = np.random.default_rng(11 + w)
    x = (rng.standard_normal((n, h, w, 48)) * 2).astype(np.float16)
    wt = (rng.standard_normal((48, 48, 3, 3)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(48) * 0.2).astype(np.float32)
    base = (rng.random((n, 3, 4 * h, 4 * w)) * 340 - 40).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)   # noqa: E731
    flag = torch.zeros(1, dtype=torch.int32, device=hip_device)
    wpk = K.f16_pack_weights(dev(wt))
    f32 = K.f16_conv3x3_shuffle_base(dev(x), wpk, dev(b), dev(base))
    want = K.f32_chw_to_u8_hwc(f32).cpu().numpy()
    got = K.f16_conv3x3_shuffle_base_u8(dev(x), wpk, dev(b), dev(base), flag).cpu().numpy()
    assert (want == 0).mean() > 0.05 and (want == 255).mean() > 0.05   # (both clamps act)
    assert got.shape == (n, 4 * h, 4 * w, 3) and np.array_equal(got, want)
    assert int(flag.item()) == 0
    base[0, 1, 4 * h - 1, 4 * w - 1] = np.nan   # a non-finite value raises the flag instead of becoming a byte silently
    K.f16_conv3x3_shuffle_base_u8(dev(x), wpk, dev(b), dev(base), flag)
    assert int(flag.item()) == 1


# ---------------------------------------------------------------- networks (GPU)
SIZES = ((64, 64), (37, 127), (339, 510))
NETWORKS = [("LarvaNet", ()), ("LarvaNetV2", ()), ("LarvaLeg", ("--leg=2",)), ("LarvaLeg", ("--leg=0",))]
CASES = [(name, extra, "fp32", scale) for name, extra in NETWORKS for scale in (2, 3, 4)]
CASES += [(name, extra, "fp16", 4) for name, extra in NETWORKS]
CASES += [("LarvaNet", ("--num_filters=32",), "fp32", 4), ("LarvaNet", ("--interpolate=bilinear",), "fp32", 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra,precision,scale", CASES, ids=lambda v: "".join(v) if isinstance(v, tuple) else str(v))
def test_upscale_u8_equals_image_to_uint8_of_upscale(hip_device, name, extra, precision, scale):
    from larvanet_amd.metrics import image_to_uint8
    mf = _model(name, extra, precision, scale=scale)
    mu = _model(name, extra, precision, scale=scale)
    for h, w in SIZES:
        for call in range(3):   # eager, capture, replay (339 x 510 runs eagerly every time)
            a = _blocks_image(h * 1000 + w + call, h, w)
            f = mf.upscale([np.ascontiguousarray(a.transpose(2, 0, 1))], scale)[0]
            assert (f < -0.5).mean() >= 0.01 and (f > 255.5).mean() >= 0.01, "the input does not exercise both clamps"
            want = image_to_uint8(f).transpose(1, 2, 0)
            got = mu.upscale_u8([a], scale)
            assert got.dtype == np.uint8 and got.shape == (1, scale * h, scale * w, 3)
            assert np.array_equal(got[0], want), (h, w, call)
            t = mu.upscale_u8_tensor(torch.from_numpy(a[None]).to(hip_device))
            assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy()[0], want), (h, w, call)
    keys = list(getattr(mu, "_infer_graphs_u8", {}))
    assert keys and all(k[2] == "u8" and k[1] == precision for k in keys)
    assert all(v is not False for v in mu._infer_graphs_u8.values())
    assert not getattr(mu, "_infer_graphs", None)   # the uint8 path captured nothing under the float path's keys


@pytest.mark.gpu
def test_upscale_u8_batches(hip_device):
    from larvanet_amd.metrics import image_to_uint8
    m = _model("LarvaNet", blocks=(2, 2))
    imgs = [_blocks_image(40 + i, 24, 36) for i in range(3)]
    want = image_to_uint8(m.upscale([np.ascontiguousarray(a.transpose(2, 0, 1)) for a in imgs], 4)).transpose(0, 2, 3, 1)
    assert np.array_equal(m.upscale_u8(imgs, 4), want)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_float_paths_are_unchanged_by_u8_calls(hip_device, precision):
    m = _model("LarvaNet", precision=precision)
    fresh = _model("LarvaNet", precision=precision)
    for h, w in ((64, 64), (37, 127)):
        a = _blocks_image(7 + h, h, w)
        chw = np.ascontiguousarray(a.transpose(2, 0, 1))
        for _ in range(3):
            m.upscale_u8([a], 4)
        for call in range(3):
            assert np.array_equal(m.upscale([chw], 4), fresh.upscale([chw], 4)), (h, w, call)
    assert set(m._infer_graphs) == set(fresh._infer_graphs)


# ---------------------------------------------------------------- the stream (GPU)
def _stream_inputs():
    """12 images of 5 sizes; two sizes come 4 times each with different content (capture, then replays)."""
    sizes = [(40, 56), (33, 47), (40, 56), (64, 64), (33, 47), (40, 56), (21, 90), (33, 47), (40, 56), (339, 510),
             (33, 47), (64, 64)]
    return [_blocks_image(500 + i, h, w) for i, (h, w) in enumerate(sizes)]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_upscale_stream_equals_upscale_u8_one_by_one(hip_device, precision):
    from larvanet_amd import pipeline
    images = _stream_inputs()
    assert len({a.shape for a in images}) == 5
    one = _model("LarvaNet", precision=precision)
    want = [one.upscale_u8([a], 4)[0] for a in images]
    for depth in (1, 2, 3):
        m = _model("LarvaNet", precision=precision)
        got = list(pipeline.upscale_stream(m, iter(images), 4, depth=depth))
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.uint8 and np.array_equal(g, w), (depth, i)
        assert len(m._infer_graphs_u8) >= 2   # (the repeated sizes were replayed, not only run eagerly)
    # the results are the caller's: a later image does not write into an earlier result
    m = _model("LarvaNet", precision=precision)
    kept = []
    for g in pipeline.upscale_stream(m, images, 4, depth=2):
        kept.append(g)
    assert all(np.array_equal(g, w) for g, w in zip(kept, want))


@pytest.mark.gpu
def test_fp16_overflow_raises_from_upscale_u8_and_from_the_stream_at_the_right_image(hip_device):
    from larvanet_amd import pipeline
    images = _stream_inputs()[:6]
    m = _model("LarvaNet", precision="fp16")
    want = [m.upscale_u8([a], 4)[0] for a in images]
    bad_at = 3

    def feed():
        for i, a in enumerate(images):
            if i == bad_at:
                with torch.no_grad():
                    m.model.head.feature_extraction.weight.mul_(1e4)   # head output >> 65504
                m.model.invalidate_packed_weights()
            yield a

    for depth in (1, 2, 3):
        m = _model("LarvaNet", precision="fp16")
        got = []
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            for g in pipeline.upscale_stream(m, feed(), 4, depth=depth):
                got.append(g)
        assert len(got) == bad_at and all(np.array_equal(g, w) for g, w in zip(got, want)), depth
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            m.upscale_u8([images[0]], 4)
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            m.upscale_u8_tensor(torch.from_numpy(images[0][None]).to(hip_device))
