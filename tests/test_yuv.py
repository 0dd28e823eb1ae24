"""The video path's colour conversions and entry points: image_utils.i420_to_rgb_f32 / rgb_u8_to_i420 (the exact integer
definition), kernels.i420_to_rgb_f32 / rgb_u8_to_i420 (csrc/larva_yuv.hip), upscale_yuv420 / upscale_yuv420_tensor on the
plugins and pipeline.upscale_yuv_stream.  Host logic runs anywhere; kernels and networks are marked gpu and every GPU
comparison is exact (np.array_equal) against the numpy definition."""
import gc
import importlib
import itertools
import os

import numpy as np
import pytest
import torch

from larvanet_amd import image_utils as U

PLUGINS = ("LarvaNet", "LarvaNetV2", "LarvaLeg", "LarvaLegV2")
COMBOS = list(itertools.product(("bt601", "bt709"), (False, True)))


def _collect():
    """A plugin holds its captured graphs in reference cycles, so a dropped model lives until the collector runs.  If that
    happens while another graph is being captured, the freed graph's destructor calls into the HIP runtime during the
    capture and the process aborts ("operation not permitted when stream is capturing").  Every model of this file is
    made after a collection, and a model is dropped (set to None) before its successor is made."""
    gc.collect()


def _model(name="LarvaNet", extra=(), precision="fp32", blocks=(2, 2), scale=4):
    _collect()
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks)),
                  "--precision=" + precision] + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[scale])
    m.strict_graph = True
    return m


def _frame(seed, w, h):
    """Random bytes over the full 0..255 range."""
    return np.random.default_rng(seed).integers(0, 256, U.i420_frame_bytes(w, h), dtype=np.uint8)


def _smooth_frame(seed, w, h):
    """A frame a network can take at fp16: a smooth luma ramp with mild noise, chroma near the centre."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = (40 + 150 * (xx + yy) / max(1, w + h - 2) + rng.integers(0, 12, (h, w))).astype(np.uint8)
    c = rng.integers(100, 156, 2 * ((w + 1) // 2) * ((h + 1) // 2)).astype(np.uint8)
    return np.concatenate([y.reshape(-1), c])


# ---------------------------------------------------------------- the float64 textbook evaluation
def _upsample_padded(c, w, h):
    """The centre-sited bilinear chroma at every luma pixel in float64, from a plane padded by its edge explicitly: luma
    pixel 2 i + a lies a quarter sample from chroma sample i, towards i - 1 (a = 0) or i + 1 (a = 1)."""
    p = np.pad(c.astype(np.float64), 1, mode="edge")
    out = np.empty((h, w))
    for y in range(h):
        i, dy = y // 2 + 1, (-1 if y % 2 == 0 else 1)
        for x in range(w):
            j, dx = x // 2 + 1, (-1 if x % 2 == 0 else 1)
            out[y, x] = (0.5625 * p[i, j] + 0.1875 * p[i, j + dx] + 0.1875 * p[i + dy, j] + 0.0625 * p[i + dy, j + dx])
    return out


def _to_rgb_f64(frame, w, h, matrix, full_range):
    y, u, v = U.i420_planes(frame, w, h)
    off, cy, crv, cgu, cgv, cbu = U.yuv_to_rgb_matrix(matrix, full_range)
    lum = (y.astype(np.float64) - off) * cy
    uu, vv = _upsample_padded(u, w, h) - 128.0, _upsample_padded(v, w, h) - 128.0
    return np.clip(np.stack([lum + crv * vv, lum + cgu * uu + cgv * vv, lum + cbu * uu]), 0.0, 255.0)


def _to_yuv_f64(img, matrix, full_range):
    """-> unrounded float64 (Y [H][W], U [ch][cw], V [ch][cw]), chroma from the mean of the 2 x 2 block of the image padded
    by its edge explicitly to even sides."""
    off, yr, ur, vr = U.rgb_to_yuv_matrix(matrix, full_range)
    a = img.astype(np.float64)
    y = off + a @ np.array(yr)
    p = np.pad(a, ((0, a.shape[0] % 2), (0, a.shape[1] % 2), (0, 0)), mode="edge")
    mean = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4.0
    return y, 128.0 + mean @ np.array(ur), 128.0 + mean @ np.array(vr)


# ---------------------------------------------------------------- host: the definition
@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_i420_to_rgb_f32_against_float64(matrix, full_range):
    table = U.yuv_to_rgb_table(matrix, full_range)
    exact = U.yuv_to_rgb_matrix(matrix, full_range)
    assert len(table) == U.YUV_TO_RGB_TABLE_WORDS and table[0] == exact[0]
    d = [abs(q / 4096.0 - k) for q, k in zip(table[1:], exact[1:])]
    # operands: |Y - offset| <= 255, |C - 128| <= 128; a plane is the luma term plus at most two chroma terms; the final
    # rounding to 1 / 256 adds half a step
    bar = 1.0 / 512 + d[0] * 255 + max(d[1], d[2] + d[3], d[4]) * 128
    assert bar < 0.1
    for w, h in ((16, 12), (7, 5), (1, 1)):
        f = _frame(w * 100 + h, w, h)
        got = U.i420_to_rgb_f32(f, w, h, matrix, full_range)
        assert got.dtype == np.float32 and got.shape == (3, h, w)
        assert np.array_equal(got * 256, np.rint(got * 256)) and got.min() >= 0 and got.max() <= 255
        err = np.abs(got.astype(np.float64) - _to_rgb_f64(f, w, h, matrix, full_range)).max()
        print("i420_to_rgb_f32", matrix, full_range, (w, h), "err", err, "bar", bar)
        assert err <= bar


@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_rgb_u8_to_i420_against_float64(matrix, full_range):
    table = U.rgb_to_yuv_table(matrix, full_range)
    off, *rows = U.rgb_to_yuv_matrix(matrix, full_range)
    assert len(table) == U.RGB_TO_YUV_TABLE_WORDS and table[0] == off
    span = 255 if full_range else 219
    assert sum(table[1:4]) == round(span / 255 * 65536) and sum(table[4:7]) == 0 and sum(table[7:10]) == 0
    # every operand (a byte, or the block mean S / 4) is at most 255; rounding to a byte adds 0.5
    bars = [0.5 + 255 * sum(abs(table[1 + 3 * r + c] / 65536.0 - rows[r][c]) for c in range(3)) for r in range(3)]
    assert max(bars) < 0.51
    for w, h in ((16, 12), (7, 5), (1, 1)):
        img = np.random.default_rng(w * 10 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        frame = U.rgb_u8_to_i420(img, matrix, full_range)
        assert frame.dtype == np.uint8 and frame.shape == (U.i420_frame_bytes(w, h),)
        for got, want, bar in zip(U.i420_planes(frame, w, h), _to_yuv_f64(img, matrix, full_range), bars):
            err = np.abs(got.astype(np.float64) - np.clip(want, 0, 255)).max()
            print("rgb_u8_to_i420", matrix, full_range, (w, h), "err", err, "bar", bar)
            assert got.shape == want.shape and err <= bar


@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_exactness_properties(matrix, full_range):
    w, h = 6, 4
    nc = 2 * 3 * 2
    for yv in range(256):   # U = V = 128: R = G = B
        rgb = U.i420_to_rgb_f32(np.concatenate([np.full(w * h, yv, np.uint8), np.full(nc, 128, np.uint8)]), w, h, matrix,
                                full_range)
        assert np.array_equal(rgb[0], rgb[1]) and np.array_equal(rgb[1], rgb[2]) and np.all(rgb == rgb[0, 0, 0])
        lo, hi = (0, 255) if full_range else (16, 235)
        if yv <= lo:
            assert rgb[0, 0, 0] == 0.0     # black, and what lies below it clamps
        if yv >= hi:
            assert rgb[0, 0, 0] == 255.0   # white, and what lies above it clamps
        if lo < yv < hi:
            assert 0.0 < rgb[0, 0, 0] < 255.0
    for g in range(256):   # grey RGB: U = V = 128 exactly
        frame = U.rgb_u8_to_i420(np.full((5, 3, 3), g, np.uint8), matrix, full_range)
        y, u, v = U.i420_planes(frame, 3, 5)
        assert np.all(u == 128) and np.all(v == 128) and np.all(y == y[0, 0])
    if not full_range:
        assert U.i420_planes(U.rgb_u8_to_i420(np.zeros((2, 2, 3), np.uint8), matrix, False), 2, 2)[0][0, 0] == 16
        assert U.i420_planes(U.rgb_u8_to_i420(np.full((2, 2, 3), 255, np.uint8), matrix, False), 2, 2)[0][0, 0] == 235


@pytest.mark.parametrize("matrix,full_range", COMBOS)
def test_round_trip_of_flat_colours_is_within_one_code_value(matrix, full_range):
    """RGB bytes -> I420 -> RGB (rounded half to even to bytes, as the network's output is) -> I420: within 1 code value
    of the first frame.  Measured on this definition over the colours below: exactly 1 for all four combinations (a
    luma byte carries an error of up to 0.5, a decoded channel then up to ~1.2 after its own rounding, and re-encoding
    weights the three channel errors by coefficients that sum to <= 1 in luma and <= 1 in magnitude per chroma row)."""
    rng = np.random.default_rng(3)
    colours = np.concatenate([rng.integers(0, 256, (3000, 3)),
                              np.array(list(itertools.product((0, 1, 127, 128, 254, 255), repeat=3)))]).astype(np.uint8)
    worst = 0
    for col in colours:
        img = np.ascontiguousarray(np.broadcast_to(col, (4, 4, 3)))
        f1 = U.rgb_u8_to_i420(img, matrix, full_range)
        rgb = U.i420_to_rgb_f32(f1, 4, 4, matrix, full_range)
        img2 = np.ascontiguousarray(np.clip(np.rint(rgb), 0, 255).astype(np.uint8).transpose(1, 2, 0))
        f2 = U.rgb_u8_to_i420(img2, matrix, full_range)
        worst = max(worst, int(np.abs(f1.astype(int) - f2.astype(int)).max()))
    print("round trip", matrix, full_range, "worst", worst)
    assert worst <= 1


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (5, 3)])
def test_odd_sizes_plane_sizes_and_edge_clamping(w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert U.i420_frame_bytes(w, h) == w * h + 2 * cw * ch
    f = _frame(w + 10 * h, w, h)
    y, u, v = U.i420_planes(f, w, h)
    assert y.shape == (h, w) and u.shape == (ch, cw) and v.shape == (ch, cw)
    assert np.array_equal(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]), f)
    for plane in (u, v):   # the clamped indices are the explicitly padded plane
        want = 16.0 * (_upsample_padded(plane, w, h) - 128.0)
        assert np.array_equal(U._chroma16(plane, w, h).astype(np.float64), want)
    img = np.random.default_rng(w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    padded = np.pad(img, ((0, h % 2), (0, w % 2), (0, 0)), mode="edge")   # even sides: no clamping takes place
    got = U.i420_planes(U.rgb_u8_to_i420(img, "bt709", True), w, h)
    ref = U.i420_planes(U.rgb_u8_to_i420(padded, "bt709", True), padded.shape[1], padded.shape[0])
    assert np.array_equal(got[0], ref[0][:h, :w]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    with pytest.raises(ValueError):
        U.i420_frame_bytes(0, 4)
    with pytest.raises(ValueError):
        U.i420_to_rgb_f32(f[:-1], w, h)
    with pytest.raises(ValueError):
        U.i420_to_rgb_f32(f, w, h, "bt2020")


def test_yuv_source_is_built_and_its_entry_points_refuse_null_pointers():
    from larvanet_amd import hip_lib
    from larvanet_amd.build import SOURCES
    if not os.path.exists(hip_lib.LIB_PATH):
        from larvanet_amd.build import build_extension
        build_extension(verbose=False)
    lib = hip_lib.load()
    assert "larva_yuv.hip" in SOURCES
    # refused before any launch, so this runs without a device: NULL pointers
    assert lib.larva_i420_to_rgb_f32(None, 0, None, 1, 1, 1, hip_lib.int_array([0] * 6), None) != 0
    assert lib.larva_rgb_u8_to_i420(None, None, 0, 1, 1, 1, hip_lib.int_array([0] * 10), None) != 0


@pytest.mark.parametrize("name", PLUGINS)
def test_plugins_have_the_video_entry_points_and_check_arguments_before_device_work(name):
    from larvanet_amd import pipeline
    extra = ("--leg=1",) if name.startswith("LarvaLeg") else ()
    m = _model(name, extra, blocks=(1, 1))
    good = _frame(1, 8, 6)
    assert good.size == 72
    with pytest.raises(TypeError):
        m.upscale_yuv420([good.astype(np.float32)], 4, 8, 6)
    with pytest.raises(ValueError):
        m.upscale_yuv420([good[:-1]], 4, 8, 6)                  # a short frame
    with pytest.raises(ValueError):
        m.upscale_yuv420([good, _frame(2, 8, 8)], 4, 8, 6)     # one size per call
    with pytest.raises(ValueError):
        m.upscale_yuv420([good.reshape(2, -1)], 4, 8, 6)       # not flat
    with pytest.raises(ValueError):
        m.upscale_yuv420([], 4, 8, 6)
    with pytest.raises(ValueError):
        m.upscale_yuv420([good], 4, 8, 6, matrix="bt2020")
    with pytest.raises(TypeError):
        m.upscale_yuv420([good], 4, 8, 6, full_range="full")
    for bad_scale in (2, 3, 8):
        with pytest.raises(ValueError):
            m.upscale_yuv420([good], bad_scale, 8, 6)
    with pytest.raises(TypeError):
        m.upscale_yuv420_tensor(torch.zeros(1, 72), 8, 6)
    with pytest.raises(ValueError):
        m.upscale_yuv420_tensor(torch.zeros(1, 73, dtype=torch.uint8), 8, 6)
    with pytest.raises(ValueError):
        m.upscale_yuv420_tensor(torch.zeros(72, dtype=torch.uint8), 8, 6)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.upscale_yuv420_tensor(torch.zeros(1, 72, dtype=torch.uint8), 8, 6)   # a host tensor
    with pytest.raises(ValueError):
        pipeline.upscale_yuv_stream(m, [good], 2, 8, 6)
    with pytest.raises(ValueError):
        pipeline.upscale_yuv_stream(m, [good], 4, 8, 6, depth=0)
    with pytest.raises(ValueError):
        pipeline.upscale_yuv_stream(m, [good], 4, 8, None)
    with pytest.raises(ValueError):
        pipeline.upscale_yuv_stream(m, [good], 4, 8, 6, matrix="rec2020")


# ---------------------------------------------------------------- kernels (GPU)
def _padded_batch(frames, pitch, device, fill=0xA5):
    buf = np.full((len(frames), pitch), fill, np.uint8)
    for n, f in enumerate(frames):
        buf[n, :f.size] = f
    return torch.from_numpy(buf).to(device)


TO_RGB_SIZES = [(1, 1), (2, 2), (3, 5), (5, 3), (7, 4), (48, 48), (127, 37), (515, 67), (510, 339)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", TO_RGB_SIZES)
def test_i420_to_rgb_f32_kernel_is_the_numpy_spec(hip_device, w, h):
    from larvanet_amd import kernels as K
    nbytes = U.i420_frame_bytes(w, h)
    combos = COMBOS if (w, h) == (127, 37) else [("bt601", False)]
    for matrix, full_range in combos:
        for n, pitch in ((1, nbytes), (3, nbytes), (3, nbytes + 13), (2, (nbytes + 64) // 4 * 4)):
            frames = [_frame(1000 * w + 10 * h + k, w, h) for k in range(n)]
            got = K.i420_to_rgb_f32(_padded_batch(frames, pitch, hip_device), w, h, matrix, full_range).cpu().numpy()
            want = np.stack([U.i420_to_rgb_f32(f, w, h, matrix, full_range) for f in frames])
            assert got.dtype == np.float32 and got.shape == (n, 3, h, w)
            assert np.array_equal(got, want), (matrix, full_range, n, pitch)


@pytest.mark.gpu
def test_i420_to_rgb_f32_kernel_past_its_grid_cap(hip_device):
    """2052 x 2050: 513 x 1025 thread blocks of 4 x 2 pixels are more than the 2048 x 256 threads of the capped grid, so
    the grid-stride loop runs a second round."""
    from larvanet_amd import kernels as K
    w, h = 2052, 2050
    assert ((w + 3) // 4) * ((h + 1) // 2) > 2048 * 256
    f = _frame(77, w, h)
    got = K.i420_to_rgb_f32(torch.from_numpy(f[None]).to(hip_device), w, h, "bt709", False).cpu().numpy()
    assert np.array_equal(got[0], U.i420_to_rgb_f32(f, w, h, "bt709", False))


TO_YUV_SIZES = [(3, 3), (4, 4), (9, 15), (15, 9), (21, 12), (192, 192), (381, 111), (2060, 268)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", TO_YUV_SIZES)
def test_rgb_u8_to_i420_kernel_is_the_numpy_spec(hip_device, w, h):
    from larvanet_amd import kernels as K
    nbytes = U.i420_frame_bytes(w, h)
    combos = COMBOS if (w, h) == (381, 111) else [("bt601", False)]
    for matrix, full_range in combos:
        for n, pitch in ((1, nbytes), (3, nbytes), (3, nbytes + 13), (2, (nbytes + 64) // 4 * 4)):
            imgs = np.random.default_rng(w * 7 + h + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
            out = torch.full((n, pitch), 0xA5, dtype=torch.uint8, device=hip_device)
            ret = K.rgb_u8_to_i420(torch.from_numpy(imgs).to(hip_device), matrix, full_range, out=out)
            assert ret is out
            got = out.cpu().numpy()
            want = np.stack([U.rgb_u8_to_i420(a, matrix, full_range) for a in imgs])
            assert np.array_equal(got[:, :nbytes], want), (matrix, full_range, n, pitch)
            assert np.all(got[:, nbytes:] == 0xA5)   # nothing beyond a frame is written
        got = K.rgb_u8_to_i420(torch.from_numpy(imgs).to(hip_device), matrix, full_range).cpu().numpy()
        assert got.shape == (imgs.shape[0], nbytes) and np.array_equal(got, want)


@pytest.mark.gpu
def test_rgb_u8_to_i420_kernel_past_its_grid_cap(hip_device):
    from larvanet_amd import kernels as K
    w, h = 2052, 2050
    img = np.random.default_rng(5).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    got = K.rgb_u8_to_i420(torch.from_numpy(img).to(hip_device), "bt601", True).cpu().numpy()
    assert np.array_equal(got[0], U.rgb_u8_to_i420(img[0], "bt601", True))


@pytest.mark.gpu
def test_kernel_wrappers_refuse_bad_operands(hip_device):
    from larvanet_amd import kernels as K
    f = torch.zeros((1, 24), dtype=torch.uint8, device=hip_device)
    with pytest.raises(RuntimeError):
        K.i420_to_rgb_f32(f, 4, 5)                       # the frame is too short for 4 x 5
    with pytest.raises(RuntimeError):
        K.i420_to_rgb_f32(f.cpu(), 4, 4)
    with pytest.raises(RuntimeError):
        K.i420_to_rgb_f32(f.float(), 4, 4)
    with pytest.raises(ValueError):
        K.i420_to_rgb_f32(f, 4, 4, "bt2020")
    with pytest.raises(RuntimeError):
        K.rgb_u8_to_i420(torch.zeros((1, 3, 4, 4), dtype=torch.uint8, device=hip_device))   # CHW
    with pytest.raises(RuntimeError):
        K.rgb_u8_to_i420(torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=hip_device), out=f[:, :23])


# ---------------------------------------------------------------- networks (GPU)
def _composition(model, frames, w, h, matrix, full_range):
    """rgb_u8_to_i420(f32_chw_to_u8_hwc(forward(i420_to_rgb_f32(frame)))) from the numpy definition, the model's float
    entry point and the existing quantising kernel."""
    from larvanet_amd import kernels as K
    x = [U.i420_to_rgb_f32(f, w, h, matrix, full_range) for f in frames]
    hr = K.f32_chw_to_u8_hwc(model.upscale_tensor(x).contiguous()).cpu().numpy()
    return [U.rgb_u8_to_i420(a, matrix, full_range) for a in hr]


NET_CASES = [("LarvaNet", (), "fp32", 4), ("LarvaNet", (), "fp32", 3), ("LarvaNet", (), "fp32", 2),
             ("LarvaNet", (), "fp16", 4), ("LarvaNetV2", (), "fp16", 4), ("LarvaLeg", ("--leg=1",), "fp32", 4),
             ("LarvaNet", ("--self_ensemble",), "fp32", 4), ("LarvaNet", ("--self_ensemble",), "fp16", 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra,precision,scale", NET_CASES, ids=lambda v: "".join(v) if isinstance(v, tuple) else str(v))
def test_upscale_yuv420_tensor_equals_the_composition(hip_device, name, extra, precision, scale):
    ref = _model(name, extra, precision, scale=scale)
    m = _model(name, extra, precision, scale=scale)
    for (w, h), (matrix, full_range) in zip(((48, 48), (37, 23)), (("bt601", False), ("bt709", True))):
        for call in range(3):   # eager, capture, replay
            frames = [_smooth_frame(100 * call + k + w, w, h) for k in range(2)]
            want = _composition(ref, frames, w, h, matrix, full_range)
            got = m.upscale_yuv420_tensor(torch.from_numpy(np.stack(frames)).to(hip_device), w, h, matrix, full_range)
            assert got.is_cuda and got.dtype == torch.uint8
            assert tuple(got.shape) == (2, U.i420_frame_bytes(scale * w, scale * h))
            assert all(np.array_equal(g, t) for g, t in zip(got.cpu().numpy(), want)), (w, h, call)
            host = m.upscale_yuv420(frames, scale, w, h, matrix, full_range)
            assert len(host) == 2 and all(g.ndim == 1 and np.array_equal(g, t) for g, t in zip(host, want)), (w, h, call)
    table = m._infer_graphs_se if "--self_ensemble" in extra else m._infer_graphs_u8
    assert table and all(k[-1] == "f32in" and v is not False for k, v in table.items())   # captured under keys of its own


def _sized(seed, w, h):
    return (_smooth_frame(seed, w, h), w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_upscale_yuv_stream_equals_upscale_yuv420_frame_by_frame(hip_device, precision):
    from larvanet_amd import pipeline
    items = [_sized(i, *((40, 24) if i % 2 == 0 else (33, 47))) for i in range(5)]
    one = _model(precision=precision)
    want = [one.upscale_yuv420([f], 4, w, h, "bt709", False)[0] for f, w, h in items]
    m = None
    for depth in (1, 3):
        m = None   # (see _collect)
        m = _model(precision=precision)
        got = list(pipeline.upscale_yuv_stream(m, iter(items), 4, matrix="bt709", depth=depth))
        assert len(got) == 5
        for i, (g, t) in enumerate(zip(got, want)):
            assert g.dtype == np.uint8 and g.ndim == 1 and np.array_equal(g, t), (depth, i)
    same = [f for f, w, h in items if (w, h) == (40, 24)]   # one size, given once
    m = None
    m = _model(precision=precision)
    got = list(pipeline.upscale_yuv_stream(m, same, 4, 40, 24, matrix="bt709", depth=2))
    assert len(got) == 3 and all(np.array_equal(g, t) for g, t in zip(got, want[0::2]))


@pytest.mark.gpu
def test_fp16_overflow_raises_from_the_video_entry_points_at_the_right_frame(hip_device):
    from larvanet_amd import pipeline
    items = [_sized(i, *((40, 24) if i % 2 == 0 else (33, 47))) for i in range(5)]
    m = _model(precision="fp16")
    want = [m.upscale_yuv420([f], 4, w, h)[0] for f, w, h in items]
    bad_at = 3
    for depth in (1, 3):
        m = None   # (see _collect)
        m = _model(precision="fp16")

        def feed():
            for i, item in enumerate(items):
                if i == bad_at:
                    with torch.no_grad():
                        m.model.head.feature_extraction.weight.mul_(1e4)   # head output >> 65504
                    m.model.invalidate_packed_weights()
                yield item

        got = []
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            for g in pipeline.upscale_yuv_stream(m, feed(), 4, depth=depth):
                got.append(g)
        assert len(got) == bad_at and all(np.array_equal(g, t) for g, t in zip(got, want)), depth
        f, w, h = items[0]
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            m.upscale_yuv420([f], 4, w, h)
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            m.upscale_yuv420_tensor(torch.from_numpy(f[None]).to(hip_device), w, h)


@pytest.mark.gpu
def test_training_and_the_u8_path_are_unchanged_by_video_calls(hip_device):
    """A training step and upscale_u8 before and after YUV calls, against a model that never saw a frame: bit for bit,
    with the u8 path's graphs replaying."""
    def make():
        _collect()
        m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
        m.parse_args(["--num_modules=2", "--num_blocks=2,2"])
        torch.manual_seed(0)
        m.prepare(is_training=True, scales=[4])
        m.strict_graph = True
        return m

    class NoImages:
        def get_num_images(self):
            return 0

    g = torch.Generator().manual_seed(1)
    x = (torch.rand(16, 3, 48, 48, generator=g) * 255).to(hip_device)
    truth = (torch.rand(16, 3, 192, 192, generator=g) * 255).to(hip_device)
    img = np.random.default_rng(9).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    frame = _smooth_frame(4, 40, 24)
    args = None
    m, fresh = make(), make()
    for rnd in range(3):
        a, b = (mm.train_step_larva(args, NoImages(), x, truth) for mm in (m, fresh))
        assert a == b, rnd
        for (k, p), (_, q) in zip(m.model.named_parameters(), fresh.model.named_parameters()):
            assert torch.equal(p, q), (rnd, k)
        with torch.no_grad():
            for call in range(3):
                assert np.array_equal(m.upscale_u8([img], 4), fresh.upscale_u8([img], 4)), (rnd, call)
                m.upscale_yuv420([frame], 4, 40, 24)
    assert set(m._infer_graphs_u8) - set(fresh._infer_graphs_u8) == {k for k in m._infer_graphs_u8 if k[-1] == "f32in"}
    assert all(v is not False for v in m._infer_graphs_u8.values())
