"""output_size on the public surface: --output_size of the two drivers (parsing, refusals, the Y4M header), and on the GPU
the plugins' upscale_u8 / upscale_u8_tensor / upscale_yuv420 / upscale_yuv420_tensor and the two upscaling streams, each
equal, byte for byte, to image_utils.resize_u8 of what the call without the argument gives."""
import gc
import importlib
import io

import numpy as np
import pytest
import torch

from larvanet_amd import image_utils as U


def _model(extra=(), precision="fp32", blocks=(1, 1), scale=4):
    gc.collect()   # (a dropped plugin's captured graphs must be gone before the next capture: see tests/test_yuv.py)
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks)),
                  "--precision=" + precision] + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[scale])
    m.strict_graph = True
    return m


def _smooth_image(seed, h, w):
    """An image a network can take at fp16: colour ramps with mild noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = 40 + 150 * (xx + yy) / max(1, w + h - 2)
    return np.stack([ramp + rng.integers(0, 12, (h, w)), 220 - ramp + rng.integers(0, 12, (h, w)),
                     100 + rng.integers(0, 24, (h, w))], axis=-1).astype(np.uint8)


def _smooth_frame(seed, w, h):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = (40 + 150 * (xx + yy) / max(1, w + h - 2) + rng.integers(0, 12, (h, w))).astype(np.uint8)
    c = rng.integers(100, 156, 2 * ((w + 1) // 2) * ((h + 1) // 2)).astype(np.uint8)
    return np.concatenate([y.reshape(-1), c])


# ---------------------------------------------------------------- host: parsing, refusals, the header
def test_parse_output_size():
    assert U.parse_output_size("1920x1080") == (1080, 1920)
    assert U.parse_output_size("71X51") == (51, 71)
    assert U.parse_output_size("1x1") == (1, 1)
    for bad in ("", "1920", "1920x", "x1080", "1920x1080x3", "1920*1080", "19.2x10", "-4x8", "0x8", "8x0", "axb", "8 x 8"):
        with pytest.raises(ValueError):
            U.parse_output_size(bad)


def test_check_output_size():
    assert U.check_output_size(None, 96, 128) is None
    assert U.check_output_size((50, 70), 96, 128) == (50, 70)
    assert U.check_output_size([24, np.int64(32)], 96, 128) == (24, 32)       # exactly 4
    assert U.check_output_size((500, 7000), 96, 128) == (500, 7000)           # any upsampling
    for bad in ((23, 70), (50, 31), (0, 70), (50, -1)):
        with pytest.raises(ValueError):
            U.check_output_size(bad, 96, 128)
    for bad in ("50x70", 50, (50,), (50, 70, 3), (50.5, 70)):
        with pytest.raises(TypeError):
            U.check_output_size(bad, 96, 128)


def test_upscale_video_output_size_arguments_and_header():
    from larvanet_amd import upscale_video as V, y4m
    base = ["--input", "in.y4m", "--output", "out.y4m"]
    args = V.build_parser().parse_args(base)
    V.check_args(args)
    assert args.output_size is None and V.output_size_of(args) is None and V.output_size_of(args, (480, 270)) is None
    args = V.build_parser().parse_args(base + ["--output_size", "1920x1080"])
    V.check_args(args)
    assert V.output_size_of(args) == (1080, 1920)
    assert V.output_size_of(args, (854, 480)) == (1080, 1920)        # x4 gives 3416 x 1920: down by 1.78
    assert V.output_size_of(args, (1920, 1080)) == (1080, 1920)      # down by exactly 4
    with pytest.raises(ValueError):
        V.output_size_of(args, (1922, 1080))                         # 7688 -> 1920 is beyond 4
    for bad in ("1920", "1920x", "0x1080", "wxh", "1920x1080x2"):
        with pytest.raises(ValueError):                              # malformed: refused by check_args, before any input
            V.check_args(V.build_parser().parse_args(base + ["--output_size", bad]))
    header = y4m.parse_header(b"YUV4MPEG2 W480 H270 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n")
    assert V.output_header(header, 4) == header.scaled(4)
    out = io.BytesIO()
    y4m.write_header(out, V.output_header(header, 4, (1080, 1917)))
    assert out.getvalue() == b"YUV4MPEG2 W1917 H1080 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
    again = y4m.parse_header(out.getvalue())
    assert (again.width, again.height) == (1917, 1080) and again.frame_bytes == U.i420_frame_bytes(1917, 1080)
    assert again.full_range is True


def test_upscale_images_output_size_arguments(tmp_path):
    from PIL import Image
    from larvanet_amd import upscale_images as I
    args = I.build_parser().parse_args([])
    assert args.output_size is None and I.output_size_of(args) is None
    assert I.output_size_of(I.build_parser().parse_args(["--output_size", "70x50"])) == (50, 70)
    for bad in ("70", "70x", "70x0", "70by50"):
        with pytest.raises(ValueError):
            I.output_size_of(I.build_parser().parse_args(["--output_size", bad]))
    with pytest.raises(ValueError):
        I.output_size_of(I.build_parser().parse_args(["--output_size", "70x50", "--all_exits"]))
    path = str(tmp_path / "a.png")
    Image.fromarray(np.zeros((24, 32, 3), np.uint8)).save(path)
    assert I.png_size(path) == (24, 32)
    # a folder whose image is out of range for the target is refused from the PNG header: no model is made, nothing decoded
    with pytest.raises(ValueError):
        I.main(["--input_path", str(tmp_path), "--output_path", str(tmp_path / "sr"), "--output_size", "31x50"])
    with pytest.raises(ValueError):
        I.main(["--input_path", str(tmp_path), "--output_path", str(tmp_path / "sr"), "--output_size", "31by50"])


def test_plugin_entry_points_refuse_a_bad_output_size_before_device_work():
    from larvanet_amd import pipeline
    m = _model()
    img = _smooth_image(0, 24, 32)
    frame = _smooth_frame(0, 32, 24)
    for bad in ((23, 70), (50, 31), (0, 70)):
        with pytest.raises(ValueError):
            m.upscale_u8([img], 4, output_size=bad)
        with pytest.raises(ValueError):
            m.upscale_u8_tensor(torch.from_numpy(img[None]), output_size=bad)
        with pytest.raises(ValueError):
            m.upscale_yuv420([frame], 4, 32, 24, output_size=bad)
        with pytest.raises(ValueError):
            m.upscale_yuv420_tensor(torch.from_numpy(frame[None]), 32, 24, output_size=bad)
    with pytest.raises(TypeError):
        m.upscale_u8([img], 4, output_size="70x50")
    with pytest.raises(TypeError):
        pipeline.upscale_stream(m, [img], 4, output_size=70)
    with pytest.raises(ValueError):
        pipeline.upscale_yuv_stream(m, [frame], 4, 32, 24, output_size=(23, 70))


# ---------------------------------------------------------------- networks (GPU)
NET_CASES = [((), "fp32"), ((), "fp16"), (("--self_ensemble",), "fp32")]


@pytest.mark.gpu
@pytest.mark.parametrize("extra,precision", NET_CASES, ids=["fp32", "fp16", "self_ensemble"])
def test_output_size_on_the_entry_points_equals_resize_of_the_plain_result(hip_device, extra, precision):
    m = _model(extra, precision)
    imgs = [_smooth_image(k, 24, 32) for k in range(2)]
    plain = m.upscale_u8(imgs, 4)
    assert plain.shape == (2, 96, 128, 3)
    want = np.stack([U.resize_u8(plain[i], 50, 70) for i in range(2)])
    first = m.upscale_u8(imgs, 4, output_size=(50, 70))
    assert first.dtype == np.uint8 and first.shape == (2, 50, 70, 3) and np.array_equal(first, want)
    second = m.upscale_u8(imgs, 4, output_size=(50, 70))               # the graph is replayed by now
    assert np.array_equal(second, first)
    assert np.array_equal(m.upscale_u8(imgs, 4, output_size=None), plain)
    assert np.array_equal(m.upscale_u8(imgs, 4), plain)
    x = torch.from_numpy(np.stack(imgs)).to(hip_device)
    got = m.upscale_u8_tensor(x, output_size=(50, 70))
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    up = m.upscale_u8_tensor(x, output_size=(131, 96))                 # up on one axis, down on the other
    assert np.array_equal(up.cpu().numpy(), np.stack([U.resize_u8(plain[i], 131, 96) for i in range(2)]))
    assert np.array_equal(m.upscale_u8_tensor(x).cpu().numpy(), plain)
    # video: the resize sits between the forward's uint8 RGB image and rgb_u8_to_i420; an odd target on purpose
    frames = [_smooth_frame(10 + k, 32, 24) for k in range(2)]
    rgb = m._infer_checked(torch.from_numpy(np.stack([U.i420_to_rgb_f32(f, 32, 24, "bt709", False) for f in frames]))
                           .to(hip_device), u8=True).cpu().numpy()
    want_yuv = [U.rgb_u8_to_i420(U.resize_u8(a, 51, 71), "bt709", False) for a in rgb]
    plain_yuv = m.upscale_yuv420(frames, 4, 32, 24, "bt709", False)
    assert all(np.array_equal(p, U.rgb_u8_to_i420(a, "bt709", False)) for p, a in zip(plain_yuv, rgb))
    for call in range(2):
        got = m.upscale_yuv420(frames, 4, 32, 24, "bt709", False, output_size=(51, 71))
        assert len(got) == 2
        for g, t in zip(got, want_yuv):
            assert g.dtype == np.uint8 and g.shape == (U.i420_frame_bytes(71, 51),) and np.array_equal(g, t), call
    dev = m.upscale_yuv420_tensor(torch.from_numpy(np.stack(frames)).to(hip_device), 32, 24, "bt709", False,
                                  output_size=(51, 71))
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), np.stack(want_yuv))
    again = m.upscale_yuv420(frames, 4, 32, 24, "bt709", False)
    assert all(np.array_equal(a, b) for a, b in zip(again, plain_yuv))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_streams_with_one_target_size_equal_the_single_calls(hip_device, precision):
    from larvanet_amd import pipeline
    m = _model((), precision)
    sizes = [(24, 32), (20, 28), (24, 32)]
    imgs = [_smooth_image(20 + i, h, w) for i, (h, w) in enumerate(sizes)]
    want = [m.upscale_u8([a], 4, output_size=(50, 70))[0] for a in imgs]
    items = [(_smooth_frame(30 + i, w, h), w, h) for i, (h, w) in enumerate(sizes)]
    want_yuv = [m.upscale_yuv420([f], 4, w, h, "bt601", True, output_size=(51, 71))[0] for f, w, h in items]
    for depth in (1, 2):
        got = list(pipeline.upscale_stream(m, iter(imgs), 4, depth=depth, output_size=(50, 70)))
        assert len(got) == 3
        for i, (g, t) in enumerate(zip(got, want)):
            assert g.dtype == np.uint8 and g.shape == (50, 70, 3) and np.array_equal(g, t), (depth, i)
        got = list(pipeline.upscale_yuv_stream(m, iter(items), 4, matrix="bt601", full_range=True, depth=depth,
                                               output_size=(51, 71)))
        assert len(got) == 3
        for i, (g, t) in enumerate(zip(got, want_yuv)):
            assert g.dtype == np.uint8 and g.ndim == 1 and np.array_equal(g, t), (depth, i)
    plain = list(pipeline.upscale_stream(m, iter(imgs), 4, depth=2))           # without the argument: today's results
    assert all(np.array_equal(g, m.upscale_u8([a], 4)[0]) for g, a in zip(plain, imgs))
    with pytest.raises(ValueError):                                            # 80 -> 19: refused at that image's turn
        list(pipeline.upscale_stream(m, iter(imgs), 4, depth=2, output_size=(19, 70)))
