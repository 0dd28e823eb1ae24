"""Transparency on the public surface: the plugins' upscale_rgba_u8 / upscale_rgba_u8_tensor, pipeline.upscale_stream with
keep_alpha and --keep_alpha of larvanet_amd.upscale_images.  Refusals, flags and the decoder run anywhere; on the GPU every
result is compared byte for byte with the definition: the colour is upscale_u8 of the RGB part, the alpha is the merge
(image_utils.rgba_merge_u8: (r + g + b + 1) // 3) of upscale_u8 of the alpha plane as a grey image, 255 for an opaque image."""
import gc
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from larvanet_amd import image_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGINS = ("LarvaNet", "LarvaNetV2", "LarvaLeg", "LarvaLegV2")


def _model(name="LarvaNet", extra=(), precision="fp32", blocks=(2, 2), scale=4, seed=0):
    gc.collect()   # (a dropped plugin's captured graphs must be gone before the next capture: see tests/test_yuv.py)
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks)),
                  "--precision=" + precision] + list(extra))
    torch.manual_seed(seed)
    m.prepare(is_training=False, scales=[scale])
    m.strict_graph = True
    return m


def _smooth_rgb(seed, h, w):
    """An image a network can take at fp16: colour ramps with mild noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = 40 + 150 * (xx + yy) / max(1, w + h - 2)
    return np.stack([ramp + rng.integers(0, 12, (h, w)), 220 - ramp + rng.integers(0, 12, (h, w)),
                     100 + rng.integers(0, 24, (h, w))], axis=-1).astype(np.uint8)


def _rgba(seed, h, w, opaque=False):
    """_smooth_rgb with a smooth alpha ramp that reaches 0 and 255 (or alpha 255 everywhere)."""
    yy, xx = np.mgrid[0:h, 0:w]
    alpha = np.clip(355.0 * (xx + (h - 1 - yy)) / max(1, w + h - 2) - 50.0, 0, 255).astype(np.uint8)
    if opaque:
        alpha[:] = 255
    else:
        assert alpha.min() == 0 and alpha.max() == 255
    return np.ascontiguousarray(np.concatenate([_smooth_rgb(seed, h, w), alpha[:, :, None]], axis=2))


def _expected(m, img, scale, size=None):
    """The definition, from upscale_u8 alone."""
    out = np.empty(((scale * img.shape[0], scale * img.shape[1]) if size is None else tuple(size)) + (4,), np.uint8)
    out[..., :3] = m.upscale_u8([np.ascontiguousarray(img[..., :3])], scale, output_size=size)[0]
    if img[..., 3].min() == 255:
        out[..., 3] = 255
    else:
        grey = np.ascontiguousarray(np.repeat(img[..., 3:4], 3, axis=2))
        a3 = m.upscale_u8([grey], scale, output_size=size)[0]
        out[..., 3] = (a3.astype(np.int32).sum(axis=2) + 1) // 3
    return out


# ---------------------------------------------------------------- host: refusals before any device work
@pytest.mark.parametrize("name", PLUGINS)
def test_plugins_have_the_rgba_entry_points_and_check_arguments_before_device_work(name, monkeypatch):
    from larvanet_amd import kernels as K

    def no_device_work(*a, **k):
        raise AssertionError("device work was started before the arguments were checked")

    extra = ("--leg=1",) if name.startswith("LarvaLeg") else ()
    m = _model(name, extra, blocks=(1, 1))
    monkeypatch.setattr(m, "_eager_or_graph", no_device_work)
    monkeypatch.setattr(K, "rgba_u8_split_f32", no_device_work)
    monkeypatch.setattr(K, "rgb_u8_merge_rgba", no_device_work)
    good = _rgba(0, 6, 8)
    with pytest.raises(TypeError):
        m.upscale_rgba_u8([good.astype(np.float32)], 4)
    with pytest.raises(ValueError):
        m.upscale_rgba_u8([good[..., :3]], 4)                    # an RGB image
    with pytest.raises(ValueError):
        m.upscale_rgba_u8([good, _rgba(1, 8, 8)], 4)             # one shape per call
    with pytest.raises(ValueError):
        m.upscale_rgba_u8([], 4)
    with pytest.raises(ValueError):
        m.upscale_rgba_u8(good[None], 4)                         # a list, not an array
    for bad_scale in (2, 3, 8):
        with pytest.raises(ValueError):
            m.upscale_rgba_u8([good], bad_scale)
    with pytest.raises(ValueError):
        m.upscale_rgba_u8([good], 4, output_size=(5, 32))        # beyond a ratio of 4
    host = torch.from_numpy(good[None])
    with pytest.raises(TypeError):
        m.upscale_rgba_u8_tensor(host.float())
    with pytest.raises(TypeError):
        m.upscale_rgba_u8_tensor(good[None])
    with pytest.raises(ValueError):
        m.upscale_rgba_u8_tensor(host[..., :3])
    with pytest.raises(ValueError):
        m.upscale_rgba_u8_tensor(host[0])
    for bad_opaque in ([], [True, False], [1], "n"):
        with pytest.raises(ValueError):
            m.upscale_rgba_u8_tensor(host, opaque=bad_opaque)
    with pytest.raises(ValueError):
        m.upscale_rgba_u8_tensor(host, output_size=(5, 32))
    with pytest.raises(RuntimeError, match="HIP device"):
        m.upscale_rgba_u8_tensor(host, opaque=[False])           # a host tensor


def test_the_stream_refuses_four_channels_unless_keep_alpha():
    from larvanet_amd import pipeline
    rgba, rgb = _rgba(0, 6, 8), _smooth_rgb(0, 6, 8)
    pipeline._check_image(rgb)
    pipeline._check_image(rgb, keep_alpha=True)
    pipeline._check_image(rgba, keep_alpha=True)
    with pytest.raises(ValueError, match=r"takes \(H, W, 3\) images, got shape \(6, 8, 4\)"):
        pipeline._check_image(rgba)                              # the default: today's refusal, word for word
    with pytest.raises(ValueError):
        pipeline._check_image(rgba, "evaluate_stream")
    for bad in (rgba[..., :2], rgba[..., 0], np.zeros((0, 8, 4), np.uint8)):
        with pytest.raises(ValueError):
            pipeline._check_image(bad, keep_alpha=True)
    with pytest.raises(TypeError):
        pipeline._check_image(rgba.astype(np.float32), keep_alpha=True)


# ---------------------------------------------------------------- host: the folder tool
def test_keep_alpha_flag_and_its_refusal_with_all_exits(tmp_path):
    from larvanet_amd import upscale_images as I
    assert I.build_parser().parse_args([]).keep_alpha is False
    args = I.build_parser().parse_args(["--keep_alpha"])
    assert args.keep_alpha is True
    I.check_keep_alpha(args)
    with pytest.raises(ValueError, match="--keep_alpha together with --all_exits"):
        I.check_keep_alpha(I.build_parser().parse_args(["--keep_alpha", "--all_exits"]))
    # refused before the folder is listed or any image is read: the folder does not even exist
    with pytest.raises(ValueError, match="--keep_alpha together with --all_exits"):
        I.main(["--input_path", str(tmp_path / "missing"), "--output_path", str(tmp_path / "sr"), "--keep_alpha", "--all_exits"])
    assert not (tmp_path / "sr").exists()


def test_the_decoder_keeps_alpha_for_the_modes_that_carry_it(tmp_path):
    from PIL import Image
    from larvanet_amd import upscale_images as I
    rgba = _rgba(3, 5, 7)
    rgb = np.ascontiguousarray(rgba[..., :3])
    rgb[0, 0] = (9, 8, 7)
    rgb[1:] = np.maximum(rgb[1:], 10)             # (9, 8, 7) occurs once: the colour key of the tRNS file
    grey = np.ascontiguousarray(rgba[..., 0])
    paths = {}

    def save(name, im, **kw):
        paths[name] = str(tmp_path / (name + ".png"))
        im.save(paths[name], **kw)

    save("RGBA", Image.fromarray(rgba))
    save("LA", Image.merge("LA", (Image.fromarray(grey), Image.fromarray(np.ascontiguousarray(rgba[..., 3])))))
    save("P_trns", Image.fromarray(rgb).quantize(8), transparency=0)
    save("RGB_trns", Image.fromarray(rgb), transparency=(9, 8, 7))
    save("RGB", Image.fromarray(rgb))
    save("L", Image.fromarray(grey))
    save("P", Image.fromarray(rgb).quantize(8))
    for name, mode in (("RGBA", "RGBA"), ("LA", "LA"), ("P_trns", "P"), ("RGB_trns", "RGB"), ("RGB", "RGB"), ("L", "L"), ("P", "P")):
        with Image.open(paths[name]) as im:
            assert im.mode == mode, name
            assert I.carries_alpha(im) is (name in ("RGBA", "LA", "P_trns", "RGB_trns")), name
    for name in paths:
        a = I.read_image(paths[name], keep_alpha=True)
        assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
        assert a.shape == (5, 7, 4 if name in ("RGBA", "LA", "P_trns", "RGB_trns") else 3), name
        dropped = I.read_image(paths[name])      # without the flag: the RGB way, as read_rgb
        assert dropped.shape == (5, 7, 3) and np.array_equal(dropped, I.read_rgb(paths[name])), name
        if a.shape[2] == 3:
            assert np.array_equal(a, dropped), name
    assert np.array_equal(I.read_image(paths["RGBA"], True), rgba)
    la = I.read_image(paths["LA"], True)
    assert np.array_equal(la[..., 3], rgba[..., 3]) and all(np.array_equal(la[..., c], grey) for c in range(3))
    keyed = I.read_image(paths["RGB_trns"], True)
    assert np.array_equal(keyed[..., :3], rgb) and keyed[0, 0, 3] == 0 and np.all(keyed[1:, :, 3] == 255)
    pal = I.read_image(paths["P_trns"], True)
    assert set(np.unique(pal[..., 3])) <= {0, 255} and 255 in pal[..., 3]
    # written back: 4 channels make an RGBA PNG, 3 an RGB one
    I.write_rgb(rgba, str(tmp_path / "w4.png"))
    I.write_rgb(rgb, str(tmp_path / "w3.png"))
    with Image.open(str(tmp_path / "w4.png")) as im:
        assert im.mode == "RGBA" and np.array_equal(np.asarray(im), rgba)
    with Image.open(str(tmp_path / "w3.png")) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), rgb)


# ---------------------------------------------------------------- networks (GPU)
NET_CASES = [((), "fp32", 4), ((), "fp32", 3), ((), "fp32", 2), ((), "fp16", 4), (("--self_ensemble",), "fp32", 4),
             (("--self_ensemble",), "fp16", 4)]
NET_IDS = ["fp32x4", "fp32x3", "fp32x2", "fp16x4", "ensemble_fp32x4", "ensemble_fp16x4"]


@pytest.mark.gpu
@pytest.mark.parametrize("extra,precision,scale", NET_CASES, ids=NET_IDS)
def test_upscale_rgba_u8_is_upscale_u8_of_colour_and_of_alpha(hip_device, extra, precision, scale):
    m = _model(extra=extra, precision=precision, scale=scale)
    for h, w in ((12, 20), (37, 50)):
        img, other, solid = _rgba(h, h, w), _rgba(h + 1, h, w), _rgba(h + 2, h, w, opaque=True)
        want = {id(a): _expected(m, a, scale) for a in (img, other, solid)}
        for call in range(3):   # eager, capture, replay: identical bytes
            got = m.upscale_rgba_u8([img], scale)
            assert got.dtype == np.uint8 and got.shape == (1, scale * h, scale * w, 4)
            assert np.array_equal(got[0][..., :3], want[id(img)][..., :3]), (h, w, call)
            assert np.array_equal(got[0][..., 3], want[id(img)][..., 3]), (h, w, call)
        assert int(np.ptp(want[id(img)][..., 3])) > 100   # (a real alpha plane came back, not a constant)
        for call in range(3):
            got = m.upscale_rgba_u8([img, other], scale)
            assert got.shape[0] == 2 and np.array_equal(got[0], want[id(img)]) and np.array_equal(got[1], want[id(other)]), call
        got = m.upscale_rgba_u8([solid], scale)[0]
        assert np.all(got[..., 3] == 255) and np.array_equal(got, want[id(solid)])
        assert np.array_equal(got[..., :3], m.upscale_u8([np.ascontiguousarray(solid[..., :3])], scale)[0])
        # mixed on the host: the opaque image is found by its alpha plane
        got = m.upscale_rgba_u8([solid, img, other], scale)
        assert all(np.array_equal(g, want[id(a)]) for g, a in zip(got, (solid, img, other)))
        # the tensor form: told which image is opaque, and told nothing
        x = torch.from_numpy(np.stack([solid, img])).to(hip_device)
        got = m.upscale_rgba_u8_tensor(x, opaque=[True, False])
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (2, scale * h, scale * w, 4)
        got = got.cpu().numpy()
        assert np.array_equal(got[0], want[id(solid)]) and np.array_equal(got[1], want[id(img)])
        blind = m.upscale_rgba_u8_tensor(x).cpu().numpy()      # (no flags: the flat alpha plane goes through the network too)
        assert np.array_equal(blind[1], want[id(img)]) and np.array_equal(blind[0][..., :3], want[id(solid)][..., :3])
        flat = m.upscale_u8([np.full((h, w, 3), 255, np.uint8)], scale)[0]
        assert np.array_equal(blind[0][..., 3], (flat.astype(np.int32).sum(axis=2) + 1) // 3)
    table = m._infer_graphs_se if "--self_ensemble" in extra else m._infer_graphs_u8
    assert any(k[-1] == "f32in" for k in table) and all(v is not False for v in table.values())   # replays, not eager runs


@pytest.mark.gpu
@pytest.mark.parametrize("extra,precision", [((), "fp32"), ((), "fp16"), (("--self_ensemble",), "fp32")],
                         ids=["fp32", "fp16", "ensemble"])
def test_output_size_resizes_colour_and_alpha_before_the_merge(hip_device, extra, precision):
    m = _model(extra=extra, precision=precision)
    h, w = 12, 20
    img, solid = _rgba(5, h, w), _rgba(6, h, w, opaque=True)
    for size in ((4 * h - 1, 4 * w - 1), (4 * h + 1, 4 * w + 1)):
        want, want_solid = _expected(m, img, 4, size), _expected(m, solid, 4, size)
        # the definition once more, from the unresized results and the host resize
        full = m.upscale_rgba_u8([img], 4)[0]
        grey = np.ascontiguousarray(np.repeat(img[..., 3:4], 3, axis=2))
        a3 = U.resize_u8(m.upscale_u8([grey], 4)[0], *size)
        assert np.array_equal(want[..., :3], U.resize_u8(np.ascontiguousarray(full[..., :3]), *size))
        assert np.array_equal(want[..., 3], (a3.astype(np.int32).sum(axis=2) + 1) // 3)
        for call in range(2):
            got = m.upscale_rgba_u8([img, solid], 4, output_size=size)
            assert got.shape == (2,) + size + (4,)
            assert np.array_equal(got[0], want) and np.array_equal(got[1], want_solid), (size, call)
            assert np.all(got[1][..., 3] == 255)
        x = torch.from_numpy(np.stack([solid, img])).to(hip_device)
        got = m.upscale_rgba_u8_tensor(x, opaque=[True, False], output_size=size).cpu().numpy()
        assert np.array_equal(got[0], want_solid) and np.array_equal(got[1], want)


@pytest.mark.gpu
def test_an_opaque_batch_runs_the_forward_on_n_slots(hip_device, monkeypatch):
    m = _model()
    seen = []
    inner = m._eager_or_graph

    def spy(x, form):
        seen.append((tuple(x.shape), x.dtype))
        return inner(x, form)

    monkeypatch.setattr(m, "_eager_or_graph", spy)
    a, b, c = _rgba(1, 12, 20, opaque=True), _rgba(2, 12, 20, opaque=True), _rgba(3, 12, 20)
    m.upscale_rgba_u8([a, b], 4)
    m.upscale_rgba_u8([a, c], 4)
    m.upscale_rgba_u8([c, c], 4)
    x = torch.from_numpy(np.stack([a, b])).to(hip_device)
    m.upscale_rgba_u8_tensor(x, opaque=[True, True])
    m.upscale_rgba_u8_tensor(x)
    assert [s[0][0] for s in seen] == [2, 3, 4, 2, 4]
    assert all(s == ((s[0][0], 3, 12, 20), torch.float32) for s in seen)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--self_ensemble",)], ids=["plain", "ensemble"])
def test_colour_keeps_its_bytes_where_the_extra_slot_crosses_the_large_inference_rule(hip_device, extra):
    """200 x 260 = 52000 LR pixels: one image is below the rule for "a large inference batch" (100000 pixels), the two
    slots of a translucent RGBA image are above it.  The head kernel, whose two forms differ in the last bits, must be
    the one upscale_u8 of the RGB part takes."""
    from larvanet_amd.autograd import LARGE_INFERENCE_PIXELS
    h, w = 200, 260
    assert h * w <= LARGE_INFERENCE_PIXELS < 2 * h * w
    m = _model(extra=extra)
    img = _rgba(11, h, w)
    want = _expected(m, img, 4)
    for call in range(2):
        assert np.array_equal(m.upscale_rgba_u8([img], 4)[0], want), call


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_results_follow_restored_weights(hip_device, tmp_path, precision):
    m = _model(precision=precision)
    img = _rgba(4, 12, 20)
    first = [m.upscale_rgba_u8([img], 4)[0] for _ in range(3)]   # (captured and replaying)
    assert np.array_equal(first[0], first[2])
    other = _model(precision=precision, seed=5)
    ckpt = other.save(str(tmp_path))
    want = _expected(other, img, 4)
    assert not np.array_equal(want, first[0])
    m.restore(ckpt)
    for call in range(2):
        assert np.array_equal(m.upscale_rgba_u8([img], 4)[0], want), call


# ---------------------------------------------------------------- the stream (GPU)
def _mixed_images():
    return [_smooth_rgb(1, 24, 40), _rgba(2, 24, 40), _rgba(3, 33, 47, opaque=True), _smooth_rgb(4, 33, 47), _rgba(5, 33, 47)]


@pytest.mark.gpu
@pytest.mark.parametrize("extra,precision", [((), "fp32"), ((), "fp16"), (("--self_ensemble",), "fp32")],
                         ids=["fp32", "fp16", "ensemble"])
def test_upscale_stream_with_keep_alpha_equals_the_entry_points_image_by_image(hip_device, extra, precision):
    from larvanet_amd import pipeline
    images = _mixed_images()
    one = _model(extra=extra, precision=precision)
    want = [(one.upscale_rgba_u8 if a.shape[2] == 4 else one.upscale_u8)([a], 4)[0] for a in images]
    sized = [(one.upscale_rgba_u8 if a.shape[2] == 4 else one.upscale_u8)([a], 4, output_size=(101, 150))[0] for a in images]
    one = None
    for depth in (1, 3):
        m = None   # (dropped before its successor is made: see tests/test_yuv.py, _collect)
        m = _model(extra=extra, precision=precision)
        got = list(pipeline.upscale_stream(m, iter(images), 4, depth=depth, keep_alpha=True))
        assert [g.shape for g in got] == [t.shape for t in want] and [g.shape[2] for g in got] == [3, 4, 4, 3, 4]
        assert all(g.dtype == np.uint8 and np.array_equal(g, t) for g, t in zip(got, want)), depth
        got = list(pipeline.upscale_stream(m, iter(images), 4, depth=depth, keep_alpha=True, output_size=(101, 150)))
        assert all(np.array_equal(g, t) for g, t in zip(got, sized)), depth
    # the default still refuses four channels, at the image's turn, after the images before it were taken
    got = []
    with pytest.raises(ValueError, match=r"takes \(H, W, 3\) images"):
        for g in pipeline.upscale_stream(m, iter(images), 4, depth=1):
            got.append(g)
    assert len(got) == 0 or np.array_equal(got[0], want[0])


@pytest.mark.gpu
def test_fp16_overflow_inside_an_rgba_image_raises_at_its_turn(hip_device):
    from larvanet_amd import pipeline
    images = _mixed_images()
    m = _model(precision="fp16")
    want = [(m.upscale_rgba_u8 if a.shape[2] == 4 else m.upscale_u8)([a], 4)[0] for a in images]
    bad_at = 4   # (an RGBA image)
    for depth in (1, 3):
        m = None
        m = _model(precision="fp16")

        def feed():
            for i, a in enumerate(images):
                if i == bad_at:
                    with torch.no_grad():
                        m.model.head.feature_extraction.weight.mul_(1e4)   # head output >> 65504
                    m.model.invalidate_packed_weights()
                yield a

        got = []
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            for g in pipeline.upscale_stream(m, feed(), 4, depth=depth, keep_alpha=True):
                got.append(g)
        assert len(got) == bad_at and all(np.array_equal(g, t) for g, t in zip(got, want)), depth
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            m.upscale_rgba_u8([images[1]], 4)
        with pytest.raises(FloatingPointError, match="--precision fp16"):
            m.upscale_rgba_u8_tensor(torch.from_numpy(images[1][None]).to(hip_device))


# ---------------------------------------------------------------- the folder tool (GPU, a child process)
MODEL_FLAGS = ["--model=LarvaNet", "--num_modules=2", "--num_blocks=2,2", "--scale=4"]


def _run_module(argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "larvanet_amd.upscale_images"] + argv, cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.gpu
def test_upscale_images_keep_alpha_end_to_end(hip_device, tmp_path):
    from PIL import Image
    src, kept, dropped = tmp_path / "in", tmp_path / "kept", tmp_path / "dropped"
    src.mkdir()
    rgb, rgba, la = _smooth_rgb(1, 24, 40), _rgba(2, 24, 40), _rgba(3, 33, 47)
    la[..., 1] = la[..., 0]
    la[..., 2] = la[..., 0]        # grey colour: what an LA file decodes to
    Image.fromarray(rgb).save(str(src / "a_rgb.png"))
    Image.fromarray(rgba).save(str(src / "b_rgba.png"))
    Image.merge("LA", (Image.fromarray(np.ascontiguousarray(la[..., 0])), Image.fromarray(np.ascontiguousarray(la[..., 3])))).save(
        str(src / "c_la.png"))
    m = _model()
    ckpt = m.save(str(tmp_path))
    for out, flag in ((kept, ["--keep_alpha"]), (dropped, [])):
        r = _run_module(MODEL_FLAGS + ["--restore_path", ckpt, "--input_path", str(src), "--output_path", str(out)] + flag)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert sorted(os.listdir(str(out))) == ["a_rgb.png", "b_rgba.png", "c_la.png"]
    want = {"a_rgb.png": ("RGB", m.upscale_u8([rgb], 4)[0]), "b_rgba.png": ("RGBA", m.upscale_rgba_u8([rgba], 4)[0]),
            "c_la.png": ("RGBA", m.upscale_rgba_u8([la], 4)[0])}
    for name, (mode, image) in want.items():
        with Image.open(str(kept / name)) as im:
            assert im.mode == mode and np.array_equal(np.asarray(im), image), name
        with Image.open(str(dropped / name)) as im:   # without the flag: the RGB bytes, as before
            flat = {"a_rgb.png": rgb, "b_rgba.png": rgba[..., :3], "c_la.png": la[..., :3]}[name]
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), m.upscale_u8([np.ascontiguousarray(flat)], 4)[0]), name
