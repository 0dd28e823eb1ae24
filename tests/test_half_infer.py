"""--precision fp16: grad-free x4 inference on fp16 channels-last activations with fp32 accumulation
(csrc/conv3x3_f16.hip, larvanet_amd/half.py).  Host logic runs anywhere; kernels and networks are marked gpu.

Kernel bar: a float64 conv of the fp16-rounded operands (the head: of its fp32 operands), bias and epilogue in float64,
rounded to fp16; every element within 1 fp16 ulp and >= 99.9 % of them exactly equal.  The leg end's fp32 HR image is
within 2e-5 of the float64 result's scale.  Network bar: against the fp32 path on a trained M4B4 model, uint8-protocol
PSNR within 0.02 dB, max |d| <= 0.25, mean |d| <= 0.03."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

BLOCKS = (4, 4, 4, 4)


def _model(name="LarvaNet", extra=(), precision="fp16", training=False, blocks=BLOCKS, scale=4):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    args = ["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks))]
    if precision is not None:
        args.append("--precision=" + precision)
    m.parse_args(args + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=training, scales=[scale])
    m.strict_graph = True
    return m


def _load(m, sd):
    with torch.no_grad():
        for k, p in m.model.state_dict().items():
            p.copy_(sd[k])
    m.model.invalidate_packed_weights()
    return m


# ---------------------------------------------------------------- host
def test_precision_flag_parses_and_defaults_to_fp32():
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    args, _ = m.parse_args([])
    assert args.precision == "fp32"
    for name in ("LarvaNet", "LarvaNetV2", "LarvaLeg", "LarvaLegV2"):
        m = importlib.import_module("larvanet_amd.models." + name).create_model()
        args, _ = m.parse_args(["--precision=fp16"])
        assert args.precision == "fp16"


def test_bad_precision_is_refused_by_parse_args():
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    for bad in ("bf16", "fp8", "half", "FP16"):
        with pytest.raises(SystemExit):
            m.parse_args(["--precision=" + bad])


@pytest.mark.parametrize("scale,nf", [(2, 48), (3, 48), (4, 32), (4, 64)])
@pytest.mark.parametrize("name", ["LarvaNet", "LarvaNetV2"])
def test_fp16_is_refused_outside_x4_at_48_filters(name, scale, nf):
    with pytest.raises(ValueError, match="--precision fp16"):
        _model(name, ("--num_filters=%d" % nf,), blocks=(1, 1), scale=scale)
    _model(name, ("--num_filters=%d" % nf,), precision="fp32", blocks=(1, 1), scale=scale)   # (fp32 builds them)


def test_fp16_prepares_at_x4_48():
    m = _model("LarvaLegV2", ("--leg=2",), blocks=(1, 1))
    assert m.precision == "fp16" and m.fp16_overflowed() is False


def test_f16_weight_image_size_helper_sizes_and_refuses():
    from larvanet_amd import hip_lib
    if not os.path.exists(hip_lib.LIB_PATH):
        from larvanet_amd.build import build_extension
        build_extension(verbose=False)
    lib = hip_lib.load()
    for m in range(1, 9):   # [src m][K-step 14][M tile 3][lane 64][8]
        assert lib.larva_f16_packed_weight_halves(48, 48 * m) == m * 14 * 3 * 64 * 8
    for cout, cin in ((32, 32), (64, 64), (48, 40), (48, 48 * 9), (12, 48)):
        assert lib.larva_f16_packed_weight_halves(cout, cin) == -1


# ---------------------------------------------------------------- kernels (GPU)
def _pack_ref(w):
    """numpy re-layout of [48][48 m][3][3] into [m][ks][mt][lane][8] fp16: cout = 16 mt + lane % 16, K group
    g = 4 ks + lane // 16 = 6 tap + cg (zero for g >= 54), element j = input channel 48 s + 8 cg + j."""
    cout, cin = w.shape[:2]
    m = cin // 48
    out = np.zeros((m, 14, 3, 64, 8), np.float16)
    w16 = w.astype(np.float16)
    for s in range(m):
        for ks in range(14):
            for mt in range(3):
                for lane in range(64):
                    g = 4 * ks + lane // 16
                    if g >= 54:
                        continue
                    tap, cg = divmod(g, 6)
                    co = 16 * mt + lane % 16
                    out[s, ks, mt, lane] = w16[co, 48 * s + 8 * cg:48 * s + 8 * cg + 8, tap // 3, tap % 3]
    return out.reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 4])
def test_weight_pack_is_the_fp16_relayout_bit_for_bit(hip_device, m):
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(10 + m)
    w = (rng.standard_normal((48, 48 * m, 3, 3)) * 0.3).astype(np.float32)
    w[0, 0, 0, 0] = 1e-8          # fp16 subnormal / underflow to zero
    w[1, 1, 1, 1] = 70000.0       # beyond fp16: inf, as numpy rounds it
    got = K.f16_pack_weights(torch.from_numpy(w).to(hip_device)).cpu().numpy()
    with np.errstate(over="ignore"):
        ref = _pack_ref(w)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), ref.view(np.uint16))


def _ordered(a16):
    v = a16.view(np.int16).astype(np.int32)
    return np.where(v < 0, -(v & 0x7FFF), v)


def _assert_fp16_bar(got16, ref16, what):
    assert got16.shape == ref16.shape, what
    assert np.isfinite(got16.astype(np.float32)).all(), what
    d = np.abs(_ordered(got16) - _ordered(ref16))
    exact = float((d == 0).mean())
    assert d.max() <= 1 and exact >= 0.999, "%s: max %d ulp, %.5f exact" % (what, d.max(), exact)


def _conv64(x_nhwc, w):
    """float64 conv of NHWC input with [cout][cin][3][3] w -> NHWC float64."""
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc.transpose(0, 3, 1, 2))).double()
    y = F.conv2d(x, torch.from_numpy(w).double(), padding=1)
    return y.permute(0, 2, 3, 1).numpy()


SHAPES = [(1, 3, 4), (2, 48, 48), (16, 48, 48), (1, 339, 510), (1, 37, 127)]
EPILOGUES = ["relu", "res0", "res01", "merge4"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_conv_kernel_against_float64(hip_device, shape):
    from larvanet_amd import kernels as K
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    n, h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    flag = torch.zeros(1, dtype=torch.int32, device=hip_device)
    # Feature-like operands: non-negative inputs (ReLU / image features) and weights with a positive mean.  Each output
    # then stays within a few times sum |w x|, so the fp32 accumulation error is far below half an fp16 ulp and the
    # exact-fraction clause measures the kernel, not cancellation: on zero-mean random signs at K = 1728 (merge) the
    # error of any fp32-accumulating order flips ~0.3 % of the roundings.
    xs = [np.abs(rng.standard_normal((n, h, w, 48)) * 2).astype(np.float16) for _ in range(4)]
    res = [np.abs(rng.standard_normal((n, h, w, 48)) * 4).astype(np.float16) for _ in range(2)]
    bias = (rng.standard_normal(48) * 0.2).astype(np.float32)
    w1 = (rng.standard_normal((48, 48, 3, 3)) * 0.05 + 0.02).astype(np.float32)
    w4 = (rng.standard_normal((48, 192, 3, 3)) * 0.03 + 0.01).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)   # noqa: E731
    xd, rd = [dev(a) for a in xs], [dev(a) for a in res]
    wpk1, wpk4 = K.f16_pack_weights(dev(w1)), K.f16_pack_weights(dev(w4))
    bd = dev(bias)
    y1 = _conv64(xs[0].astype(np.float64), w1.astype(np.float16).astype(np.float64)) + bias.astype(np.float64)
    for epi in EPILOGUES:
        if epi == "merge4":
            got = K.f16_conv3x3(xd, wpk4, bd, flag)
            cat = np.concatenate([a.astype(np.float64) for a in xs], axis=3)
            ref = _conv64(cat, w4.astype(np.float16).astype(np.float64)) + bias.astype(np.float64)
        elif epi == "relu":
            got = K.f16_conv3x3(xd[0], wpk1, bd, flag, relu=True)
            ref = np.maximum(y1, 0.0)
        elif epi == "res0":
            got = K.f16_conv3x3(xd[0], wpk1, bd, flag, res0=rd[0])
            ref = y1 + res[0].astype(np.float64)
        else:
            got = K.f16_conv3x3(xd[0], wpk1, bd, flag, res0=rd[0], res1=rd[1])
            ref = y1 + res[0].astype(np.float64) + res[1].astype(np.float64)
        _assert_fp16_bar(got.cpu().numpy(), ref.astype(np.float16), "%s %s" % (epi, shape))
    # zero-mean random signs: near-zero outputs have tiny ulps, so the bar is 1 ulp plus the fp32 accumulation scale
    xr = (rng.standard_normal((n, h, w, 48)) * 2).astype(np.float16)
    wr = (rng.standard_normal((48, 48, 3, 3)) * 0.05).astype(np.float32)
    got = K.f16_conv3x3(dev(xr), K.f16_pack_weights(dev(wr)), bd, flag).cpu().numpy().astype(np.float64)
    w16 = wr.astype(np.float16).astype(np.float64)
    ref = _conv64(xr.astype(np.float64), w16) + bias.astype(np.float64)
    mag = _conv64(np.abs(xr.astype(np.float64)), np.abs(w16))
    ref16 = ref.astype(np.float16)
    ulp = np.abs(np.spacing(ref16)).astype(np.float64)
    assert (np.abs(got - ref16.astype(np.float64)) <= ulp + 4e-6 * mag).all()
    assert float((got == ref16.astype(np.float64)).mean()) >= 0.99
    assert int(flag.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 4), (2, 48, 48), (1, 339, 510), (1, 37, 127)])
def test_head_kernel_against_float64_of_its_fp32_operands(hip_device, shape):
    from larvanet_amd import kernels as K
    n, h, w = shape
    rng = np.random.default_rng(7 + h)
    x = (rng.random((n, 3, h, w)) * 255).astype(np.float32)
    # positive weights and bias: no output near zero, where an fp32 sum's error is many fp16 ulps of the result
    wt = (np.abs(rng.standard_normal((48, 3, 3, 3))) * 0.02 + 0.002).astype(np.float32)
    b = np.abs(rng.standard_normal(48) * 0.5).astype(np.float32)
    flag = torch.zeros(1, dtype=torch.int32, device=hip_device)
    got = K.f16_head(torch.from_numpy(x).to(hip_device), torch.from_numpy(wt).to(hip_device),
                     torch.from_numpy(b).to(hip_device), flag).cpu().numpy()
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    _assert_fp16_bar(got, ref.permute(0, 2, 3, 1).numpy().astype(np.float16), "head %s" % (shape,))
    assert int(flag.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 4), (2, 48, 48), (1, 339, 510), (1, 37, 127)])
def test_leg_end_against_float64(hip_device, shape):
    from larvanet_amd import kernels as K
    n, h, w = shape
    rng = np.random.default_rng(11 + w)
    x = (rng.standard_normal((n, h, w, 48)) * 2).astype(np.float16)
    wt = (rng.standard_normal((48, 48, 3, 3)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(48) * 0.2).astype(np.float32)
    base = (rng.random((n, 3, 4 * h, 4 * w)) * 255).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)   # noqa: E731
    got = K.f16_conv3x3_shuffle_base(dev(x), K.f16_pack_weights(dev(wt)), dev(b), dev(base)).cpu().numpy()
    y = _conv64(x.astype(np.float64), wt.astype(np.float16).astype(np.float64)) + b.astype(np.float64)
    ref = F.pixel_shuffle(torch.from_numpy(np.ascontiguousarray(y.transpose(0, 3, 1, 2))), 4).numpy() + base
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max()


# ---------------------------------------------------------------- networks (GPU)
def _smooth_hr(g, n, h, w):
    """Seeded bicubic-smooth colour images (n, 3, h, w) on 0..255."""
    low = torch.rand(n, 3, h // 16 + 1, w // 16 + 1, generator=g)
    mid = torch.rand(n, 3, h // 4 + 1, w // 4 + 1, generator=g)
    img = F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False) * 0.85 + \
        F.interpolate(mid, size=(h, w), mode="bicubic", align_corners=False) * 0.15
    return (img * 255).clamp(0, 255)


def _lr(hr):
    return F.interpolate(hr, scale_factor=0.25, mode="area")


class _NoVal:
    def get_num_images(self):
        return 0


def _train(name, steps, extra=()):
    """A seeded M4B4 model trained with the fp32 step on random 48x48 crops of smooth synthetic images."""
    m = _model(name, extra, precision="fp32", training=True)
    g = torch.Generator().manual_seed(5)
    hr = _smooth_hr(g, 4, 512, 512)
    lr = _lr(hr)
    hr, lr = hr.to(m.device), lr.to(m.device)
    pick = np.random.default_rng(6)
    for _ in range(steps):
        idx = pick.integers(0, 4, 16)
        ys, xs = pick.integers(0, 128 - 48, 16), pick.integers(0, 128 - 48, 16)
        x = torch.stack([lr[i, :, y:y + 48, c:c + 48] for i, y, c in zip(idx, ys, xs)])
        t = torch.stack([hr[i, :, 4 * y:4 * y + 192, 4 * c:4 * c + 192] for i, y, c in zip(idx, ys, xs)])
        m.train_step_larva(None, _NoVal(), x.contiguous(), t.contiguous())
    return {k: v.detach().clone() for k, v in m.model.state_dict().items()}


@pytest.fixture(scope="module")
def trained():
    if not torch.cuda.is_available():
        pytest.fail("a test marked gpu ran without a HIP device")
    return {"LarvaNet": _train("LarvaNet", 200), "LarvaNetV2": _train("LarvaNetV2", 200)}


def _eval_images():
    g = torch.Generator().manual_seed(9)
    out = []
    for h, w in ((339, 510), (64, 64)):
        hr = _smooth_hr(g, 1, 4 * h, 4 * w)
        out.append((_lr(hr)[0].numpy(), hr[0].numpy()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra,weights", [("LarvaNet", (), "LarvaNet"), ("LarvaNetV2", (), "LarvaNetV2"),
                                                ("LarvaLeg", ("--leg=2",), "LarvaNet")])
def test_fp16_network_quality_against_fp32(hip_device, trained, name, extra, weights):
    from larvanet_amd.metrics import image_psnr, image_to_uint8
    m32 = _load(_model(name, extra, precision="fp32"), trained[weights])
    m16 = _load(_model(name, extra), trained[weights])
    for lr, hr in _eval_images():
        o32 = m32.upscale([lr], 4)[0]
        o16 = m16.upscale([lr], 4)[0]
        truth = image_to_uint8(hr)
        p32 = float(image_psnr(output_image=image_to_uint8(o32), truth_image=truth))
        p16 = float(image_psnr(output_image=image_to_uint8(o16), truth_image=truth))
        d = np.abs(o16.astype(np.float64) - o32)
        # the model must have learned something for the comparison to mean anything
        base = m32.model.base(torch.from_numpy(lr[None]).to(hip_device))[0].cpu().numpy()
        assert np.abs(o32 - base).mean() > 0.01
        print("%s %s: psnr fp32 %.5f fp16 %.5f (d %.2e dB), max |d| %.4f, mean |d| %.5f"
              % (name, lr.shape, p32, p16, p16 - p32, d.max(), d.mean()))
        assert abs(p16 - p32) <= 0.02 and d.max() <= 0.25 and d.mean() <= 0.03, (p32, p16, d.max(), d.mean())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["LarvaNet", "LarvaNetV2"])
def test_fp16_runs_are_bit_identical_and_bands_equal_the_whole_image(hip_device, trained, name):
    from larvanet_amd import image_utils
    m = _load(_model(name), trained[name])
    g = torch.Generator().manual_seed(12)
    x = _lr(_smooth_hr(g, 1, 4 * 160, 4 * 96))[0].numpy()
    a = m.upscale([x], 4)[0]
    b = m.upscale([x], 4)[0]
    assert np.array_equal(a, b)
    halo = m.receptive_halo()
    bands = [image_utils.upscale_band(m, x, 4, r0, r1, halo) for r0, r1 in ((0, 50), (50, 110), (110, 160))]
    assert np.array_equal(np.concatenate(bands, axis=1), a)


@pytest.mark.gpu
def test_captured_fp16_batch_forward_equals_eager(hip_device, trained):
    m = _load(_model("LarvaNetV2"), trained["LarvaNetV2"])
    g = torch.Generator().manual_seed(13)
    x = _lr(_smooth_hr(g, 16, 192, 192)).to(hip_device)
    with torch.no_grad():
        eager = m._forward_nograd(x).clone()
        outs = [m.fwd_runtime(x).clone() for _ in range(3)]   # the second call captures, the third replays
        m32 = m._infer_graphs.get(((16, 3, 48, 48), "fp32"))
        assert m32 is None and m._infer_graphs[((16, 3, 48, 48), "fp16")] is not False
    assert all(torch.equal(o, eager) for o in outs)
    assert not m.fp16_overflowed()


@pytest.mark.gpu
def test_overflow_raises_floating_point_error(hip_device, trained):
    m = _load(_model("LarvaNet"), trained["LarvaNet"])
    x = _eval_images()[1][0]
    m.upscale([x], 4)
    with torch.no_grad():
        m.model.head.feature_extraction.weight.mul_(1e4)   # head output >> 65504
    with pytest.raises(FloatingPointError, match="--precision fp16"):
        m.upscale([x], 4)
    with torch.no_grad(), pytest.raises(FloatingPointError, match="--precision fp16"):
        m.test([x])
    with torch.no_grad():
        m.fwd_runtime(torch.from_numpy(x[None]).to(hip_device))   # no sync, no raise ...
    assert m.fp16_overflowed() is True                             # ... but the flag is exposed
    assert m.fp16_overflowed() is False


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["LarvaNet", "LarvaNetV2"])
def test_training_is_unchanged_and_fp16_follows_new_weights(hip_device, tmp_path, name):
    a = _model(name, precision="fp32", training=True, blocks=(2, 2))
    b = _model(name, precision="fp16", training=True, blocks=(2, 2))
    for k, v in a.model.state_dict().items():
        assert torch.equal(v, b.model.state_dict()[k]), k
    ckpt0 = b.save(str(tmp_path))
    g = torch.Generator().manual_seed(14)
    img = _lr(_smooth_hr(g, 1, 4 * 40, 4 * 52))[0].numpy()
    first = b.upscale([img], 4)[0]
    assert np.array_equal(b.upscale([img], 4)[0], first)   # (the second call of the shape replays a captured graph)
    for step in range(3):
        hr = _smooth_hr(g, 16, 192, 192)
        x, t = _lr(hr).to(hip_device), hr.to(hip_device)
        la = a.train_step_larva(None, _NoVal(), x, t)
        lb = b.train_step_larva(None, _NoVal(), x, t)
        assert la == lb, step
    for k, v in a.model.state_dict().items():
        assert torch.equal(v, b.model.state_dict()[k]), k
    fresh = _load(_model(name, blocks=(2, 2)), {k: v.clone() for k, v in b.model.state_dict().items()})
    after = b.upscale([img], 4)[0]
    assert not np.array_equal(after, first) and np.array_equal(after, fresh.upscale([img], 4)[0])
    b.restore(ckpt0)
    again = _model(name, blocks=(2, 2))
    again.restore(ckpt0)
    assert np.array_equal(b.upscale([img], 4)[0], again.upscale([img], 4)[0])
    assert np.array_equal(b.upscale([img], 4)[0], first)
