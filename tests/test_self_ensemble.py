"""Geometric self-ensemble (--self_ensemble): image_utils.dihedral / dihedral_inv / self_ensemble, the kernels of
csrc/larva_ensemble.hip (kernels.dihedral_inputs / dihedral_mean) and the plugins' image entry points with the flag.
Host logic runs anywhere; kernels and networks are marked gpu.

Every GPU comparison but one is exact (np.array_equal).  The contract: with the flag, upscale / upscale_u8 return

    E(x) = (((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125f,   v_t = dihedral_inv(f(dihedral(x, t)), t)

in float32 in this order (and image_to_uint8 of it), f being the plain upscale of a second instance of the same plugin
with the same weights and the flag off.  The one inexact comparison is the equivariance of E, whose two sides add the same
eight images in different orders: its bound is derived at the test."""
import importlib

import numpy as np
import pytest
import torch

PLUGINS = ("LarvaNet", "LarvaNetV2", "LarvaLeg", "LarvaLegV2")
BLOCKS = (1, 1)


def _model(name="LarvaNet", extra=(), precision="fp32", ensemble=False, blocks=BLOCKS, scale=4):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks)),
                  "--precision=" + precision] + (["--self_ensemble"] if ensemble else []) + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[scale])
    m.strict_graph = True
    return m


def _blocks_image(seed, h, w):
    """uint8 (h, w, 3): hard-edged 4 x 4 blocks, every block and colour drawn from {0, 64, 200, 255}."""
    rng = np.random.default_rng(seed)
    levels = np.array([0, 64, 200, 255], np.uint8)
    grid = levels[rng.integers(0, 4, ((h + 3) // 4, (w + 3) // 4, 3))]
    return np.ascontiguousarray(np.repeat(np.repeat(grid, 4, 0), 4, 1)[:h, :w])


def _chw(a):
    return np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32)


def _composition(plain, a_u8, scale):
    """E(x) float32 (3, sH, sW) from eight plain upscale calls on the host, as the module docstring defines it."""
    from larvanet_amd import image_utils as U
    return U.self_ensemble(lambda x: plain.upscale([x], scale)[0], _chw(a_u8), axes=(1, 2))


# ---------------------------------------------------------------- host
def test_dihedral_inverts_and_its_eight_images_differ():
    from larvanet_amd import image_utils as U
    for shape, axes in (((5, 7, 3), (0, 1)), ((3, 5, 7), (1, 2))):
        a = np.arange(np.prod(shape), dtype=np.int64).reshape(shape)
        images = [np.ascontiguousarray(U.dihedral(a, t, axes)) for t in range(8)]
        for t in range(8):
            assert np.array_equal(U.dihedral_inv(U.dihedral(a, t, axes), t, axes), a), (shape, t)
            swapped = list(shape)
            if t & 4:
                swapped[axes[0]], swapped[axes[1]] = swapped[axes[1]], swapped[axes[0]]
            assert images[t].shape == tuple(swapped)
    a = np.arange(6 * 6 * 3).reshape(6, 6, 3)   # (square: all eight have one shape, so they can be compared)
    images = [U.dihedral(a, t) for t in range(8)]
    for t in range(8):
        for u in range(t + 1, 8):
            assert not np.array_equal(images[t], images[u]), (t, u)
    # the written-out definition: rows, then columns, then the swap
    assert np.array_equal(U.dihedral(a, 7), a[::-1][:, ::-1].swapaxes(0, 1))
    assert np.array_equal(U.dihedral_inv(a, 7), a.swapaxes(0, 1)[:, ::-1][::-1])


def test_self_ensemble_on_the_host_is_the_fixed_order_float32_sum():
    from larvanet_amd import image_utils as U
    rng = np.random.default_rng(3)
    x = rng.random((3, 5, 7)).astype(np.float32)
    calls = []

    def f(a):
        calls.append(a.shape)
        return a * np.float32(3.0) + np.float32(1.0)   # (pointwise: commutes with every transform)

    e = U.self_ensemble(f, x, axes=(1, 2))
    assert calls == [(3, 5, 7)] * 4 + [(3, 7, 5)] * 4 and e.dtype == np.float32
    v = x * np.float32(3.0) + np.float32(1.0)
    acc = v
    for _ in range(7):
        acc = acc + v
    assert np.array_equal(e, acc * np.float32(0.125))


@pytest.mark.parametrize("name", PLUGINS)
def test_self_ensemble_flag_parses_and_is_off_by_default(name):
    extra = ["--leg=2"] if name.startswith("LarvaLeg") else []
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    args, rest = m.parse_args(["--num_modules=2", "--num_blocks=1,1", "--something_else=1"] + extra)
    assert args.self_ensemble is False and rest == ["--something_else=1"] and m._self_ensemble() is False
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    args, rest = m.parse_args(["--num_modules=2", "--num_blocks=1,1", "--self_ensemble"] + extra)
    assert args.self_ensemble is True and rest == [] and m._self_ensemble() is True


def test_ensemble_source_is_built_and_wrapped_and_the_drivers_document_the_flag():
    from larvanet_amd import build, kernels as K
    assert "larva_ensemble.hip" in build.SOURCES
    assert callable(K.dihedral_inputs) and callable(K.dihedral_mean)
    for mod in ("upscale_images", "evaluate"):
        assert "--self_ensemble" in importlib.import_module("larvanet_amd." + mod).__doc__


# ---------------------------------------------------------------- kernels (GPU)
INPUT_SHAPES = [(2, 5, 7), (1, 8, 8), (1, 1, 1), (1, 33, 70)]


def _want_inputs(x_nchw):
    from larvanet_amd import image_utils as U
    a = np.stack([U.dihedral(img, t, (1, 2)) for img in x_nchw for t in range(4)])
    b = np.stack([U.dihedral(img, t, (1, 2)) for img in x_nchw for t in range(4, 8)])
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("shape", INPUT_SHAPES)
def test_dihedral_inputs_equal_the_numpy_definition(hip_device, shape):
    from larvanet_amd import kernels as K
    n, h, w = shape
    x = np.random.default_rng(h * 100 + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    want_a, want_b = _want_inputs(x.transpose(0, 3, 1, 2).astype(np.float32))
    a, b = K.dihedral_inputs(torch.from_numpy(x).to(hip_device))
    assert a.dtype == torch.float32 and tuple(a.shape) == (4 * n, 3, h, w) and tuple(b.shape) == (4 * n, 3, w, h)
    assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(b.cpu().numpy(), want_b)
    # the float form, on values a byte cannot hold
    xf = (np.random.default_rng(h + w).random((n, 3, h, w)) * 300 - 20).astype(np.float32)
    want_a, want_b = _want_inputs(xf)
    a, b = K.dihedral_inputs(torch.from_numpy(xf).to(hip_device))
    assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(b.cpu().numpy(), want_b)


MEAN_SHAPES = [(2, 20, 28), (1, 32, 32), (1, 1, 1), (1, 27, 42), (1, 132, 280)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MEAN_SHAPES)
def test_dihedral_mean_equals_the_fixed_order_sum(hip_device, shape):
    from larvanet_amd import image_utils as U, kernels as K
    from larvanet_amd.metrics import image_to_uint8
    n, h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    # eight noisy copies (+-5) of one image on -15 .. 275 per slot group: all values in [-20, 280], and the mean leaves
    # 0 .. 255 on both sides (eight independent draws would average to ~130 everywhere and never meet a clamp)
    base = (rng.random((n, 3, h, w)) * 290 - 15).astype(np.float32)
    noisy = [base + (rng.random(base.shape) * 10 - 5).astype(np.float32) for _ in range(8)]
    a = np.ascontiguousarray(np.stack([U.dihedral(noisy[t][i], t, (1, 2)) for i in range(n) for t in range(4)]))
    b = np.ascontiguousarray(np.stack([U.dihedral(noisy[t][i], t, (1, 2)) for i in range(n) for t in range(4, 8)]))
    assert a.min() >= -20 and a.max() <= 280 and b.min() >= -20 and b.max() <= 280
    want = np.empty((n, 3, h, w), np.float32)
    for i in range(n):
        acc = None
        for t in range(8):
            v = U.dihedral_inv(a[4 * i + t] if t < 4 else b[4 * i + t - 4], t, (1, 2))
            acc = v if acc is None else acc + v
        want[i] = acc * np.float32(0.125)
    da, db = torch.from_numpy(a).to(hip_device), torch.from_numpy(b).to(hip_device)
    got = K.dihedral_mean(da, db)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3, h, w)
    assert np.array_equal(got.cpu().numpy(), want)
    got8 = K.dihedral_mean(da, db, u8=True)
    want8 = image_to_uint8(want).transpose(0, 2, 3, 1)
    if h * w >= 100:
        assert (want < -0.5).any() and (want > 255.5).any()   # (both clamps act)
    assert got8.dtype == torch.uint8 and np.array_equal(got8.cpu().numpy(), want8)
    assert torch.equal(K.f32_chw_to_u8_hwc(got), got8)
    assert torch.equal(K.dihedral_mean(da, db), got) and torch.equal(K.dihedral_mean(da, db, u8=True), got8)


# ---------------------------------------------------------------- networks (GPU)
NETWORKS = [("LarvaNet", ()), ("LarvaNetV2", ()), ("LarvaLeg", ("--leg=1",))]
SIZES = ((16, 16), (9, 14), (12, 20))


def _assert_ensemble_equals_composition(ens, plain, a, scale, tag):
    from larvanet_amd.metrics import image_to_uint8
    want = _composition(plain, a, scale)
    got = ens.upscale([_chw(a)], scale)
    assert got.dtype == np.float32 and got.shape == (1,) + want.shape
    assert np.array_equal(got[0], want), tag
    got8 = ens.upscale_u8([a], scale)
    assert got8.dtype == np.uint8 and np.array_equal(got8[0], image_to_uint8(want).transpose(1, 2, 0)), tag
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("name,extra", NETWORKS, ids=[n for n, _ in NETWORKS])
def test_ensemble_equals_the_host_composition_of_plain_calls(hip_device, name, extra, precision):
    ens, plain = _model(name, extra, precision, ensemble=True), _model(name, extra, precision)
    for h, w in SIZES:
        a = _blocks_image(h * 100 + w, h, w)
        want = _assert_ensemble_equals_composition(ens, plain, a, 4, (name, precision, h, w))
        assert (want < -0.5).any() and (want > 255.5).any(), "the input does not exercise both clamps"
        t = ens.upscale_tensor([_chw(a)])
        assert t.is_cuda and np.array_equal(t.cpu().numpy()[0], want)
        t8 = ens.upscale_u8_tensor(torch.from_numpy(a[None]).to(hip_device))
        assert t8.is_cuda and np.array_equal(t8.cpu().numpy(), ens.upscale_u8([a], 4))


@pytest.mark.gpu
@pytest.mark.parametrize("scale,size", [(3, (9, 14)), (2, (12, 20))])
@pytest.mark.parametrize("name,extra", NETWORKS, ids=[n for n, _ in NETWORKS])
def test_ensemble_at_x2_and_x3(hip_device, name, extra, scale, size):
    ens, plain = _model(name, extra, ensemble=True, scale=scale), _model(name, extra, scale=scale)
    a = _blocks_image(scale, *size)
    _assert_ensemble_equals_composition(ens, plain, a, scale, (name, scale))


@pytest.mark.gpu
def test_ensemble_of_an_image_above_the_large_inference_rule(hip_device):
    from larvanet_amd.autograd import is_large_inference
    assert is_large_inference(1, 320, 330)
    ens, plain = _model("LarvaNet", precision="fp16", ensemble=True), _model("LarvaNet", precision="fp16")
    a = _blocks_image(5, 320, 330)
    _assert_ensemble_equals_composition(ens, plain, a, 4, "320 x 330")
    assert not getattr(ens, "_infer_graphs_se", None)   # (runs eagerly, repeated shape or not)


@pytest.mark.gpu
def test_eight_slots_above_the_rule_of_an_image_below_it(hip_device):
    """120 x 120 is a small inference, its eight slots together are a large one: the ensemble's forward runs eagerly, but
    with the head kernel of the plain call (the two head kernels differ in the last bits)."""
    from larvanet_amd.autograd import HeadFn, is_large_inference
    assert not is_large_inference(1, 120, 120) and is_large_inference(8, 120, 120)
    ens, plain = _model("LarvaNet", ensemble=True), _model("LarvaNet")
    a = _blocks_image(12, 120, 120)
    for _ in range(2):
        _assert_ensemble_equals_composition(ens, plain, a, 4, "120 x 120")
    assert not getattr(ens, "_infer_graphs_se", None) and HeadFn.rule_batch is None


@pytest.mark.gpu
def test_batch_of_two_images_keeps_each_image_apart(hip_device):
    ens, plain = _model("LarvaNet", ensemble=True), _model("LarvaNet")
    imgs = [_blocks_image(70 + i, 9, 14) for i in range(2)]
    got = ens.upscale([_chw(a) for a in imgs], 4)
    for i, a in enumerate(imgs):
        assert np.array_equal(got[i], _composition(plain, a, 4)), i


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_eager_capture_replay_agree_and_the_plain_paths_capture_what_they_did(hip_device, precision):
    ens, plain = _model("LarvaNet", precision=precision, ensemble=True), _model("LarvaNet", precision=precision)
    for h, w in ((16, 16), (9, 14)):
        a = _blocks_image(h + w, h, w)
        first8, firstf = ens.upscale_u8([a], 4), ens.upscale([_chw(a)], 4)
        for call in range(2):   # the capture, then a replay
            assert np.array_equal(ens.upscale_u8([a], 4), first8), (h, w, call)
            assert np.array_equal(ens.upscale([_chw(a)], 4), firstf), (h, w, call)
    keys = set(ens._infer_graphs_se)
    assert keys == {((1, h, w, 3), precision, "u8", "se") for h, w in ((16, 16), (9, 14))} | \
        {((1, 3, h, w), precision, "f32", "se") for h, w in ((16, 16), (9, 14))}
    assert all(v is not False for v in ens._infer_graphs_se.values())
    assert not getattr(ens, "_infer_graphs", None) and not getattr(ens, "_infer_graphs_u8", None)
    # with the flag off: the bytes of the plain call, its own two tables and no third
    a = _blocks_image(25, 9, 14)
    want = plain.upscale([_chw(a)], 4)
    from larvanet_amd.metrics import image_to_uint8
    for call in range(3):
        assert np.array_equal(plain.upscale_u8([a], 4)[0], image_to_uint8(want[0]).transpose(1, 2, 0))
        assert np.array_equal(plain.upscale([_chw(a)], 4), want)
    assert set(plain._infer_graphs_u8) == {((1, 9, 14, 3), precision, "u8")}
    assert set(plain._infer_graphs) == {((1, 3, 9, 14), precision)}
    assert not plain._infer_graphs_se and not plain._infer_graphs_se.seen
    # test / fwd_runtime never ensemble
    with torch.no_grad():
        x = torch.from_numpy(_chw(a)[None]).to(hip_device)
        assert np.array_equal(ens.test([_chw(a)]).cpu().numpy(), want)
        assert np.array_equal(ens.fwd_runtime(x).cpu().numpy(), want)


@pytest.mark.gpu
def test_evaluate_u8_tensor_scores_the_ensemble_image(hip_device):
    from larvanet_amd import kernels as K
    ens = _model("LarvaNet", ensemble=True)
    a = _blocks_image(31, 12, 20)
    truth = np.random.default_rng(32).integers(0, 256, (1, 48 + 3, 80 + 5, 3), dtype=np.uint8)
    x, t = torch.from_numpy(a[None]).to(hip_device), torch.from_numpy(truth).to(hip_device)
    image = ens.upscale_u8_tensor(x)
    for channel, shave, ssim in (("y", None, True), ("rgb", 0, True), ("y", 2, False)):
        got = ens.evaluate_u8_tensor(x, t, shave=shave, channel=channel, ssim=ssim)
        rec = K.u8_metrics(image[0], t[0], 4 if shave is None else shave, channel, ssim).cpu().numpy()
        assert got == [K.metrics_from_record(rec)], (channel, shave, ssim)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_streams_with_the_flag_equal_per_image_calls(hip_device, precision):
    from larvanet_amd import kernels as K, pipeline
    images = [_blocks_image(40 + i, h, w) for i, (h, w) in enumerate(((12, 20), (16, 16), (12, 20), (16, 16)))]
    one = _model("LarvaNet", precision=precision, ensemble=True)
    want = [one.upscale_u8([a], 4)[0] for a in images]
    m = _model("LarvaNet", precision=precision, ensemble=True)
    got = list(pipeline.upscale_stream(m, iter(images), 4, depth=2))
    assert len(got) == 4 and all(np.array_equal(g, w) for g, w in zip(got, want))
    truths = [np.random.default_rng(60 + i).integers(0, 256, (4 * a.shape[0], 4 * a.shape[1], 3), dtype=np.uint8)
              for i, a in enumerate(images)]
    scored = list(pipeline.evaluate_stream(m, zip(images, truths), 4, channel="rgb", depth=2))
    for i, (s, w, t) in enumerate(zip(scored, want, truths)):
        rec = K.u8_metrics(torch.from_numpy(w).to(hip_device), torch.from_numpy(t).to(hip_device), 4, "rgb").cpu().numpy()
        assert s == K.metrics_from_record(rec), i


@pytest.mark.gpu
def test_ensemble_is_equivariant_up_to_the_order_of_an_eight_term_sum(hip_device):
    """E(dihedral(x, t)) and dihedral(E(x), t) add the same eight images -- the transforms form a group, so the eight
    inputs of one side are a permutation of the other's, and a pixel's result does not depend on its slot -- in two
    orders.  An 8-term fp32 sum has 7 roundings of relative size 2^-24 each on partial sums of at most 8 max|v_i|; after
    the exact division by 8 two orders differ by at most 2 * 7 * 2^-24 * max|v_i| to first order = 7 * 2^-23 max|v_i|,
    and the bar is twice that for the higher-order terms: 2 * 7 * 2^-23 * max_i |v_i| per pixel."""
    from larvanet_amd import image_utils as U
    ens, plain = _model("LarvaNet", ensemble=True), _model("LarvaNet")
    a = _blocks_image(9, 12, 20)
    x = _chw(a)
    members = np.stack([U.dihedral_inv(plain.upscale([np.ascontiguousarray(U.dihedral(x, t, (1, 2)))], 4)[0], t, (1, 2))
                        for t in range(8)])
    bound = 2 * 7 * 2.0 ** -23 * np.abs(members).max(axis=0)
    e = ens.upscale([x], 4)[0]
    for t in range(8):
        et = ens.upscale([np.ascontiguousarray(U.dihedral(x, t, (1, 2)))], 4)[0]
        d = np.abs(et.astype(np.float64) - U.dihedral(e, t, (1, 2)))
        bt = U.dihedral(bound, t, (1, 2))
        print("t = %d: max |d| %.3e, max |d| / bound %.3f" % (t, d.max(), (d / bt).max()))
        assert (d <= bt).all(), t


@pytest.mark.gpu
def test_fp16_overflow_raises_from_the_ensemble_as_from_a_plain_call(hip_device):
    ens, plain = _model("LarvaNet", precision="fp16", ensemble=True), _model("LarvaNet", precision="fp16")
    a = _blocks_image(4, 12, 20)
    ens.upscale_u8([a], 4)
    for m in (plain, ens):
        with torch.no_grad():
            m.model.head.feature_extraction.weight.mul_(1e4)   # head output >> 65504
        m.model.invalidate_packed_weights()
    with pytest.raises(FloatingPointError, match="--precision fp16"):
        plain.upscale([_chw(a)], 4)
    with pytest.raises(FloatingPointError, match="--precision fp16"):
        ens.upscale([_chw(a)], 4)
    with pytest.raises(FloatingPointError, match="--precision fp16"):
        ens.upscale_u8([a], 4)
    with pytest.raises(FloatingPointError, match="--precision fp16"):
        ens.evaluate_u8_tensor(torch.from_numpy(a[None]).to(hip_device),
                               torch.zeros((1, 48, 80, 3), dtype=torch.uint8, device=hip_device))
