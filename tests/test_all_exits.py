"""All-exit inference: every exit's image of the multi-exit network from one forward pass (upscale_exits and its
siblings, half.HalfForward.exits, LarvaNetModule.forward_exits) and the two fp16 job launches under it
(larva_f16_conv3x3_jobs, larva_f16_conv3x3_shuffle_base_jobs).  Host logic runs anywhere; kernels, networks and the driver
are marked gpu.

Every comparison is bitwise.  The oracle of a job launch is the single-job entry point on the same operands (and, on
small-integer operands, the float64 sum of tests/exact_ref.py); the oracle of exit i is a `LarvaLeg --leg=i+1` plugin
with the same state_dict, precision and input, the last exit also LarvaNet.upscale itself.  No pixel of this library
depends on its tile, batch slot or launch grouping, so nothing weaker than equality is asked."""
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

import exact_ref as X

gpu = pytest.mark.gpu
NEW_METHODS = ("upscale_exits", "upscale_exits_tensor", "upscale_exits_u8", "upscale_exits_u8_tensor",
               "evaluate_exits_u8_tensor")
BLOCKS = (1, 2, 1, 1)
NET_ARGS = ["--num_modules=%d" % len(BLOCKS), "--num_blocks=" + ",".join(map(str, BLOCKS))]


def _plugin(name="LarvaNet", extra=(), precision="fp32", scale=4):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(NET_ARGS + ["--precision=" + precision] + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[scale])
    m.strict_graph = True
    return m


def _load(m, sd):
    m.model.load_state_dict({k: v.to(m.device) for k, v in sd.items()})
    m.model.invalidate_packed_weights()
    return m


def _random_state(m, seed):
    """Weights as init_conv draws them (kaiming normal, fan_in, * 0.1) from `seed`, and small non-zero biases so that a
    leg run with another leg's bias cannot pass."""
    from larvanet_amd.models.LarvaNet import init_conv
    torch.manual_seed(seed)
    sd = {}
    for name, mod in m.model.named_modules():
        if isinstance(mod, torch.nn.Conv2d):
            conv = torch.nn.Conv2d(mod.in_channels, mod.out_channels, 3, padding=1)
            init_conv(conv)
            sd[name + ".weight"] = conv.weight.detach().clone()
            sd[name + ".bias"] = torch.randn(mod.out_channels) * 0.05
    assert set(sd) == set(m.model.state_dict())
    return sd


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------- host
def test_all_exits_flag_parses_in_both_drivers_and_defaults_to_off():
    from larvanet_amd import evaluate, upscale_images
    for mod in (evaluate, upscale_images):
        args, _ = mod.build_parser().parse_known_args([])
        assert args.all_exits is False
        args, rest = mod.build_parser().parse_known_args(["--all_exits", "--num_modules=4"])
        assert args.all_exits is True and rest == ["--num_modules=4"]
    assert upscale_images.exit_output_name("0801x4.PNG", 0) == "0801x4_exit1.png"


def test_result_line_without_an_exit_index_is_the_line_it_was():
    from larvanet_amd.evaluate import result_line
    both = {"psnr": 31.23456, "ssim": 0.87654}
    assert result_line(4, 3, 10, both) == "x4, 3/10, psnr=31.2346, ssim=0.8765"
    assert result_line(2, 1, 1, {"psnr": 31.0, "ssim": None}) == "x2, 1/1, psnr=31.0000"
    assert result_line(4, 3, 10, both, exit_index=0) == "x4, 3/10, exit 1, psnr=31.2346, ssim=0.8765"
    assert result_line(4, 3, 10, {"psnr": 31.0, "ssim": None}, exit_index=3) == "x4, 3/10, exit 4, psnr=31.0000"


def test_every_plugin_of_the_family_has_the_methods_and_a_form_field():
    from larvanet_amd.infer_graphs import Form
    assert not Form().exits and Form(exits=True).exits and not Form(True, True).exits
    assert tuple(Form(True, False, exits=True)) == (True, False)   # (callers unpack the pair; exits rides along)
    assert Form(exits=True) != Form() and Form(True, exits=True) == Form(True, False, True)
    for name in ("LarvaNet", "LarvaLeg"):
        m = importlib.import_module("larvanet_amd.models." + name).create_model()
        for method in NEW_METHODS:
            assert callable(getattr(m, method)), (name, method)


def test_exit_route_lists_the_legs_of_the_route():
    full = _plugin("LarvaNet")
    bodies, legs = full.model.exit_route()
    assert bodies == 4 and [id(leg) for leg in legs] == [id(getattr(full.model, "body_%d" % i).leg) for i in range(4)]
    two = _plugin("LarvaLeg", ("--leg=2",))
    bodies, legs = two.model.exit_route()
    assert bodies == 2 and len(legs) == 2 and legs[1] is two.model.body_1.leg
    assert len(_plugin("LarvaLegV2", ("--leg=3",)).model.exit_route()[1]) == 3   # (V2's early exits are legs too)
    with pytest.raises(ValueError, match="LarvaLeg"):
        _plugin("LarvaLeg", ("--leg=0",)).model.exit_route()


def test_models_without_per_body_exits_and_the_self_ensemble_are_refused():
    image = np.zeros((3, 8, 8), np.float32)
    image8 = np.zeros((8, 8, 3), np.uint8)
    v2 = _plugin("LarvaNetV2")
    with pytest.raises(ValueError, match="LarvaNetV2"):
        v2.model.exit_route()
    with pytest.raises(ValueError, match="LarvaNetV2"):
        v2.upscale_exits([image], 4)
    with pytest.raises(ValueError, match="LarvaNetV2"):
        v2.upscale_exits_u8([image8], 4)
    with pytest.raises(ValueError, match="LarvaNetV2"):
        v2.evaluate_exits_u8_tensor(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
    ens = _plugin("LarvaNet", ("--self_ensemble",))
    for call in (lambda: ens.upscale_exits([image], 4), lambda: ens.upscale_exits_tensor([image]),
                 lambda: ens.upscale_exits_u8([image8], 4)):
        with pytest.raises(ValueError, match="self_ensemble"):
            call()
    plain = _plugin("LarvaNet")
    with pytest.raises(ValueError, match="upscales by 4"):
        plain.upscale_exits([image], 2)
    with pytest.raises(TypeError):
        plain.upscale_exits_u8([image], 4)   # (float images: upscale_u8's own argument checks)


# ---------------------------------------------------------------- the job launches (GPU)
JOB_SHAPES = [(1, 3, 4), (2, 48, 48), (1, 37, 127)]   # thinner than a tile; several tiles; partial row and column tiles
JOB_COUNTS = [1, 2, 3, 8]
PATTERN = 0xA5


@functools.lru_cache(maxsize=None)
def _job_operands(shape, njobs):
    """Per job its own source, weight, bias (first conv) and a second weight and bias (leg end), and one shared base."""
    n, h, w = shape
    rng = np.random.default_rng([n, h, w, njobs])
    jobs = []
    for _ in range(njobs):
        jobs.append({"src": np.abs(rng.standard_normal((n, h, w, 48)) * 2).astype(np.float16),
                     "w": (rng.standard_normal((48, 48, 3, 3)) * 0.05 + 0.02).astype(np.float32),
                     "b": (rng.standard_normal(48) * 0.2).astype(np.float32),
                     "w2": (rng.standard_normal((48, 48, 3, 3)) * 0.05).astype(np.float32),
                     "b2": (rng.standard_normal(48) * 3).astype(np.float32)})
    base = (rng.random((n, 3, 4 * h, 4 * w)) * 300 - 20).astype(np.float32)   # (both uint8 clamps are reached)
    return jobs, base


def _guarded(njobs, per_job_shape, dtype, dev):
    """A buffer of njobs + 2 outputs filled with a byte pattern; the launch gets the njobs in the middle."""
    buf = torch.full((njobs + 2,) + tuple(per_job_shape), PATTERN, dtype=torch.uint8, device=dev)
    elem = torch.empty((), dtype=dtype).element_size()
    typed = buf.view(-1).view(dtype).view((njobs + 2,) + tuple(per_job_shape[:-1]) + (per_job_shape[-1] // elem,))
    return buf, typed[1:1 + njobs]


def _assert_guards(buf, what):
    edge = torch.stack([buf[0].reshape(-1), buf[-1].reshape(-1)])
    assert bool((edge == PATTERN).all()), "%s: bytes outside the njobs outputs were written" % what


@gpu
@pytest.mark.parametrize("njobs", JOB_COUNTS)
@pytest.mark.parametrize("shape", JOB_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_job_launches_equal_the_single_job_entry_points(hip_device, shape, njobs):
    """Job j of both launches, bit for bit against the single-job entry point on job j's operands: both epilogues of the
    first conv, the fp32 and the uint8 leg end; the slots before and after the njobs outputs keep their bytes."""
    from larvanet_amd import kernels as K
    n, h, w = shape
    jobs, base = _job_operands(shape, njobs)
    flag = torch.zeros(1, dtype=torch.int32, device=hip_device)
    srcs = [_dev(j["src"], hip_device) for j in jobs]
    wpk = [K.f16_pack_weights(_dev(j["w"], hip_device)) for j in jobs]
    bias = [_dev(j["b"], hip_device) for j in jobs]
    wpk2 = [K.f16_pack_weights(_dev(j["w2"], hip_device)) for j in jobs]
    bias2 = [_dev(j["b2"], hip_device) for j in jobs]
    based = _dev(base, hip_device)
    tag = "%s, %d jobs" % (shape, njobs)
    hidden = None
    for relu in (False, True):
        buf, out = _guarded(njobs, (n, h, w, 48 * 2), torch.float16, hip_device)
        got = K.f16_conv3x3_jobs(srcs, wpk, bias, flag, relu=relu, out=out)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (njobs, n, h, w, 48)
        for j in range(njobs):
            single = K.f16_conv3x3(srcs[j], wpk[j], bias[j], flag, relu=relu)
            X.assert_bits_equal(got[j], single, "larva_f16_conv3x3_jobs %s relu=%s job %d" % (tag, relu, j))
        _assert_guards(buf, "larva_f16_conv3x3_jobs " + tag)
        hidden = got
    mids = [hidden[j] for j in range(njobs)]   # (the ReLU outputs: what the leg ends read in the network)
    buf, out = _guarded(njobs, (n, 3, 4 * h, 4 * w * 4), torch.float32, hip_device)
    got = K.f16_conv3x3_shuffle_base_jobs(mids, wpk2, bias2, based, out=out)
    buf8, out8 = _guarded(njobs, (n, 4 * h, 4 * w, 3), torch.uint8, hip_device)
    got8 = K.f16_conv3x3_shuffle_base_jobs(mids, wpk2, bias2, based, flag, u8=True, out=out8)
    assert tuple(got.shape) == (njobs, n, 3, 4 * h, 4 * w) and tuple(got8.shape) == (njobs, n, 4 * h, 4 * w, 3)
    for j in range(njobs):
        X.assert_bits_equal(got[j], K.f16_conv3x3_shuffle_base(mids[j], wpk2[j], bias2[j], based),
                            "larva_f16_conv3x3_shuffle_base_jobs fp32 %s job %d" % (tag, j))
        X.assert_bits_equal(got8[j], K.f16_conv3x3_shuffle_base_u8(mids[j], wpk2[j], bias2[j], based, flag),
                            "larva_f16_conv3x3_shuffle_base_jobs uint8 %s job %d" % (tag, j))
    _assert_guards(buf, "larva_f16_conv3x3_shuffle_base_jobs fp32 " + tag)
    _assert_guards(buf8, "larva_f16_conv3x3_shuffle_base_jobs uint8 " + tag)
    assert int(flag.item()) == 0


@gpu
def test_job_launches_on_integer_operands_equal_the_float64_sums(hip_device):
    """(1, 13, 21), 4 jobs, operands of tests/exact_ref.py: |x| <= 4, |w| <= 2 over K = 432 gives |sum| <= 3 456 + bias,
    far below 65 504 and 2^24, so the fp16 of the exact sum (first conv) and the exact fp32 sum + base (leg end) are the
    only right answers."""
    from larvanet_amd import kernels as K
    n, h, w, njobs = 1, 13, 21, 4
    rng = X.rng_of(n, h, w, njobs, 7)
    flag = torch.zeros(1, dtype=torch.int32, device=hip_device)
    srcs = [X.ints(rng, (n, h, w, 48), 4) for _ in range(njobs)]
    ws = [X.weights(rng, (48, 48, 3, 3), 2) for _ in range(njobs)]
    bs = [X.ints(rng, (48,), 3) for _ in range(njobs)]
    base = X.ints(rng, (n, 3, 4 * h, 4 * w), 400, lo=-150)
    refs = {"plain": [], "relu": [], "img": []}
    for j in range(njobs):
        for epi in ("plain", "relu"):
            y, inter = X.conv([srcs[j].transpose(0, 3, 1, 2)], ws[j], bs[j], relu=epi == "relu")
            X.assert_exact_precondition(inter)
            X.assert_exact_precondition([y], X.HALF_MAX + 1)
            refs[epi].append(y.transpose(0, 2, 3, 1))
        img = X.pixel_shuffle(X.conv([srcs[j].transpose(0, 3, 1, 2)], ws[j], bs[j])[0], 4) + base
        X.assert_exact_precondition([img])
        refs["img"].append(img)
    assert any((r < 0).any() for r in refs["img"]) and any((r > 255).any() for r in refs["img"])
    sd = [_dev(s.astype(np.float16), hip_device) for s in srcs]
    wpk = [K.f16_pack_weights(_dev(wt, hip_device)) for wt in ws]
    bd = [_dev(b, hip_device) for b in bs]
    based = _dev(base, hip_device)
    for epi in ("plain", "relu"):
        got = K.f16_conv3x3_jobs(sd, wpk, bd, flag, relu=epi == "relu")
        for j in range(njobs):
            X.assert_bits_equal(got[j], refs[epi][j].astype(np.float16), "larva_f16_conv3x3_jobs %s job %d" % (epi, j))
    got = K.f16_conv3x3_shuffle_base_jobs(sd, wpk, bd, based)
    got8 = K.f16_conv3x3_shuffle_base_jobs(sd, wpk, bd, based, flag, u8=True)
    for j in range(njobs):
        X.assert_bits_equal(got[j], refs["img"][j], "larva_f16_conv3x3_shuffle_base_jobs fp32 job %d" % j)
        want8 = np.clip(refs["img"][j], 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
        X.assert_bits_equal(got8[j], want8, "larva_f16_conv3x3_shuffle_base_jobs uint8 job %d" % j)
    assert int(flag.item()) == 0


@gpu
def test_job_launch_overflow_flag_is_set_by_one_job_alone(hip_device):
    """One-hot input, centre-tap weight 65504 in every job: 65504 is stored and leaves the flag at 0; with a bias of 1 in
    job 2 of 4 alone (65505 before rounding) the flag is set.  The uint8 leg end sets it for a NaN in job 2 alone."""
    from larvanet_amd import kernels as K
    n, h, w, njobs = 1, 6, 70, 4
    ci, co = 5, 37
    x = np.zeros((n, h, w, 48), np.float16)
    x[0, h - 1, w - 1, ci] = 1.0
    wt = np.zeros((48, 48, 3, 3), np.float32)
    wt[co, ci, 1, 1] = 65504.0
    wpk = K.f16_pack_weights(_dev(wt, hip_device))
    xd = _dev(x, hip_device)
    zero = np.zeros(48, np.float32)
    one, nan = zero.copy(), zero.copy()
    one[co], nan[co] = 1.0, np.nan
    want = np.zeros((n, h, w, 48), np.float16)
    want[0, h - 1, w - 1, co] = 65504.0
    for bias2, expect in ((zero, 0), (one, 1)):
        flag = torch.zeros(1, dtype=torch.int32, device=hip_device)
        biases = [_dev(bias2 if j == 2 else zero, hip_device) for j in range(njobs)]
        got = K.f16_conv3x3_jobs([xd] * njobs, [wpk] * njobs, biases, flag)
        assert int(flag.item()) == expect
        for j in range(njobs):
            if j != 2 or not expect:
                X.assert_bits_equal(got[j], want, "job %d beside an overflowing one" % j)
    base = _dev(np.zeros((n, 3, 4 * h, 4 * w), np.float32), hip_device)
    small = K.f16_pack_weights(_dev(np.zeros((48, 48, 3, 3), np.float32), hip_device))
    for bias2, expect in ((zero, 0), (nan, 1)):
        flag = torch.zeros(1, dtype=torch.int32, device=hip_device)
        biases = [_dev(bias2 if j == 2 else zero, hip_device) for j in range(njobs)]
        K.f16_conv3x3_shuffle_base_jobs([xd] * njobs, [small] * njobs, biases, base, flag, u8=True)
        assert int(flag.item()) == expect


@gpu
def test_job_launches_refuse_bad_arguments_before_any_launch(hip_device):
    """The C entry points themselves: njobs out of range, a NULL pointer in an array, both or neither output array, a
    missing flag for uint8 and a grid that fits one job but not eight return hipErrorInvalidValue (1)."""
    from larvanet_amd import hip_lib, kernels as K
    lib = hip_lib.load()
    n, h, w = 1, 3, 4
    x = torch.zeros((n, h, w, 48), dtype=torch.float16, device=hip_device)
    wpk = K.f16_pack_weights(torch.zeros((48, 48, 3, 3), device=hip_device))
    b = torch.zeros(48, device=hip_device)
    out = torch.zeros((9, n, 3, 4 * h, 4 * w), device=hip_device)
    base = torch.zeros((n, 3, 4 * h, 4 * w), device=hip_device)
    flag = torch.zeros(1, dtype=torch.int32, device=hip_device)
    stream = torch.cuda.current_stream().cuda_stream

    def arr(t, k, hole=None):
        return hip_lib.ptr_array([None if i == hole else t.data_ptr() for i in range(k)])

    def outs(k):
        return hip_lib.ptr_array([out[i].data_ptr() for i in range(k)])

    def first(k, hole=(None, None, None), fl=flag, shape=(n, h, w)):
        return lib.larva_f16_conv3x3_jobs(k, arr(x, max(k, 1), hole[0]), arr(wpk, max(k, 1), hole[1]), arr(b, max(k, 1), hole[2]),
                                          1, outs(max(k, 1)), None if fl is None else fl.data_ptr(), *shape, stream)

    def second(k, f32=True, u8=False, fl=flag, hole=None):
        return lib.larva_f16_conv3x3_shuffle_base_jobs(k, arr(x, k, hole), arr(wpk, k), arr(b, k), base.data_ptr(),
                                                       outs(k) if f32 else None, outs(k) if u8 else None,
                                                       None if fl is None else fl.data_ptr(), n, h, w, stream)

    assert first(2) == 0 and second(2) == 0 and second(2, f32=False, u8=True) == 0 and second(2, fl=None) == 0
    bad = [first(0), first(9), first(2, hole=(1, None, None)), first(2, hole=(None, 0, None)), first(2, hole=(None, None, 1)),
           first(2, fl=None), first(2, shape=(0, h, w)), first(8, shape=(1 << 28, 1, 1)),   # (2^28 tiles fit one job's grid, not eight jobs')
           second(0), second(9), second(2, f32=True, u8=True), second(2, f32=False, u8=False),
           second(2, f32=False, u8=True, fl=None), second(2, hole=0)]
    assert bad == [1] * len(bad), bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------- networks (GPU)
@functools.lru_cache(maxsize=None)
def _family(precision, scale=4):
    """One LarvaNet and its four LarvaLeg --leg=k plugins over one random state_dict."""
    net = _plugin("LarvaNet", (), precision, scale)
    sd = _random_state(net, 1234)
    _load(net, sd)
    legs = [_load(_plugin("LarvaLeg", ("--leg=%d" % k,), precision, scale), sd) for k in range(1, len(BLOCKS) + 1)]
    return net, legs, sd


def _images(shape, seed):
    n, h, w = shape
    rng = np.random.default_rng([n, h, w, seed])
    return rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


@gpu
@pytest.mark.parametrize("precision,scale,shape", [("fp32", 4, (1, 13, 21)), ("fp32", 4, (2, 16, 24)), ("fp16", 4, (1, 13, 21)),
                                                   ("fp16", 4, (2, 16, 24)), ("fp32", 3, (1, 13, 21))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_exit_equals_its_larvaleg_plugin(hip_device, precision, scale, shape):
    """upscale_exits / upscale_exits_u8 [i] == LarvaLeg --leg=i+1 .upscale / .upscale_u8, the last also LarvaNet's own;
    LarvaLeg --leg=2 .upscale_exits is the first two.  (1, 13, 21): a width that is no multiple of 4 (row-padded
    activations at fp32); (2, 16, 24): a batch."""
    net, legs, _ = _family(precision, scale)
    img8 = _images(shape, 3)
    chw = [np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) + 0.25 for a in img8]   # (not byte-valued)
    n, h, w = shape
    tag = "%s x%d %s " % (precision, scale, shape)
    got = net.upscale_exits(chw, scale)
    got8 = net.upscale_exits_u8(list(img8), scale)
    assert got.shape == (4, n, 3, scale * h, scale * w) and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
    assert got8.shape == (4, n, scale * h, scale * w, 3) and got8.dtype == np.uint8
    for i, leg in enumerate(legs):
        X.assert_bits_equal(got[i], leg.upscale(chw, scale), tag + "upscale_exits[%d]" % i)
        X.assert_bits_equal(got8[i], leg.upscale_u8(list(img8), scale), tag + "upscale_exits_u8[%d]" % i)
    X.assert_bits_equal(got[-1], net.upscale(chw, scale), tag + "last exit against LarvaNet.upscale")
    X.assert_bits_equal(got8[-1], net.upscale_u8(list(img8), scale), tag + "last exit against LarvaNet.upscale_u8")
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[2], got[3])   # (the exits do differ)
    two = legs[1].upscale_exits(chw, scale)
    assert two.shape[0] == 2
    X.assert_bits_equal(two, got[:2], tag + "LarvaLeg --leg=2 .upscale_exits")
    X.assert_bits_equal(net.upscale_exits_tensor(chw), got, tag + "upscale_exits_tensor")
    X.assert_bits_equal(net.upscale_exits_u8_tensor(_dev(img8, hip_device)), got8, tag + "upscale_exits_u8_tensor")
    # one leg after the other instead of the batched launches: the same bits
    net.batch_exit_legs = False
    try:
        with torch.no_grad():
            X.assert_bits_equal(net._forward_nograd(_dev(np.stack(chw), hip_device), exits=True), got, tag + "legs one by one")
    finally:
        net.batch_exit_legs = None


@gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_captured_all_exit_forward_follows_restored_weights(hip_device, precision, tmp_path):
    """The second call at one shape is captured into the all-exit table and equals the first (eager) call; the plain
    upscale tables gain nothing; after restore() of other weights the replay follows them."""
    m = _plugin("LarvaNet", (), precision)
    sd = _random_state(m, 99)
    _load(m, sd)
    img8 = _images((2, 16, 24), 5)
    chw = [np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) for a in img8]
    eager = m.upscale_exits(chw, 4)
    assert not m._infer_graphs_ex
    second = m.upscale_exits(chw, 4)
    third = m.upscale_exits(chw, 4)
    key = ((2, 3, 16, 24), precision)
    assert set(m._infer_graphs_ex) == {key} and m._infer_graphs_ex[key] is not False
    assert not m._infer_graphs and not m._infer_graphs_u8 and not m._infer_graphs_se
    X.assert_bits_equal(second, eager, "captured call against the eager one")
    X.assert_bits_equal(third, eager, "replay against the eager one")
    eager8 = m.upscale_exits_u8(list(img8), 4)
    X.assert_bits_equal(m.upscale_exits_u8(list(img8), 4), eager8, "captured uint8 call against the eager one")
    assert set(m._infer_graphs_ex) == {key, ((2, 16, 24, 3), precision, "u8")} and not m._infer_graphs_u8
    other = _random_state(m, 100)
    path = os.path.join(str(tmp_path), "other.pth")
    torch.save(other, path)
    m.restore(path)
    fresh = _load(_plugin("LarvaNet", (), precision), other)
    want = fresh.upscale_exits(chw, 4)
    assert not np.array_equal(want, eager)
    X.assert_bits_equal(m.upscale_exits(chw, 4), want, "replay after restore()")
    X.assert_bits_equal(want[-1], fresh.upscale(chw, 4), "last exit of the restored weights")
    assert set(m._infer_graphs_ex) == {key, ((2, 16, 24, 3), precision, "u8")} and not m._infer_graphs


@gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_evaluate_exits_equals_the_larvaleg_plugins(hip_device, precision):
    """8 x 8 LR against a 32 x 32 truth, Y, shave 4: a 24 x 24 window (>= 11 for SSIM).  sse, psnr and ssim of every exit
    equal evaluate_u8_tensor of the matching LarvaLeg plugin exactly."""
    net, legs, _ = _family(precision)
    x = _dev(_images((2, 8, 8), 11), hip_device)
    truth = _dev(_images((2, 32, 32), 12), hip_device)
    got = net.evaluate_exits_u8_tensor(x, truth, shave=4, channel="y", ssim=True)
    assert len(got) == 2 and all(len(per_image) == 4 for per_image in got)
    for i, leg in enumerate(legs):
        want = leg.evaluate_u8_tensor(x, truth, shave=4, channel="y", ssim=True)
        for n in range(2):
            for field in ("sse", "psnr", "ssim", "n"):
                assert got[n][i][field] == want[n][field], (precision, n, i, field, got[n][i][field], want[n][field])
    rgb = net.evaluate_exits_u8_tensor(x, truth, channel="rgb", ssim=False)
    assert rgb[0][0]["ssim"] is None and rgb[0][3]["psnr"] == net.evaluate_u8_tensor(x, truth, channel="rgb", ssim=False)[0]["psnr"]
    with pytest.raises(ValueError):
        net.evaluate_exits_u8_tensor(x, truth[:1])


@gpu
def test_evaluate_driver_prints_and_writes_every_exit(hip_device, tmp_path, capsys):
    """evaluate --all_exits --lr_from_truth on two 32 x 32 PNGs: 4 result lines per image, 4 average lines, and with
    --output_path 8 files whose pixels are upscale_exits_u8 of the device-made inputs."""
    from larvanet_amd import evaluate, kernels as K
    from larvanet_amd.upscale_images import read_rgb, write_rgb
    net, legs, sd = _family("fp32")
    hr, sr = os.path.join(str(tmp_path), "HR"), os.path.join(str(tmp_path), "SR")
    os.makedirs(hr)
    truths = _images((2, 32, 32), 21)
    for k, name in enumerate(("a.png", "b.png")):
        write_rgb(truths[k], os.path.join(hr, name))
    ckpt = os.path.join(str(tmp_path), "w.pth")
    torch.save(sd, ckpt)
    capsys.readouterr()
    results = evaluate.main(["--model=LarvaNet", "--truth_path=" + hr, "--lr_from_truth", "--all_exits", "--output_path=" + sr,
                             "--restore_path=" + ckpt, "--io_threads=2"] + NET_ARGS)
    text = capsys.readouterr().out.splitlines()
    per_image = [line for line in text if re.match(r"x4, [12]/2, exit [1-4], psnr=[0-9.]+, ssim=[0-9.]+$", line)]
    averages = [line for line in text if re.match(r"- exit [1-4] average psnr=[0-9.]+, ssim=[0-9.]+$", line)]
    assert len(per_image) == 8 and len(averages) == 4, text
    assert [line.split(", ")[1:3] for line in per_image] == [["%d/2" % (i + 1), "exit %d" % (k + 1)] for i in range(2) for k in range(4)]
    assert sorted(os.listdir(sr)) == sorted("%s_exit%d.png" % (s, k) for s in "ab" for k in range(1, 5))
    for i, stem in enumerate("ab"):
        lr = K.bicubic_down_u8(_dev(truths[i], hip_device), 4).cpu().numpy()
        want = net.upscale_exits_u8([lr], 4)
        scored = net.evaluate_exits_u8_tensor(_dev(lr[None], hip_device), _dev(truths[i][None], hip_device))[0]
        for k in range(4):
            X.assert_bits_equal(read_rgb(os.path.join(sr, "%s_exit%d.png" % (stem, k + 1))), want[k, 0], "%s exit %d" % (stem, k + 1))
            assert results["%s.png" % stem][k] == scored[k]
    mean = sum(results[name][3]["psnr"] for name in ("a.png", "b.png")) / 2
    assert averages[3].startswith("- exit 4 average psnr=%.4f" % mean)


@gpu
def test_upscale_driver_writes_every_exit(hip_device, tmp_path):
    from larvanet_amd import upscale_images
    net, _, sd = _family("fp16")
    lr_dir, sr = os.path.join(str(tmp_path), "LR"), os.path.join(str(tmp_path), "SR")
    os.makedirs(lr_dir)
    image = _images((1, 9, 14), 31)[0]
    upscale_images.write_rgb(image, os.path.join(lr_dir, "p.png"))
    ckpt = os.path.join(str(tmp_path), "w.pth")
    torch.save(sd, ckpt)
    upscale_images.main(["--model=LarvaNet", "--input_path=" + lr_dir, "--output_path=" + sr, "--all_exits", "--precision=fp16",
                         "--restore_path=" + ckpt, "--io_threads=2"] + NET_ARGS)
    want = net.upscale_exits_u8([image], 4)
    assert sorted(os.listdir(sr)) == ["p_exit%d.png" % k for k in range(1, 5)]
    for k in range(4):
        X.assert_bits_equal(upscale_images.read_rgb(os.path.join(sr, "p_exit%d.png" % (k + 1))), want[k, 0], "exit %d" % (k + 1))
