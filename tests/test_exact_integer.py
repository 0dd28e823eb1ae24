"""The conv, weight-gradient, exit and fp16 kernels on small-integer data, bit for bit against float64.

Every matrix instruction of the library is v_mfma_f32_16x16x4f32 or v_mfma_f32_16x16x32_f16 with fp32 accumulation:
exact on operands whose products and partial sums are integers below 2^24.  On such data the result of every launch
family is independent of summation order, tiling, split count and staging mode and EQUALS the integer reference
(tests/exact_ref.py: torch's conv2d on float64 and numpy index maps).  No tolerance: a wrong tap, channel, halo column,
padding column or partition fails, however small its effect, and the failure names the element.  Each test asserts the
condition that makes equality legitimate (exact_ref.assert_exact_precondition) on the reference's own values BEFORE it
looks at a device result.  The one comparison that is not bitwise is the loss scalar of larva_loss_from_partials:
n multiplications, n - 1 additions and one division in fp32, bound (2n + 1) 2^-24 relative -- derived, not measured.

Ranges (derived): |x| <= 8, |w| <= 4 over K = 9 * 48 * 8 (an 8-source merge conv): |sum| <= 110 592; weight gradient
with |dy| <= 2, |x| <= 2 over 64 * 48 * 48 pixels: 589 824; fp16 operands |x| <= 4, |w| <= 2 over 8 sources: 27 648
< 65 504.  All far below 2^24 = 16 777 216."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import exact_ref as X

gpu = pytest.mark.gpu
LIMIT = X.LIMIT_F32


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


# =====================================================================================================================
# case lists (shared by the CPU precondition test and the GPU tests)
# =====================================================================================================================
EPIS = ("plain", "relu", "mask", "res0", "res01", "shuffle", "shuffle_base")

# (cout, cin per source, sources, N, H, W, pitch or None): what each shape is there for
CONV_SHAPES = [
    (48, 48, 1, 2, 9, 48, None),      # 16-byte staging, one tile column, three tile rows
    (48, 48, 1, 1, 7, 52, None),      # 16-byte staging; tile boundaries inside the image in both directions
    (48, 48, 1, 1, 5, 13, None),      # register-staged (W % 4 != 0)
    (48, 48, 1, 2, 9, 13, 16),        # pitched, W < pitch
    (48, 48, 1, 1, 10, 50, 52),       # pitched, W < pitch, two tile columns
    (48, 48, 1, 2, 1, 1, None),       # thinner than a tile
    (48, 48, 1, 1, 1, 97, None),
    (48, 48, 1, 2, 3, 1, None),
    (48, 48, 1, 3, 13, 20, None),     # strip tables: 5 + 4 + 4 rows
    (48, 48, 1, 1, 45, 128, None),    # 72 strip tiles per image: more than travel inside the kernel arguments
    (48, 48, 2, 2, 8, 36, None),      # n_src 2
    (48, 24, 4, 1, 9, 20, None),      # n_src 4 of 24 channels
    (48, 48, 8, 1, 9, 16, None),      # n_src 8: the V2 merge conv at its widest, K = 3456
    (48, 16, 1, 2, 9, 24, None),      # the head's shape on the MFMA kernel (two chunks)
    (32, 32, 1, 2, 9, 48, None),
    (32, 32, 2, 1, 7, 13, None),
    (32, 48, 1, 2, 8, 20, None),      # the padded x2 / x3 leg end
    (64, 64, 1, 2, 9, 52, None),
    (64, 64, 2, 1, 5, 15, 16),
]


def _conv_id(s):
    cout, cps, nsrc, n, h, w, p = s
    return "c%d-%dx%d-N%d-%dx%d%s" % (cout, nsrc, cps, n, h, w, "" if p is None else "-pitch%d" % p)


def _conv_problem(shape, epi, seed=0, a=8, b=4):
    """Operands (unpadded numpy) and the float64 reference of one conv problem."""
    cout, cps, nsrc, n, h, w, _ = shape
    rng = X.rng_of(cout, cps, nsrc, n, h, w, EPIS.index(epi), seed)
    p = {"xs": [X.ints(rng, (n, cps, h, w), a) for _ in range(nsrc)], "w": X.weights(rng, (cout, cps * nsrc, 3, 3), b),
         "bias": X.ints(rng, (cout,), 3)}
    kw = {}
    if epi == "relu":
        kw["relu"] = True
    if epi == "mask":
        kw["mask"] = p["mask"] = X.masks(rng, (n, cout, h, w))
    if epi in ("res0", "res01"):
        kw["res0"] = p["res0"] = X.ints(rng, (n, cout, h, w), a)
    if epi == "res01":
        kw["res1"] = p["res1"] = X.ints(rng, (n, cout, h, w), a)
    ref, inter = X.conv(p["xs"], p["w"], p["bias"], **kw)
    if epi.startswith("shuffle"):
        ref = X.pixel_shuffle(ref, 4)
        if epi == "shuffle_base":
            p["base"] = X.ints(rng, ref.shape, 255, lo=0)
            ref = ref + p["base"]
            inter.append(ref)
    p["ref"], p["inter"] = ref, inter
    return p


def _epis_for(shape):
    return [e for e in EPIS if shape[0] == 48 or not e.startswith("shuffle")]


WGRAD_CASES = [
    # (cout, cin, cin_valid, N, H, W, jobs)
    (48, 48, 48, 2, 9, 48, 2), (48, 48, 48, 1, 5, 13, 1), (48, 48, 48, 3, 7, 50, 2), (48, 16, 3, 2, 6, 48, 2),
    (48, 16, 3, 1, 7, 13, 1), (32, 32, 32, 2, 6, 48, 2), (32, 32, 32, 1, 5, 21, 1), (64, 64, 64, 1, 6, 52, 2),
    (64, 64, 64, 2, 4, 15, 1), (32, 48, 48, 2, 12, 16, 1), (32, 48, 48, 1, 7, 13, 1),
]


def _wgrad_problem(case, job, a=2):
    cout, cin, valid, n, h, w, _ = case
    rng = X.rng_of(cout, cin, n, h, w, job)
    dy = X.ints(rng, (n, cout, h, w), a)
    x = np.zeros((n, cin, h, w), np.float32)
    x[:, :valid] = X.ints(rng, (n, valid, h, w), a)
    dw, db, inter = X.wgrad(dy, x[:, :valid])
    return {"dy": dy, "x": x, "dw": dw, "db": db, "inter": inter}


F16_SHAPES = [(1, 3, 4), (2, 48, 48), (16, 48, 48), (1, 339, 510), (1, 37, 127),
              (1, 5, 70),      # the width ends inside an N tile (70 = 64 + 6)
              (1, 6, 128)]     # the width ends exactly on a 64-column tile
F16_EPIS = ("plain", "relu", "res0", "res01")


def _f16_sources(shape):
    """Source counts of larva_f16_conv3x3 driven at `shape`: all of {1, 2, 3, 4, 8} except at the two large shapes,
    whose float64 references (K up to 3456 over 173 k pixels) would take minutes on the host."""
    n, h, w = shape
    return (1, 2, 3, 4, 8) if n * h * w <= 5000 else ((1, 2) if n * h * w <= 40000 else (1,))


def _f16_problem(shape, nsrc, epi):
    n, h, w = shape
    rng = X.rng_of(n, h, w, nsrc, F16_EPIS.index(epi))
    p = {"xs": [X.ints(rng, (n, h, w, 48), 4) for _ in range(nsrc)], "w": X.weights(rng, (48, 48 * nsrc, 3, 3), 2),
         "bias": X.ints(rng, (48,), 3)}
    kw = {}
    if epi == "relu":
        kw["relu"] = True
    if epi in ("res0", "res01"):
        p["res0"] = X.ints(rng, (n, h, w, 48), 4)
        kw["res0"] = p["res0"].transpose(0, 3, 1, 2)
    if epi == "res01":
        p["res1"] = X.ints(rng, (n, h, w, 48), 4)
        kw["res1"] = p["res1"].transpose(0, 3, 1, 2)
    ref, inter = X.conv([x.transpose(0, 3, 1, 2) for x in p["xs"]], p["w"], p["bias"], **kw)
    p["ref"], p["inter"] = np.ascontiguousarray(ref.transpose(0, 2, 3, 1)), inter
    return p


NETS = {"M2": ([2, 1], 4), "M4": ([4, 4, 4, 4], 2)}     # blocks, non-zero +-1 weights per output channel


def _net_shapes(blocks, v2):
    sd = {"head.feature_extraction.weight": (48, 3, 3, 3), "head.feature_extraction.bias": (48,)}
    for i, nb in enumerate(blocks):
        for j in range(nb):
            for k in (0, 2):
                sd["body_%d.res_blocks.%d.body.%d.weight" % (i, j, k)] = (48, 48, 3, 3)
                sd["body_%d.res_blocks.%d.body.%d.bias" % (i, j, k)] = (48,)
        for k in (0, 2):
            sd["body_%d.leg.recon_block.%d.weight" % (i, k)] = (48, 48, 3, 3)
            sd["body_%d.leg.recon_block.%d.bias" % (i, k)] = (48,)
    if v2:
        sd["tail.merge_conv.weight"], sd["tail.merge_conv.bias"] = (48, 48 * len(blocks), 3, 3), (48,)
        for k in (0, 2):
            sd["tail.recon_block.%d.weight" % k], sd["tail.recon_block.%d.bias" % k] = (48, 48, 3, 3), (48,)
    return sd


def _net_state(net, v2):
    blocks, nz = NETS[net]
    return X.int_state_dict(_net_shapes(blocks, v2), seed=len(blocks) * 10 + int(v2), nz=nz)


def _net_image(n, h, w):
    return X.ints(X.rng_of(n, h, w, 77), (n, h, w, 3), 15, lo=0).astype(np.uint8)     # HWC bytes 0..15


def _net_reference(net, v2, img_u8, half=False, exit_index=None):
    """float64 conv part [N][3][4H][4W] of the network on the image, its precondition asserted layer by layer."""
    blocks, _ = NETS[net]
    r = X.Net(_net_state(net, v2), blocks, half=half)
    x = img_u8.transpose(0, 3, 1, 2).astype(np.float64)
    out = r.forward_v2(x) if v2 else r.forward(x, exit_index)
    X.assert_exact_precondition(r.inter, LIMIT)
    if half:
        X.assert_exact_precondition(r.stored, X.HALF_MAX + 1)
    return out, r


# =====================================================================================================================
# CPU part
# =====================================================================================================================
@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 16, 8, 5, 7), (1, 24, 32, 4, 9)], ids=["2x16to8-5x7", "1x24to32-4x9"])
def test_references_agree_with_the_c_restatement_bit_for_bit(n, cin, cout, h, w):
    from oracle import larva_ref as R
    rng = X.rng_of(n, cin, cout, h, w)
    x, wt, b = X.ints(rng, (n, cin, h, w), 8), X.weights(rng, (cout, cin, 3, 3), 4), X.ints(rng, (cout,), 3)
    dy = X.ints(rng, (n, cout, h, w), 2)
    y, inter = X.conv([x], wt, b)
    X.assert_exact_precondition(inter)
    X.assert_bits_equal(R.conv3x3(x, wt, b), y, "conv")
    y2, inter = X.conv([x[:, :8], x[:, 8:]], wt, b, relu=True)       # (sources are a channel concatenation)
    X.assert_bits_equal(np.maximum(R.conv3x3(x, wt, b), 0), y2, "conv+relu over two sources")
    dx, inter = X.dgrad(dy, wt)
    X.assert_exact_precondition(inter)
    X.assert_bits_equal(R.conv3x3_dgrad(dy, wt), dx, "dgrad")
    dw, db, inter = X.wgrad(dy, x)
    X.assert_exact_precondition(inter)
    dw_c, db_c = R.conv3x3_wgrad(dy, x)
    X.assert_bits_equal(dw_c, dw, "wgrad")
    X.assert_bits_equal(db_c, db, "bias grad")
    for s, c in ((2, 8), (3, 18), (4, 16)):
        t = X.ints(rng, (n, c if c % (s * s) == 0 else s * s * 2, h, w), 100)
        up = X.pixel_shuffle(t, s)
        X.assert_bits_equal(R.pixel_shuffle(t, s), up, "pixel_shuffle(%d)" % s)
        X.assert_bits_equal(R.pixel_unshuffle(up, s), t, "pixel_unshuffle(%d)" % s)
        X.assert_bits_equal(X.pixel_unshuffle(up, s), t, "unshuffle inverts shuffle (%d)" % s)


def test_epilogue_order_masks_and_assertions():
    rng = X.rng_of(5)
    m = X.masks(rng, (4000,))
    bits = set(m.view(np.uint32).tolist())
    assert bits == {0xBF800000, 0x80000000, 0x00000000, 0x3F800000}      # -1, -0.0, +0.0, 1: both zeros appear
    x, w = X.ints(rng, (1, 8, 3, 3), 8), X.weights(rng, (8, 8, 3, 3), 4)
    mask, r0 = X.masks(rng, (1, 8, 3, 3)), X.ints(rng, (1, 8, 3, 3), 8)
    y, _ = X.conv([x], w, relu=False, mask=mask, res0=r0)
    plain, _ = X.conv([x], w)
    assert np.array_equal(y, np.where(mask > 0, plain, 0.0) + r0)
    with pytest.raises(AssertionError, match="set-up"):
        X.assert_exact_precondition([np.array([1.0, 2.5])])
    with pytest.raises(AssertionError, match="set-up"):
        X.assert_exact_precondition([np.array([2.0 ** 24])])
    X.assert_exact_precondition([np.array([2.0 ** 24 - 1]), 3.0])
    with pytest.raises(AssertionError, match=r"1 of 4 elements differ\n  at \[1, 0\] got -0.0 .* expected 0.0"):
        X.assert_bits_equal(np.array([[1.0, 2.0], [-0.0, 3.0]], np.float32), np.array([[1.0, 2.0], [0.0, 3.0]]), "zeros")
    sparse = X.weights(rng, (48, 48, 3, 3), 1, nz=4)
    assert set(np.unique(sparse).tolist()) == {-1.0, 0.0, 1.0} and 2 < (sparse != 0).sum() / 48 < 6


def test_every_gpu_case_list_satisfies_the_precondition():
    """The operands the GPU part draws, at every shape small enough for the host: integers, and every partial-sum bound
    below 2^24 (below 65 504 for what an fp16 launch stores)."""
    _threads()
    for shape in CONV_SHAPES:
        for epi in _epis_for(shape):
            X.assert_exact_precondition(_conv_problem(shape, epi)["inter"])
    # the ranges themselves, at the largest K and the largest pixel count of the module
    assert 8 * 4 * 9 * 48 * 8 + 3 + 8 + 8 < LIMIT and 2 * 2 * 64 * 48 * 48 < LIMIT and 2 * 2 * 16 * 96 * 96 < LIMIT
    assert 4 * 2 * 9 * 48 * 8 + 3 + 4 + 4 < X.HALF_MAX
    assert 3 * 16 * 3 * 192 * 192 < LIMIT and 3 * 2 * 3 * (2 * 384) * (2 * 352) < LIMIT
    for case in WGRAD_CASES:
        for job in range(case[6]):
            X.assert_exact_precondition(_wgrad_problem(case, job)["inter"])
    for shape in F16_SHAPES[:2] + F16_SHAPES[4:]:
        for nsrc in _f16_sources(shape):
            p = _f16_problem(shape, nsrc, "res01")
            X.assert_exact_precondition(p["inter"])
            X.assert_exact_precondition([p["ref"]], X.HALF_MAX + 1)


@pytest.mark.parametrize("net,v2,shape", [("M2", False, (1, 13, 21)), ("M2", True, (1, 16, 24)), ("M4", False, (2, 24, 24)),
                                          ("M4", True, (2, 24, 24))],
                         ids=["M2-LarvaNet-13x21", "M2-LarvaNetV2-16x24", "M4-LarvaNet-2x24x24", "M4-LarvaNetV2-2x24x24"])
def test_network_intermediates_stay_below_the_limit(net, v2, shape):
    _threads()
    blocks, _ = NETS[net]
    m = importlib.import_module("larvanet_amd.models." + ("LarvaNetV2" if v2 else "LarvaNet")).create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks))])
    m.prepare(is_training=False, scales=[4])
    assert {k: tuple(v.shape) for k, v in m.model.state_dict().items()} == _net_shapes(blocks, v2)
    img = _net_image(*shape)
    out, r = _net_reference(net, v2, img)
    print("%s v2=%s %s: largest intermediate %.0f (partial-sum bounds included)" % (net, v2, shape, r.largest()))
    assert r.largest() < LIMIT and float(np.abs(out).max()) > 0
    if net == "M2":
        out16, r16 = _net_reference(net, v2, img, half=True)
        print("   fp16: largest stored value %.0f" % max(r16.stored))
        assert max(r16.stored) <= X.HALF_MAX


# =====================================================================================================================
# GPU part 1: fp32 conv, all launch families
# =====================================================================================================================
def _padded(p, key, pitch, dev):
    t = p.get(key)
    if t is None:
        return None
    return _dev(t if pitch is None else X.pad_pitch(t, pitch), dev)


def _device_operands(p, pitch, dev, K, bwd=False):
    d = {"xs": [_dev(x if pitch is None else X.pad_pitch(x, pitch), dev) for x in p["xs"]], "bias": _dev(p["bias"], dev)}
    fwd, back = K.pack_weights(_dev(p["w"], dev), want_bwd=bwd)
    d["wpk"], d["wpk_bwd"] = fwd, back
    for k in ("mask", "res0", "res1"):
        d[k] = _padded(p, k, pitch, dev)
    d["base"] = _dev(p["base"], dev) if "base" in p else None
    return d


def _expected(p, shape, epi):
    """The reference in the layout a launch writes: mode-0 outputs padded to the pitch with +0.0 columns."""
    pitch = shape[6]
    ref = p["ref"].astype(np.float32)
    if pitch is not None and not epi.startswith("shuffle"):
        ref = X.pad_pitch(ref, pitch)
    return ref


def _raw_conv_args(d, shape, epi, out):
    from larvanet_amd import hip_lib
    cout, cps, nsrc, n, h, w, pitch = shape
    opt = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    return (hip_lib.ptr_array([x.data_ptr() for x in d["xs"]]), nsrc, cps, d["wpk"].data_ptr(), d["bias"].data_ptr(),
            opt(d["res0"]), opt(d["res1"]), opt(d["mask"]), opt(d["base"]), out.data_ptr(), n, cout, h, w)


def _strips_applicable(shape, K, dev):
    cout, cps, nsrc, n, h, w, pitch = shape
    return (pitch or w) % 4 == 0 and cps * nsrc >= 16 and K.strip_tile_table(h, pitch or w, dev) is not None


@gpu
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_conv_id)
def test_fp32_conv_families_equal_the_integer_reference(hip_device, monkeypatch, shape):
    """larva_conv3x3_fwd, _pitched, _tiled (3 and 4 rows), _strips (both table phases, host table given and NULL, both
    store policies) and _batch (2 to 4 jobs) at one shape, every epilogue."""
    from larvanet_amd import hip_lib, kernels as K
    lib = hip_lib.load()
    _threads()
    cout, cps, nsrc, n, h, w, pitch = shape
    aligned = (pitch or w) % 4 == 0
    stream = torch.cuda.current_stream().cuda_stream
    for epi in _epis_for(shape):
        p = _conv_problem(shape, epi)
        X.assert_exact_precondition(p["inter"])
        want = _expected(p, shape, epi)
        d = _device_operands(p, pitch, hip_device, K)
        relu, shuffle = epi == "relu", epi.startswith("shuffle")
        kw = dict(bias=d["bias"], relu=relu, mask=d["mask"], res0=d["res0"], res1=d["res1"], shuffle=shuffle, base=d["base"],
                  logical_w=None if pitch is None else w)
        tag = "%s %s " % (_conv_id(shape), epi)

        def fresh():
            return torch.full(want.shape, float("nan"), device=hip_device)

        if pitch is None:
            out = fresh()
            hip_lib.check(lib.larva_conv3x3_fwd(*_raw_conv_args(d, shape, epi, out), int(relu), int(shuffle), stream), "fwd")
            X.assert_bits_equal(out, want, tag + "larva_conv3x3_fwd")
        X.assert_bits_equal(K.conv3x3(d["xs"], d["wpk"], cout, out=fresh(), **kw), want, tag + "larva_conv3x3_fwd_pitched")
        X.assert_bits_equal(K.conv3x3(d["xs"], d["wpk"], cout, out=fresh(), tile_rows=3, **kw), want, tag + "_tiled(3)")
        if aligned and cout in (48, 32) and epi != "mask":
            X.assert_bits_equal(K.conv3x3(d["xs"], d["wpk"], cout, out=fresh(), tile_rows=4, **kw), want, tag + "_tiled(4)")
        if _strips_applicable(shape, K, hip_device):
            for phase in (0, 1):
                tab = K.strip_tile_table(h, pitch or w, hip_device, phase=phase)
                for host in (tab[2], None):
                    out = fresh()
                    code = lib.larva_conv3x3_fwd_strips(*_raw_conv_args(d, shape, epi, out), pitch or w, int(relu), int(shuffle),
                                                        tab[0].data_ptr(), host, tab[1], phase, stream)   # (plain stores: phase 1)
                    hip_lib.check(code, "larva_conv3x3_fwd_strips")
                    X.assert_bits_equal(out, want, tag + "_strips(phase %d, host table %s)" % (phase, host is not None))
        if aligned:
            for njobs in (2, 3, 4):
                if njobs > 2 and epi not in ("relu", "res01", "shuffle_base"):
                    continue
                probs = [p] + [_conv_problem(shape, epi, seed=j) for j in range(1, njobs)]
                for q in probs:
                    X.assert_exact_precondition(q["inter"])
                ds = [d] + [_device_operands(q, pitch, hip_device, K) for q in probs[1:]]
                jobs = [{k: v for k, v in dict(srcs=e["xs"], wpk=e["wpk"], bias=e["bias"], mask=e["mask"], res0=e["res0"],
                                               res1=e["res1"], base=e["base"]).items() if v is not None} for e in ds]
                code = []
                real = lib.larva_conv3x3_fwd_batch
                monkeypatch.setattr(lib, "larva_conv3x3_fwd_batch", lambda *a: code.append(real(*a)) or code[-1])
                outs = K.conv3x3_batch(jobs, cout, relu=relu, shuffle=shuffle, logical_w=None if pitch is None else w)
                monkeypatch.setattr(lib, "larva_conv3x3_fwd_batch", real)
                assert code == [0], "the batched launch itself must have run (no one-by-one replacement): %r" % code
                for j, (q, o) in enumerate(zip(probs, outs)):
                    X.assert_bits_equal(o, _expected(q, shape, epi), tag + "_batch(%d jobs) job %d" % (njobs, j))


SLOT_CASES = [(c, n, h, w, e) for (c, n, h, w) in ((48, 1, 339, 510), (32, 2, 200, 200), (64, 3, 120, 196))
              for e in ("relu", "res01", "shuffle_base", "mask") if c == 48 or e != "shuffle_base"]


@gpu
@pytest.mark.parametrize("cout,n,h,w,epi", SLOT_CASES, ids=["c%d-%dx%dx%d-%s" % c for c in SLOT_CASES])
def test_whole_images_past_the_workgroup_slots(hip_device, monkeypatch, cout, n, h, w, epi):
    """More tiles than the chip has workgroup slots: the persistent-tile launch and, with LARVA_PERSIST=0, the per-tile
    launch; 3- and 4-row tiles; 339 x 510 both row-padded to 512 (16-byte staging) and unpadded (register staging).
    (Pixel-shuffle exits have 48 output channels: no such case at 32 / 64.)"""
    from larvanet_amd import kernels as K
    _threads()
    pitch = (w + 3) // 4 * 4
    slots = 2 * torch.cuda.get_device_properties(hip_device).multi_processor_count
    assert n * ((h + 2) // 3) * ((pitch + 47) // 48) > slots
    shape = (cout, cout, 1, n, h, w, pitch)
    p = _conv_problem(shape, epi)
    X.assert_exact_precondition(p["inter"])
    want = _expected(p, shape, epi)
    d = _device_operands(p, pitch, hip_device, K)
    kw = dict(bias=d["bias"], relu=epi == "relu", mask=d["mask"], res0=d["res0"], res1=d["res1"],
              shuffle=epi == "shuffle_base", base=d["base"], logical_w=w)
    tag = "c%d %dx%dx%d %s " % (cout, n, h, w, epi)
    monkeypatch.delenv("LARVA_PERSIST", raising=False)
    X.assert_bits_equal(K.conv3x3(d["xs"], d["wpk"], cout, tile_rows=3, **kw), want, tag + "persistent tiles (3 rows)")
    X.assert_bits_equal(K.conv3x3(d["xs"], d["wpk"], cout, **kw), want, tag + "the library's choice")
    if cout != 64 and epi != "mask":
        X.assert_bits_equal(K.conv3x3(d["xs"], d["wpk"], cout, tile_rows=4, **kw), want, tag + "4-row tiles")
    monkeypatch.setenv("LARVA_PERSIST", "0")
    X.assert_bits_equal(K.conv3x3(d["xs"], d["wpk"], cout, tile_rows=3, **kw), want, tag + "one workgroup per tile")
    monkeypatch.delenv("LARVA_PERSIST", raising=False)
    if w % 4:      # the same image without row padding: the register-staged kernel over 1243 tiles
        du = _device_operands(p, None, hip_device, K)
        out = K.conv3x3(du["xs"], du["wpk"], cout, bias=du["bias"], relu=epi == "relu", mask=du["mask"], res0=du["res0"],
                        res1=du["res1"], shuffle=epi == "shuffle_base", base=du["base"])
        X.assert_bits_equal(out, p["ref"], tag + "unpadded rows (register staging)")


@gpu
@pytest.mark.parametrize("shape", [(48, 48, 1, 2, 9, 48, None), (48, 48, 1, 1, 5, 13, None), (48, 48, 1, 2, 9, 13, 16),
                                   (48, 48, 1, 3, 13, 20, None), (32, 32, 1, 2, 9, 48, None), (64, 64, 1, 2, 9, 52, None),
                                   (48, 48, 1, 1, 1, 97, None), (48, 48, 1, 2, 3, 1, None), (48, 48, 1, 2, 1, 1, None),
                                   (48, 48, 1, 16, 48, 48, None)], ids=_conv_id)
def test_input_gradient_image_equals_the_float64_dgrad(hip_device, shape):
    """The tap-mirrored, channel-transposed weight image (wpk_bwd) through the same launches against the float64 input
    gradient: plain, with the ReLU-backward mask of +-0.0 / +-1 values, and with mask-free skip gradients (res0, res0 +
    res1); wide tiles, strips and the batched launch."""
    from larvanet_amd import kernels as K
    _threads()
    c, _, _, n, h, w, pitch = shape
    rng = X.rng_of(c, n, h, w, 99)
    dy, wt = X.ints(rng, (n, c, h, w), 8), X.weights(rng, (c, c, 3, 3), 4)
    mask, r0, r1 = X.masks(rng, (n, c, h, w)), X.ints(rng, (n, c, h, w), 8), X.ints(rng, (n, c, h, w), 8)
    _, bwd = K.pack_weights(_dev(wt, hip_device))
    pad = (lambda t: t) if pitch is None else (lambda t: X.pad_pitch(t, pitch))
    dyd = _dev(pad(dy), hip_device)
    lw = None if pitch is None else w
    for name, kw_ref, kw_dev in (("plain", {}, {}), ("mask", {"mask": mask}, {"mask": _dev(pad(mask), hip_device)}),
                                 ("res0", {"res0": r0}, {"res0": _dev(pad(r0), hip_device)}),
                                 ("res01", {"res0": r0, "res1": r1},
                                  {"res0": _dev(pad(r0), hip_device), "res1": _dev(pad(r1), hip_device)})):
        ref, inter = X.dgrad(dy, wt, **kw_ref)
        X.assert_exact_precondition(inter)
        want = pad(ref.astype(np.float32))
        tag = "dgrad %s %s " % (_conv_id(shape), name)
        X.assert_bits_equal(K.conv3x3(dyd, bwd, c, logical_w=lw, **kw_dev), want, tag + "wide tiles")
        if _strips_applicable(shape, K, hip_device):
            X.assert_bits_equal(K.conv3x3(dyd, bwd, c, logical_w=lw, strips=2, **kw_dev), want, tag + "strips")
        if (pitch or w) % 4 == 0:
            job = dict(srcs=dyd, wpk=bwd, **kw_dev)
            for o in K.conv3x3_batch([job, dict(job)], c, logical_w=lw):
                X.assert_bits_equal(o, want, tag + "batched")


# =====================================================================================================================
# GPU part 2: weight packing
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("cout,cin,total,off,pad", [(32, 32, 32, 0, None), (48, 48, 48, 0, None), (64, 64, 64, 0, None),
                                                    (48, 48, 144, 48, None), (32, 64, 64, 0, None), (48, 3, 3, 0, 16),
                                                    (64, 3, 3, 0, 16), (32, 48, 48, 0, None)],
                         ids=["32x32", "48x48", "64x64", "48x48-slice-of-144-at-48", "32x64", "48-head-3-as-16", "64-head-3-as-16",
                              "32x48-padded-leg"])
def test_weight_image_names_the_element_that_was_read(hip_device, cout, cin, total, off, pad):
    """w[co][ci][ky][kx] = 1 + co + 64 ci + 4096 (3 ky + kx): its own index.  A one-hot input (channel ci, one pixel)
    then makes output channel co at the pixel displaced by the tap read back exactly that number: the stride(c) rows,
    the c ^ 16 swizzle of the odd rows, channel slices and the zero-padded head are pinned from outside, for the
    forward image and for the tap-mirrored, transposed one."""
    from larvanet_amd import kernels as K
    co, ci, ky, kx = np.meshgrid(np.arange(cout), np.arange(total), np.arange(3), np.arange(3), indexing="ij")
    wt = (1 + co + 64 * ci + 4096 * (3 * ky + kx)).astype(np.float32)
    X.assert_exact_precondition([wt])
    fwd, bwd = K.pack_weights(_dev(wt, hip_device), cin_off=off, cin=cin, cin_pad=pad, want_bwd=pad is None)
    cin_k = pad or cin
    h, w = 3, 4                                     # every input channel in its own image, the one at the centre pixel
    x = np.zeros((cin_k, cin_k, h, w), np.float32)
    x[np.arange(cin_k), np.arange(cin_k), 1, 1] = 1.0
    sub = np.zeros((cout, cin_k, 3, 3), np.float64)
    sub[:, :cin] = wt[:, off:off + cin]             # (channels past the weight's own pack as zeros)
    ref, inter = X.conv([x], sub)
    X.assert_exact_precondition(inter)
    # out[n = ci, co, 1 - (ky - 1), 1 - (kx - 1)] = w[co, off + ci, ky, kx]: spelled out, independent of conv2d
    spelled = np.zeros_like(ref)
    for a in range(3):
        for b in range(3):
            spelled[:, :, 2 - a, 2 - b] = sub[:, :, a, b].T
    assert np.array_equal(ref[:, :, 0:3, 0:3], spelled[:, :, 0:3, 0:3]) and not ref[:, :, :, 3].any()
    X.assert_bits_equal(K.conv3x3(_dev(x, hip_device), fwd, cout), ref, "forward image %dx%d" % (cout, cin_k))
    if bwd is not None:
        dy = np.zeros((cout, cout, h, w), np.float32)
        dy[np.arange(cout), np.arange(cout), 1, 1] = 1.0
        dref, inter = X.dgrad(dy, sub)
        X.assert_exact_precondition(inter)
        if cin_k in (32, 48, 64):
            X.assert_bits_equal(K.conv3x3(_dev(dy, hip_device), bwd, cin_k), dref, "input-gradient image %dx%d" % (cin_k, cout))


# =====================================================================================================================
# GPU part 3: head conv
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("n,h,w,pitch,cout", [(16, 48, 48, None, 48), (1, 9, 13, 16, 48), (2, 5, 7, None, 48), (1, 7, 18, 20, 48),
                                              (2, 33, 50, 64, 32), (1, 20, 95, 96, 64), (3, 1, 16, None, 32), (1, 2, 40, 48, 64),
                                              (2, 11, 37, 39, 48), (1, 1, 1, None, 48), (1, 339, 510, 512, 48)],
                         ids=lambda v: str(v))
def test_direct_head_conv_equals_the_reference_and_the_mfma_head(hip_device, n, h, w, pitch, cout):
    """larva_head_conv3_direct at 32 / 48 / 64 outputs, the 4-pixel kernel (pitch % 4 == 0) and the one-pixel kernel, with
    padding columns and without: equal to the float64 conv, +0.0 in the padding columns, and equal to the same layer on
    the MFMA kernel over the image zero-padded to 16 channels."""
    from larvanet_amd import kernels as K
    _threads()
    rng = X.rng_of(n, h, w, cout)
    x, wt, b = X.ints(rng, (n, 3, h, w), 255, lo=0), X.weights(rng, (cout, 3, 3, 3), 4), X.ints(rng, (cout,), 3)
    ref, inter = X.conv([x], wt, b)
    X.assert_exact_precondition(inter)
    P = pitch or w
    want = X.pad_pitch(ref.astype(np.float32), P)
    out = K.head_conv3_direct(_dev(x, hip_device), _dev(wt, hip_device), _dev(b, hip_device), pitch=pitch)
    X.assert_bits_equal(out, want, "direct head %s" % ((n, h, w, pitch, cout),))
    if P % 4 == 0:
        x16 = np.zeros((n, 16, h, P), np.float32)
        x16[:, :3, :, :w] = x
        fwd, _ = K.pack_weights(_dev(wt, hip_device), cin_pad=16, want_bwd=False)
        mf = K.conv3x3(_dev(x16, hip_device), fwd, cout, bias=_dev(b, hip_device), logical_w=w if P > w else None)
        X.assert_bits_equal(mf, want, "MFMA head on the padded input")
    else:
        other = K.head_conv3_direct(_dev(x, hip_device), _dev(wt, hip_device), _dev(b, hip_device), pitch=(P + 3) // 4 * 4)
        X.assert_bits_equal(other[..., :w], ref, "the 4-pixel kernel at the next pitch")


# =====================================================================================================================
# GPU part 4: exits
# =====================================================================================================================
def _loss_bound(n):
    return (2 * n + 1) * 2.0 ** -24


def _check_l1(parts, grad, got_loss, out64, truth, g, cpad_ref, what):
    """grad == sign(out - truth) g in the unshuffled (padded) layout; every tie is 0 and nothing else is; the partial
    sums are integers and add up to the exact total; the finished scalar is within (2n + 1) 2^-24 of it."""
    d = out64 - truth.astype(np.float64)
    total = float(np.abs(d).sum())
    X.assert_exact_precondition([d, total, 3.0 * d.size])
    X.assert_bits_equal(grad, cpad_ref, what + " gradient")
    gz = grad.cpu().numpy() == 0
    assert np.array_equal(gz, cpad_ref == 0), what + ": the zeros of the gradient are not exactly the ties"
    pv = parts.cpu().numpy().astype(np.float64)
    assert (pv == np.rint(pv)).all() and (pv >= 0).all(), what + ": a partial sum is not a non-negative integer"
    assert float(pv.sum()) == total, "%s: partial sums add up to %r, exact total %r" % (what, float(pv.sum()), total)
    if got_loss is not None:
        exact = total / d.size
        assert abs(float(got_loss) - exact) <= _loss_bound(len(pv)) * exact, (what, float(got_loss), exact, len(pv))
    return total


@gpu
@pytest.mark.parametrize("njobs,n,h,w,nsrc", [(2, 2, 9, 48, 1), (4, 1, 7, 20, 1), (3, 16, 48, 48, 1), (2, 1, 5, 52, 2)],
                         ids=["2jobs-2x9x48", "4jobs-1x7x20", "3jobs-16x48x48", "2jobs-1x5x52-2src"])
def test_exits_scored_inside_the_conv_launch_are_exact(hip_device, n, h, w, njobs, nsrc):
    from larvanet_amd import kernels as K
    _threads()
    shape = (48, 48, nsrc, n, h, w, None)
    probs = [_conv_problem(shape, "shuffle_base", seed=10 + j) for j in range(njobs)]
    jobs = []
    for p in probs:
        X.assert_exact_precondition(p["inter"])
        d = _device_operands(p, None, hip_device, K)
        jobs.append({"srcs": d["xs"], "wpk": d["wpk"], "bias": d["bias"], "base": d["base"]})
    rng = X.rng_of(njobs, n, h, w)
    # one truth for all exits: exit 0's image plus integers in [-3, 3] (a seventh of its elements tie); the other exits
    # sit further away: their truth differences must stay small enough for 3 numel < 2^24 -> their own check below
    truth = (probs[0]["ref"] + X.ints(rng, probs[0]["ref"].shape, 3)).astype(np.float32)
    for p in probs[1:]:
        # exits share the truth pointer per job in the C ABI; the wrapper passes one truth, so make every exit's image
        # close to it: same weights' image is not available, instead move each job's base by (truth - its own image)
        delta = X.ints(rng, p["ref"].shape, 3)
        p["base"] = (p["base"] + (truth - p["ref"]) + delta).astype(np.float32)
        p["ref"] = truth.astype(np.float64) + delta
        X.assert_exact_precondition([p["base"], p["ref"]])
    for p, j in zip(probs, jobs):
        j["base"] = _dev(p["base"], hip_device)
    numel = truth.size
    assert 3 * numel < LIMIT
    gvalue, gscale = 1.0, float(np.float32(1.0) / np.float32(njobs))
    g = np.float32((np.float32(gvalue) * np.float32(gscale)) * (np.float32(1.0) / np.float32(numel)))
    want = [j % 2 == 0 for j in range(njobs)]
    res = K.conv3x3_exit_l1_batch(jobs, 48, _dev(truth, hip_device), gvalue, gscale, want)
    assert res is not None, "the fused exit launch must apply at this shape"
    outs, parts, grads = res
    totals = []
    for j, p in enumerate(probs):
        what = "exit %d of %d at %dx%dx%d" % (j, njobs, n, h, w)
        if want[j]:
            X.assert_bits_equal(outs[j], p["ref"], what + " image")
        else:
            assert outs[j] is None
        gref = X.pixel_unshuffle(X.l1_sign_grad(p["ref"], truth, g), 4)
        loss = K.loss_from_partials([parts[j]], [1.0 / numel], 1.0)
        totals.append(_check_l1(parts[j], grads[j], loss, p["ref"], truth, g, gref, what))
        ties = int((p["ref"] == truth).sum())
        assert 0.10 * numel < ties < 0.19 * numel, (what, ties, numel)     # about a seventh
    # the step's loss: all exits finished in one launch, mean over exits
    inv = 1.0 / numel
    loss = float(K.loss_from_partials(parts, [inv] * njobs, float(njobs)))
    exact = sum(totals) / numel / njobs
    nparts = sum(int(p.numel()) for p in parts)
    # (nparts multiplications and nparts - 1 additions, the division, and the njobs roundings of the scales 1 / numel)
    assert abs(loss - exact) <= (2 * nparts + njobs + 1) * 2.0 ** -24 * exact, (loss, exact)


@gpu
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("n,h,w,pitch", [(2, 12, 16, None), (2, 9, 13, 16), (1, 7, 13, None), (16, 48, 48, None)],
                         ids=["2x12x16", "2x9x13-pitch16", "1x7x13", "16x48x48"])
def test_x2_x3_exit_pieces_on_the_padded_conv_are_exact(hip_device, s, n, h, w, pitch):
    """The 32-output conv on zero-padded weight rows, then larva_pixel_shuffle_base, larva_shuffle_l1_partial_grad,
    larva_l1_bwd_unshuffle and larva_pixel_unshuffle: images, gradients (padding channels +0.0) and L1 sums."""
    from larvanet_amd import kernels as K
    _threads()
    c2 = 3 * s * s
    rng = X.rng_of(s, n, h, w)
    x = X.ints(rng, (n, 48, h, w), 8)
    wt = np.zeros((32, 48, 3, 3), np.float32)
    wt[:c2] = X.weights(rng, (c2, 48, 3, 3), 4)
    b = np.zeros(32, np.float32)
    b[:c2] = X.ints(rng, (c2,), 3)
    base = X.ints(rng, (n, 3, s * h, s * w), 255, lo=0)
    yref, inter = X.conv([x], wt, b)
    X.assert_exact_precondition(inter)
    fwd, _ = K.pack_weights(_dev(wt, hip_device), want_bwd=False)
    xd = _dev(x if pitch is None else X.pad_pitch(x, pitch), hip_device)
    y = K.conv3x3(xd, fwd, 32, bias=_dev(b, hip_device), logical_w=None if pitch is None else w)
    X.assert_bits_equal(y, yref if pitch is None else X.pad_pitch(yref, pitch), "padded 32-output conv x%d" % s)
    img_ref = X.pixel_shuffle(yref[:, :c2], s) + base
    img = K.pixel_shuffle_base(y, _dev(base, hip_device), s, logical_w=None if pitch is None else w)
    X.assert_bits_equal(img, img_ref, "larva_pixel_shuffle_base x%d" % s)
    X.assert_bits_equal(K.pixel_shuffle_base(y, None, s, logical_w=None if pitch is None else w),
                        X.pixel_shuffle(yref[:, :c2], s), "larva_pixel_shuffle_base x%d without a base" % s)
    if pitch is not None:
        return                                          # (the L1 pieces take unpitched tensors)
    _check_x_exit(K, hip_device, s, y, yref, base, rng)


def _check_x_exit(K, dev, s, y, yref, base, rng):
    c2 = 3 * s * s
    n, _, h, w = yref.shape
    img_ref = X.pixel_shuffle(yref[:, :c2], s) + base
    truth = (img_ref + X.ints(rng, img_ref.shape, 3)).astype(np.float32)
    numel = truth.size
    assert 3 * numel < LIMIT
    g = np.float32((np.float32(1.0) * np.float32(0.5)) * (np.float32(1.0) / np.float32(numel)))
    gref = X.pad_channels(X.pixel_unshuffle(X.l1_sign_grad(img_ref, truth, g), s), 32)
    td, bd = _dev(truth, dev), _dev(base, dev)
    part, inv, grad, img = K.shuffle_l1_partial_grad(y, bd, td, 1.0, 0.5, s)
    what = "larva_shuffle_l1_partial_grad x%d %s" % (s, (n, h, w))
    X.assert_bits_equal(img, img_ref, what + " image")
    loss = K.loss_from_partials([part], [inv], 1.0)
    _check_l1(part, grad, loss, img_ref, truth, g, gref, what)
    part2, _, grad2, none = K.shuffle_l1_partial_grad(y, bd, td, 1.0, 0.5, s, want_image=False)
    assert none is None
    X.assert_bits_equal(grad2, gref, what + " (no image) gradient")
    X.assert_bits_equal(part2, part.cpu().numpy(), what + " (no image) partial sums")
    g2 = K.l1_bwd_unshuffle(img, td, torch.tensor(1.0, device=dev), s, 32, 0.5)
    X.assert_bits_equal(g2, gref, "larva_l1_bwd_unshuffle x%d" % s)
    un = K.pixel_unshuffle(img, s, 32)
    X.assert_bits_equal(un, X.pad_channels(X.pixel_unshuffle(img_ref, s), 32), "larva_pixel_unshuffle x%d" % s)


@gpu
def test_x2_exit_pieces_past_the_grid_stride(hip_device):
    """More than 262 144 LR pixels: shuffle_l1_grad_kernel's 1024 blocks of 256 lanes take a second turn."""
    from larvanet_amd import kernels as K
    s, n, h, w = 2, 2, 384, 352
    assert n * h * w > 262144
    rng = X.rng_of(s, n, h, w)
    yref = X.pad_channels(X.ints(rng, (n, 12, h, w), 500), 32).astype(np.float64)   # (what a padded conv leaves: integers)
    base = X.ints(rng, (n, 3, s * h, s * w), 255, lo=0)
    _check_x_exit(K, hip_device, s, _dev(yref.astype(np.float32), hip_device), yref, base, rng)


# =====================================================================================================================
# GPU part 5: weight and bias gradients
# =====================================================================================================================
def _wgrad_jobs(case, dev, wide=False):
    cout, cin, valid, n, h, w, njobs = case
    probs = [_wgrad_problem(case, j) for j in range(njobs)]
    jobs = []
    wide_dw = torch.full((cout, valid * njobs + 5, 3, 3), float("nan"), device=dev) if wide else None
    for j, p in enumerate(probs):
        X.assert_exact_precondition(p["inter"])
        job = {"dy": _dev(p["dy"], dev), "x": _dev(p["x"], dev), "db": torch.full((cout,), float("nan"), device=dev),
               "cin_valid": valid}
        if wide:
            job["dw"], job["cin_off"] = wide_dw, 5 + valid * j
        else:
            job["dw"], job["cin_off"] = torch.full((cout, valid, 3, 3), float("nan"), device=dev), 0
        jobs.append(job)
    return probs, jobs, wide_dw


def _check_wgrad(probs, jobs, wide_dw, what):
    for j, (p, job) in enumerate(zip(probs, jobs)):
        valid = job["cin_valid"]
        got = job["dw"] if wide_dw is None else wide_dw[:, job["cin_off"]:job["cin_off"] + valid].contiguous()
        X.assert_bits_equal(got, p["dw"], "%s job %d dw" % (what, j))
        X.assert_bits_equal(job["db"], p["db"], "%s job %d db" % (what, j))
    if wide_dw is not None:
        assert bool(torch.isnan(wide_dw[:, :5]).all()), what + ": channels outside the slices were written"


def _refill(jobs, wide_dw):
    for j in jobs:
        j["dw"].fill_(float("nan"))
        j["db"].fill_(float("nan"))


@gpu
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "%dx%d(valid %d)-N%d-%dx%d-%djobs" % c)
def test_weight_and_bias_gradients_equal_the_integer_sums(hip_device, case):
    """larva_conv3x3_wgrad with 1 to 8 splits, channel slices of a wider gradient, the two phases separately
    (_partial + larva_wgrad_reduce) and the reduction that also finishes a loss."""
    from larvanet_amd import kernels as K
    _threads()
    cout, cin, valid, n, h, w, njobs = case
    what = "wgrad %dx%d N%d %dx%d" % (cout, cin, n, h, w)
    probs, jobs, _ = _wgrad_jobs(case, hip_device)
    for splits in range(1, 9):
        _refill(jobs, None)
        K.conv3x3_wgrad(jobs, cout, cin, splits)
        _check_wgrad(probs, jobs, None, "%s splits %d" % (what, splits))
    probs, jobs, wide = _wgrad_jobs(case, hip_device, wide=True)
    K.conv3x3_wgrad(jobs, cout, cin, 3)
    _check_wgrad(probs, jobs, wide, what + " slices of a wide gradient")
    # the two phases on their own, and the reduce launch that carries the loss
    probs, jobs, _ = _wgrad_jobs(case, hip_device)
    parts, used = K.conv3x3_wgrad_partial(jobs, cout, cin, 5)
    assert 1 <= used <= 5
    rjobs = [dict(j, partial=p, splits=used, cout=cout, cin=cin) for j, p in zip(jobs, parts)]
    K.wgrad_reduce(rjobs)
    _check_wgrad(probs, jobs, None, what + " _partial + larva_wgrad_reduce")
    _refill(jobs, None)
    terms = [_dev(X.ints(X.rng_of(7), (64,), 1000, lo=0), hip_device), torch.tensor(3.0, device=hip_device)]
    loss = torch.full((), float("nan"), device=hip_device)
    K.wgrad_reduce(rjobs, loss=(terms, [0.25, 1.0], 2.0, loss))
    _check_wgrad(probs, jobs, None, what + " larva_wgrad_reduce_with_loss")
    exact = (0.25 * float(terms[0].double().sum()) + 3.0) / 2.0        # (integers times powers of two: exact in fp32)
    assert float(loss) == exact, (float(loss), exact)
    X.assert_bits_equal(K.loss_from_partials(terms, [0.25, 1.0], 2.0), loss.cpu().numpy(), "the loss of the reduce launch")


def _flat_problem(njobs, n, c, h, w, dev, head):
    """Operands drawn on the device (32 layers of 64 x 48 x 48 x 48 are 1.8 GB): integers in [-2, 2]."""
    gen = torch.Generator(device=dev).manual_seed(njobs * 1000 + n + c + h)
    draw = lambda *shape: torch.randint(-2, 3, shape, generator=gen, device=dev).float()   # noqa: E731
    jobs = [{"dy": draw(n, c, h, w), "x": draw(n, c, h, w), "dw": torch.full((c, c, 3, 3), float("nan"), device=dev),
             "db": torch.full((c,), float("nan"), device=dev)} for _ in range(njobs)]
    hd = None
    if head:
        x16 = torch.zeros(n, 16, h, w, device=dev)
        x16[:, :3] = draw(n, 3, h, w)
        hd = {"dy": draw(n, 48, h, w), "x": x16, "dw": torch.full((48, 3, 3, 3), float("nan"), device=dev),
              "db": torch.full((48,), float("nan"), device=dev), "cin_off": 0, "cin_valid": 3}
    return jobs, hd


@gpu
@pytest.mark.parametrize("njobs,nwg,n,h,w,c,head", [(5, 7, 2, 9, 48, 48, False), (3, 64, 1, 6, 48, 48, True), (6, 4, 2, 7, 52, 48, False),
                                                    (1, 3, 2, 9, 48, 48, True), (5, 7, 2, 9, 48, 32, False), (6, 4, 2, 7, 52, 32, False),
                                                    (5, 7, 2, 9, 48, 64, False), (6, 4, 2, 7, 52, 64, False),
                                                    (2, 5, 3, 10, 52, 48, True), (8, 256, 16, 48, 48, 48, True),
                                                    # the large shares of test_flat_wgrad_grid_with_large_shares
                                                    (32, 256, 64, 48, 48, 48, False), (32, 200, 64, 48, 48, 48, False),
                                                    (8, 256, 16, 96, 96, 48, True)],
                         ids=lambda v: str(v))
def test_flat_weight_gradient_grid_equals_the_integer_sums(hip_device, njobs, nwg, n, h, w, c, head):
    """larva_conv3x3_wgrad_partial_flat / _flat_head + larva_wgrad_reduce: shares that cross layer boundaries, more
    workgroups than tiles, 128-164 tiles per share.  Every layer is checked where the host can afford it; at the large
    shapes the first and last layer, two whose first share starts inside the layer before, and the head."""
    from larvanet_amd import kernels as K
    _threads()
    jobs, hd = _flat_problem(njobs, n, c, h, w, hip_device, head)
    res = K.conv3x3_wgrad_partial_flat(jobs, c, c, nwg, head=hd)
    assert res is not None, "the flat launch must apply at this shape"
    parts, splits = res
    rj = [dict(j, partial=p, splits=s, cout=c, cin=c) for j, p, s in zip(jobs, parts, splits)]
    if hd is not None:
        rj.append(dict(hd, partial=parts[-1], splits=splits[-1], cout=48, cin=16))
    K.wgrad_reduce(rj)
    torch.cuda.synchronize()
    tiles = n * ((h + 2) // 3) * ((w + 47) // 48)
    check = list(range(njobs))
    if n * h * w > 20000 and njobs > 4:
        starts = {njobs * tiles * k // nwg for k in range(nwg)}
        crossing = [i for i in range(1, njobs) if i * tiles not in starts]
        check = sorted({0, njobs - 1, *crossing[len(crossing) // 2:len(crossing) // 2 + 2]})
    assert 2 * 2 * n * h * w < LIMIT
    todo = [(i, jobs[i], jobs[i]["x"]) for i in check] + ([("head", hd, hd["x"][:, :3])] if hd is not None else [])
    for i, j, xin in todo:
        dw, db, inter = X.wgrad(j["dy"].cpu().numpy(), xin.cpu().numpy())
        X.assert_exact_precondition(inter)
        what = "flat grid %s layer %s" % ((njobs, nwg, n, h, w, c), i)
        X.assert_bits_equal(j["dw"], dw, what + " dw")
        X.assert_bits_equal(j["db"], db, what + " db")
    for j in jobs + ([hd] if hd is not None else []):    # the layers not compared on the host: written, and integers
        v = j["dw"].double()
        assert bool(torch.isfinite(v).all()) and bool((v == v.round()).all())


# =====================================================================================================================
# GPU part 6: fp16 kernels
# =====================================================================================================================
def _flag(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


@gpu
@pytest.mark.parametrize("shape", F16_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_f16_conv_stores_the_float16_of_the_exact_sum(hip_device, shape):
    """larva_f16_conv3x3: plain, ReLU, + res0, + res0 + res1 at one source, the plain epilogue at 2, 3, 4 and 8 sources
    (host permitting).  Every element equals float16(exact sum) -- rounded once, so also above 2048 -- and the overflow
    flag stays 0, edge tiles whose lanes hang over the right or bottom edge included."""
    from larvanet_amd import kernels as K
    _threads()
    flag = _flag(hip_device)
    for nsrc in _f16_sources(shape):
        for epi in (F16_EPIS if nsrc == 1 else ("plain", "res01")):
            p = _f16_problem(shape, nsrc, epi)
            X.assert_exact_precondition(p["inter"])
            X.assert_exact_precondition([p["ref"]], X.HALF_MAX + 1)
            h16 = lambda a: _dev(a.astype(np.float16), hip_device)   # noqa: E731
            wpk = K.f16_pack_weights(_dev(p["w"], hip_device))
            got = K.f16_conv3x3([h16(x) for x in p["xs"]], wpk, _dev(p["bias"], hip_device), flag, relu=epi == "relu",
                                res0=h16(p["res0"]) if "res0" in p else None, res1=h16(p["res1"]) if "res1" in p else None)
            X.assert_bits_equal(got, p["ref"].astype(np.float16), "larva_f16_conv3x3 %s %d sources %s" % (shape, nsrc, epi))
    assert int(flag.item()) == 0


@gpu
def test_f16_conv_rounds_once_above_2048(hip_device):
    """Sums beyond fp16's integer range: |x| <= 30, |w| <= 12 over K = 432 give sums of a few thousand (standard
    deviation ~2600), so many outputs lie above 2048, where fp16 keeps every 2nd to 8th integer; the stored value is
    float16(exact sum), ties to even."""
    from larvanet_amd import kernels as K
    rng = X.rng_of(2048)
    x = X.ints(rng, (2, 9, 70, 48), 30)
    wt, b = X.weights(rng, (48, 48, 3, 3), 12), X.ints(rng, (48,), 3)
    ref, inter = X.conv([x.transpose(0, 3, 1, 2)], wt, b)
    X.assert_exact_precondition(inter)
    ref = ref.transpose(0, 2, 3, 1)
    X.assert_exact_precondition([ref], X.HALF_MAX + 1)
    assert float((np.abs(ref) > 2048).mean()) > 0.3 and float((ref % 2 != 0).mean()) > 0.3
    flag = _flag(hip_device)
    got = K.f16_conv3x3(_dev(x.astype(np.float16), hip_device), K.f16_pack_weights(_dev(wt, hip_device)), _dev(b, hip_device), flag)
    X.assert_bits_equal(got, ref.astype(np.float16), "larva_f16_conv3x3 above 2048")
    assert int(flag.item()) == 0


@gpu
@pytest.mark.parametrize("shape", [(1, 3, 4), (2, 48, 48), (1, 37, 127), (1, 5, 70), (1, 6, 128), (1, 339, 510)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_f16_head_and_leg_ends_are_exact(hip_device, shape):
    """larva_f16_head (fp32 operands, one rounding), larva_f16_conv3x3_shuffle_base with an integer base (the fp32 HR image
    exactly) and _shuffle_base_u8 (bytes = clip(sum, 0, 255), both clamps reached)."""
    from larvanet_amd import kernels as K
    _threads()
    n, h, w = shape
    rng = X.rng_of(n, h, w, 16)
    flag = _flag(hip_device)
    x, wt, b = X.ints(rng, (n, 3, h, w), 15, lo=0), X.weights(rng, (48, 3, 3, 3), 2), X.ints(rng, (48,), 3)
    ref, inter = X.conv([x], wt, b)
    X.assert_exact_precondition(inter)
    got = K.f16_head(_dev(x, hip_device), _dev(wt, hip_device), _dev(b, hip_device), flag)
    X.assert_bits_equal(got, ref.transpose(0, 2, 3, 1).astype(np.float16), "larva_f16_head %s" % (shape,))
    src = X.ints(rng, (n, h, w, 48), 4)
    w2, b2 = X.weights(rng, (48, 48, 3, 3), 2), X.ints(rng, (48,), 3)
    base = X.ints(rng, (n, 3, 4 * h, 4 * w), 400, lo=-150)
    y, inter = X.conv([src.transpose(0, 3, 1, 2)], w2, b2)
    img = X.pixel_shuffle(y, 4) + base
    X.assert_exact_precondition(inter + [img])
    wpk = K.f16_pack_weights(_dev(w2, hip_device))
    sd, bd, based = _dev(src.astype(np.float16), hip_device), _dev(b2, hip_device), _dev(base, hip_device)
    X.assert_bits_equal(K.f16_conv3x3_shuffle_base(sd, wpk, bd, based), img, "larva_f16_conv3x3_shuffle_base %s" % (shape,))
    u8 = K.f16_conv3x3_shuffle_base_u8(sd, wpk, bd, based, flag)
    want = np.clip(img, 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    assert (img < 0).any() and (img > 255).any()
    X.assert_bits_equal(u8, want, "larva_f16_conv3x3_shuffle_base_u8 %s" % (shape,))
    assert int(flag.item()) == 0


@gpu
@pytest.mark.parametrize("where", ["interior", "last-pixel-of-an-edge-tile"])
def test_f16_overflow_flag_at_its_boundary(hip_device, where):
    """include/larva_hip.h: the flag is raised when a value exceeds 65504 before it is rounded.  One-hot input, centre-tap
    weight 65504: 65504 itself is stored and leaves the flag alone; + 1 (bias), + 16 (res0) and a NaN bias under the ReLU
    raise it."""
    from larvanet_amd import kernels as K
    n, h, w = 1, 6, 70
    py, px = (2, 10) if where == "interior" else (h - 1, w - 1)
    ci, co = 5, 37
    x = np.zeros((n, h, w, 48), np.float16)
    x[0, py, px, ci] = 1.0
    wt = np.zeros((48, 48, 3, 3), np.float32)
    wt[co, ci, 1, 1] = 65504.0
    wpk = K.f16_pack_weights(_dev(wt, hip_device))
    xd = _dev(x, hip_device)
    zero = np.zeros(48, np.float32)
    one, nan = zero.copy(), zero.copy()
    one[co], nan[co] = 1.0, np.nan
    r16 = np.zeros((n, h, w, 48), np.float16)
    r16[0, py, px, co] = 16.0
    want = np.zeros((n, h, w, 48), np.float16)
    want[0, py, px, co] = 65504.0
    cases = [("65504", zero, {}, 0, want), ("65504 + res0 0", zero, {"res0": np.zeros_like(r16)}, 0, want),
             ("65504 under the ReLU", zero, {"relu": True}, 0, want),
             ("65504 + bias 1", one, {}, 1, None), ("65504 + res0 16", zero, {"res0": r16}, 1, None),
             ("NaN bias under the ReLU", nan, {"relu": True}, 1, None)]
    for name, bias, kw, expect, stored in cases:
        flag = _flag(hip_device)
        kw = {k: (_dev(v, hip_device) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        got = K.f16_conv3x3(xd, wpk, _dev(bias, hip_device), flag, **kw)
        assert int(flag.item()) == expect, "%s (%s): flag %d, expected %d" % (name, where, int(flag.item()), expect)
        if stored is not None:
            X.assert_bits_equal(got, stored, "%s (%s)" % (name, where))


# =====================================================================================================================
# GPU part 7: whole networks
# =====================================================================================================================
def _model(name, net, precision, extra=()):
    blocks, _ = NETS[net]
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks)),
                  "--precision=" + precision] + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    m.strict_graph = True
    m.model.load_state_dict({k: v.to(m.device) for k, v in _net_state(net, name.endswith("V2")).items()})
    m.model.invalidate_packed_weights()
    return m


def _with_base(conv64, base):
    """float32(exact integer conv part) + base, added once in fp32 (the leg end's `v + base`)."""
    return (conv64.astype(np.float32) + base.astype(np.float32)).astype(np.float32)


NET_CASES = [("LarvaNet", "M2", "fp32", (), (1, 16, 24)), ("LarvaNet", "M2", "fp32", (), (1, 13, 21)),
             ("LarvaNet", "M2", "fp32", (), (1, 339, 510)), ("LarvaNetV2", "M2", "fp32", (), (1, 16, 24)),
             ("LarvaNetV2", "M2", "fp32", (), (1, 13, 21)), ("LarvaLeg", "M2", "fp32", ("--leg=1",), (1, 13, 21)),
             ("LarvaNet", "M4", "fp32", (), (2, 24, 24)), ("LarvaNetV2", "M4", "fp32", (), (2, 24, 24)),
             ("LarvaLeg", "M4", "fp32", ("--leg=2",), (2, 24, 24)),
             ("LarvaNet", "M2", "fp16", (), (1, 16, 24)), ("LarvaNet", "M2", "fp16", (), (1, 13, 21)),
             ("LarvaNet", "M2", "fp16", (), (1, 339, 510)), ("LarvaNetV2", "M2", "fp16", (), (1, 16, 24)),
             ("LarvaNetV2", "M2", "fp16", (), (1, 13, 21)), ("LarvaLeg", "M2", "fp16", ("--leg=1",), (1, 16, 24))]


@gpu
@pytest.mark.parametrize("name,net,precision,extra,shape", NET_CASES,
                         ids=["%s-%s-%s-%s" % (c[0], c[1], c[2], "x".join(map(str, c[4]))) for c in NET_CASES])
def test_whole_networks_on_integer_weights(hip_device, name, net, precision, extra, shape):
    """upscale / _forward_nograd / the captured graph's replay / upscale_u8 / row bands of LarvaNet, LarvaNetV2 and
    LarvaLeg with sparse +-1 weights on an integer image: float32(exact conv part) + base, the base image being the
    library's own (tested on its own) and added once in numpy fp32."""
    from larvanet_amd import image_utils, kernels as K
    _threads()
    v2 = name.endswith("V2")
    img = _net_image(*shape)
    leg = int(extra[0].split("=")[1]) - 1 if extra else None
    conv64, r = _net_reference(net, v2, img, half=precision == "fp16", exit_index=leg)
    m = _model(name, net, precision, extra)
    chw = np.ascontiguousarray(img.transpose(0, 3, 1, 2)).astype(np.float32)
    base = K.upsample(_dev(chw, hip_device), 4, "bicubic").cpu().numpy()
    want = _with_base(conv64, base)
    tag = "%s %s %s %s " % (name, net, precision, shape)
    X.assert_bits_equal(m.upscale(list(chw), 4), want, tag + "upscale")
    assert not m.fp16_overflowed()
    with torch.no_grad():
        xd = _dev(chw, hip_device)
        X.assert_bits_equal(m._forward_nograd(xd), want, tag + "_forward_nograd")
        outs = [m.fwd_runtime(xd).clone() for _ in range(3)]            # small shapes: eager, capture, replay
    for i, o in enumerate(outs):
        X.assert_bits_equal(o, want, tag + "fwd_runtime call %d" % i)
    if shape[0] * shape[1] * shape[2] <= 100000:          # (larger batches run eagerly: autograd.is_large_inference)
        key = (tuple(xd.shape), precision)
        assert m._infer_graphs.get(key) not in (None, False), "the third call must have replayed a captured graph"
    want8 = np.clip(np.rint(want), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    X.assert_bits_equal(m.upscale_u8(list(img), 4), want8, tag + "upscale_u8")
    halo = m.receptive_halo()
    hgt = shape[1]
    cuts = [0, hgt // 3, 2 * hgt // 3, hgt]
    bands = [image_utils.upscale_band(m, chw[0], 4, a, b, halo) for a, b in zip(cuts, cuts[1:])]
    X.assert_bits_equal(np.concatenate(bands, axis=1), want[0], tag + "row bands")
    assert not m.fp16_overflowed()
