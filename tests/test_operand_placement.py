"""Every alignment-dispatched kernel at every operand placement.

Many launchers of csrc/ choose a kernel variant, or refuse, from the low address bits of their operands, the row or
frame pitch and W % 4.  The other suites reach those predicates through the dimensions only: their operands are fresh
torch tensors, 256-byte aligned.  Here every operand is a view at a chosen address residue (mod 16) inside a guarded
buffer (tests/placement.py), every result is compared with np.array_equal / exact_ref.assert_bits_equal against the
host definition the kernel already has, all placements of one problem must give identical bytes, and every case ends
with check(): no store outside an output, no store into an input.  A refusal is asserted together with an untouched
output.  DESIGN.md ("Operand placement") lists launcher -> predicate -> test.

The first tests need no device: the helper itself, and the enumeration of the resize draw."""
import ctypes
import math

import numpy as np
import pytest
import torch

import exact_ref as X
import placement as P

gpu = pytest.mark.gpu
F32, F16, U8, I32 = torch.float32, torch.float16, torch.uint8, torch.int32
HIP_INVALID_VALUE, HIP_NOT_SUPPORTED = 1, 801


# =====================================================================================================================
# the helper (no device)
# =====================================================================================================================
@pytest.mark.parametrize("offset", range(16))
def test_placed_delivers_every_residue(offset):
    a = np.arange(37, dtype=np.uint8)
    view, check = P.placed(a, U8, "cpu", offset)
    assert view.data_ptr() % 16 == offset and view.is_contiguous() and view.dtype == U8 and tuple(view.shape) == (37,)
    assert np.array_equal(view.numpy(), a)
    check()
    view.fill_(7)          # (the view itself may be written)
    check()
    with pytest.raises(AssertionError, match="placement"):
        check(untouched=True)
    blank, check_blank = P.placed((5, 3), U8, "cpu", offset)
    assert (blank == P.FILL).all()
    check_blank(untouched=True)


def test_placed_reports_a_byte_just_before_and_just_after_the_view():
    for offset in (0, 5):
        for rel in (-1, 24):          # just before, just after
            view, check = P.placed((24,), U8, "cpu", offset)
            base = view.untyped_storage()
            raw = torch.tensor([], dtype=U8).set_(base)
            start = view.data_ptr() - raw.data_ptr()
            raw[start + rel] = 0
            with pytest.raises(AssertionError, match=r"1 byte\(s\).*first at offset %d, last at offset %d " % (rel, rel)):
                check()
    view, check = P.placed((24,), U8, "cpu", 3, guard=8)
    raw = torch.tensor([], dtype=U8).set_(view.untyped_storage())
    start = view.data_ptr() - raw.data_ptr()
    raw[start - 8] = 1
    raw[start + 24 + 7] = 1
    with pytest.raises(AssertionError, match=r"2 byte\(s\).*first at offset -8, last at offset 31 "):
        check()


def test_placed_float_and_half_views_and_frame_pitch():
    a = np.linspace(-3, 3, 30, dtype=np.float32).reshape(2, 3, 5)
    for offset in (0, 4, 8, 12):
        view, check = P.placed(a, F32, "cpu", offset)
        assert view.dtype == F32 and view.data_ptr() % 16 == offset and np.array_equal(view.numpy(), a)
        check()
    for offset in range(0, 16, 2):
        view, check = P.placed(a, F16, "cpu", offset)
        assert view.dtype == F16 and view.data_ptr() % 16 == offset
        assert np.array_equal(view.numpy(), a.astype(np.float16))
        check()
    for bad, dtype in ((2, F32), (1, F16), (16, U8), (-1, U8)):
        with pytest.raises(ValueError):
            P.placed((4,), dtype, "cpu", bad)
    # frame batches: [N][pitch], the array in the first row bytes of each row, the row tails watched
    frames = np.arange(2 * 10, dtype=np.uint8).reshape(2, 10)
    view, check = P.placed(frames, U8, "cpu", 3, pitch=13)
    assert tuple(view.shape) == (2, 13) and view.is_contiguous() and view.data_ptr() % 16 == 3
    assert np.array_equal(view[:, :10].numpy(), frames) and (view[:, 10:] == P.FILL).all()
    check()
    view[:, :10] = 9
    check()
    view[0, 11] = 0
    with pytest.raises(AssertionError, match="first at offset 11, last at offset 11 "):
        check()
    with pytest.raises(ValueError):
        P.placed(frames, U8, "cpu", 0, pitch=9)
    P.same_everywhere({0: a, 4: a.copy()}, "same")
    with pytest.raises(AssertionError, match="different bytes"):
        P.same_everywhere({0: a, 4: a + 1}, "differs")


# =====================================================================================================================
# resize: the case tables (shared by the CPU enumeration and the GPU tests)
# =====================================================================================================================
RESIZE_SHAPES = [(1, 1, 5, 7), (1, 40, 1, 13), (40, 1, 13, 1), (1, 9, 3, 9), (2, 2, 8, 8), (5, 1, 5, 4),
                 (21, 37, 21, 37), (48, 64, 27, 40), (67, 129, 17, 33)]
RESIZE_FUZZ_SEED, RESIZE_FUZZ_CASES = 5, 40
RESIZE_TILE = (16, 32)      # kernels.RESIZE_TILE_ROWS / RESIZE_TILE_COLS (asserted on the device)


def resize_fuzz_cases():
    """(N, H, W, h, w, source residue, output residue) x 40: H, W in 1..90, each output side uniform on
    ceil(n / 4) .. 3 n, N in {1, 2}, the residues drawn with the shape."""
    rng = np.random.default_rng(RESIZE_FUZZ_SEED)
    cases = []
    for _ in range(RESIZE_FUZZ_CASES):
        H, W = int(rng.integers(1, 91)), int(rng.integers(1, 91))
        h, w = int(rng.integers(-(-H // 4), 3 * H + 1)), int(rng.integers(-(-W // 4), 3 * W + 1))
        cases.append((int(rng.integers(1, 3)), H, W, h, w, int(rng.integers(0, 4)), int(rng.integers(0, 4))))
    return cases


def test_the_resize_draw_covers_what_it_is_there_for():
    from larvanet_amd import image_utils as U
    cases = resize_fuzz_cases()
    assert len(cases) == RESIZE_FUZZ_CASES and cases == resize_fuzz_cases()
    for n, H, W, h, w, rs, ro in cases:
        assert n in (1, 2) and 1 <= H <= 90 and 1 <= W <= 90 and rs in range(4) and ro in range(4)
        assert math.ceil(H / 4) <= h <= 3 * H and math.ceil(W / 4) <= w <= 3 * W
        assert U.check_resize(H, W, h, w) == (h, w)          # (inside the ratio the launcher accepts)
    classes = {(rs != 0, ro != 0) for _, _, _, _, _, rs, ro in cases}
    assert classes == {(False, False), (False, True), (True, False), (True, True)}
    assert any(w < 4 for _, _, _, _, w, _, _ in cases)
    assert any(h > RESIZE_TILE[0] and w > RESIZE_TILE[1] for _, _, _, h, w, _, _ in cases)
    assert any(n == 2 and (3 * H * W) % 4 for n, H, W, _, _, _, _ in cases)    # the second image at another skew
    for H, W, h, w in RESIZE_SHAPES:
        assert U.check_resize(H, W, h, w) == (h, w)


# =====================================================================================================================
# GPU: shared pieces
# =====================================================================================================================
def _image(shape, *key):
    return np.random.default_rng([int(k) for k in key]).integers(0, 256, shape).astype(np.uint8)


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _place(a, dtype, dev, offset, checks, **kw):
    view, check = P.placed(a, dtype, dev, offset, **kw)
    checks.append(check)
    return view


def _finish(checks):
    for c in checks:
        c()


def _pitches(frame_bytes):
    """The frame bytes, the next multiple of 4 above them, and that + 1."""
    p4 = (frame_bytes // 4 + 1) * 4
    return [frame_bytes, p4, p4 + 1]


YUV_SHAPES = [(8, 6), (36, 10), (6, 5), (34, 7), (5, 3)]     # (W, H): W % 4 == 0 twice, W even only twice, odd


def _yuv_mode(W, H):
    return ("bt709", True) if (W, H) == (36, 10) else ("bt601", False)


# =====================================================================================================================
# i420 <-> rgb (csrc/larva_yuv.hip)
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("W,H", YUV_SHAPES)
def test_i420_to_rgb_at_every_placement(hip_device, W, H):
    from larvanet_amd import image_utils as U
    from larvanet_amd import kernels as K
    matrix, full = _yuv_mode(W, H)
    fb = U.i420_frame_bytes(W, H)
    for N in (1, 2):
        frames = _image((N, fb), W, H, N, 1)
        want = np.stack([U.i420_to_rgb_f32(frames[n], W, H, matrix, full) for n in range(N)])
        got = {}
        for pitch in _pitches(fb):
            for fres in range(4):
                for ores in (0, 4, 8, 12):
                    checks = []
                    src = _place(frames, U8, hip_device, fres, checks, pitch=pitch)
                    out = _place((N, 3, H, W), F32, hip_device, ores, checks)
                    ret = K.i420_to_rgb_f32(src, W, H, matrix, full, out=out)
                    key = (N, pitch, fres, ores)
                    got[key] = _cpu(out)
                    assert ret is out and np.array_equal(got[key], want), key
                    _finish(checks)
        P.same_everywhere(got, "i420_to_rgb_f32 %dx%d N=%d" % (W, H, N))


@gpu
@pytest.mark.parametrize("W,H", YUV_SHAPES)
def test_rgb_to_i420_at_every_placement(hip_device, W, H):
    from larvanet_amd import image_utils as U
    from larvanet_amd import kernels as K
    matrix, full = _yuv_mode(W, H)
    fb = U.i420_frame_bytes(W, H)
    for N in (1, 2):
        img = _image((N, H, W, 3), W, H, N, 2)
        want = np.stack([U.rgb_u8_to_i420(img[n], matrix, full) for n in range(N)])
        got = {}
        for pitch in _pitches(fb):
            for ires in range(4):
                for ores in range(4):
                    checks = []
                    x = _place(img, U8, hip_device, ires, checks)
                    out = _place((N, fb), U8, hip_device, ores, checks, pitch=pitch)    # row tails keep the fill
                    K.rgb_u8_to_i420(x, matrix, full, out=out)
                    key = (N, pitch, ires, ores)
                    got[key] = _cpu(out[:, :fb])
                    assert np.array_equal(got[key], want), key
                    _finish(checks)
        P.same_everywhere(got, "rgb_u8_to_i420 %dx%d N=%d" % (W, H, N))


# =====================================================================================================================
# uint8 HWC <-> float32 CHW (csrc/larva_pointwise.hip: u8_vec_ok)
# =====================================================================================================================
U8_SHAPES = [(1, 2, 6), (3, 4, 4), (2, 48, 48), (1, 3, 5)]     # (N, H, W): H W % 4 == 0 three times, 15 pixels once


@gpu
@pytest.mark.parametrize("N,H,W", U8_SHAPES)
def test_u8_f32_conversions_at_every_placement(hip_device, N, H, W):
    from larvanet_amd import kernels as K
    from larvanet_amd.metrics import image_to_uint8
    img = _image((N, H, W, 3), N, H, W, 3)
    want_f = np.ascontiguousarray(img.transpose(0, 3, 1, 2)).astype(np.float32)
    # float -> uint8: drawn from -3 .. 258 in steps of 0.25; the ties at both clamps and in between lead, so that the
    # smallest image has them too
    grid = np.arange(-3.0, 258.0 + 0.125, 0.25, dtype=np.float32)
    x = np.resize(np.random.default_rng(N * H * W).permutation(grid), (N, 3, H, W)).astype(np.float32)
    x.flat[:8] = [-2.5, -0.5, 0.5, 1.5, 127.5, 254.5, 255.5, 257.5]
    assert np.isin(x, grid).all() and ((x - np.floor(x)) == 0.5).sum() >= 8 and x.min() < -0.5 and x.max() > 255.5
    want_q = np.ascontiguousarray(image_to_uint8(x).transpose(0, 2, 3, 1))
    got_f, got_q = {}, {}
    for ures in (0, 1, 4, 8):
        for fres in (0, 4, 8, 12):
            checks = []
            out = _place((N, 3, H, W), F32, hip_device, fres, checks)
            K.u8_hwc_to_f32_chw(_place(img, U8, hip_device, ures, checks), out=out)
            got_f[ures, fres] = _cpu(out)
            assert np.array_equal(got_f[ures, fres], want_f), (ures, fres)
            q = _place((N, H, W, 3), U8, hip_device, ures, checks)
            K.f32_chw_to_u8_hwc(_place(x, F32, hip_device, fres, checks), out=q)
            got_q[ures, fres] = _cpu(q)
            assert np.array_equal(got_q[ures, fres], want_q), (ures, fres)
            _finish(checks)
    P.same_everywhere(got_f, "u8_hwc_to_f32_chw")
    P.same_everywhere(got_q, "f32_chw_to_u8_hwc")


# =====================================================================================================================
# self-ensemble (csrc/larva_ensemble.hip)
# =====================================================================================================================
ENS_SHAPES = [(8, 12), (32, 36), (33, 36), (7, 5)]
ENS_MOVES = [(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 4, 4), (8, 8, 8), (12, 12, 12)]    # one at a time, then all


def _ens_inputs_ref(x_chw):
    from larvanet_amd import image_utils as U
    n = x_chw.shape[0]
    a = np.stack([np.ascontiguousarray(U.dihedral(x_chw[i], t, (1, 2))) for i in range(n) for t in range(4)])
    b = np.stack([np.ascontiguousarray(U.dihedral(x_chw[i], t, (1, 2))) for i in range(n) for t in range(4, 8)])
    return a.astype(np.float32), b.astype(np.float32)


@gpu
@pytest.mark.parametrize("H,W", ENS_SHAPES)
def test_dihedral_inputs_at_every_placement(hip_device, H, W):
    from larvanet_amd import kernels as K
    for N in (1, 2):
        img = _image((N, H, W, 3), H, W, N, 4)
        xf = (np.random.default_rng([H, W, N]).random((N, 3, H, W)) * 255).astype(np.float32)
        for x, dtype in ((img, U8), (xf, F32)):
            want = _ens_inputs_ref(img.transpose(0, 3, 1, 2) if dtype is U8 else xf)
            got = {}
            for ra, rb, rx in ENS_MOVES:
                rx = rx // 4 if dtype is U8 else rx      # (the uint8 image: residues 1, 2, 3)
                checks = []
                a = _place((4 * N, 3, H, W), F32, hip_device, ra, checks)
                b = _place((4 * N, 3, W, H), F32, hip_device, rb, checks)
                K.dihedral_inputs(_place(x, dtype, hip_device, rx, checks), out=(a, b))
                got[ra, rb, rx] = np.concatenate([_cpu(a).ravel(), _cpu(b).ravel()])
                assert np.array_equal(_cpu(a), want[0]) and np.array_equal(_cpu(b), want[1]), (N, dtype, ra, rb, rx)
                _finish(checks)
            P.same_everywhere(got, "dihedral_inputs %s" % dtype)


@gpu
@pytest.mark.parametrize("H,W", ENS_SHAPES)
def test_dihedral_mean_at_every_placement(hip_device, H, W):
    from larvanet_amd import image_utils as U
    from larvanet_amd import kernels as K
    from larvanet_amd.metrics import image_to_uint8
    for N in (1, 2):
        rng = np.random.default_rng([H, W, N, 5])
        base = (rng.random((N, 3, H, W)) * 290 - 15).astype(np.float32)     # the mean leaves 0 .. 255 on both sides
        noisy = [base + (rng.random(base.shape) * 10 - 5).astype(np.float32) for _ in range(8)]
        a = np.stack([np.ascontiguousarray(U.dihedral(noisy[t][i], t, (1, 2))) for i in range(N) for t in range(4)])
        b = np.stack([np.ascontiguousarray(U.dihedral(noisy[t][i], t, (1, 2))) for i in range(N) for t in range(4, 8)])
        want = np.empty((N, 3, H, W), np.float32)
        for i in range(N):
            acc = None
            for t in range(8):
                v = U.dihedral_inv(a[4 * i + t] if t < 4 else b[4 * i + t - 4], t, (1, 2))
                acc = v if acc is None else acc + v          # the fixed order of test_self_ensemble
            want[i] = acc * np.float32(0.125)
        want8 = np.ascontiguousarray(image_to_uint8(want).transpose(0, 2, 3, 1))
        got, got8 = {}, {}
        for ra, rb, ro in ENS_MOVES:
            checks = []
            out = _place((N, 3, H, W), F32, hip_device, ro, checks)
            K.dihedral_mean(_place(a, F32, hip_device, ra, checks), _place(b, F32, hip_device, rb, checks), out=out)
            got[ra, rb, ro] = _cpu(out)
            assert np.array_equal(got[ra, rb, ro], want), (N, ra, rb, ro)
            _finish(checks)
        for ra, rb, ro in [(0, 0, r) for r in range(5)] + [(4, 0, 0), (0, 4, 0), (4, 4, 4), (8, 8, 8), (12, 12, 12)]:
            checks = []
            out = _place((N, H, W, 3), U8, hip_device, ro, checks)
            K.dihedral_mean(_place(a, F32, hip_device, ra, checks), _place(b, F32, hip_device, rb, checks), u8=True, out=out)
            got8[ra, rb, ro] = _cpu(out)
            assert np.array_equal(got8[ra, rb, ro], want8), (N, ra, rb, ro)
            _finish(checks)
        P.same_everywhere(got, "dihedral_mean f32")
        P.same_everywhere(got8, "dihedral_mean u8")


# =====================================================================================================================
# bicubic x4 with out & 15 != 0, and the bilinear refusal (csrc/larva_pointwise.hip)
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 16, 20)])
def test_bicubic4_with_an_unaligned_output(hip_device, shape):
    """larva_bicubic4_fwd sends an `out` that is not 16-byte aligned to bicubic4_kernel<false> (four 4-byte stores per
    lane).  Its arithmetic is bicubic4_block_kernel's by construction (the same dyadic weights, the same order of the
    row and column sums), so the two launches are compared bit for bit, and each against the oracles of test_bicubic4 /
    test_upsample4_modes_match_f_interpolate at their bar."""
    import torch.nn.functional as F
    from larvanet_amd import hip_lib
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    lib = hip_lib.load()
    n, c, h, w = shape
    x = (np.random.default_rng([n, c, h, w]).random(shape) * 255).astype(np.float32)
    ref_c = R.bicubic_up(x, 4)
    ref_t = F.interpolate(torch.from_numpy(x), scale_factor=4, mode="bicubic", align_corners=False).numpy()
    wrapper = _cpu(K.bicubic4(torch.from_numpy(x).to(hip_device)))
    got = {"wrapper": wrapper}
    for xres, ores in ((0, 0), (0, 4), (0, 8), (0, 12), (4, 0), (4, 4), (12, 8)):
        checks = []
        xd = _place(x, F32, hip_device, xres, checks)
        out = _place((n, c, 4 * h, 4 * w), F32, hip_device, ores, checks)
        hip_lib.check(lib.larva_bicubic4_fwd(xd.data_ptr(), out.data_ptr(), n, c, h, w, K._stream()), "larva_bicubic4_fwd")
        got[xres, ores] = _cpu(out)
        np.testing.assert_allclose(got[xres, ores], ref_c, rtol=1e-5, atol=3e-4, err_msg=str((xres, ores)))
        np.testing.assert_allclose(got[xres, ores], ref_t, rtol=1e-5, atol=3e-4, err_msg=str((xres, ores)))
        assert np.array_equal(got[xres, ores], wrapper), (xres, ores)      # the fallback == the aligned launch
        _finish(checks)
    P.same_everywhere(got, "bicubic4")
    # bilinear has no narrow walk: a misaligned out is refused and nothing is written
    for ores in (4, 8, 12):
        checks = []
        xd = _place(x, F32, hip_device, 0, checks)
        out, check_out = P.placed((n, c, 4 * h, 4 * w), F32, hip_device, ores)
        code = lib.larva_upsample4_fwd(xd.data_ptr(), out.data_ptr(), n, c, h, w, 1, K._stream())
        assert code == HIP_INVALID_VALUE
        with pytest.raises(RuntimeError):
            hip_lib.check(code, "larva_upsample4_fwd")
        torch.cuda.synchronize()
        check_out(untouched=True)
        _finish(checks)
    checks = []
    out = _place((n, c, 4 * h, 4 * w), F32, hip_device, 0, checks)
    xd = _place(x, F32, hip_device, 4, checks)
    hip_lib.check(lib.larva_upsample4_fwd(xd.data_ptr(), out.data_ptr(), n, c, h, w, 1, K._stream()), "larva_upsample4_fwd")
    ref_b = F.interpolate(torch.from_numpy(x), scale_factor=4, mode="bilinear", align_corners=False).numpy()
    np.testing.assert_allclose(_cpu(out), ref_b, rtol=1e-5, atol=3e-4)
    assert np.array_equal(_cpu(out), _cpu(K.upsample4(torch.from_numpy(x).to(hip_device), "bilinear")))
    _finish(checks)


# =====================================================================================================================
# head_conv3_direct: direct4 <-> direct through out & 15 at pitch % 4 == 0
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("N,H,W,pitch", [(1, 5, 16, 16), (2, 6, 20, 20), (1, 7, 13, 16)])
def test_head_conv3_direct_with_an_unaligned_output(hip_device, N, H, W, pitch):
    from larvanet_amd import hip_lib
    from larvanet_amd import kernels as K
    lib = hip_lib.load()
    rng = X.rng_of(N, H, W, pitch, 6)
    x, w, bias = X.ints(rng, (N, 3, H, W), 8), X.weights(rng, (48, 3, 3, 3), 4), X.ints(rng, (48,), 3)
    ref, inter = X.conv([x], w, bias)
    X.assert_exact_precondition(inter)
    ref = X.pad_pitch(ref.astype(np.float32), pitch)
    dev = lambda a: torch.from_numpy(a).to(hip_device)    # noqa: E731
    wrapper = K.head_conv3_direct(dev(x), dev(w), dev(bias), pitch=pitch)     # the aligned launch: direct4
    X.assert_bits_equal(wrapper, ref, "head_conv3_direct, aligned")
    got = {"wrapper": _cpu(wrapper)}
    for xres, wres, bres, ores in ((0, 0, 0, 0), (0, 0, 0, 4), (0, 0, 0, 8), (0, 0, 0, 12), (4, 0, 0, 0), (0, 4, 0, 0),
                                   (0, 0, 4, 0), (4, 4, 4, 4), (8, 8, 8, 8), (12, 12, 12, 12)):
        checks = []
        xd, wd, bd = (_place(a, F32, hip_device, r, checks) for a, r in ((x, xres), (w, wres), (bias, bres)))
        out = _place((N, 48, H, pitch), F32, hip_device, ores, checks)
        hip_lib.check(lib.larva_head_conv3_direct(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), N, 48, H, W,
                                                  pitch, K._stream()), "larva_head_conv3_direct")
        key = (xres, wres, bres, ores)
        got[key] = _cpu(out)
        X.assert_bits_equal(got[key], ref, "head_conv3_direct %s" % (key,))
        _finish(checks)
    P.same_everywhere(got, "head_conv3_direct")


# =====================================================================================================================
# resize_u8: address & 3 of the source and of the output (csrc/larva_resize.hip)
# =====================================================================================================================
def _resize_case(K, dev, N, H, W, h, w, rs, ro, img, want):
    checks = []
    x = _place(img, U8, dev, rs, checks)
    out = _place((N, h, w, 3), U8, dev, ro, checks)
    ret = K.resize_u8(x, h, w, out=out)
    got = _cpu(out)
    case = (N, H, W, h, w, rs, ro)
    assert ret is out and np.array_equal(got, want), "resize_u8 (N, H, W, h, w, src residue, out residue) = %s" % (case,)
    try:
        _finish(checks)
    except AssertionError as e:
        raise AssertionError("resize_u8 %s: %s" % (case, e))
    return got


@gpu
@pytest.mark.parametrize("H,W,h,w", RESIZE_SHAPES)
def test_resize_u8_at_every_skew_pair(hip_device, H, W, h, w):
    from larvanet_amd import image_utils as U
    from larvanet_amd import kernels as K
    assert (K.RESIZE_TILE_ROWS, K.RESIZE_TILE_COLS) == RESIZE_TILE
    for N in (1, 2):
        img = _image((N, H, W, 3), H, W, h, w, N)
        want = np.stack([U.resize_u8(img[n], h, w) for n in range(N)])
        got = {}
        for rs in range(4):
            for ro in range(4):
                got[rs, ro] = _resize_case(K, hip_device, N, H, W, h, w, rs, ro, img, want)
        P.same_everywhere(got, "resize_u8 %s N=%d" % ((H, W, h, w), N))


@gpu
def test_resize_u8_seeded_fuzz_of_shapes_and_skews(hip_device):
    from larvanet_amd import image_utils as U
    from larvanet_amd import kernels as K
    for N, H, W, h, w, rs, ro in resize_fuzz_cases():
        img = _image((N, H, W, 3), H, W, h, w, N, 9)
        want = np.stack([U.resize_u8(img[n], h, w) for n in range(N)])
        _resize_case(K, hip_device, N, H, W, h, w, rs, ro, img, want)


# =====================================================================================================================
# launchers that refuse: one misaligned operand each, RuntimeError from the wrapper, nothing written
# =====================================================================================================================
def _l1_operands(dev, ares, bres, checks, shape=(2, 3, 8, 12)):
    rng = np.random.default_rng(13)
    a = (rng.random(shape) * 255).astype(np.float32)
    b = (rng.random(shape) * 255).astype(np.float32)
    return _place(a, F32, dev, ares, checks), _place(b, F32, dev, bres, checks), a, b


@gpu
def test_refusing_launchers_refuse_before_writing(hip_device):
    from larvanet_amd import hip_lib
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    lib = hip_lib.load()
    g = torch.tensor(0.25, device=hip_device)
    n, c, hh, ww = 2, 3, 8, 12
    numel = n * c * hh * ww
    nws = int(lib.larva_l1_workspace_floats())
    # the aligned launches work on placed operands (and give what the existing tests pin)
    checks = []
    a, b, a_np, b_np = _l1_operands(hip_device, 0, 0, checks)
    assert abs(float(K.l1_fwd(a, b)) - R.l1_mean(a_np, b_np)) < 2e-6 * R.l1_mean(a_np, b_np) + 1e-6
    assert np.array_equal(_cpu(K.l1_bwd(a, b, g)), R.l1_grad(a_np, b_np, 0.25))
    assert np.array_equal(_cpu(K.l1_bwd_unshuffle4(a, b, g)), R.pixel_unshuffle(R.l1_grad(a_np, b_np, 0.25), 4))
    _finish(checks)
    for ares, bres in ((4, 0), (0, 4), (8, 12)):
        checks = []
        a, b, _, _ = _l1_operands(hip_device, ares, bres, checks)
        for call in (lambda: K.l1_fwd(a, b), lambda: K.l1_partial(a, b), lambda: K.l1_partial_grad(a, b, 1.0, 0.5),
                     lambda: K.l1_partial_grad_batch([a, a], b, 1.0, 0.5), lambda: K.l1_bwd(a, b, g),
                     lambda: K.l1_bwd_unshuffle4(a, b, g)):
            with pytest.raises(RuntimeError, match="hip error"):
                call()
        # the C ABI with the outputs in guarded buffers: refused (hipErrorInvalidValue), outputs still blank
        outs = []

        def blank(shape, dtype=F32):
            t, chk = P.placed(shape, dtype, hip_device, 0)
            outs.append(chk)
            return t.data_ptr()

        blocks = ctypes.c_int(-7)
        s = K._stream()
        pa, pb = a.data_ptr(), b.data_ptr()
        assert lib.larva_l1_fwd(pa, pb, numel, blank((nws,)), blank((1,)), s) == HIP_INVALID_VALUE
        assert lib.larva_l1_partial(pa, pb, numel, blank((nws,)), ctypes.byref(blocks), s) == HIP_INVALID_VALUE
        assert lib.larva_l1_partial_grad(pa, pb, 1.0, 0.5, blank((nws,)), ctypes.byref(blocks),
                                         blank((n, 16 * c, hh // 4, ww // 4)), n, c, hh // 4, ww // 4, s) == HIP_INVALID_VALUE
        assert lib.larva_l1_partial_grad_batch(hip_lib.ptr_array([pa]), pb, 1, 1.0, 0.5, hip_lib.ptr_array([blank((nws,))]),
                                               ctypes.byref(blocks), hip_lib.ptr_array([blank((n, 16 * c, hh // 4, ww // 4))]),
                                               n, c, hh // 4, ww // 4, s) == HIP_INVALID_VALUE
        assert lib.larva_l1_bwd(pa, pb, g.data_ptr(), numel, blank((numel,)), s) == HIP_INVALID_VALUE
        assert lib.larva_l1_bwd_unshuffle4(pa, pb, g.data_ptr(), 1.0, blank((numel,)), n, c, hh // 4, ww // 4,
                                           s) == HIP_INVALID_VALUE
        assert blocks.value == -7
        torch.cuda.synchronize()
        for chk in outs:
            chk(untouched=True)
        _finish(checks)
    # l1_bwd: the gradient it writes is the third operand of its predicate
    checks = []
    a, b, _, _ = _l1_operands(hip_device, 0, 0, checks)
    ga, chk_ga = P.placed((numel,), F32, hip_device, 4)
    assert lib.larva_l1_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), numel, ga.data_ptr(), K._stream()) == HIP_INVALID_VALUE
    # pixel_unshuffle4 reads its input 16 bytes at a time
    gin, chk_gin = P.placed(np.zeros((n, c, hh, ww), np.float32), F32, hip_device, 4)
    with pytest.raises(RuntimeError, match="hip error"):
        K.pixel_unshuffle4(gin)
    po, chk_po = P.placed((numel,), F32, hip_device, 0)
    assert lib.larva_pixel_unshuffle4(gin.data_ptr(), po.data_ptr(), n, c, hh // 4, ww // 4, K._stream()) == HIP_INVALID_VALUE
    torch.cuda.synchronize()
    chk_ga(untouched=True)
    chk_po(untouched=True)
    chk_gin()
    _finish(checks)
    # the step prologue's bicubic slices store 16 bytes per lane: a misaligned base is refused, an aligned one is bicubic4
    checks = []
    x_np = (np.random.default_rng(17).random((2, 3, 5, 7)) * 255).astype(np.float32)
    x = _place(x_np, F32, hip_device, 4, checks)
    x16, chk_x16 = P.placed((2, 16, 5, 7), F32, hip_device, 0)
    base, chk_base = P.placed((2, 3, 20, 28), F32, hip_device, 4)
    with pytest.raises(RuntimeError, match="hip error 1 "):
        K.step_prologue([], x, x16, base)
    torch.cuda.synchronize()
    chk_x16(untouched=True)
    chk_base(untouched=True)
    base = _place((2, 3, 20, 28), F32, hip_device, 0, checks)
    x16 = _place(np.zeros((2, 16, 5, 7), np.float32), F32, hip_device, 8, checks)
    K.step_prologue([], x, x16, base)
    assert np.array_equal(_cpu(base), _cpu(K.bicubic4(torch.from_numpy(x_np).to(hip_device))))
    assert np.array_equal(_cpu(x16)[:, :3], x_np) and not _cpu(x16)[:, 3:].any()
    _finish(checks)


@gpu
def test_u8_metrics_refuses_a_misaligned_workspace_or_result(hip_device):
    from larvanet_amd import hip_lib
    from larvanet_amd import kernels as K
    lib = hip_lib.load()
    h, w = 16, 20
    out_np, truth_np = _image((h, w, 3), 1), _image((h, w, 3), 2)
    for ores, tres in ((0, 0), (1, 3)):        # the images may sit anywhere
        checks = []
        o, t = _place(out_np, U8, hip_device, ores, checks), _place(truth_np, U8, hip_device, tres, checks)
        rec = K.metrics_from_record(K.u8_metrics(o, t, 2, "rgb").cpu())
        d = out_np[2:-2, 2:-2].astype(np.int64) - truth_np[2:-2, 2:-2].astype(np.int64)
        assert rec["sse"] == int((d * d).sum()) and rec["n"] == d.size
        # (torch cannot express an int64 tensor at residue 4, so the wrapper cannot be handed one: the C ABI is called
        # with int32 views of the same bytes, and hip_lib.check turns its answer into the wrapper's RuntimeError)
        nbytes = int(lib.larva_u8_metrics_workspace_bytes(h - 4, w - 4, 0))
        for wres, rres in ((4, 0), (0, 4), (12, 12)):
            ws, chk_ws = P.placed((nbytes // 4,), I32, hip_device, wres)
            res2, chk_res2 = P.placed((K.METRIC_RESULT_WORDS * 2,), I32, hip_device, rres)
            code = lib.larva_u8_metrics(o.data_ptr(), 3 * w, t.data_ptr(), 3 * w, 2, 2, h - 4, w - 4, 0, 1, ws.data_ptr(),
                                        res2.data_ptr(), K._stream())
            assert code == HIP_INVALID_VALUE, (wres, rres)
            with pytest.raises(RuntimeError, match="hip error 1 "):
                hip_lib.check(code, "larva_u8_metrics")
            torch.cuda.synchronize()
            chk_ws(untouched=True)
            chk_res2(untouched=True)
        _finish(checks)


# =====================================================================================================================
# fp32 conv forward / dgrad (csrc/conv3x3_mfma.hip: conv_build's `aligned`)
# =====================================================================================================================
CONV_SHAPES = [(1, 5, 16), (2, 6, 20)]       # C = 48, pitch = W, W % 4 == 0: only the pointers decide
CONV_EPIS = ("plain", "relu", "res01", "mask", "shuffle_base")
CONV_OPERANDS = ("src", "wpk", "out", "res0", "res1", "mask")


def _conv_problem(N, H, W, epi, dgrad=False):
    rng = X.rng_of(N, H, W, CONV_EPIS.index(epi), int(dgrad))
    p = {"x": X.ints(rng, (N, 48, H, W), 8), "w": X.weights(rng, (48, 48, 3, 3), 4)}
    kw = {}
    if epi == "relu":
        kw["relu"] = True
    if epi == "mask":
        kw["mask"] = p["mask"] = X.masks(rng, (N, 48, H, W))
    if epi == "res01":
        kw["res0"] = p["res0"] = X.ints(rng, (N, 48, H, W), 8)
        kw["res1"] = p["res1"] = X.ints(rng, (N, 48, H, W), 8)
    if dgrad:
        ref, inter = X.dgrad(p["x"], p["w"], **kw)
    else:
        p["bias"] = X.ints(rng, (48,), 3)
        ref, inter = X.conv([p["x"]], p["w"], p["bias"], **kw)
    if epi == "shuffle_base":
        ref = X.pixel_shuffle(ref, 4)
        p["base"] = X.ints(rng, ref.shape, 255, lo=0)
        ref = ref + p["base"]
        inter.append(ref)
    X.assert_exact_precondition(inter)
    p["ref"] = ref.astype(np.float32)
    return p


def _conv_moves(epi):
    used = {"plain": ("src", "wpk", "out"), "relu": ("src", "wpk", "out"), "mask": ("src", "wpk", "out", "mask"),
            "res01": ("src", "wpk", "out", "res0", "res1"), "shuffle_base": ("src", "wpk")}[epi]
    moves = [{}] + [{k: 4} for k in used] + [{k: r for k in used} for r in (4, 8, 12)]
    return moves


def _conv_launch(K, dev, p, wpk_np, epi, move, checks, dgrad=False, **extra):
    r = lambda k: move.get(k, 0)       # noqa: E731
    shuffle = epi == "shuffle_base"
    out = _place(p["ref"].shape, F32, dev, r("out"), checks)
    opt = lambda k: None if k not in p else _place(p[k], F32, dev, r(k), checks)     # noqa: E731
    K.conv3x3(_place(p["x"], F32, dev, r("src"), checks), _place(wpk_np, F32, dev, r("wpk"), checks), 48,
              bias=None if dgrad else _place(p["bias"], F32, dev, r("bias"), checks), relu=epi == "relu", mask=opt("mask"),
              res0=opt("res0"), res1=opt("res1"), shuffle=shuffle, base=opt("base"), out=out, **extra)
    return out


@gpu
@pytest.mark.parametrize("dgrad", [False, True], ids=["forward", "dgrad"])
@pytest.mark.parametrize("N,H,W", CONV_SHAPES)
def test_conv3x3_with_each_operand_off_the_16_byte_grid(hip_device, N, H, W, dgrad):
    """pitch % 4 == 0 and one operand (then all) at residue 4 / 8 / 12: conv_build's `aligned` is false through a pointer,
    the register-staged kernel runs, and gives the bytes of the aligned launch and of exact_ref."""
    from larvanet_amd import kernels as K
    for epi in CONV_EPIS:
        if dgrad and epi in ("relu", "shuffle_base"):
            continue
        p = _conv_problem(N, H, W, epi, dgrad)
        fwd, bwd = K.pack_weights(torch.from_numpy(p["w"]).to(hip_device), want_bwd=True)
        wpk_np = _cpu(bwd if dgrad else fwd)
        got = {}
        for move in _conv_moves(epi):
            checks = []
            out = _conv_launch(K, hip_device, p, wpk_np, epi, move, checks, dgrad)
            key = tuple(sorted(move.items()))
            got[key] = _cpu(out)
            X.assert_bits_equal(got[key], p["ref"], "conv3x3 %s %s %s" % ("dgrad" if dgrad else "fwd", epi, move))
            _finish(checks)
        # the bias may sit anywhere a float may (scalar loads), on the aligned and on the register-staged path
        if not dgrad:
            for move in ({"bias": 4}, {"bias": 12, "src": 4}):
                checks = []
                out = _conv_launch(K, hip_device, p, wpk_np, epi, move, checks)
                X.assert_bits_equal(out, p["ref"], "conv3x3 %s %s" % (epi, move))
                _finish(checks)
        P.same_everywhere(got, "conv3x3 %s" % epi)


@gpu
def test_conv3x3_pixel_shuffle_refuses_an_unaligned_image(hip_device):
    """The pixel-shuffle epilogue moves four HR pixels as one 16-byte access on EVERY staging path: the HR output and
    the base image must be 16-byte aligned (include/larva_hip.h), whatever the other operands allow.  Refused with
    hipErrorInvalidValue by every entry point that takes mode 1, before anything is written."""
    from larvanet_amd import kernels as K
    N, H, W = CONV_SHAPES[0]
    p = _conv_problem(N, H, W, "shuffle_base")
    wpk_np = _cpu(K.pack_weights(torch.from_numpy(p["w"]).to(hip_device), want_bwd=False)[0])
    for move in ({"base": 4}, {"out": 4}, {"base": 8, "out": 12}, {"base": 4, "src": 4}):
        for extra in ({}, {"strips": True}, {"tile_rows": 3}):
            checks = []
            r = lambda k: move.get(k, 0)       # noqa: E731
            out, chk_out = P.placed(p["ref"].shape, F32, hip_device, r("out"))
            with pytest.raises(RuntimeError, match="hip error 1 "):
                K.conv3x3(_place(p["x"], F32, hip_device, r("src"), checks), _place(wpk_np, F32, hip_device, 0, checks), 48,
                          bias=_place(p["bias"], F32, hip_device, 0, checks), shuffle=True,
                          base=_place(p["base"], F32, hip_device, r("base"), checks), out=out, **extra)
            torch.cuda.synchronize()
            chk_out(untouched=True)
            _finish(checks)
    # without a base the output alone decides
    out, chk_out = P.placed(p["ref"].shape, F32, hip_device, 4)
    dev = lambda a: torch.from_numpy(a).to(hip_device)    # noqa: E731
    with pytest.raises(RuntimeError, match="hip error 1 "):
        K.conv3x3(dev(p["x"]), dev(wpk_np), 48, bias=dev(p["bias"]), shuffle=True, out=out)
    torch.cuda.synchronize()
    chk_out(untouched=True)


@gpu
def test_conv3x3_tiled_persistent_strips_and_batched_entry_points_with_a_misaligned_job(hip_device, monkeypatch):
    """What each 16-byte-only entry point answers to one operand at residue 4, and what the wrapper does next:
    4-row tiles: hipErrorNotSupported from larva_conv3x3_fwd_tiled (the wrapper raises); strips: hipErrorNotSupported,
    kernels.conv3x3 goes on to the regular tiles; batch: hipErrorNotSupported, kernels.conv3x3_batch launches the jobs
    one by one; exit-L1 batch: hipErrorNotSupported, kernels.conv3x3_exit_l1_batch returns None."""
    from larvanet_amd import hip_lib
    from larvanet_amd import kernels as K
    lib = hip_lib.load()
    N, H, W = 2, 9, 20          # 9 rows: a strip table exists (5 + 4)
    assert K.strip_tile_table(H, W, hip_device) is not None
    rng = X.rng_of(N, H, W, 31)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)    # noqa: E731
    jobs_np = []
    for j in range(2):
        x, w, bias = X.ints(rng, (N, 48, H, W), 8), X.weights(rng, (48, 48, 3, 3), 4), X.ints(rng, (48,), 3)
        ref, inter = X.conv([x], w, bias, relu=True)
        X.assert_exact_precondition(inter)
        jobs_np.append({"x": x, "w": w, "bias": bias, "ref": ref.astype(np.float32),
                        "wpk": _cpu(K.pack_weights(dev(w), want_bwd=False)[0])})
    j0 = jobs_np[0]
    codes = []
    real = {n: getattr(lib, n) for n in ("larva_conv3x3_fwd_strips", "larva_conv3x3_fwd_batch", "larva_conv3x3_fwd_tiled")}

    class Spy:
        """The library with the return codes of three entry points recorded (the wrappers call lib.<name>)."""
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in real:
                return fn

            def call(*a):
                code = fn(*a)
                codes.append((name, code))
                return code
            return call

    monkeypatch.setattr(hip_lib, "load", lambda: Spy())
    for operand in ("src", "wpk", "out"):
        r = lambda k: 4 if k == operand else 0       # noqa: E731
        # strips -> regular tiles
        checks, codes[:] = [], []
        out = _place(j0["ref"].shape, F32, hip_device, r("out"), checks)
        K.conv3x3(_place(j0["x"], F32, hip_device, r("src"), checks), _place(j0["wpk"], F32, hip_device, r("wpk"), checks),
                  48, bias=dev(j0["bias"]), relu=True, out=out, strips=True)
        assert codes == [("larva_conv3x3_fwd_strips", HIP_NOT_SUPPORTED)], (operand, codes)
        X.assert_bits_equal(out, j0["ref"], "strips fallback, %s at residue 4" % operand)
        _finish(checks)
        # 4-row tiles: not on the register-staged path
        checks, codes[:] = [], []
        out, chk_out = P.placed(j0["ref"].shape, F32, hip_device, r("out"))
        with pytest.raises(RuntimeError, match="hip error 801 "):
            K.conv3x3(_place(j0["x"], F32, hip_device, r("src"), checks), _place(j0["wpk"], F32, hip_device, r("wpk"), checks),
                      48, bias=dev(j0["bias"]), relu=True, out=out, tile_rows=4)
        torch.cuda.synchronize()
        chk_out(untouched=True)
        _finish(checks)
        # 3-row tiles asked for by name: the register-staged kernel
        checks = []
        out = _place(j0["ref"].shape, F32, hip_device, r("out"), checks)
        K.conv3x3(_place(j0["x"], F32, hip_device, r("src"), checks), _place(j0["wpk"], F32, hip_device, r("wpk"), checks),
                  48, bias=dev(j0["bias"]), relu=True, out=out, tile_rows=3)
        X.assert_bits_equal(out, j0["ref"], "tile_rows=3, %s at residue 4" % operand)
        _finish(checks)
        # batch: job 1 carries the misaligned operand -> one launch per job, both right
        checks, codes[:] = [], []
        outs = [_place(j["ref"].shape, F32, hip_device, r("out") if n else 0, checks) for n, j in enumerate(jobs_np)]
        jobs = [{"srcs": _place(j["x"], F32, hip_device, r("src") if n else 0, checks),
                 "wpk": _place(j["wpk"], F32, hip_device, r("wpk") if n else 0, checks), "bias": dev(j["bias"])}
                for n, j in enumerate(jobs_np)]
        ret = K.conv3x3_batch(jobs, 48, relu=True, outs=outs)
        assert codes[0] == ("larva_conv3x3_fwd_batch", HIP_NOT_SUPPORTED) and len(ret) == 2, (operand, codes)
        for n, j in enumerate(jobs_np):
            assert ret[n] is outs[n]
            X.assert_bits_equal(outs[n], j["ref"], "batch fallback job %d, %s at residue 4" % (n, operand))
        _finish(checks)
    monkeypatch.undo()
    # persistent tiles: a launch of more 3 x 48 tiles than the chip has workgroup slots (2 per CU) walks them with one
    # workgroup per slot on the 16-byte path only; one operand at residue 4 takes the launch to one register-staged
    # workgroup per tile.  Same bytes, and LARVA_PERSIST=0 (the per-tile launch of the aligned operands) as well.
    slots = 2 * torch.cuda.get_device_properties(hip_device).multi_processor_count
    Np, Hp, Wp = -(-(slots + 1) // (16 * 2)), 48, 96
    assert Np * 16 * 2 > slots
    xp = X.ints(rng, (Np, 48, Hp, Wp), 8)
    refp, inter = X.conv([xp], j0["w"], j0["bias"], relu=True)
    X.assert_exact_precondition(inter)
    gotp = {}
    for operand in (None, "src", "wpk", "out"):
        r = lambda k: 4 if k == operand else 0       # noqa: E731
        checks = []
        out = _place(refp.shape, F32, hip_device, r("out"), checks)
        K.conv3x3(_place(xp, F32, hip_device, r("src"), checks), _place(j0["wpk"], F32, hip_device, r("wpk"), checks), 48,
                  bias=dev(j0["bias"]), relu=True, out=out)
        gotp[operand] = _cpu(out)
        X.assert_bits_equal(gotp[operand], refp, "more tiles than slots, %s at residue 4" % operand)
        _finish(checks)
    monkeypatch.setenv("LARVA_PERSIST", "0")
    gotp["per tile"] = _cpu(K.conv3x3(dev(xp), dev(j0["wpk"]), 48, bias=dev(j0["bias"]), relu=True))
    monkeypatch.delenv("LARVA_PERSIST")
    P.same_everywhere(gotp, "conv3x3 over more tiles than slots")
    # exit-L1 batch: a misaligned source, truth or base -> None (the caller runs conv and L1 separately)
    base = X.ints(rng, (N, 3, 4 * H, 4 * W), 255, lo=0)
    truth = X.ints(rng, (N, 3, 4 * H, 4 * W), 255, lo=0)
    for operand in ("src", "base", "truth"):
        checks = []
        r = lambda k: 4 if k == operand else 0       # noqa: E731
        jobs = [{"srcs": _place(j["x"], F32, hip_device, r("src") if n else 0, checks), "wpk": dev(j["wpk"]),
                 "bias": dev(j["bias"]), "base": _place(base, F32, hip_device, r("base") if n else 0, checks)}
                for n, j in enumerate(jobs_np)]
        assert K.conv3x3_exit_l1_batch(jobs, 48, _place(truth, F32, hip_device, r("truth"), checks), 1.0, 0.5,
                                       [True, True]) is None, operand
        _finish(checks)


@gpu
def test_aligned_operands_take_the_one_launch_paths(hip_device, monkeypatch):
    """The other side of the fallbacks above, pinned on its own: with every operand on the 16-byte grid the strip launch,
    the 4-row tiles, the batched launch, the exit-L1 launch and the flat weight-gradient grid are what runs (return code
    0, not 801), and their results are the integer reference's."""
    from larvanet_amd import hip_lib
    from larvanet_amd import kernels as K
    lib = hip_lib.load()
    N, H, W = 2, 9, 20
    rng = X.rng_of(N, H, W, 32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)    # noqa: E731
    jobs_np = []
    for j in range(2):
        x, w, bias = X.ints(rng, (N, 48, H, W), 8), X.weights(rng, (48, 48, 3, 3), 4), X.ints(rng, (48,), 3)
        ref, inter = X.conv([x], w, bias, relu=True)
        X.assert_exact_precondition(inter)
        jobs_np.append({"x": x, "w": w, "bias": bias, "ref": ref.astype(np.float32),
                        "wpk": K.pack_weights(dev(w), want_bwd=False)[0]})
    codes = []
    watched = ("larva_conv3x3_fwd_strips", "larva_conv3x3_fwd_batch", "larva_conv3x3_fwd_tiled", "larva_conv3x3_exit_l1_batch",
               "larva_conv3x3_wgrad_partial_flat")

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in watched:
                return fn

            def call(*a):
                code = fn(*a)
                codes.append((name, code))
                return code
            return call

    monkeypatch.setattr(hip_lib, "load", lambda: Spy())
    j0 = jobs_np[0]
    checks = []
    place = lambda a: _place(a, F32, hip_device, 0, checks)     # noqa: E731
    for extra, name in (({"strips": True}, "larva_conv3x3_fwd_strips"), ({"tile_rows": 4}, "larva_conv3x3_fwd_tiled")):
        codes[:] = []
        out = place(j0["ref"].shape)
        K.conv3x3(place(j0["x"]), j0["wpk"], 48, bias=dev(j0["bias"]), relu=True, out=out, **extra)
        assert codes == [(name, 0)], codes
        X.assert_bits_equal(out, j0["ref"], name)
    codes[:] = []
    outs = [place(j["ref"].shape) for j in jobs_np]
    K.conv3x3_batch([{"srcs": place(j["x"]), "wpk": j["wpk"], "bias": dev(j["bias"])} for j in jobs_np], 48, relu=True, outs=outs)
    assert codes == [("larva_conv3x3_fwd_batch", 0)], codes
    for n, j in enumerate(jobs_np):
        X.assert_bits_equal(outs[n], j["ref"], "batch job %d" % n)
    base = X.ints(rng, (N, 3, 4 * H, 4 * W), 255, lo=0)
    truth = X.ints(rng, (N, 3, 4 * H, 4 * W), 255, lo=0)
    codes[:] = []
    res = K.conv3x3_exit_l1_batch([{"srcs": place(j["x"]), "wpk": j["wpk"], "bias": dev(j["bias"]), "base": place(base)}
                                   for j in jobs_np], 48, place(truth), 1.0, 0.5, [True, True])
    assert codes == [("larva_conv3x3_exit_l1_batch", 0)] and res is not None, codes
    for n, j in enumerate(jobs_np):
        ref, inter = X.conv([j["x"]], j["w"], j["bias"])
        img = X.pixel_shuffle(ref, 4) + base
        X.assert_exact_precondition(inter + [img])
        X.assert_bits_equal(res[0][n], img, "exit image %d" % n)
        X.assert_bits_equal(res[2][n], X.pixel_unshuffle(X.l1_sign_grad(img, truth, np.float32(0.5) / np.float32(truth.size)), 4),
                            "exit gradient %d" % n)
    dy, x = X.ints(rng, (N, 48, H, W), 2), X.ints(rng, (N, 48, H, W), 2)
    dw_ref, db_ref, inter = X.wgrad(dy, x)
    X.assert_exact_precondition(inter)
    codes[:] = []
    flat = K.conv3x3_wgrad_partial_flat([{"dy": place(dy), "x": place(x)}], 48, 48, 8)
    assert codes == [("larva_conv3x3_wgrad_partial_flat", 0)] and flat is not None, codes
    dw, db = place((48, 48, 3, 3)), place((48,))
    K.wgrad_reduce([{"partial": flat[0][0], "splits": flat[1][0], "dw": dw, "db": db}], 48, 48)
    X.assert_bits_equal(dw, dw_ref, "flat grid dw")
    X.assert_bits_equal(db, db_ref, "flat grid db")
    _finish(checks)


# =====================================================================================================================
# weight gradient (csrc/wgrad3x3_mfma.hip: vec_ok, the flat grid, the partial images)
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("N,H,W", CONV_SHAPES)
def test_wgrad_with_dy_or_x_off_the_16_byte_grid(hip_device, N, H, W):
    from larvanet_amd import hip_lib
    from larvanet_amd import kernels as K
    lib = hip_lib.load()
    rng = X.rng_of(N, H, W, 41)
    dy, x = X.ints(rng, (N, 48, H, W), 2), X.ints(rng, (N, 48, H, W), 2)
    dw_ref, db_ref, inter = X.wgrad(dy, x)
    X.assert_exact_precondition(inter)
    got = {}
    for rdy, rx in ((0, 0), (4, 0), (0, 4), (4, 4), (8, 8), (12, 12)):
        checks = []
        dw, db = _place((48, 48, 3, 3), F32, hip_device, rx, checks), _place((48,), F32, hip_device, rdy, checks)
        d, xx = _place(dy, F32, hip_device, rdy, checks), _place(x, F32, hip_device, rx, checks)
        K.conv3x3_wgrad([{"dy": d, "x": xx, "dw": dw, "db": db}], 48, 48, 2)
        got[rdy, rx] = np.concatenate([_cpu(dw).ravel(), _cpu(db)])
        X.assert_bits_equal(dw, dw_ref, "wgrad dw, dy at %d, x at %d" % (rdy, rx))
        X.assert_bits_equal(db, db_ref, "wgrad db, dy at %d, x at %d" % (rdy, rx))
        # the flat grid has no narrow walk: hipErrorNotSupported, the wrapper answers None and the caller (autograd)
        # goes on with conv3x3_wgrad_partial, whose result is reduced to the same gradients
        flat = K.conv3x3_wgrad_partial_flat([{"dy": d, "x": xx}], 48, 48, 8)
        if (rdy, rx) != (0, 0):
            assert flat is None, (rdy, rx)
            used = (ctypes.c_int * 1)()
            blank, chk_blank = P.placed((K.wgrad_partial_floats(48, 48, 4),), F32, hip_device, 0)
            code = lib.larva_conv3x3_wgrad_partial_flat(hip_lib.ptr_array([d.data_ptr()]), hip_lib.ptr_array([xx.data_ptr()]),
                                                        hip_lib.ptr_array([blank.data_ptr()]), 1, 8, N, 48, 48, H, W, used,
                                                        K._stream())
            assert code == HIP_NOT_SUPPORTED
            torch.cuda.synchronize()
            chk_blank(untouched=True)
        if flat is not None:     # (aligned operands: test_aligned_operands_take_the_one_launch_paths pins that it is taken)
            parts, splits = flat
        else:
            parts, used_splits = K.conv3x3_wgrad_partial([{"dy": d, "x": xx}], 48, 48, 8)
            splits = [used_splits]
            parts = [parts[0][:K.wgrad_partial_floats(48, 48, used_splits)]]
        dw2, db2 = _place((48, 48, 3, 3), F32, hip_device, 4, checks), _place((48,), F32, hip_device, 8, checks)
        K.wgrad_reduce([{"partial": parts[0], "splits": splits[0], "dw": dw2, "db": db2}], 48, 48)
        X.assert_bits_equal(dw2, dw_ref, "wgrad (flat or its fallback) dw, dy at %d, x at %d" % (rdy, rx))
        X.assert_bits_equal(db2, db_ref, "wgrad (flat or its fallback) db")
        _finish(checks)
    P.same_everywhere(got, "conv3x3_wgrad")


@gpu
def test_wgrad_refuses_a_misaligned_partial_buffer(hip_device):
    """The partial images are written and reduced 16 bytes per lane on every path (include/larva_hip.h)."""
    from larvanet_amd import kernels as K
    N, H, W = CONV_SHAPES[0]
    rng = X.rng_of(N, H, W, 43)
    dev = lambda a: torch.from_numpy(a).to(hip_device)    # noqa: E731
    dy, x = dev(X.ints(rng, (N, 48, H, W), 2)), dev(X.ints(rng, (N, 48, H, W), 2))
    nfl = K.wgrad_partial_floats(48, 48, 2)
    for res in (4, 8, 12):
        part, chk_part = P.placed((nfl,), F32, hip_device, res)
        dw, chk_dw = P.placed((48, 48, 3, 3), F32, hip_device, 0)
        db, chk_db = P.placed((48,), F32, hip_device, 0)
        with pytest.raises(RuntimeError, match="hip error 1 "):
            K.conv3x3_wgrad([{"dy": dy, "x": x, "dw": dw, "db": db, "partial": part}], 48, 48, 2)
        with pytest.raises(RuntimeError, match="hip error 1 "):
            K.wgrad_reduce([{"partial": part, "splits": 2, "dw": dw, "db": db}], 48, 48)
        torch.cuda.synchronize()
        for chk in (chk_part, chk_dw, chk_db):
            chk(untouched=True)


# =====================================================================================================================
# fp16 inference kernels (csrc/conv3x3_f16.hip)
# =====================================================================================================================
def _f16_problem(N, H, W, epi):
    rng = X.rng_of(N, H, W, 51, ("plain", "relu", "res01").index(epi))
    p = {"x": X.ints(rng, (N, H, W, 48), 4), "w": X.weights(rng, (48, 48, 3, 3), 2), "bias": X.ints(rng, (48,), 3)}
    kw = {"relu": True} if epi == "relu" else {}
    if epi == "res01":
        p["res0"], p["res1"] = X.ints(rng, (N, H, W, 48), 4), X.ints(rng, (N, H, W, 48), 4)
        kw = {"res0": p["res0"].transpose(0, 3, 1, 2), "res1": p["res1"].transpose(0, 3, 1, 2)}
    ref, inter = X.conv([p["x"].transpose(0, 3, 1, 2)], p["w"], p["bias"], **kw)
    X.assert_exact_precondition(inter)
    X.assert_exact_precondition([ref], X.HALF_MAX + 1)
    p["ref_nchw"] = ref
    p["ref"] = np.ascontiguousarray(ref.transpose(0, 2, 3, 1))
    return p


@gpu
def test_f16_head_operands_anywhere_their_type_allows(hip_device):
    """By reading head_kernel: the image, the fp32 weights, the bias and the flag are accessed one element at a time (any
    4-byte boundary); the fp16 output leaves as two 16-byte stores per thread (16-byte aligned, refused otherwise)."""
    from larvanet_amd import kernels as K
    N, H, W = 2, 5, 7
    rng = X.rng_of(N, H, W, 52)
    x, w, bias = X.ints(rng, (N, 3, H, W), 15, lo=0), X.weights(rng, (48, 3, 3, 3), 4), X.ints(rng, (48,), 3)
    ref, inter = X.conv([x], w, bias)
    X.assert_exact_precondition(inter)
    X.assert_exact_precondition([ref], X.HALF_MAX + 1)
    ref = np.ascontiguousarray(ref.transpose(0, 2, 3, 1))
    got = {}
    for rx, rw, rb, rf in ((0, 0, 0, 0), (4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 4, 0), (0, 0, 0, 4), (4, 4, 4, 4), (8, 8, 8, 8),
                           (12, 12, 12, 12)):
        checks = []
        flag = _place(np.zeros(1, np.int32), I32, hip_device, rf, checks)
        out = _place((N, H, W, 48), F16, hip_device, 0, checks)
        K.f16_head(_place(x, F32, hip_device, rx, checks), _place(w, F32, hip_device, rw, checks),
                   _place(bias, F32, hip_device, rb, checks), flag, out=out)
        got[rx, rw, rb, rf] = _cpu(out)
        X.assert_bits_equal(got[rx, rw, rb, rf], ref, "f16_head %s" % ((rx, rw, rb, rf),))
        assert int(flag.item()) == 0
        _finish(checks)
    P.same_everywhere(got, "f16_head")
    dev = lambda a: torch.from_numpy(a).to(hip_device)    # noqa: E731
    for ores in (2, 4, 8, 14):
        out, chk_out = P.placed((N, H, W, 48), F16, hip_device, ores)
        flag = torch.zeros(1, dtype=I32, device=hip_device)
        with pytest.raises(RuntimeError, match="hip error 1 "):
            K.f16_head(dev(x), dev(w), dev(bias), flag, out=out)
        torch.cuda.synchronize()
        chk_out(untouched=True)
        assert int(flag.item()) == 0


@gpu
def test_f16_convs_refuse_operands_their_wide_accesses_cannot_take(hip_device):
    """By reading conv_tile: sources and weight images are loaded 16 bytes at a time, the fp32 bias, base and HR output
    16, residuals and the fp16 output 8 (held to the sources' 16: an output is the next layer's source), the uint8 HR
    image as 4-byte words.  Only the flag may sit on any 4-byte boundary.  Every other placement is refused with
    hipErrorInvalidValue before a launch; none of them is launched here."""
    from larvanet_amd import kernels as K
    N, H, W = 1, 5, 70
    dev = lambda a: torch.from_numpy(a).to(hip_device)    # noqa: E731
    for epi in ("plain", "relu", "res01"):
        p = _f16_problem(N, H, W, epi)
        wpk = K.f16_pack_weights(dev(p["w"]))
        wpk_np = _cpu(wpk)
        for rf in (0, 4, 8, 12):      # aligned operands, the flag anywhere
            checks = []
            flag = _place(np.zeros(1, np.int32), I32, hip_device, rf, checks)
            out = _place((N, H, W, 48), F16, hip_device, 0, checks)
            K.f16_conv3x3(_place(p["x"], F16, hip_device, 0, checks), _place(wpk_np, F16, hip_device, 0, checks),
                          _place(p["bias"], F32, hip_device, 0, checks), flag, relu=epi == "relu",
                          res0=None if "res0" not in p else _place(p["res0"], F16, hip_device, 0, checks),
                          res1=None if "res1" not in p else _place(p["res1"], F16, hip_device, 0, checks), out=out)
            X.assert_bits_equal(out, p["ref"], "f16_conv3x3 %s, flag at %d" % (epi, rf))
            assert int(flag.item()) == 0
            _finish(checks)
        names = ["src", "wpk", "bias", "out"] + (["res0", "res1"] if epi == "res01" else [])
        for name in names:
            for res in ((4, 8, 12) if name == "bias" else (2, 8, 14)):
                r = lambda k: res if k == name else 0       # noqa: E731
                checks = []
                out, chk_out = P.placed((N, H, W, 48), F16, hip_device, r("out"))
                flag = torch.zeros(1, dtype=I32, device=hip_device)
                with pytest.raises(RuntimeError, match="hip error 1 "):
                    K.f16_conv3x3(_place(p["x"], F16, hip_device, r("src"), checks),
                                  _place(wpk_np, F16, hip_device, r("wpk"), checks),
                                  _place(p["bias"], F32, hip_device, r("bias"), checks), flag, relu=epi == "relu",
                                  res0=None if "res0" not in p else _place(p["res0"], F16, hip_device, r("res0"), checks),
                                  res1=None if "res1" not in p else _place(p["res1"], F16, hip_device, r("res1"), checks),
                                  out=out)
                torch.cuda.synchronize()
                chk_out(untouched=True)
                _finish(checks)
    # the weight image being packed
    p = _f16_problem(N, H, W, "plain")
    for res in (2, 8):
        img, chk_img = P.placed((K.f16_packed_weight_halves(48, 48),), F16, hip_device, res)
        with pytest.raises(RuntimeError, match="hip error 1 "):
            K.f16_pack_weights(dev(p["w"]), out=img)
        torch.cuda.synchronize()
        chk_img(untouched=True)
    checks = []
    img = _place((K.f16_packed_weight_halves(48, 48),), F16, hip_device, 0, checks)
    K.f16_pack_weights(_place(p["w"], F32, hip_device, 4, checks), out=img)     # (the fp32 weights: anywhere)
    assert torch.equal(img, K.f16_pack_weights(dev(p["w"])))
    _finish(checks)


@gpu
def test_f16_leg_ends_placements_and_refusals(hip_device):
    """The two leg ends (fp32 and uint8 HR image), single and as jobs: the uint8 image may sit on any 4-byte boundary
    (12 bytes per lane as three words), everything else as in test_f16_convs_refuse_...."""
    from larvanet_amd import hip_lib
    from larvanet_amd import kernels as K
    from larvanet_amd.metrics import image_to_uint8
    lib = hip_lib.load()
    N, H, W = 2, 5, 7
    dev = lambda a: torch.from_numpy(a).to(hip_device)    # noqa: E731
    p = _f16_problem(N, H, W, "plain")
    base = X.ints(X.rng_of(N, H, W, 53), (N, 3, 4 * H, 4 * W), 255, lo=0)
    hr = X.pixel_shuffle(p["ref_nchw"], 4) + base
    X.assert_exact_precondition([hr])
    hr8 = np.ascontiguousarray(image_to_uint8(hr.astype(np.float32)).transpose(0, 2, 3, 1))
    wpk_np = _cpu(K.f16_pack_weights(dev(p["w"])))
    aligned = lambda checks: (_place(p["x"], F16, hip_device, 0, checks), _place(wpk_np, F16, hip_device, 0, checks),   # noqa: E731
                              _place(p["bias"], F32, hip_device, 0, checks), _place(base, F32, hip_device, 0, checks))
    checks = []
    X.assert_bits_equal(K.f16_conv3x3_shuffle_base(*aligned(checks)), hr, "f16 leg end, fp32")
    _finish(checks)
    got = {}
    for ores, rf in ((0, 0), (4, 4), (8, 0), (12, 12)):
        checks = []
        flag = _place(np.zeros(1, np.int32), I32, hip_device, rf, checks)
        out = _place((N, 4 * H, 4 * W, 3), U8, hip_device, ores, checks)
        K.f16_conv3x3_shuffle_base_u8(*aligned(checks), flag, out=out)
        got[ores, rf] = _cpu(out)
        assert np.array_equal(got[ores, rf], hr8) and int(flag.item()) == 0, (ores, rf)
        # the same through the job launch (M = 1: out[0] is the placed image)
        out2 = _place((1, N, 4 * H, 4 * W, 3), U8, hip_device, ores, checks)
        x, wpk, bias, bs = aligned(checks)
        K.f16_conv3x3_shuffle_base_jobs([x], [wpk], [bias], bs, flag=flag, u8=True, out=out2)
        assert np.array_equal(_cpu(out2)[0], hr8), (ores, rf)
        _finish(checks)
    P.same_everywhere(got, "f16 leg end, uint8")
    s = K._stream()
    flag = torch.zeros(1, dtype=I32, device=hip_device)
    for name in ("src", "wpk", "bias", "base", "out"):
        for u8 in (False, True):
            res = {"src": 8, "wpk": 8, "bias": 4, "base": 4, "out": (1 if u8 else 4)}[name]
            r = lambda k: res if k == name else 0       # noqa: E731
            checks = []
            x, wpk = _place(p["x"], F16, hip_device, r("src"), checks), _place(wpk_np, F16, hip_device, r("wpk"), checks)
            bias, bs = _place(p["bias"], F32, hip_device, r("bias"), checks), _place(base, F32, hip_device, r("base"), checks)
            if u8:
                out, chk_out = P.placed((N, 4 * H, 4 * W, 3), U8, hip_device, r("out"))
                one = lib.larva_f16_conv3x3_shuffle_base_u8(x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), bs.data_ptr(),
                                                            out.data_ptr(), flag.data_ptr(), N, H, W, s)
            else:
                out, chk_out = P.placed((N, 3, 4 * H, 4 * W), F32, hip_device, r("out"))
                one = lib.larva_f16_conv3x3_shuffle_base(x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), bs.data_ptr(),
                                                         out.data_ptr(), N, H, W, s)
            arrays = [hip_lib.ptr_array([t.data_ptr()]) for t in (x, wpk, bias)]
            outs = hip_lib.ptr_array([out.data_ptr()])
            many = lib.larva_f16_conv3x3_shuffle_base_jobs(1, *arrays, bs.data_ptr(), None if u8 else outs, outs if u8 else None,
                                                           flag.data_ptr(), N, H, W, s)
            assert (one, many) == (HIP_INVALID_VALUE, HIP_INVALID_VALUE), (name, u8)
            torch.cuda.synchronize()
            chk_out(untouched=True)
            _finish(checks)
    # the fp16 job launch (the legs' first convs)
    for name in ("src", "wpk", "bias", "out"):
        res = 4 if name == "bias" else 8
        r = lambda k: res if k == name else 0       # noqa: E731
        checks = []
        out, chk_out = P.placed((N, H, W, 48), F16, hip_device, r("out"))
        arrays = [hip_lib.ptr_array([_place(a, dt, hip_device, r(k), checks).data_ptr()])
                  for a, dt, k in ((p["x"], F16, "src"), (wpk_np, F16, "wpk"), (p["bias"], F32, "bias"))]
        code = lib.larva_f16_conv3x3_jobs(1, *arrays, 0, hip_lib.ptr_array([out.data_ptr()]), flag.data_ptr(), N, H, W, s)
        assert code == HIP_INVALID_VALUE, name
        torch.cuda.synchronize()
        chk_out(untouched=True)
        _finish(checks)
    assert int(flag.item()) == 0
