"""The exact bicubic resize to any size: image_utils.resize_coeffs / resize_u8 (the host definition: Pillow's
Image.resize(..., BICUBIC) byte for byte) and kernels.resize_u8 (csrc/larva_resize.hip), which equals the host definition
bit for bit.  Host logic runs anywhere; the kernel tests are marked gpu and every comparison is np.array_equal."""
import math
import os

import numpy as np
import pytest
import torch

from larvanet_amd import image_utils as U

# (H, W, h, w): both axes down, nearly unchanged, exactly x4 down, one axis unchanged (each), x4 up, mixed, tiny
PAIRS = [(48, 64, 27, 40), (37, 127, 36, 100), (64, 64, 16, 16), (40, 52, 40, 30), (33, 17, 50, 17), (20, 24, 80, 96),
         (135, 203, 72, 128), (7, 5, 2, 3)]


def _random(shape, seed=0):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def _extremes(h, w):
    board = (((np.add.outer(np.arange(h), np.arange(w)) % 2) * 255).astype(np.uint8))[..., None].repeat(3, axis=2)
    return {"zeros": np.zeros((h, w, 3), np.uint8), "ones": np.full((h, w, 3), 255, np.uint8),
            "board": np.ascontiguousarray(board)}


def _pillow(a, h, w):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((w, h), Image.BICUBIC))


# ---------------------------------------------------------------- host definition
@pytest.mark.parametrize("H,W,h,w", PAIRS)
def test_resize_u8_is_pillow_byte_for_byte(H, W, h, w):
    a = _random((H, W, 3))
    got = U.resize_u8(a, h, w)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, _pillow(a, h, w))


@pytest.mark.parametrize("h,w", [(27, 33), (90, 70), (10, 13)])
def test_resize_u8_is_pillow_on_extreme_images(h, w):
    """All 0 and all 255 stay what they are; on the 0 / 255 checkerboard the cubic's overshoot runs into both clamps when
    upsampling (the sums leave [0, 255] on both sides before the clamp)."""
    for name, a in _extremes(40, 52).items():
        got = U.resize_u8(a, h, w)
        assert np.array_equal(got, _pillow(a, h, w)), name
        if name != "board":
            assert np.array_equal(got, np.full((h, w, 3), a[0, 0, 0], np.uint8)), name
    up = U.resize_u8(_extremes(40, 52)["board"], 90, 70)
    assert up.min() == 0 and up.max() == 255


def test_resize_coeffs_properties():
    for n_in, n_out in ((64, 40), (127, 100), (64, 16), (17, 17), (24, 96), (203, 128), (5, 3), (7, 2), (1, 1), (1, 9), (4, 1)):
        bounds, coeffs = U.resize_coeffs(n_in, n_out)
        fs = max(n_in / n_out, 1.0)
        ksize = 2 * math.ceil(2.0 * fs) + 1
        assert bounds.dtype == np.int32 and bounds.shape == (n_out, 2)
        assert coeffs.dtype == np.int32 and coeffs.shape == (n_out, ksize) and ksize <= U.RESIZE_MAX_TAPS
        lo, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
        assert (lo >= 0).all() and (n >= 1).all() and (n <= ksize).all() and (lo + n <= n_in).all()
        assert (np.diff(lo) >= 0).all() and (np.diff(lo + n) >= 0).all()   # the kernel's tile window relies on this
        assert (np.abs(coeffs.astype(np.int64).sum(axis=1) - (1 << 22)) <= ksize).all()
        for i in range(n_out):
            assert not coeffs[i, n[i]:].any()


def test_resize_refusals():
    a = _random((16, 20, 3))
    for h, w in ((3, 20), (16, 4), (0, 20), (16, 0), (-1, 5)):   # ratio above 4 (16 -> 3, 20 -> 4), size 0, negative
        with pytest.raises(ValueError):
            U.resize_u8(a, h, w)
    assert U.resize_u8(a, 4, 5).shape == (4, 5, 3)   # exactly 4 is in range
    with pytest.raises(ValueError):
        U.resize_coeffs(17, 4)
    with pytest.raises(ValueError):
        U.resize_coeffs(0, 4)
    with pytest.raises(ValueError):
        U.resize_coeffs(4, 0)
    with pytest.raises(TypeError):
        U.resize_u8(a.astype(np.float32), 8, 8)
    with pytest.raises(TypeError):
        U.resize_u8(a.tolist(), 8, 8)
    with pytest.raises(ValueError):
        U.resize_u8(a[..., 0], 8, 8)                                     # rank 2
    with pytest.raises(ValueError):
        U.resize_u8(np.ascontiguousarray(a.transpose(2, 0, 1)), 8, 8)    # CHW
    with pytest.raises(ValueError):
        U.resize_u8(np.zeros((0, 5, 3), np.uint8), 8, 8)


def test_resize_source_is_built_and_its_entry_point_refuses_bad_arguments():
    from larvanet_amd import hip_lib
    from larvanet_amd.build import SOURCES
    assert "larva_resize.hip" in SOURCES
    if not os.path.exists(hip_lib.LIB_PATH):
        from larvanet_amd.build import build_extension
        build_extension(verbose=False)
    lib = hip_lib.load()
    # refused before any launch, so this runs without a device: NULL pointers, a ratio above 4, a table's ksize that is
    # not the one of its axis (a non-NULL pointer that is never read)
    table = (hip_lib.ctypes.c_int * 4)()
    p = hip_lib.ctypes.addressof(table)
    assert lib.larva_resize_u8(None, None, 1, 4, 4, 4, 4, None, None, 0, None, None, 0, None) != 0
    assert lib.larva_resize_u8(p, p, 1, 17, 4, 4, 4, None, None, 0, p, p, 17, None) != 0
    assert lib.larva_resize_u8(p, p, 1, 8, 4, 4, 4, None, None, 0, p, p, 7, None) != 0     # ksize of 8 -> 4 is 9
    assert lib.larva_resize_u8(p, p, 1, 8, 4, 4, 4, None, None, 0, None, None, 0, None) != 0  # a changed axis needs a table
    assert lib.larva_resize_u8(p, p, 0, 4, 4, 4, 4, None, None, 0, None, None, 0, None) != 0


def test_kernel_wrapper_checks_its_arguments_before_device_work():
    from larvanet_amd import kernels as K
    x = torch.zeros((1, 16, 20, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        K.resize_u8(x.numpy(), 8, 8)
    with pytest.raises(TypeError):
        K.resize_u8(x.float(), 8, 8)
    with pytest.raises(ValueError):
        K.resize_u8(x[..., 0], 8, 8)
    with pytest.raises(ValueError):
        K.resize_u8(x, 3, 20)       # 16 -> 3
    with pytest.raises(ValueError):
        K.resize_u8(x, 0, 20)
    with pytest.raises(RuntimeError):
        K.resize_u8(x, 8, 8)        # a CPU tensor: there is no CPU path


# ---------------------------------------------------------------- the kernel (GPU)
def _tile_cases():
    from larvanet_amd import kernels as K
    th, tw = K.RESIZE_TILE_ROWS, K.RESIZE_TILE_COLS
    return [(3, 4, 1, 1), (20, 40, th - 1, tw - 1), (20, 40, th, tw), (20, 40, th + 1, tw + 1),
            (30, 50, 2 * th + 5, 2 * tw + 6),          # a last partial tile in both axes
            (3, 90, 1, 2 * tw + 1), (70, 3, 2 * th + 1, 1)]


KERNEL_CASES = PAIRS + [(7, 5, 28, 20),                          # x4 up
                        (21, 37, 21, 37), (40, 52, 60, 52),      # a copy; the other axis unchanged, upsampled
                        (136, 263, 34, 66),                      # x4 down over several tiles: the largest source window
                        (67, 129, 17, 33)]                       # just inside the ratio, windows at their widest


@pytest.mark.gpu
def test_resize_kernel_is_the_numpy_definition(hip_device):
    from larvanet_amd import kernels as K
    for H, W, h, w in KERNEL_CASES + _tile_cases():
        a = _random((H, W, 3), seed=H * 1000 + W)
        want = U.resize_u8(a, h, w)
        got = K.resize_u8(torch.from_numpy(a).to(hip_device), h, w)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), (H, W, h, w)
        got4 = K.resize_u8(torch.from_numpy(a[None]).to(hip_device), h, w)
        assert tuple(got4.shape) == (1, h, w, 3) and np.array_equal(got4.cpu().numpy()[0], want), (H, W, h, w)


@pytest.mark.gpu
def test_resize_kernel_batch_slots_extremes_out_reuse_and_repeatability(hip_device):
    from larvanet_amd import kernels as K
    # N = 2 (and 3: the last image ends the allocation), a different image per slot
    batch = _random((3, 37, 53, 3), seed=7)
    for h, w in ((50, 70), (19, 23), (37, 30)):
        got = K.resize_u8(torch.from_numpy(batch).to(hip_device), h, w).cpu().numpy()
        for n in range(3):
            assert np.array_equal(got[n], U.resize_u8(batch[n], h, w)), (h, w, n)
    two = K.resize_u8(torch.from_numpy(batch[:2]).to(hip_device), 50, 70).cpu().numpy()
    assert np.array_equal(two[0], U.resize_u8(batch[0], 50, 70)) and np.array_equal(two[1], U.resize_u8(batch[1], 50, 70))
    # the extreme images, down and up
    for name, a in _extremes(40, 52).items():
        for h, w in ((27, 33), (90, 70)):
            got = K.resize_u8(torch.from_numpy(a).to(hip_device), h, w).cpu().numpy()
            assert np.array_equal(got, U.resize_u8(a, h, w)), (name, h, w)
    # out= is filled and returned, and nothing around it is touched
    a = _random((48, 64, 3), seed=3)
    x = torch.from_numpy(a).to(hip_device)
    flat = torch.full((27 * 40 * 3 + 64,), 0xA5, dtype=torch.uint8, device=hip_device)
    out = flat[32:32 + 27 * 40 * 3].view(27, 40, 3)
    ret = K.resize_u8(x, 27, 40, out=out)
    assert ret is out and np.array_equal(out.cpu().numpy(), U.resize_u8(a, 27, 40))
    assert (flat[:32] == 0xA5).all() and (flat[-32:] == 0xA5).all()
    first = out.cpu().numpy().copy()
    K.resize_u8(x, 27, 40, out=out)
    assert np.array_equal(out.cpu().numpy(), first)                      # two runs, identical bytes
    assert np.array_equal(K.resize_u8(x, 27, 40).cpu().numpy(), first)
    # refusals on the device
    with pytest.raises(RuntimeError):
        K.resize_u8(x[:, ::2], 27, 40)                                   # not contiguous
    with pytest.raises(RuntimeError):
        K.resize_u8(x, 27, 40, out=torch.empty((27, 41, 3), dtype=torch.uint8, device=hip_device))
    with pytest.raises(ValueError):
        K.resize_u8(x, 11, 40)                                           # 48 -> 11
