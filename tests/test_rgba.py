"""Transparency, the definition and the two launches: image_utils.alpha_slots / rgba_split_f32 / rgba_merge_u8 (numpy) and
kernels.rgba_u8_split_f32 / rgb_u8_merge_rgba (csrc/larva_rgba.hip).  Host logic runs anywhere; the kernels are marked gpu
and every comparison is exact (np.array_equal) against the numpy definition."""
import os

import numpy as np
import pytest
import torch

import placement as P
from larvanet_amd import image_utils as U


# ---------------------------------------------------------------- host: the definition
def test_alpha_slots_hands_out_slots_in_image_order():
    table, k = U.alpha_slots([False, True, False, False, True])
    assert table.dtype == np.int32 and table.tolist() == [5, -1, 6, 7, -1] and k == 3
    table, k = U.alpha_slots([True, True])
    assert table.tolist() == [-1, -1] and k == 0
    table, k = U.alpha_slots([np.bool_(False)])
    assert table.tolist() == [1] and k == 1
    table, k = U.alpha_slots([])
    assert table.shape == (0,) and k == 0


def test_merge_rounding_is_the_nearest_integer_to_the_mean_for_every_sum():
    """(r + g + b + 1) // 3 against float64 round over all sums 0..765 (a third has no ties, so every rounding rule
    agrees), through rgba_merge_u8 itself."""
    sums = np.arange(766)
    r = np.minimum(sums, 255)
    g = np.minimum(sums - r, 255)
    b = sums - r - g
    assert b.max() == 255 and np.array_equal(r + g + b, sums)
    grey = np.stack([r, g, b], axis=-1).astype(np.uint8).reshape(1, 1, 766, 3)
    batch = np.concatenate([np.zeros_like(grey), grey])
    got = U.rgba_merge_u8(batch, [1], 1)[0, 0, :, 3]
    want = np.round(sums.astype(np.float64) / 3.0)
    assert not np.any(np.abs(sums / 3.0 - np.floor(sums / 3.0) - 0.5) < 1e-9)   # no ties
    assert np.array_equal(got.astype(np.float64), want)


def _rgba(seed, n, h, w, opaque=()):
    img = np.random.default_rng(seed).integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    for i in opaque:
        img[i, :, :, 3] = 255
    return img


def _as_u8_hwc(planes):
    return np.ascontiguousarray(planes.transpose(0, 2, 3, 1)).astype(np.uint8)


def test_split_then_merge_round_trip():
    img = _rgba(0, 3, 5, 7, opaque=(1,))
    table, k = U.alpha_slots([False, True, False])
    planes = U.rgba_split_f32(img, table)
    assert planes.dtype == np.float32 and planes.shape == (5, 3, 5, 7)
    assert np.array_equal(planes[:3], img[..., :3].transpose(0, 3, 1, 2).astype(np.float32))
    for c in range(3):
        assert np.array_equal(planes[3, c], img[0, :, :, 3]) and np.array_equal(planes[4, c], img[2, :, :, 3])
    back = U.rgba_merge_u8(_as_u8_hwc(planes), table, 3)
    assert back.dtype == np.uint8 and np.array_equal(back, img)
    # an image marked opaque gets alpha 255 whatever its alpha bytes were
    noisy = _rgba(1, 2, 4, 4)
    table, k = U.alpha_slots([True, False])
    back = U.rgba_merge_u8(_as_u8_hwc(U.rgba_split_f32(noisy, table)), table, 2)
    assert np.all(back[0, :, :, 3] == 255) and np.array_equal(back[0, :, :, :3], noisy[0, :, :, :3])
    assert np.array_equal(back[1], noisy[1])


def test_reference_functions_refuse_bad_arguments():
    img = _rgba(2, 2, 3, 3)
    for bad in ([2], [2, 2], [3, 2, -1], [1, 2], [-2, 2], [2, 4]):
        with pytest.raises(ValueError):
            U.rgba_split_f32(img, bad)
    with pytest.raises(ValueError):
        U.rgba_split_f32(img[..., :3], [-1, -1])
    with pytest.raises(ValueError):
        U.rgba_split_f32(img.astype(np.float32), [-1, -1])
    with pytest.raises(ValueError):
        U.rgba_merge_u8(np.zeros((3, 2, 2, 3), np.uint8), [2, 3], 2)   # K = 2 needs four slots
    with pytest.raises(ValueError):
        U.rgba_merge_u8(np.zeros((3, 2, 2, 4), np.uint8), [2, -1], 2)


def test_rgba_source_is_built_and_its_entry_points_refuse_bad_arguments():
    from larvanet_amd import hip_lib
    from larvanet_amd.build import SOURCES
    if not os.path.exists(hip_lib.LIB_PATH):
        from larvanet_amd.build import build_extension
        build_extension(verbose=False)
    lib = hip_lib.load()
    assert "larva_rgba.hip" in SOURCES
    # refused before any launch, so this runs without a device: NULL pointers, bad shapes
    assert lib.larva_rgba_u8_split_f32(None, None, None, 1, 0, 1, 1, None) != 0
    assert lib.larva_rgb_u8_merge_rgba(None, None, None, 1, 0, 1, 1, None) != 0
    for n, k, h, w in ((0, 0, 1, 1), (1, 2, 1, 1), (1, -1, 1, 1), (1, 0, 0, 1), (1, 0, 1, 0)):
        assert lib.larva_rgba_u8_split_f32(16, 16, 16, n, k, h, w, None) != 0
        assert lib.larva_rgb_u8_merge_rgba(16, 16, 16, n, k, h, w, None) != 0


# ---------------------------------------------------------------- kernels (GPU)
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 4, 8), (3, 37, 127), (1, 339, 510)]


def _flag_sets(n):
    """Opacity flags per batch size: mixed (N = 3: the middle image opaque), every image translucent, every image opaque
    (K = 0)."""
    sets = [[False] * n, [True] * n]
    if n == 3:
        sets.insert(0, [False, True, False])
    if n == 2:
        sets.insert(0, [True, False])
    return sets


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_split_kernel_is_the_numpy_spec_at_both_placements(hip_device, N, H, W):
    """H W odd or even, W % 4 != 0, several images; the input and the output at 16-byte boundaries and 4 bytes past one
    (the one-pixel-per-lane form): identical bytes, nothing outside the output written, the input untouched."""
    from larvanet_amd import kernels as K
    img = _rgba(100 * N + H, N, H, W)
    for flags in _flag_sets(N):
        table, k = U.alpha_slots(flags)
        want = U.rgba_split_f32(img, table)
        slot = torch.from_numpy(table).to(hip_device)
        got = K.rgba_u8_split_f32(torch.from_numpy(img).to(hip_device), slot, k).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (N + k, 3, H, W) and np.array_equal(got, want), flags
        for off_in, off_out in ((0, 0), (4, 0), (0, 4), (4, 4)):
            x, check_x = P.placed(img, torch.uint8, hip_device, off_in)
            out, check_out = P.placed((N + k, 3, H, W), torch.float32, hip_device, off_out)
            assert K.rgba_u8_split_f32(x, slot, k, out=out) is out
            assert np.array_equal(out.cpu().numpy(), want), (flags, off_in, off_out)
            check_out()
            check_x()
            assert np.array_equal(x.cpu().numpy(), img)
    # a byte-aligned image (1 past a boundary) takes the byte form
    x, _ = P.placed(img, torch.uint8, hip_device, 1)
    table, k = U.alpha_slots([False] * N)
    got = K.rgba_u8_split_f32(x, torch.from_numpy(table).to(hip_device), k).cpu().numpy()
    assert np.array_equal(got, U.rgba_split_f32(img, table))


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", SHAPES)
def test_merge_kernel_is_the_numpy_spec_at_both_placements(hip_device, N, H, W):
    from larvanet_amd import kernels as K
    for flags in _flag_sets(N):
        table, k = U.alpha_slots(flags)
        rgb = np.random.default_rng(7 * N + W + k).integers(0, 256, (N + k, H, W, 3), dtype=np.uint8)
        want = U.rgba_merge_u8(rgb, table, N)
        slot = torch.from_numpy(table).to(hip_device)
        got = K.rgb_u8_merge_rgba(torch.from_numpy(rgb).to(hip_device), slot, N).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == (N, H, W, 4) and np.array_equal(got, want), flags
        for off_in, off_out in ((0, 0), (4, 0), (0, 4), (4, 4), (1, 0), (0, 1)):
            x, check_x = P.placed(rgb, torch.uint8, hip_device, off_in)
            out, check_out = P.placed((N, H, W, 4), torch.uint8, hip_device, off_out)
            assert K.rgb_u8_merge_rgba(x, slot, N, out=out) is out
            assert np.array_equal(out.cpu().numpy(), want), (flags, off_in, off_out)
            check_out()
            check_x()


@pytest.mark.gpu
def test_a_table_entry_outside_the_slots_means_opaque(hip_device):
    """The device table is never read on the host, so the kernels themselves keep every entry inside the tensors: an
    entry outside [N, N + K) is an opaque image."""
    from larvanet_amd import kernels as K
    img = _rgba(3, 2, 6, 6)
    rgb = np.random.default_rng(4).integers(0, 256, (3, 6, 6, 3), dtype=np.uint8)
    for bad in ([2, 99], [2, 0], [2, -7]):
        slot = torch.tensor(bad, dtype=torch.int32, device=hip_device)
        out, check = P.placed((3, 3, 6, 6), torch.float32, hip_device, 0)
        K.rgba_u8_split_f32(torch.from_numpy(img).to(hip_device), slot, 1, out=out)
        check()
        assert np.array_equal(out.cpu().numpy(), U.rgba_split_f32(img, [2, -1]))
        got = K.rgb_u8_merge_rgba(torch.from_numpy(rgb).to(hip_device), slot, 2).cpu().numpy()
        assert np.array_equal(got, U.rgba_merge_u8(rgb, [2, -1], 2))


@pytest.mark.gpu
def test_kernel_wrappers_refuse_bad_operands(hip_device):
    from larvanet_amd import kernels as K
    x = torch.zeros((2, 4, 4, 4), dtype=torch.uint8, device=hip_device)
    slot, k = K.alpha_slot_table([False, True], hip_device)
    assert k == 1 and slot.cpu().tolist() == [2, -1] and K.alpha_slot_table([False, True], hip_device)[0] is slot
    with pytest.raises(RuntimeError):
        K.rgba_u8_split_f32(x.cpu(), slot, k)
    with pytest.raises(RuntimeError):
        K.rgba_u8_split_f32(x[..., :3].contiguous(), slot, k)
    with pytest.raises(RuntimeError):
        K.rgba_u8_split_f32(x, slot.cpu(), k)
    with pytest.raises(RuntimeError):
        K.rgba_u8_split_f32(x, slot.long(), k)
    with pytest.raises(RuntimeError):
        K.rgba_u8_split_f32(x, slot[:1], k)
    with pytest.raises(RuntimeError):
        K.rgba_u8_split_f32(x, slot, 3)
    with pytest.raises(RuntimeError):
        K.rgba_u8_split_f32(x, slot, k, out=torch.zeros((2, 3, 4, 4), device=hip_device))
    rgb = torch.zeros((3, 4, 4, 3), dtype=torch.uint8, device=hip_device)
    with pytest.raises(RuntimeError):
        K.rgb_u8_merge_rgba(rgb, slot, 1)            # 3 slots are more than N + N
    with pytest.raises(RuntimeError):
        K.rgb_u8_merge_rgba(rgb.float(), slot, 2)
    with pytest.raises(RuntimeError):
        K.rgb_u8_merge_rgba(rgb, slot, 2, out=torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=hip_device))
