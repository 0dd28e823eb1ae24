"""Bicubic decimation of uint8 images (kernels.bicubic_down_u8 / bicubic_down_u8_table, csrc/larva_downscale.hip) and
its host restatement image_utils.bicubic_downscale_u8: the definition against two independent restatements
(tests/downscale_ref.py) anywhere, the device against the host byte for byte on the GPU."""
import numpy as np
import pytest
import torch

import downscale_ref as R

SCALES = (2, 3, 4)
TILE_ROWS, TILE_COLS = 8, 32   # the kernel's tile in output pixels of an RGB image


def _random(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _blocks(h, w, width):
    """Isolated 255 squares of `width` pixels on 0 in the left half, 0 squares on 255 in the right half (period 5
    width + 1, so the squares meet the output grid at every phase): the cubic's negative lobes undershoot 0 around the
    former and overshoot 255 around the latter."""
    yy, xx = np.mgrid[0:h, 0:w]
    period = 5 * width + 1
    square = ((yy % period) < width) & ((xx % period) < width)
    plane = np.where(xx < w // 2, square, ~square) * 255
    return np.stack([plane, np.roll(plane, 1, axis=0), plane.copy()], axis=2).astype(np.uint8)


# ---------------------------------------------------------------- anywhere
@pytest.mark.parametrize("s", SCALES)
def test_the_products_table_is_the_exact_derivation(s):
    from larvanet_amd import image_utils as U
    assert U.BICUBIC_DOWN_TAPS[s] == R.derive_taps(s)
    D, first, taps = U.BICUBIC_DOWN_TAPS[s]
    assert sum(taps) == D and taps == taps[::-1] and first + (len(taps) - 1) / 2.0 == (s - 1) / 2.0


@pytest.mark.parametrize("s", SCALES)
def test_the_general_contribution_algorithm_gives_the_tables_taps_for_every_output(s):
    from larvanet_amd import image_utils as U
    D, first, taps = U.BICUBIC_DOWN_TAPS[s]
    want = {first + k: t / float(D) for k, t in enumerate(taps) if t}
    weights, indices = R.contributions(7 * s, s)
    assert weights.shape == (7, 4 * s + 2)
    for i in range(7):
        got = {int(j) - s * i: w for j, w in zip(indices[i], weights[i]) if w != 0.0}
        assert sorted(got) == sorted(want), (s, i)
        for o in want:
            # x2, x4: every operand is dyadic with a few bits, float64 is exact.  x3: about six roundings of
            # intermediates below 8 (2^-53 * 8 each), divided by 3, and one more for the normalisation: below 4e-15
            assert abs(got[o] - want[o]) <= (0.0 if s != 3 else 4e-15), (s, i, o, got[o], want[o])


@pytest.mark.parametrize("s", SCALES)
def test_the_host_restatement_equals_both_references_on_every_byte(s):
    from larvanet_amd import image_utils as U
    for seed, (h, w) in enumerate([(13 * s + 1, 17 * s + 2), (s, s), (s, 2 * s), (2 * s + 1, s)]):
        x = _random(100 * s + seed, h, w)
        got = U.bicubic_downscale_u8(x, s)
        assert got.dtype == np.uint8 and got.shape == (h // s, w // s, 3)
        assert np.array_equal(got, R.downscale_exact(x, s)), (s, h, w)
        f = R.downscale_f64(x, s)
        if s == 3:   # D^2 = 6561 is odd: no tie exists, the nearest miss is 1 / 13122 against a float64 error near 1e-13
            assert np.abs(f - np.floor(f) - 0.5).min() > 7e-5
        # (x2, x4: the float64 form is exact, so a tie is a tie in both and rounds to even in both)
        assert np.array_equal(got, np.clip(np.round(f), 0, 255).astype(np.uint8)), (s, h, w)
    for width in (s, s + 1):   # hard edges: the overshoot is clipped on both sides
        x = _blocks(6 * s + 1, 9 * s, width)
        raw = R.downscale_exact(x, s, clip=False)
        assert raw.min() < 0 and raw.max() > 255
        assert np.array_equal(U.bicubic_downscale_u8(x, s), np.clip(raw, 0, 255))


@pytest.mark.parametrize("s", SCALES)
def test_a_constant_image_stays_constant(s):
    from larvanet_amd import image_utils as U
    for v in (0, 1, 127, 200, 255):
        x = np.full((3 * s + 1, 5 * s + 1, 3), v, np.uint8)
        assert np.array_equal(U.bicubic_downscale_u8(x, s), np.full((3, 5, 3), v, np.uint8))


def test_refusals_on_the_host_and_before_any_launch():
    from larvanet_amd import image_utils as U, kernels as K
    good = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="scale 2, 3 or 4"):
        U.bicubic_downscale_u8(good, 5)
    with pytest.raises(ValueError, match="smaller than one pixel"):
        U.bicubic_downscale_u8(np.zeros((3, 20, 3), np.uint8), 4)
    with pytest.raises(TypeError):
        U.bicubic_downscale_u8(good.astype(np.float32), 2)
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        U.bicubic_downscale_u8(np.zeros((3, 8, 8), np.uint8), 2)
    # the device wrapper: dtype, shape, scale and size are refused before the device is asked for
    t = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="scale 2, 3 or 4"):
        K.bicubic_down_u8(t, 5)
    with pytest.raises(ValueError, match="smaller than one pixel"):
        K.bicubic_down_u8(torch.zeros((3, 20, 3), dtype=torch.uint8), 4)
    with pytest.raises(TypeError):
        K.bicubic_down_u8(t.float(), 2)
    with pytest.raises(TypeError):
        K.bicubic_down_u8(good, 2)
    with pytest.raises(ValueError, match=r"\[H\]\[W\]\[3\]"):
        K.bicubic_down_u8(torch.zeros((3, 8, 8), dtype=torch.uint8), 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        K.bicubic_down_u8(t, 2)
    with pytest.raises(TypeError):
        K.bicubic_down_u8_table(t.flatten().float(), torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 2,
                                t.flatten(), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device"):
        K.bicubic_down_u8_table(t.flatten(), torch.zeros(1, dtype=torch.int64), torch.tensor([8, 8], dtype=torch.int32), 2,
                                t.flatten(), torch.zeros(1, dtype=torch.int64))
    off, hw, nbytes = K.bicubic_down_table_layout([(8, 12), (9, 7)], 2)
    assert off.tolist() == [0, 72] and hw.tolist() == [4, 6, 4, 3] and nbytes == 72 + 36
    with pytest.raises(ValueError):
        K.bicubic_down_table_layout([(8, 12), (1, 7)], 2)


def test_driver_parsers_and_names():
    from larvanet_amd import downscale_images as D, evaluate as E
    a = D.build_parser().parse_args([])
    assert (a.input_path, a.output_path, a.scale, a.suffix, a.io_threads) == ("HR", "LR", 4, False, None)
    a = D.build_parser().parse_args(["--input_path=hr", "--output_path=lr", "--scale=3", "--suffix", "--io_threads=2"])
    assert (a.input_path, a.output_path, a.scale, a.suffix, a.io_threads) == ("hr", "lr", 3, True, 2)
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(["--scale=5"])
    assert D.output_name("0801.png", 4, True) == "0801x4.png" and D.output_name("baby.PNG", 2, False) == "baby.png"
    assert E.pair_files(["0801.png"], [D.output_name("0801.png", 3, True)], 3) == [("0801.png", "0801x3.png")]
    args, rest = E.build_parser().parse_known_args([])
    assert args.lr_from_truth is False and args.input_path == "LR"
    args, rest = E.build_parser().parse_known_args(["--lr_from_truth", "--truth_path=hr", "--num_modules=1"])
    assert args.lr_from_truth is True and args.truth_path == "hr" and rest == ["--num_modules=1"]


def test_loader_flag_and_the_truth_only_host_tables(tmp_path):
    from PIL import Image
    from larvanet_amd.dataloaders import device_patch_loader as D, div2k_train_loader
    ld = D.create_loader()
    merged, rest = ld.parse_args(["--device_source=synthetic_loader", "--synthetic_images=3", "--synthetic_lr_size=10",
                                  "--other=1"])
    assert merged.lr_from_hr is False and rest == ["--other=1"]
    merged, rest = ld.parse_args(["--device_source=synthetic_loader", "--synthetic_images=3", "--synthetic_lr_size=10",
                                  "--lr_from_hr"])
    assert merged.lr_from_hr is True and ld.args.lr_from_hr is True and rest == []
    ld.source.prepare([2, 3])
    tables, shapes = D.build_host_tables(ld.source, [2, 3], lr_from_hr=True)
    assert sorted(tables[2]) == ["hr", "hr_hw", "hr_off"] and shapes == [(10, 10), (10, 18), (10, 26)]
    for s in (2, 3):
        hw = tables[s]["hr_hw"].reshape(-1, 2)
        for i in range(3):
            hr = np.clip(np.round(ld.source.get_image_pair(i, s)[1]), 0, 255).astype(np.uint8)
            assert tuple(hw[i]) == hr.shape[1:]
            assert np.array_equal(tables[s]["hr"][tables[s]["hr_off"][i]:][:hr.size].reshape(hr.shape), hr)
    # a DIV2K folder with HR images alone: sizes that are no multiple of the scale are cropped top-left
    hr_dir = tmp_path / "hr"
    hr_dir.mkdir()
    images = {"b": _random(1, 23, 31), "a": _random(2, 20, 26)}
    for name, a in images.items():
        Image.fromarray(a).save(str(hr_dir / (name + ".png")))
    src = div2k_train_loader.create_loader()
    src.parse_args(["--data_truth_path", str(hr_dir), "--data_input_path", str(tmp_path / "absent")])
    src.prepare([3])
    hr, name = src.get_truth_image(0, 3)
    assert name == "a" and np.array_equal(hr, images["a"].transpose(2, 0, 1))
    tables, shapes = D.build_host_tables(src, [3], lr_from_hr=True)
    assert shapes == [(6, 8), (7, 10)] and tables[3]["hr_hw"].tolist() == [18, 24, 21, 30]
    assert np.array_equal(tables[3]["hr"][3 * 18 * 24:].reshape(3, 21, 30), images["b"].transpose(2, 0, 1)[:, :21, :30])


# ---------------------------------------------------------------- on the device
def _shapes(s):
    """Input sizes: one output pixel (the reflection wraps more than once), s x 2 s, a size that is cropped, and 1, T,
    T + 1 and 2 T + 1 output pixels along each axis of the kernel's tile T."""
    out = [(s, s), (s, 2 * s), (5 * s + s - 1, 7 * s + 1)]
    for h, w in [(TILE_ROWS, TILE_COLS), (TILE_ROWS + 1, TILE_COLS + 1), (2 * TILE_ROWS + 1, 2 * TILE_COLS + 1),
                 (1, 2 * TILE_COLS + 1), (2 * TILE_ROWS + 1, 1), (TILE_ROWS, 3 * TILE_COLS + 5)]:
        out.append((h * s, w * s + (s - 1 if h == TILE_ROWS else 0)))
    return out


def _device(x, s, hip_device, **kw):
    from larvanet_amd import kernels as K
    return K.bicubic_down_u8(torch.from_numpy(x).to(hip_device), s, **kw).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCALES)
def test_device_equals_host_on_every_shape(hip_device, s):
    from larvanet_amd import image_utils as U
    for k, (h, w) in enumerate(_shapes(s)):
        x = _random(1000 * s + k, h, w)
        got = _device(x, s, hip_device)
        assert got.dtype == np.uint8 and np.array_equal(got, U.bicubic_downscale_u8(x, s)), (s, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCALES)
def test_device_equals_host_on_hard_edges_and_flat_images(hip_device, s):
    from larvanet_amd import image_utils as U
    h, w = (2 * TILE_ROWS + 1) * s, (3 * TILE_COLS + 1) * s
    for width in (s, s + 1):
        x = _blocks(h, w, width)
        raw = R.downscale_f64(x, s)
        assert raw.min() < -0.5 and raw.max() > 255.5   # the clip is exercised on both sides
        want = U.bicubic_downscale_u8(x, s)
        assert want.min() == 0 and want.max() == 255
        assert np.array_equal(_device(x, s, hip_device), want), (s, width)
    for v in (0, 255):
        x = np.full((h, w, 3), v, np.uint8)
        assert np.array_equal(_device(x, s, hip_device), np.full((h // s, w // s, 3), v, np.uint8)), (s, v)


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCALES)
def test_a_window_at_an_odd_byte_offset_with_an_odd_pitch(hip_device, s):
    """Three tiles wide, so the middle tile takes the aligned-dword staging; the pitch is odd, so the rows' first bytes
    have all four alignments."""
    from larvanet_amd import image_utils as U, kernels as K
    H, W = (TILE_ROWS + 3) * s + 1, (2 * TILE_COLS + 3) * s
    W += 1 - W % 2
    big = _random(77 + s, H + 3, W + 4)
    assert W % 2 == 1 and (3 * big.shape[1]) % 2 == 1
    dev = torch.from_numpy(big).to(hip_device)
    for y0, x0 in ((1, 1), (2, 3), (0, 0)):
        window = dev[y0:y0 + H, x0:x0 + W]
        assert not window.is_contiguous()
        out = torch.empty((H // s, W // s, 3), dtype=torch.uint8, device=hip_device)
        assert K.bicubic_down_u8(window, s, out=out) is out
        assert np.array_equal(out.cpu().numpy(), U.bicubic_downscale_u8(np.ascontiguousarray(big[y0:y0 + H, x0:x0 + W]), s))
    with pytest.raises(RuntimeError, match="contiguous pixels"):
        K.bicubic_down_u8(dev[:, ::2], s)
    with pytest.raises(RuntimeError, match=r"out must be"):
        K.bicubic_down_u8(dev, s, out=torch.empty((1, 1, 3), dtype=torch.uint8, device=hip_device))


@pytest.mark.gpu
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("planar", [False, True])
def test_the_table_launch_equals_the_single_launches_and_leaves_the_gaps_alone(hip_device, s, planar):
    from larvanet_amd import image_utils as U, kernels as K
    # (the last one is three tiles wide in both forms -- a plane's tile is 96 pixels wide -- so a middle tile exists)
    shapes = [(9 * s, (TILE_COLS + 3) * s), (s, s), ((TILE_ROWS + 2) * s, (6 * TILE_COLS + 9) * s + 1)]
    images = [_random(500 + 10 * s + i, h, w) for i, (h, w) in enumerate(shapes)]
    stored = [a.transpose(2, 0, 1) if planar else a for a in images]
    gap = 5   # bytes between the images of both tables: odd offsets, and bytes that must stay as they are
    src_off = np.cumsum([gap] + [a.size + gap for a in stored])[:-1].astype(np.int64)
    src = np.full(int(src_off[-1]) + stored[-1].size + gap, 0xEE, np.uint8)
    for o, a in zip(src_off, stored):
        src[o:o + a.size] = a.ravel()
    wants = [U.bicubic_downscale_u8(a, s) for a in images]
    dst_off = np.cumsum([gap] + [a.size + gap for a in wants])[:-1].astype(np.int64)
    total = int(dst_off[-1]) + wants[-1].size + gap
    want_table = np.full(total, 0xAB, np.uint8)
    for o, a in zip(dst_off, wants):
        want_table[o:o + a.size] = (a.transpose(2, 0, 1) if planar else a).ravel()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    out = torch.full((total,), 0xAB, dtype=torch.uint8, device=hip_device)
    hw = np.asarray([d for h, w in shapes for d in (h, w)], np.int32)
    got = K.bicubic_down_u8_table(dev(src), dev(src_off), dev(hw), s, out, dev(dst_off), planar=planar)
    assert got is out and np.array_equal(out.cpu().numpy(), want_table)
    if not planar:
        for a, want in zip(images, wants):
            assert np.array_equal(_device(a, s, hip_device), want)
    with pytest.raises(ValueError, match="outside the destination"):
        K.bicubic_down_u8_table(dev(src), dev(src_off), dev(hw), s, out[:total - gap - 1], dev(dst_off), planar=planar)
    with pytest.raises(ValueError, match="overlap"):
        K.bicubic_down_u8_table(dev(src), dev(src_off), dev(hw), s, out, dev(np.zeros(3, np.int64)), planar=planar)


@pytest.mark.gpu
def test_two_launches_give_identical_bytes(hip_device):
    from larvanet_amd import kernels as K
    for s in SCALES:
        x = torch.from_numpy(_random(9 + s, 37 * s + 1, 101 * s + 2)).to(hip_device)
        a, b = K.bicubic_down_u8(x, s), K.bicubic_down_u8(x, s)
        assert torch.equal(a, b)
