"""Chop-forward of the reference (utils/image_utils.py:7-66): the LR image is cut into 2x2
overlapping quadrants, each is upscaled on its own and the results are stitched at the quadrant
boundaries.  This is approximate by design (overlap/2 = 10 LR px is less than the network's
receptive-field radius of 35) and is reproduced as is.

Also the definitions of the geometric self-ensemble (--self_ensemble): the eight flips / transposes of the square, and
of the bicubic decimation the low-resolution images of SR benchmarks are made with (bicubic_downscale_u8)."""
import numpy as np

# Bicubic decimation by an integer scale: scale -> (D, first offset, integer numerators).  Output i of an axis takes
# input s i + first offset + k with weight numerators[k] / D = c((u - j) / s) / s at u = (i + 1/2) s - 1/2, c the Keys
# cubic with a = -1/2 (the weights of a pixel sum to 1).  The one table kernels.bicubic_down_u8's checks and the host
# restatement below read; csrc/larva_downscale.hip carries the same numbers (include/larva_hip.h lists them).
BICUBIC_DOWN_TAPS = {
    2: (256, -3, (-3, -9, 29, 111, 111, 29, -9, -3)),
    3: (81, -4, (-1, -2, 0, 9, 21, 27, 21, 9, 0, -2, -1)),
    4: (4096, -6, (-7, -45, -75, -49, 93, 399, 745, 987, 987, 745, 399, 93, -49, -75, -45, -7)),
}


def bicubic_down_size(height, width, scale):
    """(h, w) = (height // scale, width // scale) of the decimated image; ValueError for a scale other than 2, 3, 4 or
    an image smaller than one output pixel."""
    if scale not in BICUBIC_DOWN_TAPS:
        raise ValueError("larvanet_amd: bicubic downscaling takes scale 2, 3 or 4, got %r" % (scale,))
    h, w = int(height) // int(scale), int(width) // int(scale)
    if h < 1 or w < 1:
        raise ValueError("larvanet_amd: a %d x %d image is smaller than one pixel at x%d" % (height, width, scale))
    return h, w


def _decimate_axis0(a, scale):
    """Exact integer FIR with stride `scale` along axis 0 of the int64 array a (length a multiple of scale), indices
    reflected symmetrically: m = j mod 2 n, j' = m if m < n else 2 n - 1 - m."""
    _, first, taps = BICUBIC_DOWN_TAPS[scale]
    n = a.shape[0]
    j = scale * np.arange(n // scale)[:, None] + first + np.arange(len(taps))[None, :]
    m = np.mod(j, 2 * n)
    j = np.where(m < n, m, 2 * n - 1 - m)
    out = np.zeros((n // scale,) + a.shape[1:], np.int64)
    for k, t in enumerate(taps):
        if t:
            out += np.int64(t) * a[j[:, k]]
    return out


def bicubic_downscale_u8(image, scale):
    """uint8 (H, W, 3) -> uint8 (H // scale, W // scale, 3): antialiased bicubic decimation in the MATLAB imresize
    convention of the top-left (H // scale) scale x (W // scale) scale pixels, in exact integers with ONE rounding at the
    end: clip(round_half_even(N / D^2), 0, 255).  The host restatement kernels.bicubic_down_u8 equals byte for byte."""
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8:
        raise TypeError("larvanet_amd: bicubic_downscale_u8 takes a uint8 numpy array, got %s"
                        % (getattr(image, "dtype", type(image).__name__),))
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("larvanet_amd: bicubic_downscale_u8 takes an (H, W, 3) image, got shape %s" % (image.shape,))
    h, w = bicubic_down_size(image.shape[0], image.shape[1], scale)
    d2 = BICUBIC_DOWN_TAPS[scale][0] ** 2
    a = image[:h * scale, :w * scale].astype(np.int64)
    a = _decimate_axis0(a, scale)                                         # rows
    a = np.swapaxes(_decimate_axis0(np.swapaxes(a, 0, 1), scale), 0, 1)   # columns
    q, r = np.floor_divide(a, d2), np.mod(a, d2)                          # floor semantics: 0 <= r < D^2
    q = q + ((2 * r > d2) | ((2 * r == d2) & (q % 2 == 1)))
    return np.clip(q, 0, 255).astype(np.uint8)


def dihedral(a, t, axes=(0, 1)):
    """Transform t (0..7) of the square on the two spatial axes `axes` = (rows, columns) of `a`: reverse the rows if
    t & 1, then reverse the columns if t & 2, then swap the two axes if t & 4."""
    r, c = axes
    if t & 1:
        a = np.flip(a, r)
    if t & 2:
        a = np.flip(a, c)
    if t & 4:
        a = np.swapaxes(a, r, c)
    return a


def dihedral_inv(a, t, axes=(0, 1)):
    """The inverse of dihedral(., t): swap the axes if t & 4, then reverse the columns if t & 2, then the rows if t & 1."""
    r, c = axes
    if t & 4:
        a = np.swapaxes(a, r, c)
    if t & 2:
        a = np.flip(a, c)
    if t & 1:
        a = np.flip(a, r)
    return a


def self_ensemble(f, x, axes=(0, 1)):
    """E(x) = (((((((v0 + v1) + v2) + v3) + v4) + v5) + v6) + v7) * 0.125 in float32, v_t = dihedral_inv(f(dihedral(x, t)),
    t): the host composition the device-side ensemble (--self_ensemble) equals bit for bit.  f maps an array to an
    array with the same axes."""
    acc = None
    for t in range(8):
        v = np.asarray(dihedral_inv(f(np.ascontiguousarray(dihedral(x, t, axes))), t, axes), dtype=np.float32)
        acc = v if acc is None else acc + v
    return acc * np.float32(0.125)


def split_quadrants(image, overlap_size):
    _, h, w = image.shape
    sh, sw, ho = h // 2, w // 2, overlap_size // 2
    rows = (slice(None, sh + ho), slice(sh - ho, None))
    cols = (slice(None, sw + ho), slice(sw - ho, None))
    return [np.array(image[:, r, c]) for r in rows for c in cols]


def stitch_quadrants(parts, input_shape, scale, overlap_size):
    _, h, w = input_shape
    top, left = (h // 2) * scale, (w // 2) * scale
    skip = (overlap_size // 2) * scale
    out = np.zeros([3, h * scale, w * scale])
    out[:, :top, :left] = parts[0][:, :top, :left]
    out[:, :top, left:] = parts[1][:, :top, skip:]
    out[:, top:, :left] = parts[2][:, skip:, :left]
    out[:, top:, left:] = parts[3][:, skip:, skip:]
    return out


def upscale_with_chop_forward(model, input_image, scale, overlap_size):
    parts = [model.upscale(input_list=[q], scale=scale)[0] for q in split_quadrants(input_image, overlap_size)]
    return stitch_quadrants(parts, input_image.shape, scale, overlap_size)


def band_rows(height, world):
    """Rows [r0, r1) of each of `world` contiguous bands of an image `height` rows tall (balanced,
    empty bands when world > height)."""
    return [((height * r) // world, (height * (r + 1)) // world) for r in range(world)]


def upscale_band(model, input_image, scale, r0, r1, halo):
    """Output rows [scale*r0, scale*r1) of model.upscale(input_image), computed from the input rows
    [r0 - halo, r1 + halo) only.  EXACT (bit for bit) when `halo` >= the network's receptive halo
    (model.receptive_halo()): the cut edges see zero padding / clamped bicubic taps instead of the
    neighbouring rows, but that only reaches `halo` rows into the sub-image, and exactly those rows
    are dropped; true image borders stay borders.  SURVEY 8e row 3 (the reference itself only has
    the approximate 2x2 chop_forward, utils/image_utils.py:30-66)."""
    height = input_image.shape[1]
    if r1 <= r0:
        return np.zeros((input_image.shape[0], 0, input_image.shape[2] * scale), np.float32)
    lo, hi = max(0, r0 - halo), min(height, r1 + halo)
    out = model.upscale(input_list=[np.ascontiguousarray(input_image[:, lo:hi, :])], scale=scale)[0]
    return out[:, (r0 - lo) * scale:(r1 - lo) * scale, :]


def upscale_banded_device(model, input_image, scale, rank, world, all_gather, halo=None):
    """upscale_banded with the bands moved by a DEVICE collective: rank r upscales band r (+ halo)
    on its GPU, crops it on the GPU into a buffer of the tallest band's size, and
    `all_gather(tensor) -> [world][...]` (larvanet_amd.dist.all_gather_tensor = one RCCL all-gather)
    hands every rank all bands; the concatenation is a device tensor [C][scale*H][scale*W].  Nothing
    is pickled and no band visits the host (upscale_banded gathers numpy arrays as Python objects:
    a 33 MB DIV2K output would be pickled once per rank).  Bit-identical to the full-image forward
    for halo >= model.receptive_halo()."""
    import torch
    halo = model.receptive_halo() if halo is None else halo
    channels, height, width = input_image.shape
    rows = band_rows(height, world)
    tallest = max(b - a for a, b in rows)
    r0, r1 = rows[rank]
    buf = torch.zeros((channels, tallest * scale, width * scale), dtype=torch.float32, device=model.device)
    if r1 > r0:
        lo, hi = max(0, r0 - halo), min(height, r1 + halo)
        out = model.upscale_tensor(input_list=[np.ascontiguousarray(input_image[:, lo:hi, :])])[0]
        buf[:, :(r1 - r0) * scale] = out[:, (r0 - lo) * scale:(r1 - lo) * scale]
    bands = all_gather(buf)
    return torch.cat([bands[q, :, :(b - a) * scale] for q, (a, b) in enumerate(rows)], dim=1)


def upscale_banded(model, input_image, scale, rank, world, gather, halo=None):
    """One image split into `world` row bands, band r computed by rank r, `gather(obj)` = every
    rank's object in rank order (larvanet_amd.dist.gather_objects).  Every rank returns the whole
    output image.  Latency mode: each rank also recomputes 2 * halo rows, so 8 GPUs on a 339-row
    image do 113 rows each instead of 339, not 42."""
    halo = model.receptive_halo() if halo is None else halo
    r0, r1 = band_rows(input_image.shape[1], world)[rank]
    mine = upscale_band(model, input_image, scale, r0, r1, halo)
    return np.concatenate(gather(mine), axis=1)
