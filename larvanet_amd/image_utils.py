"""Chop-forward of the reference (utils/image_utils.py:7-66): the LR image is cut into 2x2
overlapping quadrants, each is upscaled on its own and the results are stitched at the quadrant
boundaries.  This is approximate by design (overlap/2 = 10 LR px is less than the network's
receptive-field radius of 35) and is reproduced as is.

Also the definitions of the geometric self-ensemble (--self_ensemble): the eight flips / transposes of the square, and
of the bicubic decimation the low-resolution images of SR benchmarks are made with (bicubic_downscale_u8), and of the two
conversions of the video path between planar YUV 4:2:0 frames and RGB (i420_to_rgb_f32, rgb_u8_to_i420)."""
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


# ------------------------------------------------------------------ bicubic resize to any size: Pillow's, byte for byte
# Image.resize((w, h), Image.BICUBIC) of an RGB uint8 image restated.  Per axis: scale = n_in / n_out, fs = max(scale, 1),
# support = 2 fs, ksize = 2 ceil(support) + 1.  Output i has its centre at c = (i + 1/2) scale and takes the inputs lo ..
# lo + n - 1, lo = max(int(c - support + 1/2), 0), n = min(int(c + support + 1/2), n_in) - lo, with the weights
# cubic((j + lo - c + 1/2) / fs) (Keys, a = -1/2) summed in index order in float64, divided by their sum and fixed to
# K_j = int(k_j 2^22 +- 1/2) (away from zero).  One pass is out = clamp((2^21 + sum_j in[lo + j] K_j) >> 22, 0, 255) in
# int32 with an arithmetic shift; the horizontal pass runs first and leaves BYTES, then the vertical one; an axis whose
# size does not change is skipped.  kernels.resize_u8 (csrc/larva_resize.hip) equals resize_u8 bit for bit.
RESIZE_PRECISION_BITS = 22
RESIZE_MAX_RATIO = 4     # n_in <= 4 n_out per axis (any upsampling), so that ksize <= RESIZE_MAX_TAPS
RESIZE_MAX_TAPS = 17


def check_resize(in_h, in_w, out_h, out_w):
    """-> (out_h, out_w) as ints; ValueError for a size below 1 or an axis that shrinks by more than RESIZE_MAX_RATIO."""
    in_h, in_w, out_h, out_w = int(in_h), int(in_w), int(out_h), int(out_w)
    if min(in_h, in_w, out_h, out_w) < 1:
        raise ValueError("larvanet_amd: resizing needs sizes >= 1, got %d x %d -> %d x %d (height x width)"
                         % (in_h, in_w, out_h, out_w))
    if in_h > RESIZE_MAX_RATIO * out_h or in_w > RESIZE_MAX_RATIO * out_w:
        raise ValueError("larvanet_amd: resizing shrinks an axis by at most %d, got %d x %d -> %d x %d (height x width)"
                         % (RESIZE_MAX_RATIO, in_h, in_w, out_h, out_w))
    return out_h, out_w


def parse_output_size(text):
    """'WxH' (the --output_size of the drivers, e.g. 1920x1080) -> (height, width); ValueError for anything else."""
    parts = str(text).lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts) or int(parts[0]) < 1 or int(parts[1]) < 1:
        raise ValueError("larvanet_amd: --output_size takes WIDTHxHEIGHT with both >= 1 (e.g. 1920x1080), got %r" % (text,))
    return int(parts[1]), int(parts[0])


def check_output_size(output_size, in_h, in_w):
    """The output_size argument of the image entry points against the network's (in_h, in_w) result -> None, or
    (height, width) as ints; TypeError / ValueError for anything else."""
    if output_size is None:
        return None
    if isinstance(output_size, (str, bytes)) or not hasattr(output_size, "__len__") or len(output_size) != 2:
        raise TypeError("larvanet_amd: output_size is (height, width) or None, got %r" % (output_size,))
    h, w = output_size
    if int(h) != h or int(w) != w:
        raise TypeError("larvanet_amd: output_size is (height, width) in whole pixels, got %r" % (output_size,))
    return check_resize(in_h, in_w, h, w)


# ------------------------------------------------------------------ one image / one frame of an entry point's or a stream's input
def check_u8_image(a, who, channels, also_rgba=False):
    """A decoded image handed to `who`: a uint8 (H, W, channels) numpy array of at least one pixel, else TypeError /
    ValueError.  also_rgba: (H, W, 4) passes too (upscale_stream with keep_alpha), and the refusal says so."""
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise TypeError("larvanet_amd: %s takes uint8 numpy arrays (decoded images), got %s"
                        % (who, getattr(a, "dtype", type(a).__name__),))
    if a.ndim != 3 or a.shape[2] not in ((channels, 4) if also_rgba else (channels,)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("larvanet_amd: %s takes (H, W, %d) images%s, got shape %s"
                         % (who, channels, " and, with keep_alpha, (H, W, 4) ones" if also_rgba else "", a.shape,))


def check_i420_frame(f, who, nbytes, width, height, one_size=False):
    """An I420 frame of width x height handed to `who`: a flat uint8 numpy buffer of nbytes (i420_frame_bytes), else
    TypeError / ValueError.  one_size: the caller takes frames of one size per call and says so."""
    if not isinstance(f, np.ndarray) or f.dtype != np.uint8:
        raise TypeError("larvanet_amd: %s takes uint8 numpy frames, got %s" % (who, getattr(f, "dtype", type(f).__name__),))
    if f.ndim != 1 or f.size != nbytes:
        raise ValueError("larvanet_amd: an I420 frame of %d x %d is a flat buffer of %d bytes%s, got shape %s"
                         % (width, height, nbytes, " (one size per call)" if one_size else "", f.shape,))


def _keys_cubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resize_coeffs(n_in, n_out):
    """One axis of the resize -> (bounds int32 [n_out][2] = (lo, n), coeffs int32 [n_out][ksize], zero beyond n)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("larvanet_amd: resizing needs sizes >= 1, got %d -> %d" % (n_in, n_out))
    if n_in > RESIZE_MAX_RATIO * n_out:
        raise ValueError("larvanet_amd: resizing shrinks an axis by at most %d, got %d -> %d" % (RESIZE_MAX_RATIO, n_in, n_out))
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(np.ceil(support)) + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coeffs = np.zeros((n_out, ksize), np.int32)
    inv = 1.0 / fs
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), n_in) - lo
        k = _keys_cubic((np.arange(n, dtype=np.float64) + lo - c + 0.5) * inv)
        total = 0.0
        for v in k:   # (index order: the sum Pillow divides by)
            total += float(v)
        if total != 0.0:
            k = k / total
        k = k * float(1 << RESIZE_PRECISION_BITS)
        bounds[i] = (lo, n)
        coeffs[i, :n] = np.where(k < 0, k - 0.5, k + 0.5).astype(np.int64)   # (astype truncates towards zero, as (int))
    return bounds, coeffs


def _resize_axis0(a, n_out):
    """One pass along axis 0 of the uint8 array a -> uint8."""
    bounds, coeffs = resize_coeffs(a.shape[0], n_out)
    lo = bounds[:, 0].astype(np.int64)
    acc = np.full((n_out,) + a.shape[1:], 1 << (RESIZE_PRECISION_BITS - 1), np.int32)
    tail = (1,) * (a.ndim - 1)
    for j in range(coeffs.shape[1]):   # (a tap beyond n has weight 0: its clamped index reads a pixel that counts for nothing)
        acc += a[np.minimum(lo + j, a.shape[0] - 1)].astype(np.int32) * coeffs[:, j].reshape((n_out,) + tail)
    return np.clip(acc >> RESIZE_PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_u8(image, out_h, out_w):
    """uint8 (H, W, 3) -> uint8 (out_h, out_w, 3): Pillow's Image.resize((out_w, out_h), Image.BICUBIC) byte for byte (the
    definition above).  ValueError for a size below 1 or an axis that shrinks by more than 4."""
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8:
        raise TypeError("larvanet_amd: resize_u8 takes a uint8 numpy array, got %s"
                        % (getattr(image, "dtype", type(image).__name__),))
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("larvanet_amd: resize_u8 takes an (H, W, 3) image, got shape %s" % (image.shape,))
    out_h, out_w = check_resize(image.shape[0], image.shape[1], out_h, out_w)
    a = image
    if out_w != a.shape[1]:
        a = np.swapaxes(_resize_axis0(np.swapaxes(a, 0, 1), out_w), 0, 1)
    if out_h != a.shape[0]:
        a = _resize_axis0(a, out_h)
    return np.ascontiguousarray(a)


# ------------------------------------------------------------------ transparency: straight-alpha RGBA images
# An RGBA image keeps its alpha by running it through the network too: the colour is what upscale_u8 returns for the RGB
# part, and the alpha plane, repeated into a grey image, takes the same forward; its three result channels are merged as
# (r + g + b + 1) // 3, the nearest integer to their mean (a third has no ties), in int32.  An opaque image (alpha 255
# everywhere) keeps alpha 255 and runs no alpha forward: the network does not map flat 255 to flat 255.  Alpha is straight
# (not premultiplied); the colour under transparent pixels is used as it is.  A batch of N images, K of them not opaque,
# is N + K batch slots of the RGB forward: slot n = image n's colour, slot alpha_slot[n] >= N = its alpha.  These three
# functions are the definition; kernels.rgba_u8_split_f32 / rgb_u8_merge_rgba (csrc/larva_rgba.hip) equal them bit for bit.
def alpha_slots(opaque):
    """N opacity flags -> (int32 [N] table, K): -1 for an opaque image, else its alpha slot; the K slots N .. N + K - 1 are
    handed out in image order."""
    flags = [bool(f) for f in opaque]
    table = np.full(len(flags), -1, np.int32)
    k = 0
    for n, f in enumerate(flags):
        if not f:
            table[n] = len(flags) + k
            k += 1
    return table, k


def _check_alpha_slots(alpha_slot, n):
    """-> (int table, K); ValueError unless the entries >= 0 are the slots n .. n + K - 1, each once."""
    table = [int(s) for s in np.asarray(alpha_slot).reshape(-1)]
    used = sorted(s for s in table if s >= 0)
    if len(table) != n or any(s < -1 for s in table) or used != list(range(n, n + len(used))):
        raise ValueError("larvanet_amd: alpha_slot must hold %d entries, -1 or the slots %d .. %d + K - 1 each once, got %s"
                         % (n, n, n, table))
    return table, len(used)


def rgba_split_f32(images_u8, alpha_slot):
    """uint8 (N, H, W, 4) -> float32 (N + K, 3, H, W), exact: slot n holds image n's colour planes, slot alpha_slot[n] >= N
    its alpha plane three times; alpha_slot[n] == -1 (an opaque image) has no alpha slot."""
    a = np.asarray(images_u8)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 4 or min(a.shape) < 1:
        raise ValueError("larvanet_amd: rgba_split_f32 takes a uint8 (N, H, W, 4) batch, got %s %s" % (a.dtype, a.shape,))
    n = a.shape[0]
    table, k = _check_alpha_slots(alpha_slot, n)
    out = np.empty((n + k, 3) + a.shape[1:3], np.float32)
    out[:n] = a[..., :3].transpose(0, 3, 1, 2)
    for i, s in enumerate(table):
        if s >= 0:
            out[s] = a[i, :, :, 3][None]
    return out


def rgba_merge_u8(rgb_u8, alpha_slot, n):
    """uint8 (N + K, h, w, 3) (the forward's result for rgba_split_f32's slots) -> uint8 (N, h, w, 4): channels 0..2 from
    slot n, channel 3 = (r + g + b + 1) // 3 of slot alpha_slot[n] in int32, 255 where alpha_slot[n] == -1."""
    a = np.asarray(rgb_u8)
    n = int(n)
    table, k = _check_alpha_slots(alpha_slot, n)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[0] != n + k or min(a.shape) < 1:
        raise ValueError("larvanet_amd: rgba_merge_u8 takes a uint8 (%d, h, w, 3) batch, got %s %s" % (n + k, a.dtype, a.shape,))
    out = np.empty((n,) + a.shape[1:3] + (4,), np.uint8)
    out[..., :3] = a[:n]
    for i, s in enumerate(table):
        out[i, :, :, 3] = 255 if s < 0 else (a[s].astype(np.int32).sum(axis=2) + 1) // 3
    return out


# ------------------------------------------------------------------ planar YUV 4:2:0 (I420) <-> RGB, in exact integers
# A frame is ONE contiguous uint8 buffer: Y [H][W], then U [ch][cw], then V [ch][cw], cw = (W + 1) // 2, ch = (H + 1) // 2.
# Odd W and H are legal; a coordinate outside a plane is the edge's (clamped), reading and writing.  Chroma is centred on
# 128 and sited in the centre of its 2 x 2 luma block (the JPEG / MPEG-1 position), and only there.  These two functions
# are the definition; kernels.i420_to_rgb_f32 / rgb_u8_to_i420 (csrc/larva_yuv.hip) equal them bit for bit.
YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}   # (Kr, Kb); Kg = 1 - Kr - Kb
YUV_TO_RGB_TABLE_WORDS = 6     # luma offset, cy, crv, cgu, cgv, cbu
RGB_TO_YUV_TABLE_WORDS = 10    # luma offset, the Y row (R, G, B), the U row, the V row


def i420_frame_bytes(width, height):
    """Bytes of one I420 frame of width x height luma pixels: W H + 2 ((W + 1) // 2) ((H + 1) // 2)."""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("larvanet_amd: a frame needs width and height >= 1, got %d x %d" % (width, height))
    return width * height + 2 * ((width + 1) // 2) * ((height + 1) // 2)


def _yuv_params(matrix, full_range):
    """-> (Kr, Kg, Kb, luma offset, luma span, chroma span)."""
    if matrix not in YUV_MATRICES:
        raise ValueError("larvanet_amd: matrix must be one of %s, got %r" % (sorted(YUV_MATRICES), matrix))
    kr, kb = YUV_MATRICES[matrix]
    return (kr, 1.0 - kr - kb, kb) + ((0, 255, 255) if full_range else (16, 219, 224))


def yuv_to_rgb_matrix(matrix, full_range):
    """The float64 textbook inverse: R = cy (Y - offset) + crv (V - 128), G = cy (Y - offset) + cgu (U - 128) + cgv (V -
    128), B = cy (Y - offset) + cbu (U - 128) -> (offset, cy, crv, cgu, cgv, cbu)."""
    kr, kg, kb, offset, yspan, cspan = _yuv_params(matrix, full_range)
    c = 255.0 / cspan
    return (offset, 255.0 / yspan, 2.0 * (1.0 - kr) * c, -2.0 * (1.0 - kb) * kb / kg * c, -2.0 * (1.0 - kr) * kr / kg * c,
            2.0 * (1.0 - kb) * c)


def rgb_to_yuv_matrix(matrix, full_range):
    """The float64 textbook forward matrix: Y = offset + yr R + yg G + yb B, U = 128 + ur R + ug G + ub B, V likewise ->
    (offset, (yr, yg, yb), (ur, ug, ub), (vr, vg, vb))."""
    kr, kg, kb, offset, yspan, cspan = _yuv_params(matrix, full_range)
    sy, sc = yspan / 255.0, cspan / 255.0
    u = 0.5 * sc / (1.0 - kb)
    v = 0.5 * sc / (1.0 - kr)
    return (offset, (sy * kr, sy * kg, sy * kb), (-u * kr, -u * kg, u * (1.0 - kb)), (v * (1.0 - kr), -v * kg, -v * kb))


def yuv_to_rgb_table(matrix, full_range):
    """The int32 table of i420_to_rgb_f32 (YUV_TO_RGB_TABLE_WORDS): the luma offset and the inverse-matrix entries times
    4096.  The four chroma entries are rounded to nearest.  The luma gain is rounded UP: 219 * round(255 / 219 * 4096) is
    69 / 4096 short of 255, and white (Y = 235) has to come out as 255.0 exactly, which the final clamp then gives; it
    costs 0.69 / 4096 of gain where rounding to nearest costs 0.31 / 4096 (full range: exactly 4096 either way)."""
    m = yuv_to_rgb_matrix(matrix, full_range)
    return [int(m[0]), int(np.ceil(m[1] * 4096.0 - 1e-9))] + [int(np.rint(k * 4096.0)) for k in m[2:]]


def rgb_to_yuv_table(matrix, full_range):
    """The int32 table of rgb_u8_to_i420 (RGB_TO_YUV_TABLE_WORDS): the luma offset and the three rows times 65536, rounded
    to nearest; then the entry of largest magnitude of a row takes what the row's sum is off by, so that the Y row sums
    to round(span / 255 * 65536) exactly and the U and V rows to 0 exactly (grey stays grey)."""
    offset, *rows = rgb_to_yuv_matrix(matrix, full_range)
    span = _yuv_params(matrix, full_range)[4]
    table = [int(offset)]
    for row, want in zip(rows, (int(np.rint(span / 255.0 * 65536.0)), 0, 0)):
        q = [int(np.rint(k * 65536.0)) for k in row]
        q[int(np.argmax(np.abs(row)))] += want - sum(q)
        table += q
    return table


def _check_frame(frame, width, height, who):
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8:
        raise TypeError("larvanet_amd: %s takes a uint8 numpy frame, got %s"
                        % (who, getattr(frame, "dtype", type(frame).__name__),))
    n = i420_frame_bytes(width, height)
    if frame.ndim != 1 or frame.size != n:
        raise ValueError("larvanet_amd: an I420 frame of %d x %d is a flat buffer of %d bytes, got shape %s"
                         % (width, height, n, frame.shape,))


def i420_planes(frame, width, height):
    """Views of the Y [H][W], U [ch][cw] and V [ch][cw] planes of a flat I420 frame."""
    _check_frame(frame, width, height, "i420_planes")
    cw, ch = (width + 1) // 2, (height + 1) // 2
    y = frame[:width * height].reshape(height, width)
    u = frame[width * height:width * height + cw * ch].reshape(ch, cw)
    v = frame[width * height + cw * ch:].reshape(ch, cw)
    return y, u, v


def _chroma16(c, width, height):
    """The chroma plane c [ch][cw] at every luma pixel, times 16 and less 2048 (= 16 (C - 128)), int32 [H][W]: for luma
    pixel (2 i + a, 2 j + b), 9 C[i][j] + 3 C[i][j +- 1] + 3 C[i +- 1][j] + C[i +- 1][j +- 1] - 2048, the sign towards the
    nearer neighbour (a, b = 0: -1; 1: +1), indices clamped: the bilinear filter of centre-sited chroma."""
    ch, cw = c.shape
    c = c.astype(np.int32)
    rows, cols = np.arange(height), np.arange(width)
    i, j = rows // 2, cols // 2
    i2 = np.clip(i + 2 * (rows % 2) - 1, 0, ch - 1)
    j2 = np.clip(j + 2 * (cols % 2) - 1, 0, cw - 1)
    return (9 * c[i[:, None], j[None, :]] + 3 * c[i[:, None], j2[None, :]] + 3 * c[i2[:, None], j[None, :]]
            + c[i2[:, None], j2[None, :]] - 2048)


def i420_to_rgb_f32(frame, width, height, matrix="bt601", full_range=False):
    """One I420 frame -> float32 [3][H][W] RGB on [0, 255] in steps of 1 / 256 (exact in fp32): the network sees the frame
    without an intermediate rounding to bytes.  With the table (offset, cy, crv, cgu, cgv, cbu) of yuv_to_rgb_table,
    L = (Y - offset) 16 cy and u, v = _chroma16 of the two planes, the int32 sums with 16 fractional bits are
    R = L + crv v, G = L + cgu u + cgv v, B = L + cbu u, and a value is clamp((N + 128) >> 8, 0, 255 * 256) / 256 (an
    arithmetic shift)."""
    y, u, v = i420_planes(frame, width, height)
    offset, cy, crv, cgu, cgv, cbu = (np.int32(t) for t in yuv_to_rgb_table(matrix, full_range))
    lum = (y.astype(np.int32) - offset) * (np.int32(16) * cy)
    u16, v16 = _chroma16(u, width, height), _chroma16(v, width, height)
    n = np.stack([lum + crv * v16, lum + cgu * u16 + cgv * v16, lum + cbu * u16])
    assert n.dtype == np.int32
    return np.clip((n + 128) >> 8, 0, 255 * 256).astype(np.float32) * np.float32(1.0 / 256.0)


def rgb_u8_to_i420(image, matrix="bt601", full_range=False):
    """uint8 (H, W, 3) RGB -> the flat I420 frame.  With the table (offset, Y row, U row, V row) of rgb_to_yuv_table, all
    in int32: Y = clamp((sum c v + (offset << 16) + 2^15) >> 16, 0, 255) per pixel, and per chroma sample, S the
    per-channel sums of its 2 x 2 luma block with the edge pixels repeated, C = clamp((sum c S + (128 << 18) + 2^17) >> 18,
    0, 255): the block's mean and the matrix in one rounding."""
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8:
        raise TypeError("larvanet_amd: rgb_u8_to_i420 takes a uint8 numpy array, got %s"
                        % (getattr(image, "dtype", type(image).__name__),))
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("larvanet_amd: rgb_u8_to_i420 takes an (H, W, 3) image, got shape %s" % (image.shape,))
    t = [np.int32(k) for k in rgb_to_yuv_table(matrix, full_range)]
    height, width = image.shape[:2]
    a = image.astype(np.int32)
    y = (a[..., 0] * t[1] + a[..., 1] * t[2] + a[..., 2] * t[3] + (t[0] << 16) + (1 << 15)) >> 16
    r0, c0 = np.arange(0, height, 2), np.arange(0, width, 2)
    r1, c1 = np.minimum(r0 + 1, height - 1), np.minimum(c0 + 1, width - 1)
    s = a[r0][:, c0] + a[r0][:, c1] + a[r1][:, c0] + a[r1][:, c1]
    planes = [np.clip(y, 0, 255)]
    for k in (4, 7):
        c = (s[..., 0] * t[k] + s[..., 1] * t[k + 1] + s[..., 2] * t[k + 2] + (128 << 18) + (1 << 17)) >> 18
        planes.append(np.clip(c, 0, 255))
    assert all(p.dtype == np.int32 for p in planes)
    return np.concatenate([p.astype(np.uint8).reshape(-1) for p in planes])


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
