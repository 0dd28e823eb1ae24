"""Validation metric of the reference (validate.py:17-27), host side, numpy like the reference:
uint8 conversion by round-half-to-even + clip, top-left crop of the truth to the output size,
PSNR over all RGB pixels (no border shave, no Y conversion)."""
import numpy as np


def image_to_uint8(image):
    return np.clip(np.round(image), a_min=0, a_max=255).astype(np.uint8)


def fit_truth_image_size(output_image, truth_image):
    return truth_image[:, 0:output_image.shape[1], 0:output_image.shape[2]]


def image_psnr(output_image, truth_image):
    diff = np.float32(truth_image) - np.float32(output_image)
    mse = np.mean(np.power(diff, 2))
    return 10.0 * np.log10(255.0 ** 2 / mse)


# ---------------------------------------------------------------------------------------------
# The benchmark protocols (larvanet_amd.evaluate): the host-side definitions the device kernels of csrc/larva_metrics.hip
# are written against.  uint8 (H, W, 3) images.
# ---------------------------------------------------------------------------------------------
def shave(image, border):
    """image (H, W[, C]) without `border` pixels on every side; border 0 returns the image itself."""
    border = int(border)
    if border < 0:
        raise ValueError("larvanet_amd: shave needs a border >= 0, got %d" % border)
    if border == 0:
        return image
    return image[border:image.shape[0] - border, border:image.shape[1] - border]


def rgb_to_y_u8(image_hwc_uint8):
    """BT.601 luma of an 8-bit RGB image (..., 3) -> uint8 (...), 16..235: with N = 65481 R + 128553 G + 24966 B,
    Y = 16 + round_half_even(N / 255000), all in integers -- rgb2ycbcr + round + clip of the float protocol, stated so
    that a device and a host agree bit for bit."""
    a = np.asarray(image_hwc_uint8)
    if a.dtype != np.uint8 or a.shape[-1] != 3:
        raise ValueError("larvanet_amd: rgb_to_y_u8 takes uint8 (..., 3) images")
    n = a[..., 0].astype(np.int64) * 65481 + a[..., 1].astype(np.int64) * 128553 + a[..., 2].astype(np.int64) * 24966
    q, rem = np.divmod(n, 255000)
    q = q + ((2 * rem > 255000) | ((2 * rem == 255000) & (q % 2 == 1)))
    return (16 + q).astype(np.uint8)


def psnr_from_sse(sse, n):
    """10 log10(255^2 n / sse) for an exact integer sum of squared differences over n values; inf for sse == 0."""
    sse, n = int(sse), int(n)
    if n <= 0 or sse < 0:
        raise ValueError("larvanet_amd: psnr_from_sse needs n > 0 and sse >= 0")
    if sse == 0:
        return float("inf")
    return 10.0 * float(np.log10(255.0 ** 2 * n / sse))
