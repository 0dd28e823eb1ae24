"""Float64 host oracle of the benchmark metrics (test helper, not a test): the calls skimage's structural_similarity
makes (gaussian_weights=True, sigma=1.5, use_sample_covariance=False, K1=0.01, K2=0.03, data_range=255) --
scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5) over x, y, x^2, y^2, x y, the S map, a crop by 5, the mean -- and
the exact squared error, over the window larvanet_amd.kernels.metric_window defines."""
import numpy as np

from larvanet_amd.metrics import psnr_from_sse, rgb_to_y_u8, shave as shave_image

C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2


def ssim_plane(x, y):
    from scipy.ndimage import gaussian_filter
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    if min(x.shape) < 11:
        raise ValueError("window below 11 pixels")
    f = lambda a: gaussian_filter(a, sigma=1.5, truncate=3.5)   # noqa: E731
    ux, uy = f(x), f(y)
    vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(s[5:-5, 5:-5].mean(dtype=np.float64))


def windows(out, truth, shave):
    """The two (h, w, 3) uint8 windows: truth cropped top-left to the output, both shaved."""
    out = np.asarray(out)
    truth = np.asarray(truth)[:out.shape[0], :out.shape[1]]
    return shave_image(out, shave), shave_image(truth, shave)


def planes(window, channel):
    if channel == "y":
        return [rgb_to_y_u8(window)]
    return [window[:, :, c] for c in range(3)]


def evaluate(out, truth, shave, channel, ssim=True):
    a, b = windows(out, truth, shave)
    pa, pb = planes(a, channel), planes(b, channel)
    sse = sum(int(((p.astype(np.int64) - q.astype(np.int64)) ** 2).sum()) for p, q in zip(pa, pb))
    n = sum(p.size for p in pa)
    value = float(np.mean([ssim_plane(p, q) for p, q in zip(pa, pb)])) if ssim else None
    return {"psnr": psnr_from_sse(sse, n), "ssim": value, "sse": sse, "n": n}
