"""What keeping transparency costs at one 339 x 510 image (x4), at fp32 and fp16: medians of
  * each of the two launches alone (kernels.rgba_u8_split_f32 on the LR image, kernels.rgb_u8_merge_rgba on the HR result),
    for a translucent image (K = 1) and an opaque one (K = 0), with the bytes it moves as a fraction of the HBM peak;
  * model.upscale_rgba_u8_tensor for a translucent and for an opaque image, against model.upscale_u8_tensor of the RGB
    image: existing code, the yardstick (an opaque RGBA image should cost what the RGB image costs, a translucent one
    about twice that);
  * pipeline.upscale_stream per image with keep_alpha over translucent and over opaque RGBA images, and without it over
    the RGB images.

    python tools/time_rgba.py [--images 40] [--repeats 5] [--num_blocks 4,4,4,4]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from larvanet_amd import kernels as K       # noqa: E402
from larvanet_amd import pipeline           # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X
W, H, S = 510, 339, 4


def _image(seed, opaque):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = 40 + 150 * (xx + yy) / (W + H)
    alpha = np.full((H, W), 255.0) if opaque else np.clip(355.0 * (xx + (H - 1 - yy)) / (W + H) - 50.0, 0, 255)
    return np.ascontiguousarray(np.stack([ramp + rng.integers(0, 12, (H, W)), 220 - ramp + rng.integers(0, 12, (H, W)),
                                          100 + rng.integers(0, 24, (H, W)), alpha], axis=-1).astype(np.uint8))


def _device_median(fn, repeats, inner=20):
    """Median over `repeats` of the mean device time of `inner` back-to-back calls (events around the batch), in seconds."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / inner)
    return statistics.median(out), min(out), max(out)


def _stream_median(make, images, repeats):
    """Median over `repeats` of the wall time per image of a whole stream (after one warm-up pass), in seconds."""
    for _ in make(images[:8]):
        pass
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in make(images))
        out.append((time.perf_counter() - t0) / n)
    return statistics.median(out), min(out), max(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=40)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--num_blocks", type=str, default="4,4,4,4")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    clear = [_image(i, False) for i in range(4)]
    solid = [_image(i, True) for i in range(4)]
    rows = []
    fmt = lambda t: "%8.1f us  (%.1f .. %.1f)" % (t[0] * 1e6, t[1] * 1e6, t[2] * 1e6)   # noqa: E731
    lr = torch.from_numpy(clear[0][None]).to(dev)
    for name, flags in (("translucent", [False]), ("opaque", [True])):
        slot, k = K.alpha_slot_table(flags, dev)
        planes = torch.empty((1 + k, 3, H, W), device=dev)
        t = _device_median(lambda: K.rgba_u8_split_f32(lr, slot, k, out=planes), args.repeats)
        moved = 4 * W * H + 12 * W * H * (1 + k)
        rows.append(("rgba_u8_split_f32, %d x %d, %s" % (W, H, name), fmt(t) + "  %.1f MB, %.0f %% of HBM peak"
                     % (moved / 1e6, 100 * moved / t[0] / HBM_PEAK)))
        hr = torch.randint(0, 256, (1 + k, S * H, S * W, 3), dtype=torch.uint8, device=dev)
        hr_out = torch.empty((1, S * H, S * W, 4), dtype=torch.uint8, device=dev)
        t = _device_median(lambda: K.rgb_u8_merge_rgba(hr, slot, 1, out=hr_out), args.repeats)
        moved = 3 * S * S * W * H * (1 + k) + 4 * S * S * W * H
        rows.append(("rgb_u8_merge_rgba, %d x %d, %s" % (S * W, S * H, name), fmt(t) + "  %.1f MB, %.0f %% of HBM peak"
                     % (moved / 1e6, 100 * moved / t[0] / HBM_PEAK)))
    for precision in ("fp32", "fp16"):
        m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
        blocks = args.num_blocks.split(",")
        m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + args.num_blocks, "--precision=" + precision])
        torch.manual_seed(0)
        m.prepare(is_training=False, scales=[S])
        rgb = lr[..., :3].contiguous()
        t = _device_median(lambda: m.upscale_u8_tensor(rgb), args.repeats, inner=10)
        rows.append(("%s upscale_u8_tensor (RGB)" % precision, fmt(t)))
        t = _device_median(lambda: m.upscale_rgba_u8_tensor(lr, opaque=[True]), args.repeats, inner=10)
        rows.append(("%s upscale_rgba_u8_tensor, opaque" % precision, fmt(t)))
        t = _device_median(lambda: m.upscale_rgba_u8_tensor(lr, opaque=[False]), args.repeats, inner=10)
        rows.append(("%s upscale_rgba_u8_tensor, translucent" % precision, fmt(t)))
        for name, pool, keep in (("RGB", [np.ascontiguousarray(a[..., :3]) for a in clear], False), ("opaque RGBA", solid, True),
                                 ("translucent RGBA", clear, True)):
            images = [pool[i % 4] for i in range(args.images)]
            t = _stream_median(lambda xs: pipeline.upscale_stream(m, xs, S, keep_alpha=keep), images, args.repeats)
            rows.append(("%s upscale_stream / image, %s" % (precision, name), fmt(t)))
    print("median (min .. max) over %d repeats, %d images per stream, LarvaNet num_blocks %s, x%d"
          % (args.repeats, args.images, args.num_blocks, S))
    for name, value in rows:
        print("  %-48s %s" % (name, value))


if __name__ == "__main__":
    main()
