"""What --output_size costs at the x4 output of one 339 x 510 image (1356 x 2040) resized to 1080 x 1620: medians of
  * the resize launch alone (kernels.resize_u8), with the bytes it reads plus the bytes it writes as a fraction of the
    HBM peak;
  * Pillow's Image.resize(..., BICUBIC) of the same image on the host (what a user runs today on every frame);
  * pipeline.upscale_yuv_stream per frame at fp32 and fp16, without and with output_size.

    python tools/time_resize.py [--frames 60] [--repeats 5] [--num_blocks 4,4,4,4]
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

from larvanet_amd import image_utils as U   # noqa: E402
from larvanet_amd import kernels as K       # noqa: E402
from larvanet_amd import pipeline           # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X
W, H, S = 510, 339, 4
OUT_H, OUT_W = 1080, 1620


def _frame(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    y = (40 + 150 * (xx + yy) / (W + H) + rng.integers(0, 12, (H, W))).astype(np.uint8)
    c = rng.integers(100, 156, 2 * ((W + 1) // 2) * ((H + 1) // 2)).astype(np.uint8)
    return np.concatenate([y.reshape(-1), c])


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


def _host_median(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def _stream_median(make, frames, repeats):
    """Median over `repeats` of the wall time per frame of a whole stream (after one warm-up pass), in seconds."""
    for _ in make(frames[:8]):
        pass
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in make(frames))
        out.append((time.perf_counter() - t0) / n)
    return statistics.median(out), min(out), max(out)


def main():
    from PIL import Image
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=60)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--num_blocks", type=str, default="4,4,4,4")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    frames = [_frame(i) for i in range(args.frames)]
    host_img = np.random.default_rng(0).integers(0, 256, (S * H, S * W, 3), dtype=np.uint8)
    hr_img = torch.from_numpy(host_img[None]).to(dev)
    out = torch.empty((1, OUT_H, OUT_W, 3), dtype=torch.uint8, device=dev)
    rows = []
    fmt = lambda t: "%8.1f us  (%.1f .. %.1f)" % (t[0] * 1e6, t[1] * 1e6, t[2] * 1e6)   # noqa: E731
    got = K.resize_u8(hr_img, OUT_H, OUT_W, out=out).cpu().numpy()[0]
    pil = Image.fromarray(host_img)
    same = np.array_equal(got, np.asarray(pil.resize((OUT_W, OUT_H), Image.BICUBIC)))
    t = _device_median(lambda: K.resize_u8(hr_img, OUT_H, OUT_W, out=out), args.repeats)
    moved = hr_img.numel() + out.numel()
    rows.append(("resize_u8, %d x %d -> %d x %d" % (S * W, S * H, OUT_W, OUT_H), fmt(t) + "  %.1f MB, %.1f %% of HBM peak"
                 % (moved / 1e6, 100 * moved / t[0] / HBM_PEAK)))
    t = _host_median(lambda: pil.resize((OUT_W, OUT_H), Image.BICUBIC), args.repeats)
    rows.append(("Pillow on the host, same image", fmt(t) + "  (device bytes equal Pillow's: %s)" % same))
    for precision in ("fp32", "fp16"):
        m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
        blocks = args.num_blocks.split(",")
        m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + args.num_blocks, "--precision=" + precision])
        torch.manual_seed(0)
        m.prepare(is_training=False, scales=[S])
        t = _stream_median(lambda fs: pipeline.upscale_yuv_stream(m, fs, S, W, H), frames, args.repeats)
        rows.append(("%s upscale_yuv_stream / frame" % precision, fmt(t)))
        t = _stream_median(lambda fs: pipeline.upscale_yuv_stream(m, fs, S, W, H, output_size=(OUT_H, OUT_W)), frames,
                           args.repeats)
        rows.append(("%s ... with output_size %dx%d" % (precision, OUT_W, OUT_H), fmt(t)))
    print("median (min .. max) over %d repeats, %d frames per stream, LarvaNet num_blocks %s, x%d"
          % (args.repeats, args.frames, args.num_blocks, S))
    for name, value in rows:
        print("  %-40s %s" % (name, value))


if __name__ == "__main__":
    main()
