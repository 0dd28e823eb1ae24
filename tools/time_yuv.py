"""What the video path costs at one 339 x 510 frame (x4), at fp32 and fp16: medians of
  * each colour-conversion launch alone (kernels.i420_to_rgb_f32 on the LR frame, kernels.rgb_u8_to_i420 on the HR image),
    with the bytes it moves as a fraction of the HBM peak;
  * model.upscale_yuv420_tensor (both conversions and the forward, on the device);
  * pipeline.upscale_yuv_stream per frame (host frames in, host frames out, copies overlapped);
  * pipeline.upscale_stream per frame on the RGB image of the same frame: existing code, the yardstick.

    python tools/time_yuv.py [--frames 60] [--repeats 5] [--num_blocks 4,4,4,4]
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
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=60)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--num_blocks", type=str, default="4,4,4,4")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    frames = [_frame(i) for i in range(args.frames)]
    rgb = [np.ascontiguousarray(np.clip(np.rint(U.i420_to_rgb_f32(f, W, H)), 0, 255).astype(np.uint8).transpose(1, 2, 0))
           for f in frames[:4]]
    rgb = [rgb[i % 4] for i in range(args.frames)]
    lr = torch.from_numpy(frames[0][None]).to(dev)
    hr_img = torch.randint(0, 256, (1, S * H, S * W, 3), dtype=torch.uint8, device=dev)
    lr_out = torch.empty((1, 3, H, W), device=dev)
    hr_out = torch.empty((1, U.i420_frame_bytes(S * W, S * H)), dtype=torch.uint8, device=dev)
    rows = []
    fmt = lambda t: "%8.1f us  (%.1f .. %.1f)" % (t[0] * 1e6, t[1] * 1e6, t[2] * 1e6)   # noqa: E731
    t = _device_median(lambda: K.i420_to_rgb_f32(lr, W, H, out=lr_out), args.repeats)
    moved = frames[0].size + 12 * W * H
    rows.append(("i420_to_rgb_f32, %d x %d" % (W, H), fmt(t) + "  %.1f MB, %.0f %% of HBM peak"
                 % (moved / 1e6, 100 * moved / t[0] / HBM_PEAK)))
    t = _device_median(lambda: K.rgb_u8_to_i420(hr_img, out=hr_out), args.repeats)
    moved = 3 * S * S * W * H + hr_out.numel()
    rows.append(("rgb_u8_to_i420, %d x %d" % (S * W, S * H), fmt(t) + "  %.1f MB, %.0f %% of HBM peak"
                 % (moved / 1e6, 100 * moved / t[0] / HBM_PEAK)))
    for precision in ("fp32", "fp16"):
        m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
        blocks = args.num_blocks.split(",")
        m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + args.num_blocks, "--precision=" + precision])
        torch.manual_seed(0)
        m.prepare(is_training=False, scales=[S])
        t = _device_median(lambda: m.upscale_yuv420_tensor(lr, W, H), args.repeats, inner=10)
        rows.append(("%s upscale_yuv420_tensor" % precision, fmt(t)))
        t = _stream_median(lambda fs: pipeline.upscale_yuv_stream(m, fs, S, W, H), frames, args.repeats)
        rows.append(("%s upscale_yuv_stream / frame" % precision, fmt(t)))
        t = _stream_median(lambda fs: pipeline.upscale_stream(m, fs, S), rgb, args.repeats)
        rows.append(("%s upscale_stream / frame (RGB)" % precision, fmt(t)))
    print("median (min .. max) over %d repeats, %d frames per stream, LarvaNet num_blocks %s, x%d"
          % (args.repeats, args.frames, args.num_blocks, S))
    for name, value in rows:
        print("  %-36s %s" % (name, value))


if __name__ == "__main__":
    main()
