#!/usr/bin/env python3
"""What an image costs end to end: one seeded 339 x 510 uint8 image at x4 (V1, M4B4, 48 channels), fp32 and fp16, host
clock around work that ends with the result usable on the host.

    python tools/time_u8.py                      # A, B, C and the forward alone, profiler off
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o u8 -- python tools/time_u8.py --kernels      # a run of its own
    python tools/time_u8.py --summarize DIR      # the two pointwise kernels' time, bytes/s and share of the HBM peak

  A  image_to_uint8(model.upscale([chw_float], 4)[0])            today's way: fp32 HR image over the link, host pass
  B  model.upscale_u8([hwc_u8], 4)[0]                            uint8 both ways, pageable host memory
  C  pipeline.upscale_stream over 64 such images, per image      pinned staging, copies beside the forward
  F  fwd_runtime + synchronize                                   the forward alone (device only, no copies)

One process, every shape warmed, the variants alternated inside every round, each variant at least a second per
precision in all; min / median / max over the rounds.  Needs an MI355X: there is no CPU timing."""
import argparse
import glob
import importlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

H, W, SCALE = 339, 510, 4
HBM_PEAK = 8.0e12   # bytes / s (specification)
HR_VALUES = 3 * H * SCALE * W * SCALE
# algorithmic bytes of the two pointwise kernels for this image: read + written
BYTES = {"f32_chw_to_u8_hwc": HR_VALUES * 4 + HR_VALUES, "u8_hwc_to_f32_chw": 3 * H * W + 3 * H * W * 4}


def model(precision):
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(["--num_modules=4", "--num_blocks=4,4,4,4", "--precision=" + precision])
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[SCALE])
    return m


def image(seed=2):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def spread(v):
    return "%.3f / %.3f / %.3f" % (min(v), statistics.median(v), max(v))


def measure(rounds, reps):
    from larvanet_amd import pipeline
    from larvanet_amd.metrics import image_to_uint8
    hwc = image()
    chw = np.ascontiguousarray(hwc.transpose(2, 0, 1)).astype(np.float32)
    many = [image(100 + i) for i in range(64)]
    result = {}
    for precision in ("fp32", "fp16"):
        m = model(precision)
        x_dev = torch.from_numpy(chw[None]).to(m.device)
        variants = {
            "A": lambda: image_to_uint8(m.upscale([chw], SCALE)[0]),
            "B": lambda: m.upscale_u8([hwc], SCALE)[0],
            "F": lambda: m.fwd_runtime(x_dev),
        }
        with torch.no_grad():
            a, b = variants["A"](), variants["B"]()
            assert np.array_equal(a.transpose(1, 2, 0), b), "the two paths disagree"
            for fn in variants.values():   # (warm-up of every shape and path)
                for _ in range(5):
                    fn()
            assert len(list(pipeline.upscale_stream(m, many[:8], SCALE))) == 8
            t = {k: [] for k in "ABCF"}
            for _ in range(rounds):
                for k, fn in variants.items():
                    t[k].append(timed(fn, reps))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = sum(1 for _ in pipeline.upscale_stream(m, many, SCALE, depth=2))
                t["C"].append((time.perf_counter() - t0) / n * 1e3)
        result[precision] = t
        print("%s, ms per image (min / median / max of %d rounds; A, B, F: %d calls per round, C: 64 images per round)"
              % (precision, rounds, reps))
        for k, what in (("A", "image_to_uint8(upscale(float CHW))"), ("B", "upscale_u8(uint8 HWC)"),
                        ("C", "upscale_stream, depth 2, per image"), ("F", "fwd_runtime + synchronize (device only)")):
            print("  %s  %-42s %s" % (k, what, spread(t[k])))
        ma, mb, mc = (statistics.median(t[k]) for k in "ABC")
        print("  A / B = %.2f   B / C = %.2f   %s   %s" % (ma / mb, mb / mc, "B < A: yes" if mb < ma else "B < A: NO",
                                                         "C <= B: yes" if mc <= mb else "C <= B: NO"), flush=True)
    return result


def kernels_only():
    """The work rocprofv3 should see: both pointwise kernels on this image's shapes and the uint8 forwards."""
    from larvanet_amd import kernels as K
    dev = torch.device("cuda", 0)
    hwc = torch.from_numpy(image()[None]).to(dev)
    hr = (torch.rand(1, 3, H * SCALE, W * SCALE, generator=torch.Generator().manual_seed(3)) * 320 - 32).to(dev)
    for _ in range(50):
        K.u8_hwc_to_f32_chw(hwc)
        K.f32_chw_to_u8_hwc(hr)
    with torch.no_grad():
        for precision in ("fp32", "fp16"):
            m = model(precision)
            for _ in range(20):
                m.upscale_u8_tensor(hwc)
    torch.cuda.synchronize()


def summarize(path):
    import csv
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_stats.csv under %s" % path)
    for row in csv.DictReader(open(files[0])):
        name = row.get("Name", "")
        for key, nbytes in BYTES.items():
            if key + "_kernel" in name:
                ns = float(row["AverageNs"])
                print("%-24s %5s calls  avg %.2f us  %.2f TB/s  %.2f of the HBM peak (%d bytes, %.0f TB/s)"
                      % (key, row.get("Calls", "?"), ns / 1e3, nbytes / ns / 1e3, nbytes / (ns * 1e-9) / HBM_PEAK, nbytes,
                         HBM_PEAK / 1e12))
        if "conv_kernelILi5E" in name or "conv_kernelILi4E" in name:
            print("%-24s %5s calls  avg %.2f us" % ("fp16 leg end, uint8" if "Li5E" in name else "fp16 leg end, fp32",
                                                   row.get("Calls", "?"), float(row["AverageNs"]) / 1e3))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=160)
    p.add_argument("--kernels", action="store_true")
    p.add_argument("--summarize", type=str, default=None)
    a = p.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        if not torch.cuda.is_available():
            sys.exit("tools/time_u8.py needs an MI355X: nothing here can be timed on a CPU")
        kernels_only() if a.kernels else measure(a.rounds, a.reps)
