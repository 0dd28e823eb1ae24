#!/usr/bin/env python3
"""What the device bicubic downscaler costs: seeded 1356 x 2040 uint8 images, one process, profiler off,
the variants alternated inside every round; min / median / max over the rounds.

    python tools/time_downscale.py
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o down -- python tools/time_downscale.py --kernels

  1  kernels.bicubic_down_u8, one image, x2 / x3 / x4                by events around 50 launches back to back
  2  kernels.bicubic_down_u8_table, 16 such images, x2 / x3 / x4     one launch by events; bytes read + written per
     (HWC and the sampler's CHW tables)                              second against the 8 TB/s HBM peak
  3  pipeline.evaluate_stream per image at x4 (V1 M4B4), 16 images   host clock: LR supplied against LR made on the device

Needs an MI355X: there is no CPU timing."""
import argparse
import importlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

H, W, IMAGES = 1356, 2040, 16
HBM_PEAK = 8.0e12   # bytes / s (specification)


def image(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def spread(v):
    return "%.2f / %.2f / %.2f" % (min(v), statistics.median(v), max(v))


def by_events(fn, reps):
    """us per call of `reps` calls back to back."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def launches(rounds):
    from larvanet_amd import image_utils, kernels as K
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(image(1)).to(dev)
    raw = K.hip_lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    single, tables = {}, {}
    for s in (2, 3, 4):
        out = K.bicubic_down_u8(x, s)
        assert np.array_equal(out.cpu().numpy(), image_utils.bicubic_downscale_u8(image(1), s))
        single[s] = (lambda s=s, out=out: K.bicubic_down_u8(x, s, out=out))
        for planar in (False, True):
            h, w = H // s, W // s
            n_in, n_out = 3 * h * s * w * s, 3 * h * w
            data = torch.randint(0, 256, (IMAGES * n_in,), dtype=torch.uint8, device=dev)
            off = torch.arange(IMAGES, dtype=torch.int64, device=dev) * n_in
            hw = torch.tensor([h * s, w * s] * IMAGES, dtype=torch.int32, device=dev)
            dst = torch.empty(IMAGES * n_out, dtype=torch.uint8, device=dev)
            dst_off = torch.arange(IMAGES, dtype=torch.int64, device=dev) * n_out
            K.bicubic_down_u8_table(data, off, hw, s, dst, dst_off, planar=planar)   # (checked once)
            per = -(-h // K.DOWN_TILE_ROWS) * -(-w // (K.DOWN_TILE_BYTES // (1 if planar else 3))) * (3 if planar else 1)
            prefix = (torch.arange(IMAGES + 1, dtype=torch.int32) * per).to(dev)
            keep = (data, off, hw, dst, dst_off, prefix)

            def table(s=s, planar=planar, keep=keep, per=per):   # (the raw entry point: the launch alone)
                data, off, hw, dst, dst_off, prefix = keep
                raw.larva_bicubic_down_u8_table(data.data_ptr(), off.data_ptr(), hw.data_ptr(), IMAGES, s, int(planar),
                                                dst.data_ptr(), dst_off.data_ptr(), prefix.data_ptr(), IMAGES * per, stream)
            tables[(s, planar)] = (table, IMAGES * (n_in + n_out))
    t1 = {s: [] for s in single}
    t2 = {k: [] for k in tables}
    for fn in list(single.values()) + [v[0] for v in tables.values()]:
        for _ in range(3):
            fn()
    for _ in range(rounds):
        for s, fn in single.items():
            t1[s].append(by_events(fn, 50))
        for k, (fn, _) in tables.items():
            t2[k].append(by_events(fn, 5))
    print("1  single launch, %d x %d -> / s, us per launch (min / median / max of %d rounds, 50 launches back to back)" % (H, W, rounds))
    for s in t1:
        nbytes = 3 * (H // s) * s * (W // s) * s + 3 * (H // s) * (W // s)
        med = statistics.median(t1[s])
        print("   x%d  %s   %.2f TB/s = %.2f of the HBM peak" % (s, spread(t1[s]), nbytes / med / 1e6, nbytes / (med * 1e-6) / HBM_PEAK))
    print("2  table launch, %d images, us per launch (5 launches back to back per round)" % IMAGES)
    for (s, planar), v in t2.items():
        med, nbytes = statistics.median(v), tables[(s, planar)][1]
        print("   x%d %s  %s   %.1f MB  %.2f TB/s = %.2f of the HBM peak"
              % (s, "CHW" if planar else "HWC", spread(v), nbytes / 1e6, nbytes / med / 1e6, nbytes / (med * 1e-6) / HBM_PEAK))
    return statistics.median(t1[4])


def streams(rounds, launch_us):
    from larvanet_amd import image_utils, pipeline
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(["--num_modules=4", "--num_blocks=4,4,4,4"])
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    truths = [image(10 + i) for i in range(IMAGES)]
    supplied = [(image_utils.bicubic_downscale_u8(t, 4), t) for t in truths]
    made = [(None, t) for t in truths]
    a = list(pipeline.evaluate_stream(m, supplied[:4], 4))
    b = list(pipeline.evaluate_stream(m, made[:4], 4))
    assert a == b, "the two forms disagree"
    t = {"supplied": [], "made": []}
    for _ in range(rounds):
        for name, pairs in (("supplied", supplied), ("made", made)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(1 for _ in pipeline.evaluate_stream(m, pairs, 4))
            t[name].append((time.perf_counter() - t0) / n * 1e3)
    print("3  evaluate_stream at x4, V1 M4B4, ms per image (%d images per round, decoded images in memory)" % IMAGES)
    for name in t:
        print("   LR %-9s %s" % (name, "%.3f / %.3f / %.3f" % (min(t[name]), statistics.median(t[name]), max(t[name]))))
    ms, mm = statistics.median(t["supplied"]), statistics.median(t["made"])
    print("   made - supplied = %+.3f ms against one launch = %.3f ms: %s"
          % (mm - ms, launch_us / 1e3, "condition met" if mm <= ms + launch_us / 1e3 else "condition MISSED"))


def kernels_only():
    """The work rocprofv3 should see: 50 single launches per scale."""
    from larvanet_amd import kernels as K
    x = torch.from_numpy(image(1)).to(torch.device("cuda", 0))
    for s in (2, 3, 4):
        out = K.bicubic_down_u8(x, s)
        for _ in range(50):
            K.bicubic_down_u8(x, s, out=out)
    torch.cuda.synchronize()


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--kernels", action="store_true")
    p.add_argument("--no_stream", action="store_true", help="the launches only")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_downscale.py needs an MI355X: nothing here can be timed on a CPU")
    if a.kernels:
        kernels_only()
    else:
        with torch.no_grad():
            us = launches(a.rounds)
            if not a.no_stream:
                streams(a.rounds, us)
