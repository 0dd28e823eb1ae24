#!/usr/bin/env python3
"""What scoring an image costs: one seeded 339 x 510 uint8 image at x4 and fp16 (V1, M4B4, 48 channels), its 1356 x 2040
truth, RGB PSNR + SSIM on the whole image.

    python tools/time_metrics.py                 # a .. e below, profiler off
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o met -- python tools/time_metrics.py --kernels   # a run of its own
    python tools/time_metrics.py --summarize DIR # the metric kernels' time per dispatch and share of the fp64 vector peak

  a  host metrics (tests/metrics_ref.py: numpy + scipy, float64) on the image upscale_u8 returned
  b  model.evaluate_u8_tensor(x, truth)                          forward + metrics, one record back, device-resident inputs
  c  pipeline.evaluate_stream over 32 pairs, per image           pinned staging, truth in beside the input, record back
  d  pipeline.upscale_stream over the same 32 inputs, per image  the image back, no metrics
  e  kernels.u8_metrics alone, by events, beside the fp16 forward alone (fwd_runtime), by events

One process, every shape warmed, the variants alternated inside every round; min / median / max over the rounds.  Needs an
MI355X: there is no CPU timing."""
import argparse
import glob
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

H, W, SCALE = 339, 510, 4
FP64_VECTOR_PEAK = 78.6e12   # flop / s (specification, FMA = 2)
# double-precision operations per SSIM sample and plane as built (csrc/larva_metrics.hip): the row pass runs on 32 staged
# rows for 22 rows of samples and costs 2 mul + 2 add + 3 fma per tap, the column pass 5 fma per tap, S 19 + a division
FMA_PER_SAMPLE = 11 * 3 * 32 / 22 + 11 * 5
OTHER_PER_SAMPLE = 11 * 4 * 32 / 22 + 19


def model(precision="fp16"):
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(["--num_modules=4", "--num_blocks=4,4,4,4", "--precision=" + precision])
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[SCALE])
    return m


def image(seed=2):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def truth(seed=3):
    return np.random.default_rng(seed).integers(0, 256, (H * SCALE, W * SCALE, 3), dtype=np.uint8)


def spread(v):
    return "%.3f / %.3f / %.3f" % (min(v), statistics.median(v), max(v))


def by_events(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def by_clock(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def measure(rounds, reps):
    import metrics_ref
    from larvanet_amd import kernels as K, pipeline
    m = model()
    lr, hr = image(), truth()
    x_dev = torch.from_numpy(lr[None]).to(m.device)
    t_dev = torch.from_numpy(hr[None]).to(m.device)
    chw = torch.from_numpy(np.ascontiguousarray(lr.transpose(2, 0, 1)[None]).astype(np.float32)).to(m.device)
    pairs = [(image(100 + i), hr) for i in range(32)]
    with torch.no_grad():
        sr = m.upscale_u8_tensor(x_dev)
        sr_host = sr[0].cpu().numpy()
        got = m.evaluate_u8_tensor(x_dev, t_dev, shave=0, channel="rgb")[0]
        want = metrics_ref.evaluate(sr_host, hr, 0, "rgb")
        assert got["sse"] == want["sse"] and abs(got["ssim"] - want["ssim"]) <= 2e-5, (got, want)
        record = torch.empty(K.METRIC_RESULT_WORDS, device=m.device, dtype=torch.int64)
        launches = {"metrics": lambda: K.u8_metrics(sr[0], t_dev[0], 0, "rgb", True, result=record),
                    "psnr only": lambda: K.u8_metrics(sr[0], t_dev[0], 0, "rgb", False, result=record),
                    "metrics y": lambda: K.u8_metrics(sr[0], t_dev[0], SCALE, "y", True, result=record),
                    "forward": lambda: m.fwd_runtime(chw)}
        for fn in launches.values():
            for _ in range(5):
                fn()
        for _ in range(5):
            m.evaluate_u8_tensor(x_dev, t_dev, shave=0, channel="rgb")
        assert len(list(pipeline.evaluate_stream(m, pairs[:4], SCALE, shave=0, channel="rgb"))) == 4
        assert len(list(pipeline.upscale_stream(m, [p[0] for p in pairs[:4]], SCALE))) == 4
        t = {k: [] for k in ["a", "b", "c", "d"] + list(launches)}
        for r in range(rounds):
            if r < 3:   # (1.8 s a call: three are enough for a median)
                t0 = time.perf_counter()
                metrics_ref.evaluate(sr_host, hr, 0, "rgb")
                t["a"].append((time.perf_counter() - t0) * 1e3)
            t["b"].append(by_clock(lambda: m.evaluate_u8_tensor(x_dev, t_dev, shave=0, channel="rgb"), reps))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(1 for _ in pipeline.evaluate_stream(m, pairs, SCALE, shave=0, channel="rgb"))
            t["c"].append((time.perf_counter() - t0) / n * 1e3)
            t0 = time.perf_counter()
            n = sum(1 for _ in pipeline.upscale_stream(m, [p[0] for p in pairs], SCALE))
            t["d"].append((time.perf_counter() - t0) / n * 1e3)
            for k, fn in launches.items():
                t[k].append(by_events(fn, reps))
    print("ms (min / median / max of %d rounds; b, e: %d calls per round; c, d: 32 images per round; a: 3 calls)" % (rounds, reps))
    for k, what in (("a", "host scipy metrics, rgb PSNR + SSIM"), ("b", "evaluate_u8_tensor (forward + metrics)"),
                    ("c", "evaluate_stream, depth 2, per image"), ("d", "upscale_stream, depth 2, per image"),
                    ("metrics", "e  u8_metrics rgb PSNR + SSIM, by events"), ("psnr only", "e  u8_metrics rgb PSNR only, by events"),
                    ("metrics y", "e  u8_metrics y shave 4, by events"), ("forward", "e  fp16 forward alone, by events")):
        print("  %-46s %s" % (what if k in launches else k + "  " + what, spread(t[k])))
    met, fwd = statistics.median(t["metrics"]), statistics.median(t["forward"])
    samples = 3 * (H * SCALE - 10) * (W * SCALE - 10)
    flop = samples * (2 * FMA_PER_SAMPLE + OTHER_PER_SAMPLE)
    print("  metrics / forward = %.3f   %s" % (met / fwd, "metrics <= forward: yes" if met <= fwd else "metrics <= forward: NO"))
    print("  %.0f fma + %.0f other fp64 operations per sample and plane, %.2f Gflop per image: %.1f %% of the fp64 vector peak "
          "(%.1f Tflop/s)" % (FMA_PER_SAMPLE, OTHER_PER_SAMPLE, flop / 1e9, 100 * flop / (met * 1e-3) / FP64_VECTOR_PEAK,
                              FP64_VECTOR_PEAK / 1e12), flush=True)


def kernels_only():
    """The work rocprofv3 should see: the metric launches on this image's shapes."""
    from larvanet_amd import kernels as K
    dev = torch.device("cuda", 0)
    a, b = torch.from_numpy(truth(4)).to(dev), torch.from_numpy(truth(3)).to(dev)
    for _ in range(50):
        K.u8_metrics(a, b, 0, "rgb")
        K.u8_metrics(a, b, SCALE, "y")
        K.u8_metrics(a, b, 0, "rgb", ssim=False)
    torch.cuda.synchronize()


def summarize(path):
    import csv
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_stats.csv under %s" % path)
    for row in csv.DictReader(open(files[0])):
        if "u8_metrics" in row.get("Name", ""):
            print("%-60s %5s calls  avg %.2f us  min %s  max %s" % (row["Name"][:60], row.get("Calls", "?"),
                                                                    float(row["AverageNs"]) / 1e3, row.get("MinNs"), row.get("MaxNs")))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--kernels", action="store_true")
    p.add_argument("--summarize", type=str, default=None)
    a = p.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        if not torch.cuda.is_available():
            sys.exit("tools/time_metrics.py needs an MI355X: nothing here can be timed on a CPU")
        kernels_only() if a.kernels else measure(a.rounds, a.reps)
