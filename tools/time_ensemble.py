#!/usr/bin/env python3
"""What the geometric self-ensemble costs end to end: one seeded 339 x 510 uint8 image at x4 (V1, M4B4, 48 channels),
fp32 and fp16, host clock around work that ends with the uint8 result usable on the host.

    python tools/time_ensemble.py            # a, b, c and the merge launch alone
    python tools/time_ensemble.py --psnr     # also: what the ensemble does to the PSNR of a briefly trained model

  a  model.upscale_u8([hwc_u8], 4)[0]                                    one plain image
  b  the ensemble by hand: eight model.upscale calls on image_utils.dihedral inputs, a numpy inverse + mean
     (image_utils.self_ensemble), metrics.image_to_uint8                 what a user writes without the flag
  c  model_with_flag.upscale_u8([hwc_u8], 4)[0]                          --self_ensemble: merged on the device
  M  kernels.dihedral_mean alone on this image's eight fp32 HR results, by events (uint8 and float outputs)

One process, every shape warmed, the variants alternated inside every round; min / median / max over the rounds.  b and c
return the same bytes (asserted).  Needs an MI355X: there is no CPU timing."""
import argparse
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
MERGE_BYTES = {"u8": 8 * HR_VALUES * 4 + HR_VALUES, "f32": 8 * HR_VALUES * 4 + HR_VALUES * 4}   # read + written


def model(precision, ensemble, weights=None):
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(["--num_modules=4", "--num_blocks=4,4,4,4", "--precision=" + precision]
                 + (["--self_ensemble"] if ensemble else []))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[SCALE])
    if weights is not None:
        m.model.load_state_dict(weights)
        m.model.invalidate_packed_weights()
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


def by_hand(m, hwc):
    from larvanet_amd import image_utils as U
    from larvanet_amd.metrics import image_to_uint8
    chw = np.ascontiguousarray(hwc.transpose(2, 0, 1)).astype(np.float32)
    e = U.self_ensemble(lambda x: m.upscale([x], SCALE)[0], chw, axes=(1, 2))
    return image_to_uint8(e).transpose(1, 2, 0)


def merge_alone(rounds, reps):
    """The merge launch on fp32 data of this image's HR shapes, by events: us per launch."""
    from larvanet_amd import kernels as K
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    a = (torch.rand(4, 3, H * SCALE, W * SCALE, generator=g) * 300 - 20).to(dev)
    b = (torch.rand(4, 3, W * SCALE, H * SCALE, generator=g) * 300 - 20).to(dev)
    out = {}
    for kind in ("u8", "f32"):
        dst = K.dihedral_mean(a, b, u8=kind == "u8")
        for _ in range(10):
            K.dihedral_mean(a, b, u8=kind == "u8", out=dst)
        us = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                K.dihedral_mean(a, b, u8=kind == "u8", out=dst)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / reps * 1e3)
        out[kind] = us
        med = statistics.median(us)
        print("  M  dihedral_mean -> %-3s  %s us per launch (%d launches back to back per round); %.2f TB/s = %.2f of the "
              "HBM peak (%d bytes, %.0f TB/s)" % (kind, spread(us), reps, MERGE_BYTES[kind] / med / 1e6,
                                                  MERGE_BYTES[kind] / (med * 1e-6) / HBM_PEAK, MERGE_BYTES[kind],
                                                  HBM_PEAK / 1e12), flush=True)
    return out


def measure(rounds, reps):
    hwc = image()
    result = {}
    for precision in ("fp32", "fp16"):
        plain, ens = model(precision, False), model(precision, True)
        variants = {
            "a": (lambda: plain.upscale_u8([hwc], SCALE)[0], reps),
            "b": (lambda: by_hand(plain, hwc), max(1, reps // 8)),
            "c": (lambda: ens.upscale_u8([hwc], SCALE)[0], max(1, reps // 4)),
        }
        with torch.no_grad():
            assert np.array_equal(variants["b"][0](), variants["c"][0]()), "the by-hand ensemble and the flag disagree"
            for fn, _ in variants.values():   # (warm-up of every shape and path)
                for _ in range(3):
                    fn()
            t = {k: [] for k in variants}
            for _ in range(rounds):
                for k, (fn, n) in variants.items():
                    t[k].append(timed(fn, n))
        result[precision] = t
        print("%s, ms per result (min / median / max of %d rounds; calls per round: a %d, b %d, c %d)"
              % (precision, rounds, variants["a"][1], variants["b"][1], variants["c"][1]))
        for k, what in (("a", "upscale_u8, plain"), ("b", "ensemble by hand: 8 upscale + numpy + image_to_uint8"),
                        ("c", "upscale_u8 with --self_ensemble")):
            print("  %s  %-52s %s" % (k, what, spread(t[k])))
        ma, mb, mc = (statistics.median(t[k]) for k in "abc")
        print("  b / c = %.2f   c / (8 a) = %.3f   %s" % (mb / mc, mc / (8 * ma), "c < b: yes" if mc < mb else "c < b: NO"),
              flush=True)
    print("merge launch alone, 8 x fp32 %d x %d x 3:" % (H * SCALE, W * SCALE))
    result["merge_us"] = merge_alone(rounds, 50)
    return result


def psnr_change():
    """Observation, no bar: PSNR (uint8 protocol, RGB, whole image) of plain and ensembled outputs of an M4B4 model trained
    for 200 fp32 steps on synthetic smooth images, against the images it was not trained on."""
    import torch.nn.functional as F
    from larvanet_amd.metrics import image_psnr, image_to_uint8

    def smooth_hr(g, n, h, w):
        low = torch.rand(n, 3, h // 16 + 1, w // 16 + 1, generator=g)
        mid = torch.rand(n, 3, h // 4 + 1, w // 4 + 1, generator=g)
        img = F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False) * 0.85 + \
            F.interpolate(mid, size=(h, w), mode="bicubic", align_corners=False) * 0.15
        return (img * 255).clamp(0, 255)

    class NoVal:
        def get_num_images(self):
            return 0

    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(["--num_modules=4", "--num_blocks=4,4,4,4"])
    torch.manual_seed(0)
    m.prepare(is_training=True, scales=[SCALE])
    g = torch.Generator().manual_seed(5)
    hr = smooth_hr(g, 4, 512, 512)
    lr = F.interpolate(hr, scale_factor=0.25, mode="area")
    hr, lr = hr.to(m.device), lr.to(m.device)
    pick = np.random.default_rng(6)
    for _ in range(200):
        idx = pick.integers(0, 4, 16)
        ys, xs = pick.integers(0, 128 - 48, 16), pick.integers(0, 128 - 48, 16)
        x = torch.stack([lr[i, :, y:y + 48, c:c + 48] for i, y, c in zip(idx, ys, xs)])
        t = torch.stack([hr[i, :, 4 * y:4 * y + 192, 4 * c:4 * c + 192] for i, y, c in zip(idx, ys, xs)])
        m.train_step_larva(None, NoVal(), x.contiguous(), t.contiguous())
    weights = {k: v.detach().clone() for k, v in m.model.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    for h, w in ((339, 510), (64, 64)):
        truth = smooth_hr(g, 1, 4 * h, 4 * w)
        lr8 = image_to_uint8(F.interpolate(truth, scale_factor=0.25, mode="area")[0].numpy()).transpose(1, 2, 0)
        truth8 = image_to_uint8(truth[0].numpy()).transpose(1, 2, 0)
        for precision in ("fp32", "fp16"):
            p = [float(image_psnr(output_image=model(precision, e, weights).upscale_u8([np.ascontiguousarray(lr8)], SCALE)[0],
                                  truth_image=truth8)) for e in (False, True)]
            print("psnr %d x %d %s: plain %.4f dB, ensemble %.4f dB, change %+.4f dB" % (h, w, precision, p[0], p[1], p[1] - p[0]),
                  flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=80)
    p.add_argument("--psnr", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_ensemble.py needs an MI355X: nothing here can be timed on a CPU")
    measure(a.rounds, a.reps)
    if a.psnr:
        psnr_change()
