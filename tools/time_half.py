"""fp16 inference (--precision fp16) against fp32: one 339 x 510 image through M4B4 V1 and V2 (4 modules of 4 residual
blocks), the captured 16 x 3 x 48 x 48 batch forward, and the per-launch time of the dominant fp16 conv kernel (48 -> 48
on a 339 x 510 image, ReLU and +res0 epilogues) with its fraction of the HBM-byte roofline (8 TB/s) and of the f16
matrix roofline (2.5 PF dense).  Prints one JSON line per measurement.  Usage: python tools/time_half.py [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12
F16_FLOPS = 2.5e15


def _median_ms(fn, reps, inner=1):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return float(np.median(times))


def _model(name, precision):
    import importlib
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=4", "--num_blocks=4,4,4,4", "--precision=" + precision])
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    m.strict_graph = True
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from larvanet_amd import kernels as K
    dev = torch.device("cuda", 0)
    img = [np.random.default_rng(2).random((3, 339, 510)).astype(np.float32) * 255]
    batch = (torch.rand(16, 3, 48, 48, generator=torch.Generator().manual_seed(3)) * 255).to(dev)
    with torch.no_grad():
        for name in ("LarvaNet", "LarvaNetV2"):
            res = {"model": name + " M4B4"}
            for prec in ("fp32", "fp16"):
                m = _model(name, prec)
                m.upscale_tensor(img)
                inp = m._to_input_tensor(img)
                res["image_339x510_ms_" + prec] = round(_median_ms(lambda: m._infer(inp), a.reps), 4)
                for _ in range(3):   # (the second call of a shape captures the graph)
                    m._infer(batch)
                res["batch_16x3x48x48_captured_ms_" + prec] = round(_median_ms(lambda: m._infer(batch), a.reps), 4)
                if prec == "fp16":
                    res["fp16_overflowed"] = m.fp16_overflowed()
            res["image_speedup"] = round(res["image_339x510_ms_fp32"] / res["image_339x510_ms_fp16"], 3)
            print(json.dumps(res), flush=True)

        # the dominant kernel: a 48 -> 48 body conv on a whole 339 x 510 image
        g = torch.Generator().manual_seed(4)
        h, w = 339, 510
        x = (torch.rand(1, h, w, 48, generator=g) * 2).half().to(dev)
        r = (torch.rand(1, h, w, 48, generator=g) * 2).half().to(dev)
        wt = (torch.randn(48, 48, 3, 3, generator=g) * 0.02).to(dev)
        b = torch.zeros(48, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        wpk = K.f16_pack_weights(wt)
        out = torch.empty_like(x)
        act = h * w * 48 * 2
        flop = 2.0 * h * w * 48 * 48 * 9
        for epi, kw, nbytes in (("relu", {"relu": True}, 2 * act), ("res0", {"res0": r}, 3 * act)):
            fn = lambda: K.f16_conv3x3(x, wpk, b, flag, out=out, **kw)   # noqa: E731
            fn()
            us = _median_ms(fn, a.reps, inner=20) * 1e3
            print(json.dumps({"kernel": "f16 conv 48->48 339x510 " + epi, "us": round(us, 2),
                              "hbm_bytes_MB": round(nbytes / 1e6, 2),
                              "hbm_roofline_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2),
                              "frac_hbm_roofline": round(nbytes / HBM_BYTES_PER_S * 1e6 / us, 3),
                              "f16_roofline_us": round(flop / F16_FLOPS * 1e6, 2),
                              "frac_f16_roofline": round(flop / F16_FLOPS * 1e6 / us, 3)}), flush=True)


if __name__ == "__main__":
    main()
