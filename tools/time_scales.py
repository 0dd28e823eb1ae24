"""Step and whole-image times of the network at x2, x3 and x4: the captured training step at 16 x 3 x 48 x 48 with
M4B4 (4 modules of 4 residual blocks) and the inference forward of one 339 x 510 image (a DIV2K x4 validation size).
Prints one JSON line per scale.  Usage: python tools/time_scales.py [--steps 30] [--scales 2,3,4]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _NoVal:
    def get_num_images(self):
        return 0


def _median_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--scales", type=str, default="2,3,4")
    a = ap.parse_args()
    from larvanet_amd.models import LarvaNet as V1
    dev = torch.device("cuda", 0)
    for s in (int(v) for v in a.scales.split(",")):
        m = V1.create_model()
        m.parse_args(["--num_modules=4", "--num_blocks=4,4,4,4"])
        torch.manual_seed(0)
        m.prepare(is_training=True, scales=[s])
        m.strict_graph = True
        g = torch.Generator().manual_seed(1)
        x = (torch.rand(16, 3, 48, 48, generator=g) * 255).to(dev)
        truth = (torch.rand(16, 3, 48 * s, 48 * s, generator=g) * 255).to(dev)
        args = types.SimpleNamespace(train_path="/tmp")
        for _ in range(5):
            m.train_step_larva(args, _NoVal(), x, truth)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            m.train_step_larva(args, _NoVal(), x, truth)
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
        img = [np.random.default_rng(2).random((3, 339, 510)).astype(np.float32) * 255]
        with torch.no_grad():
            m.upscale_tensor(img)
            inp = m._to_input_tensor(img)
            infer_ms = _median_ms(lambda: m._infer(inp), 10)
        print(json.dumps({"scale": s, "train_step_ms_16x48x48_M4B4": round(step_ms, 4),
                          "infer_ms_339x510": round(infer_ms, 4), "graph": bool(m.use_hip_graph)}), flush=True)


if __name__ == "__main__":
    main()
