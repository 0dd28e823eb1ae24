"""All-exit inference against M separate LarvaLeg runs: M4B4 (4 modules of 4 residual blocks), one 339 x 510 image (eager:
autograd.is_large_inference) and the captured 16 x 3 x 48 x 48 batch, fp32 and fp16.  Variants, per shape and precision:
  (a) the M LarvaLeg --leg=k plugins one after another (what the curve over the exits cost before),
  (b) all exits from one forward, the legs launched one by one,
  (c) all exits from one forward, the legs as batched launches (conv3x3_batch / the fp16 job launches),
  (d) a plain upscale (the last exit alone): what the other M - 1 exits cost on top.
Then the two fp16 job launches alone against M single launches, at both shapes.
The variants of one shape run in alternation, `--rounds` rounds of `--reps` timed calls after a warm-up round; a value
is the median over the rounds of each round's median, its spread the least and the largest round median.  Device events
around a call that ends on the stream; nothing else runs on the device in between.  Prints one JSON line per
measurement.  Usage: python tools/time_exits.py [--reps 20] [--rounds 5]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M = 4


def _round_ms(fn, reps, inner=1):
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


def _alternate(variants, reps, rounds, inner=1):
    """{name: fn} -> {name: {"ms", "lo", "hi"}}: one warm-up round, then `rounds` rounds in which every variant takes its
    turn."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            meds[k].append(_round_ms(fn, reps, inner))
    return {k: {"ms": round(float(np.median(v)), 4), "lo": round(min(v), 4), "hi": round(max(v), 4)} for k, v in meds.items()}


def _model(name, precision, extra=()):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=%d" % M, "--num_blocks=4,4,4,4", "--precision=" + precision] + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    m.strict_graph = True
    return m


def _exits_model(precision, batched):
    m = _model("LarvaNet", precision)
    m.batch_exit_legs = batched
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from larvanet_amd import kernels as K
    from larvanet_amd.infer_graphs import Form
    dev = torch.device("cuda", 0)
    image = (torch.rand(1, 3, 339, 510, generator=torch.Generator().manual_seed(2)) * 255).to(dev)
    batch = (torch.rand(16, 3, 48, 48, generator=torch.Generator().manual_seed(3)) * 255).to(dev)
    with torch.no_grad():
        for prec in ("fp32", "fp16"):
            legs = [_model("LarvaLeg", prec, ("--leg=%d" % k,)) for k in range(1, M + 1)]
            one_by_one, batched, plain = _exits_model(prec, False), _exits_model(prec, True), _model("LarvaNet", prec)
            for shape, x in (("image_339x510", image), ("batch_16x3x48x48_captured", batch)):
                variants = {
                    "a_separate_larvaleg_runs": lambda: [m._infer(x) for m in legs],
                    "b_all_exits_legs_one_by_one": lambda: one_by_one._eager_or_graph(x, Form(exits=True)),
                    "c_all_exits_batched_legs": lambda: batched._eager_or_graph(x, Form(exits=True)),
                    "d_plain_upscale": lambda: plain._infer(x),
                }
                res = _alternate(variants, a.reps, a.rounds)
                captured = {"b": bool(one_by_one._infer_graphs_ex), "c": bool(batched._infer_graphs_ex)}
                line = {"shape": shape, "precision": prec, "exits": M, "captured": captured}
                line.update(res)
                line["a_over_c"] = round(res["a_separate_larvaleg_runs"]["ms"] / res["c_all_exits_batched_legs"]["ms"], 3)
                line["b_over_c"] = round(res["b_all_exits_legs_one_by_one"]["ms"] / res["c_all_exits_batched_legs"]["ms"], 3)
                line["c_over_d"] = round(res["c_all_exits_batched_legs"]["ms"] / res["d_plain_upscale"]["ms"], 3)
                if prec == "fp16":
                    line["fp16_overflowed"] = any(m.fp16_overflowed() for m in legs + [one_by_one, batched, plain])
                print(json.dumps(line), flush=True)

        # the two fp16 job launches alone against M single launches
        g = torch.Generator().manual_seed(4)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        for n, h, w in ((1, 339, 510), (16, 48, 48)):
            srcs = [(torch.rand(n, h, w, 48, generator=g) * 2).half().to(dev) for _ in range(M)]
            wpk = [K.f16_pack_weights((torch.randn(48, 48, 3, 3, generator=g) * 0.02).to(dev)) for _ in range(M)]
            bias = [torch.zeros(48, device=dev) for _ in range(M)]
            base = (torch.rand(n, 3, 4 * h, 4 * w, generator=g) * 255).to(dev)
            outs16 = torch.empty((M, n, h, w, 48), dtype=torch.float16, device=dev)
            out32 = torch.empty((M, n, 3, 4 * h, 4 * w), dtype=torch.float32, device=dev)
            out8 = torch.empty((M, n, 4 * h, 4 * w, 3), dtype=torch.uint8, device=dev)
            variants = {
                "relu_single_x%d" % M: lambda: [K.f16_conv3x3(srcs[j], wpk[j], bias[j], flag, relu=True, out=outs16[j]) for j in range(M)],
                "relu_jobs": lambda: K.f16_conv3x3_jobs(srcs, wpk, bias, flag, relu=True, out=outs16),
                "shuffle_f32_single_x%d" % M: lambda: [K.f16_conv3x3_shuffle_base(srcs[j], wpk[j], bias[j], base) for j in range(M)],
                "shuffle_f32_jobs": lambda: K.f16_conv3x3_shuffle_base_jobs(srcs, wpk, bias, base, out=out32),
                "shuffle_u8_single_x%d" % M: lambda: [K.f16_conv3x3_shuffle_base_u8(srcs[j], wpk[j], bias[j], base, flag, out=out8[j])
                                                      for j in range(M)],
                "shuffle_u8_jobs": lambda: K.f16_conv3x3_shuffle_base_jobs(srcs, wpk, bias, base, flag, u8=True, out=out8),
            }
            res = _alternate(variants, a.reps, a.rounds, inner=10)
            line = {"kernel": "fp16 leg launches %dx%dx%d, %d legs" % (n, h, w, M)}
            line.update({k: {"us": round(v["ms"] * 1e3, 2), "lo": round(v["lo"] * 1e3, 2), "hi": round(v["hi"] * 1e3, 2)}
                         for k, v in res.items()})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
