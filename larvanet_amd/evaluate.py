"""Benchmark evaluator: counterpart of the reference's test.py.  Every truth image of --truth_path is paired with its
low-resolution input of --input_path, upscaled, and scored on the device: PSNR and SSIM.

    python -m larvanet_amd.evaluate --model=LarvaNet --num_modules=4 --num_blocks=4,4,4,4 --restore_path=model.pth \\
        --input_path=LR --truth_path=HR [--output_path=SR] [--channel y|rgb] [--shave N] [--no_ssim] [--log FILE]
        [--precision fp16] [--self_ensemble] [--io_threads 8] [--depth 2] [--all_exits]
    python -m larvanet_amd.evaluate ... --truth_path=HR --lr_from_truth        (no LR folder: --input_path is ignored)

--lr_from_truth makes every input on the device from its truth image: the bicubic decimation by --scale in the MATLAB
imresize convention (kernels.bicubic_down_u8), the degradation SR benchmarks are prepared with.  The results equal
those over the folder `python -m larvanet_amd.downscale_images --suffix` writes.

--self_ensemble (a model flag, like --precision) scores the geometric self-ensemble, the "+" column of SR tables: the
mean of the eight flips / transposes of each image run through the network and mapped back, merged on the device.

--all_exits scores EVERY exit of the multi-exit network from one forward pass per image (model.evaluate_exits_u8_tensor:
the head and the bodies run once, the legs go out together): per image one result line per exit ("exit k", k from 1
like --leg), at the end one average line per exit -- the curve "exit k: this PSNR / SSIM at this cost".  With
--output_path it writes <stem>_exit<k>.png.  It runs image by image, not through pipeline.evaluate_stream.

The two protocols super-resolution results are reported under:
    --channel y (the default, with the default shave = scale)   Y-channel PSNR / SSIM with a border of `scale` pixels
                                                                 shaved off: Set5, Set14, BSD100, Urban100, Manga109
    --channel rgb --shave 0                                      RGB PSNR and multichannel SSIM on whole images: DIV2K
Truth <stem>.png pairs with input <stem>.png or <stem>x<scale>.png (the DIV2K naming).  The images stay 8-bit and the
metrics are computed where both images are (pipeline.evaluate_stream, csrc/larva_metrics.hip): per image a 64-byte
record comes back, or the upscaled image too when --output_path asks for it.  Under torchrun file i goes to rank i mod
world and the sums are all-reduced, as validate.py does."""
import argparse
import collections
import concurrent.futures
import os
import time

from . import dist as ldist
from .upscale_images import (_prefetched, exit_output_name, io_threads, list_pngs, output_name, prepare_model, read_rgb, shard,
                             write_rgb)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--model", type=str, default="LarvaNet")
    p.add_argument("--scale", type=int, default=4)
    p.add_argument("--cuda_device", type=str, default=None)
    p.add_argument("--restore_path", type=str, default=None,
                   help="checkpoint (bare state_dict); omitted = freshly initialised weights")
    p.add_argument("--restore_target", type=str)
    p.add_argument("--restore_global_step", type=int, default=0)
    p.add_argument("--input_path", type=str, default="LR")
    p.add_argument("--truth_path", type=str, default="HR")
    p.add_argument("--lr_from_truth", action="store_true",
                   help="make each input from its truth image on the device (bicubic, MATLAB convention); ignores --input_path")
    p.add_argument("--output_path", type=str, default=None, help="where to write the upscaled images; omitted = nowhere")
    p.add_argument("--channel", type=str, default="y", choices=("y", "rgb"),
                   help="y: BT.601 luma plane; rgb: the three colour planes (SSIM: their mean)")
    p.add_argument("--shave", type=int, default=None, help="border pixels left out on every side; default: the scale")
    p.add_argument("--no_ssim", action="store_true", help="PSNR only")
    p.add_argument("--log", type=str, default=None, help="file that receives the printed result lines")
    p.add_argument("--io_threads", type=int, default=None,
                   help="PNG decode / encode threads; default and upper limit: this rank's share of the host's cores")
    p.add_argument("--depth", type=int, default=2, help="images in flight on the device (1 = no copy overlap)")
    p.add_argument("--all_exits", action="store_true",
                   help="score every exit from one forward pass per image: one result line per exit and image, one average "
                        "line per exit; --output_path then gets <stem>_exit<k>.png (k from 1, like --leg).  Runs image by "
                        "image over evaluate_exits_u8_tensor: it is NOT wired into pipeline.evaluate_stream (no copy "
                        "overlap, --depth is ignored) and runs on one rank.  LarvaNet / LarvaLeg only, not with "
                        "--self_ensemble")
    return p


def pair_files(truth_names, input_names, scale):
    """[(truth name, input name)] for every truth name, in order: the input is the file with the truth's stem, or
    <stem>x<scale>, and a .png extension of any letter case.  A truth without an input is a FileNotFoundError naming it."""
    by_stem = {}
    for name in input_names:
        by_stem.setdefault(os.path.splitext(name)[0], name)
    pairs = []
    for name in truth_names:
        stem = os.path.splitext(name)[0]
        found = by_stem.get(stem) or by_stem.get("%sx%d" % (stem, scale))
        if found is None:
            raise FileNotFoundError("larvanet_amd.evaluate: no input image for truth %s (looked for %s.png and %sx%d.png)"
                                    % (name, stem, stem, scale))
        pairs.append((name, found))
    return pairs


def result_line(scale, index, count, result, exit_index=None):
    """exit_index: the 0-based exit of an --all_exits run, printed 1-based like --leg; None = the line as it always was."""
    line = "x%d, %d/%d, " % (scale, index, count) + ("" if exit_index is None else "exit %d, " % (exit_index + 1))
    line += "psnr=%.4f" % result["psnr"]
    return line if result["ssim"] is None else line + ", ssim=%.4f" % result["ssim"]


def _evaluate_all_exits(model, args, mine, say, results):
    """The --all_exits loop: image by image over model.evaluate_exits_u8_tensor -> per-exit sums [{"psnr", "ssim",
    "count"}] (results[name] becomes the list of the image's per-exit records)."""
    import torch

    from . import kernels as K
    threads = io_threads(args.io_threads)
    keep = args.output_path is not None
    writes = collections.deque()
    sums = []

    def read_pair(names):
        truth = read_rgb(os.path.join(args.truth_path, names[0]))
        return (None if names[1] is None else read_rgb(os.path.join(args.input_path, names[1]))), truth

    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        for i, (image, truth) in enumerate(_prefetched(pool, read_pair, mine, ahead=threads + 1)):
            truth_dev = torch.from_numpy(truth).to(model.device)
            if image is None:   # --lr_from_truth: the input is made from the truth on the device
                x = K.bicubic_down_u8(truth_dev, model.scale).unsqueeze(0)
            else:
                x = torch.from_numpy(image).to(model.device).unsqueeze(0)
            got = model.evaluate_exits_u8_tensor(x, truth_dev.unsqueeze(0), shave=args.shave, channel=args.channel,
                                                 ssim=not args.no_ssim, return_images=keep)
            per_exit, images = (got[0][0], got[1].cpu().numpy()) if keep else (got[0], None)
            results[mine[i][0]] = per_exit
            if not sums:
                sums = [{"psnr": 0.0, "ssim": 0.0, "count": 0.0} for _ in per_exit]
            for k, result in enumerate(per_exit):
                sums[k]["psnr"] += result["psnr"]
                sums[k]["ssim"] += result["ssim"] or 0.0
                sums[k]["count"] += 1
                say(result_line(args.scale, i + 1, len(mine), result, exit_index=k))
                if keep:
                    writes.append(pool.submit(write_rgb, images[k, 0],
                                              os.path.join(args.output_path, exit_output_name(mine[i][0], k))))
            while len(writes) > threads:
                writes.popleft().result()
        for w in writes:
            w.result()
    return sums


def main(argv=None):
    args, remaining = build_parser().parse_known_args(argv)
    if args.cuda_device is not None and "LOCAL_RANK" not in os.environ:
        os.environ["HIP_VISIBLE_DEVICES"] = args.cuda_device
    if args.shave is not None and args.shave < 0:
        raise ValueError("larvanet_amd.evaluate: --shave must be >= 0")
    rank, world = ldist.init_from_env()
    ldist.limit_host_threads()
    if args.all_exits and world > 1:
        raise ValueError("larvanet_amd.evaluate: --all_exits runs on one rank (it is not sharded over torchrun ranks)")
    if args.lr_from_truth:
        pairs = [(name, None) for name in list_pngs(args.truth_path)]
    else:
        pairs = pair_files(list_pngs(args.truth_path), list_pngs(args.input_path), args.scale)
    print("data: %d images are prepared" % len(pairs))
    mine = shard(pairs, rank, world)
    if args.output_path is not None:
        os.makedirs(args.output_path, exist_ok=True)
    lines = []

    def say(line):
        print(line)
        lines.append(line)

    results = {}
    sums = {"psnr": 0.0, "ssim": 0.0, "count": 0.0}
    exit_sums = []
    device = "cuda" if ldist.active() else "cpu"   # (a rank with an empty shard still takes part in the sums)
    begin = time.perf_counter()
    if mine:   # (an empty shard launches nothing and prepares no model)
        from . import pipeline
        model = prepare_model(args, remaining)
        device = model.device
        if args.all_exits:
            model._check_exits()   # (a model without per-body exits or --self_ensemble: refused before any image is read)
        print("begin evaluation")
        threads = io_threads(args.io_threads)
        keep = args.output_path is not None
        writes = collections.deque()

        def read_pair(names):
            truth = read_rgb(os.path.join(args.truth_path, names[0]))
            return (None if names[1] is None else read_rgb(os.path.join(args.input_path, names[1]))), truth

        begin = time.perf_counter()
        if args.all_exits:   # (image by image, outside the stream)
            exit_sums = _evaluate_all_exits(model, args, mine, say, results)
        else:
            with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
                decoded = _prefetched(pool, read_pair, mine, ahead=threads + args.depth)
                stream = pipeline.evaluate_stream(model, decoded, args.scale, shave=args.shave, channel=args.channel,
                                                  ssim=not args.no_ssim, depth=args.depth, keep_images=keep)
                for i, item in enumerate(stream):
                    result, image = item if keep else (item, None)
                    if keep:
                        writes.append(pool.submit(write_rgb, image, os.path.join(args.output_path, output_name(mine[i][0]))))
                        while len(writes) > threads:   # (bounds the results waiting to be encoded)
                            writes.popleft().result()
                    results[mine[i][0]] = result
                    sums["psnr"] += result["psnr"]
                    sums["ssim"] += result["ssim"] or 0.0
                    sums["count"] += 1
                    say(result_line(args.scale, i + 1, len(mine), result))
                for w in writes:
                    w.result()
    duration = time.perf_counter() - begin
    if args.all_exits:
        m_exits = len(exit_sums)
        say("finished")
        for k in range(m_exits):
            total = exit_sums[k]   # (one rank: see the refusal above)
            mean = "- exit %d average psnr=%.4f" % (k + 1, total["psnr"] / total["count"])
            if not args.no_ssim:
                mean += ", ssim=%.4f" % (total["ssim"] / total["count"])
            say(mean)
        if m_exits:
            say("- duration: %.4fs" % duration)
        if args.log is not None and rank == 0:
            with open(args.log, "w") as f:
                f.write("\n".join(lines) + "\n")
        return results
    total = {k: ldist.allreduce_scalar_sum(v, device) for k, v in sums.items()}
    if total["count"]:
        say("finished")
        mean = "- average psnr=%.4f" % (total["psnr"] / total["count"])
        if not args.no_ssim:
            mean += ", ssim=%.4f" % (total["ssim"] / total["count"])
        say(mean)
        say("- duration: %.4fs" % duration)
    else:
        say("finished")
    if args.log is not None and rank == 0:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return results


if __name__ == "__main__":
    main()
