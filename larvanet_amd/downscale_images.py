"""Folder downscaler: the low-resolution side of an SR data set from its high-resolution images alone.  Every *.png
of --input_path is decimated by --scale (2, 3 or 4) and written as <output_path>/<stem>.png, or <stem>x<scale>.png with
--suffix: the DIV2K naming evaluate.pair_files and dataloaders/div2k_train_loader read.

    python -m larvanet_amd.downscale_images --input_path=HR --output_path=LR --scale=4 [--suffix] [--io_threads 8]
    python -m larvanet_amd.downscale_images --input_path=DIV2K_train_HR --output_path=LR_bicubic/X2 --scale=2 --suffix

The degradation is the one behind the numbers of SR tables: antialiased bicubic decimation in the MATLAB imresize
convention of the image cropped top-left to a multiple of the scale, in exact integers with one rounding
(kernels.bicubic_down_u8; image_utils.bicubic_downscale_u8 is the same on the host).  PNGs are decoded and encoded by a
thread pool around the device; under torchrun file i goes to rank i mod world, as upscale_images shards."""
import argparse
import collections
import concurrent.futures
import os

import numpy as np

from . import dist as ldist
from .upscale_images import _prefetched, io_threads, list_pngs, read_rgb, shard, write_rgb


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--input_path", type=str, default="HR")
    p.add_argument("--output_path", type=str, default="LR")
    p.add_argument("--scale", type=int, default=4, choices=(2, 3, 4))
    p.add_argument("--suffix", action="store_true", help="name the outputs <stem>x<scale>.png (the DIV2K naming)")
    p.add_argument("--cuda_device", type=str, default=None)
    p.add_argument("--io_threads", type=int, default=None,
                   help="PNG decode / encode threads; default and upper limit: this rank's share of the host's cores")
    return p


def output_name(image_name, scale, suffix):
    stem = os.path.splitext(image_name)[0]
    return "%sx%d.png" % (stem, scale) if suffix else stem + ".png"


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.cuda_device is not None and "LOCAL_RANK" not in os.environ:
        os.environ["HIP_VISIBLE_DEVICES"] = args.cuda_device
    rank, world = ldist.init_from_env()
    ldist.limit_host_threads()
    names = list_pngs(args.input_path)
    print("data: %d images are prepared" % len(names))
    mine = shard(names, rank, world)
    os.makedirs(args.output_path, exist_ok=True)
    written = []
    if mine:
        import torch
        from . import kernels as K
        if not torch.cuda.is_available():
            raise RuntimeError("larvanet_amd: downscale_images only runs on a HIP device (MI355X); there is no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
        threads = io_threads(args.io_threads)
        writes = collections.deque()
        with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
            decoded = _prefetched(pool, read_rgb, [os.path.join(args.input_path, n) for n in mine], ahead=threads + 2)
            for i, image in enumerate(decoded):
                K.bicubic_down_size(image.shape[0], image.shape[1], args.scale)   # (refused before anything is copied)
                small = K.bicubic_down_u8(torch.from_numpy(np.array(image)).to(device), args.scale).cpu().numpy()
                name = output_name(mine[i], args.scale, args.suffix)
                writes.append(pool.submit(write_rgb, small, os.path.join(args.output_path, name)))
                while len(writes) > threads:   # (bounds the results waiting to be encoded)
                    writes.popleft().result()
                written.append(name)
                print("%d/%d, %s -> %s, %d x %d" % (i + 1, len(mine), mine[i], name, small.shape[0], small.shape[1]))
            for w in writes:
                w.result()
    print("finished")
    return written


if __name__ == "__main__":
    main()
