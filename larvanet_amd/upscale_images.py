"""Folder upscaler: counterpart of the reference's get_sr.py.  Every *.png of --input_path goes through the network and
is written as <output_path>/<stem>.png.

    python -m larvanet_amd.upscale_images --model=LarvaNet --num_modules=4 --num_blocks=4,4,4,4 \\
        --restore_path=model.pth --input_path=LR --output_path=SR [--precision fp16] [--self_ensemble]
        [--io_threads 8] [--all_exits] [--output_size 1920x1080] [--keep_alpha]

--output_size WxH writes every image at exactly that size instead of the network's integer multiple: the upscaled image is
resized on the device before it leaves it (Pillow's bicubic, byte for byte: image_utils.resize_u8).  An axis may shrink
by at most 4 from the network's output; the PNG headers are checked against that before any image is decoded.

--keep_alpha keeps transparency: a file whose mode carries alpha (RGBA, LA, PA, or P / RGB / L with a transparency entry)
is decoded as straight-alpha RGBA, its alpha plane goes through the network beside the colour (as a grey image, merged on
the device: model.upscale_rgba_u8) and it is written as an RGBA PNG; an image whose alpha is 255 everywhere costs what an
RGB image costs.  Every other file goes the RGB way.  Without the flag alpha is dropped, as before.  The colour under
fully transparent pixels is used as it is: garbage there rings into visible neighbours.  Not together with --all_exits.

--all_exits writes every exit of the multi-exit network from ONE forward pass per image, as <stem>_exit<k>.png with k
counted from 1 like --leg (model.upscale_exits_u8): the head and the bodies run once, the legs go out together.  It runs
image by image, outside the stream below.

--self_ensemble (a model flag, like --precision) writes the geometric self-ensemble: the mean of the eight flips /
transposes of each image run through the network and mapped back, merged on the device.

The images stay 8-bit end to end (pipeline.upscale_stream over model._infer_u8_images): PNGs are decoded and encoded by a
thread pool around the stream, a quarter of the float path's bytes cross the host link, and the copies of neighbouring
images run beside the forward.  Under torchrun file i goes to rank i mod world, as validate.py shards.  The
reference's --chop_forward is not carried over (approximate by design; image_utils has exact bands)."""
import argparse
import collections
import concurrent.futures
import importlib
import os
import time

import numpy as np

from . import dist as ldist
from .image_utils import check_resize, parse_output_size


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
    p.add_argument("--output_path", type=str, default="SR")
    p.add_argument("--io_threads", type=int, default=None,
                   help="PNG decode / encode threads; default and upper limit: this rank's share of the host's cores")
    p.add_argument("--depth", type=int, default=2, help="images in flight on the device (1 = no copy overlap)")
    p.add_argument("--all_exits", action="store_true",
                   help="write every exit's image from one forward pass per image, as <stem>_exit<k>.png (k from 1, like "
                        "--leg); runs image by image, not through the copy-overlapped stream; LarvaNet / LarvaLeg only")
    p.add_argument("--output_size", type=str, default=None,
                   help="WIDTHxHEIGHT of the written images (e.g. 1920x1080): the upscaled image is resized on the device "
                        "(bicubic, Pillow's bytes); default: scale times the input size")
    p.add_argument("--keep_alpha", action="store_true",
                   help="files with an alpha channel or a transparency entry are upscaled and written as RGBA (the alpha "
                        "plane goes through the network too); default: alpha is dropped")
    return p


def check_keep_alpha(args):
    """ValueError for --keep_alpha together with --all_exits (there is no all-exit RGBA)."""
    if args.keep_alpha and args.all_exits:
        raise ValueError("larvanet_amd.upscale_images: --keep_alpha together with --all_exits is not supported")


def parsed_output_size(args):
    """--output_size as (height, width), or None where the flag was not given; ValueError for a malformed value."""
    return None if args.output_size is None else parse_output_size(args.output_size)


def output_size_of(args):
    """--output_size as (height, width), or None; ValueError for a malformed value or together with --all_exits."""
    if args.output_size is not None and args.all_exits:
        raise ValueError("larvanet_amd.upscale_images: --output_size together with --all_exits is not supported")
    return parsed_output_size(args)


def prepare_model(args, remaining, log=None, import_module=None):
    """The plugin --model names, made from the arguments the driver's own parser left over (`remaining`), prepared for
    inference at --scale and restored from --restore_path: what upscale_images, upscale_video and evaluate do alike.
    log: the file the progress lines go to (None: stdout).  import_module: what loads the plugin's module, by default this
    module's importlib.import_module as it is when called; upscale_video hands in its own, which its tests replace to show
    that no model is loaded before the input has been checked."""
    print("prepare model - %s" % args.model, file=log)
    model = (import_module or importlib.import_module)("larvanet_amd.models." + args.model).create_model()
    _, remaining = model.parse_args(remaining)
    model.prepare(is_training=False, scales=[args.scale], global_step=args.restore_global_step)
    if remaining:
        print("WARNING: found unhandled arguments: %s" % remaining, file=log)
    if args.restore_path is not None:
        model.restore(ckpt_path=args.restore_path, target=args.restore_target)
        print("restored the model", file=log)
    return model


def png_size(path):
    """(height, width) from the file's header, without decoding it."""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


def list_pngs(input_path):
    """File names of input_path ending in .png (any letter case), sorted."""
    return sorted(f for f in os.listdir(input_path) if f.lower().endswith(".png"))


def shard(files, rank, world):
    return list(files[rank::world])


def output_name(image_name):
    return os.path.splitext(image_name)[0] + ".png"


def exit_output_name(image_name, exit_index):
    """<stem>_exit<k>.png for the 0-based exit_index: k counts from 1, like --leg."""
    return "%s_exit%d.png" % (os.path.splitext(image_name)[0], exit_index + 1)


def io_threads(requested):
    """--io_threads clamped to [1, this rank's cores]; OMP_NUM_THREADS, where set, lowers the limit further."""
    cap = ldist.host_threads()
    try:
        cap = max(1, min(cap, int(os.environ.get("OMP_NUM_THREADS", "") or cap)))
    except ValueError:
        pass
    return cap if requested is None else max(1, min(int(requested), cap))


def read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def carries_alpha(im):
    """Does this opened PIL image carry transparency: an alpha band (RGBA, LA, PA) or a `transparency` entry (P, RGB, L)?"""
    return im.mode in ("RGBA", "LA", "PA") or "transparency" in im.info


def read_image(path, keep_alpha=False):
    """read_rgb; with keep_alpha a file that carries transparency is decoded as (H, W, 4) straight-alpha RGBA instead."""
    from PIL import Image
    with Image.open(path) as im:
        mode = "RGBA" if keep_alpha and carries_alpha(im) else "RGB"
        return np.ascontiguousarray(np.asarray(im.convert(mode), dtype=np.uint8))


def write_rgb(image_hwc_uint8, path):
    """(H, W, 3) -> an RGB PNG, (H, W, 4) -> an RGBA PNG."""
    from PIL import Image
    Image.fromarray(image_hwc_uint8).save(path)


def _prefetched(pool, fn, items, ahead):
    """fn(item) for every item in order, at most `ahead` of them running or waiting in the pool."""
    pending = collections.deque()
    for item in items:
        pending.append(pool.submit(fn, item))
        if len(pending) >= ahead:
            yield pending.popleft().result()
    while pending:
        yield pending.popleft().result()


def main(argv=None):
    args, remaining = build_parser().parse_known_args(argv)
    check_keep_alpha(args)
    target = output_size_of(args)
    if args.cuda_device is not None and "LOCAL_RANK" not in os.environ:
        os.environ["HIP_VISIBLE_DEVICES"] = args.cuda_device
    rank, world = ldist.init_from_env()
    ldist.limit_host_threads()
    names = list_pngs(args.input_path)
    print("data: %d images are prepared" % len(names))
    mine = shard(names, rank, world)
    os.makedirs(args.output_path, exist_ok=True)
    if not mine:
        print("finished")
        return {}
    if target is not None:   # (a ratio beyond 4: refused from the headers, before any image is decoded)
        for name in mine:
            in_h, in_w = png_size(os.path.join(args.input_path, name))
            check_resize(in_h * args.scale, in_w * args.scale, *target)

    from . import pipeline
    model = prepare_model(args, remaining)
    if args.all_exits:
        model._check_exits()   # (a model without per-body exits or --self_ensemble: refused before any image is read)
    print("begin super-resolution")
    threads = io_threads(args.io_threads)
    durations = {}
    writes = collections.deque()
    if args.all_exits:
        with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
            decoded = _prefetched(pool, read_rgb, [os.path.join(args.input_path, n) for n in mine], ahead=threads + 1)
            last = time.perf_counter()
            for i, image in enumerate(decoded):
                outs = model.upscale_exits_u8([image], args.scale)
                durations[mine[i]] = time.perf_counter() - last
                for k in range(outs.shape[0]):
                    writes.append(pool.submit(write_rgb, outs[k, 0], os.path.join(args.output_path, exit_output_name(mine[i], k))))
                while len(writes) > threads:
                    writes.popleft().result()
                print("%d/%d, %s, %d exits, duration: %.4fs" % (i + 1, len(mine), mine[i], outs.shape[0], durations[mine[i]]))
                last = time.perf_counter()
            for w in writes:
                w.result()
        print("finished")
        print("- average duration: %.4fs" % np.mean(list(durations.values())))
        return durations
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        read = (lambda path: read_image(path, True)) if args.keep_alpha else read_rgb
        decoded = _prefetched(pool, read, [os.path.join(args.input_path, n) for n in mine], ahead=threads + args.depth)
        last = time.perf_counter()
        for i, out in enumerate(pipeline.upscale_stream(model, decoded, args.scale, depth=args.depth, output_size=target,
                                                        keep_alpha=args.keep_alpha)):
            now = time.perf_counter()
            durations[mine[i]] = now - last   # (time between results: the stream's rate, not one image's latency)
            writes.append(pool.submit(write_rgb, out, os.path.join(args.output_path, output_name(mine[i]))))
            while len(writes) > threads:   # (bounds the results waiting to be encoded)
                writes.popleft().result()
            print("%d/%d, %s, duration: %.4fs" % (i + 1, len(mine), mine[i], durations[mine[i]]))
            last = time.perf_counter()
        for w in writes:
            w.result()
    print("finished")
    print("- average duration: %.4fs" % np.mean(list(durations.values())))
    return durations


if __name__ == "__main__":
    main()
