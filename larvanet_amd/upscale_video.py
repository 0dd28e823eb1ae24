"""Video upscaler: 8-bit planar YUV 4:2:0 frames in, the upscaled frames out, as a Y4M (YUV4MPEG2) stream or a headerless
.yuv file; `-` is stdin / stdout, so it sits between two ffmpeg processes (the package never calls ffmpeg itself):

    ffmpeg -i in.mp4 -f yuv4mpegpipe -pix_fmt yuv420p - | \\
    python -m larvanet_amd.upscale_video --model=LarvaNet --num_modules=4 --num_blocks=4,4,4,4 --restore_path=model.pth \\
        --input - --output - [--precision fp16] [--self_ensemble] [--matrix bt709] [--range limited|full] \\
        [--output_size 1920x1080] | \\
    ffmpeg -i - out.mp4

    python -m larvanet_amd.upscale_video ... --input in.yuv --width 510 --height 339 --output out.yuv

The frames stay YUV end to end (pipeline.upscale_yuv_stream): 1.5 bytes per pixel cross the host link each way, the two
colour conversions run on the device, and no pass over a frame happens on the host.  One thread reads frames, one writes
them; the stream runs between them.  A file whose name ends in .y4m, and stdin / stdout unless --width and --height are
given, is a Y4M stream: its header gives the size, and XCOLORRANGE=FULL selects full range unless --range is given.  The
output header carries the upscaled size and the input's F, A, C and X tags.  Only 8-bit 4:2:0 is processed (y4m.py lists
what is refused), always as centre-sited chroma.

--output_size WxH writes frames of exactly that size instead of the network's integer multiple: the upscaled RGB image is
resized on the device (Pillow's bicubic, byte for byte: image_utils.resize_u8) before it is converted back, so only
target-sized frames cross the host link.  The Y4M header carries the new W and H; a raw .yuv output simply has that size.
An axis may shrink by at most 4 from the network's output."""
import argparse
import importlib
import os
import queue
import sys
import threading
import time

from . import y4m
from .image_utils import YUV_MATRICES, check_resize
from .upscale_images import parsed_output_size, prepare_model

_END = object()


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--model", type=str, default="LarvaNet")
    p.add_argument("--scale", type=int, default=4)
    p.add_argument("--cuda_device", type=str, default=None)
    p.add_argument("--restore_path", type=str, default=None,
                   help="checkpoint (bare state_dict); omitted = freshly initialised weights")
    p.add_argument("--restore_target", type=str)
    p.add_argument("--restore_global_step", type=int, default=0)
    p.add_argument("--input", type=str, required=True, help="a .y4m or .yuv file, or - for stdin")
    p.add_argument("--output", type=str, required=True, help="a .y4m or .yuv file, or - for stdout")
    p.add_argument("--matrix", type=str, default="bt601", choices=sorted(YUV_MATRICES))
    p.add_argument("--range", type=str, default=None, choices=["limited", "full"],
                   help="default: what the Y4M header's XCOLORRANGE says, else limited")
    p.add_argument("--width", type=int, default=None, help="frame width of a headerless .yuv input")
    p.add_argument("--height", type=int, default=None, help="frame height of a headerless .yuv input")
    p.add_argument("--depth", type=int, default=2, help="frames in flight on the device (1 = no copy overlap)")
    p.add_argument("--output_size", type=str, default=None,
                   help="WIDTHxHEIGHT of the written frames (e.g. 1920x1080): the upscaled frame is resized on the device "
                        "(bicubic, Pillow's bytes); default: scale times the input size")
    return p


def output_size_of(args, size=None):
    """--output_size as (height, width), or None; ValueError for a malformed value and, with the input's `size` = (width,
    height) known, for a target an axis of the upscaled frame would shrink by more than 4 to reach."""
    target = parsed_output_size(args)
    if target is not None and size is not None:
        check_resize(size[1] * args.scale, size[0] * args.scale, *target)
    return target


def output_header(header, scale, output_size=None):
    """The Y4M header of the output: the input's with W and H of the upscaled, or the --output_size, frame."""
    if output_size is None:
        return header.scaled(scale)
    return header.resized(output_size[1], output_size[0])


def input_is_y4m(args):
    """A name ending in .y4m is Y4M, one ending in .yuv is headerless; anything else (stdin) is headerless exactly when
    --width and --height are given."""
    name = args.input.lower()
    if name.endswith(".y4m"):
        return True
    if name.endswith(".yuv"):
        return False
    return args.width is None and args.height is None


def check_args(args):
    """Refusals that need neither the input nor a device."""
    if args.depth < 1:
        raise ValueError("larvanet_amd.upscale_video: --depth must be >= 1")
    if args.scale not in (2, 3, 4):
        raise ValueError("larvanet_amd.upscale_video: --scale must be 2, 3 or 4, got %d" % args.scale)
    output_size_of(args)
    if (args.width is None) != (args.height is None):
        raise ValueError("larvanet_amd.upscale_video: --width and --height go together")
    if input_is_y4m(args):
        if args.width is not None:
            raise ValueError("larvanet_amd.upscale_video: a Y4M input carries its own size; drop --width and --height")
    else:
        if args.width is None:
            raise ValueError("larvanet_amd.upscale_video: a headerless .yuv input needs --width and --height")
        if args.width < 1 or args.height < 1:
            raise ValueError("larvanet_amd.upscale_video: --width and --height must be >= 1")


def open_input(args, stream=None):
    """-> (Header or None, (width, height), full_range, frame generator, the stream to close).  Reads the Y4M header:
    everything this package cannot process is refused here, before any device work."""
    if stream is None:
        stream = sys.stdin.buffer if args.input == "-" else open(args.input, "rb")
    if input_is_y4m(args):
        header = y4m.read_header(stream)
        size = (header.width, header.height)
        frames = y4m.read_frames(stream, header)
        said = header.full_range
    else:
        header, size, said = None, (args.width, args.height), None
        frames = y4m.read_raw_frames(stream, *size)
    full = (args.range == "full") if args.range is not None else bool(said)
    return header, size, full, frames, stream


def _reader(frames, q, stop):
    try:
        for f in frames:
            while not stop.is_set():
                try:
                    q.put(f, timeout=0.1)
                    break
                except queue.Full:
                    pass
            if stop.is_set():
                return
        q.put(_END)
    except BaseException as e:   # (a truncated frame: handed to the main thread, which raises it at that frame's turn)
        q.put(e)


def _writer(out, is_y4m, q, failed):
    f = None
    try:
        while True:
            f = q.get()
            if f is _END:
                return
            if is_y4m:
                y4m.write_frame(out, f)
            else:
                out.write(memoryview(f))
    except BaseException as e:   # (a closed pipe, a full disk: raised by the main thread)
        failed.append(e)
        while f is not _END:   # (keep draining so the main thread never blocks on a full queue)
            f = q.get()


def _queued(q):
    while True:
        f = q.get()
        if f is _END:
            return
        if isinstance(f, BaseException):
            raise f
        yield f


def run(model, args, header, size, full_range, frames, out_raw):
    """The reader thread, pipeline.upscale_yuv_stream and the writer thread -> the number of frames written."""
    from . import pipeline
    target = output_size_of(args, size)
    if header is not None:
        y4m.write_header(out_raw, output_header(header, args.scale, target))
    q_in, q_out = queue.Queue(maxsize=args.depth + 2), queue.Queue(maxsize=args.depth + 2)
    stop, failed = threading.Event(), []
    reader = threading.Thread(target=_reader, args=(frames, q_in, stop), daemon=True)
    writer = threading.Thread(target=_writer, args=(out_raw, header is not None, q_out, failed), daemon=True)
    reader.start()
    writer.start()
    count = 0
    try:
        for hr in pipeline.upscale_yuv_stream(model, _queued(q_in), args.scale, size[0], size[1], matrix=args.matrix,
                                              full_range=full_range, depth=args.depth, output_size=target):
            if failed:
                raise failed[0]
            q_out.put(hr)
            count += 1
    finally:
        stop.set()
        q_out.put(_END)
        writer.join()
    if failed:
        raise failed[0]
    out_raw.flush()
    return count


def main(argv=None):
    args, remaining = build_parser().parse_known_args(argv)
    check_args(args)
    log = sys.stderr   # (stdout may be the video)
    if args.cuda_device is not None and "LOCAL_RANK" not in os.environ:
        os.environ["HIP_VISIBLE_DEVICES"] = args.cuda_device
    header, size, full_range, frames, in_stream = open_input(args)
    try:
        if header is not None and header.siting_warning():
            print(header.siting_warning(), file=log)
        target = output_size_of(args, size)   # (a ratio beyond 4: refused with the header read and no frame yet)
        out_w, out_h = (size[0] * args.scale, size[1] * args.scale) if target is None else (target[1], target[0])
        print("video: %d x %d -> %d x %d, %s, %s range" % (size[0], size[1], out_w, out_h,
                                                          args.matrix, "full" if full_range else "limited"), file=log)
        model = prepare_model(args, remaining, log, importlib.import_module)
        out_raw = sys.stdout.buffer if args.output == "-" else open(args.output, "wb")
        try:
            t0 = time.perf_counter()
            count = run(model, args, header, size, full_range, frames, out_raw)
            dt = time.perf_counter() - t0
        finally:
            if args.output != "-":
                out_raw.close()
    finally:
        if args.input != "-":
            in_stream.close()
    print("finished: %d frames, %.2f frames per second" % (count, count / dt if dt > 0 else 0.0), file=log)
    return count


if __name__ == "__main__":
    main()
