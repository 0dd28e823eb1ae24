"""Images in, images out, with the host link hidden behind the forward.

upscale_stream() walks an iterable of uint8 (H, W, 3) images of any mix of sizes through model._infer_u8_images (the
uint8 form of the plugin's one grad-free dispatch; under --self_ensemble the device-side x8 ensemble) and yields the
uint8 (sH, sW, 3) results in input order.  Image i+1's host-to-device copy and image i-1's device-to-host copy run on
ONE extra stream beside image i's forward:

    copy stream     H2D(0) H2D(1) D2H(0) H2D(2) D2H(1) ...        (issue order; D2H(i) waits for forward i's event)
    compute stream         fwd(0)        fwd(1)        fwd(2) ...  (fwd(i) waits for H2D(i)'s event)

Every buffer a copy touches belongs to the pipeline: `depth` slots of flat pinned and device buffers, grown to the
largest image seen and viewed at each image's size.  The forward's result is copied (device to device, ~10 us for an
8 MB image) into the slot's own output buffer on the compute stream, because a replayed graph's output buffer is
overwritten by the next image of that shape and an eager result is the caching allocator's, which knows nothing of
the copy stream.  A slot is reused only after its device-to-host copy has been waited for, which orders every reuse; a
device buffer that is new (first use, or grown) is the compute stream's allocation, so the copy stream waits for that stream
once before it first writes there (tests/test_stream_order.py).

evaluate_stream() is the same pipeline over (input, truth) pairs: the truth image travels in on the copy stream beside
the input, the metric launch (kernels.u8_metrics) follows the forward on the compute stream, and only the 64-byte result
record comes back unless the images are kept.  A pair whose input is None has it made from the truth on the device
(kernels.bicubic_down_u8 on the compute stream, between the truth's arrival and the forward): no LR image is read,
pinned or copied.

upscale_yuv_stream() is the same pipeline over planar YUV 4:2:0 video frames: a frame travels in and out as its 1.5 bytes
per pixel, and the two colour conversions (kernels.i420_to_rgb_f32 / rgb_u8_to_i420) are two launches on the compute
stream around the forward, the second one writing straight into the slot's output buffer.

With output_size = (height, width) both upscaling streams resize every result to that one size on the device
(kernels.resize_u8, one eager launch on the compute stream behind the forward; for video between the forward's uint8 RGB
image and rgb_u8_to_i420): the slot's output buffers, and what crosses the host link on the way back, have the target size.

With keep_alpha upscale_stream also takes (H, W, 4) straight-alpha RGBA images, freely mixed with RGB ones: one launch
splits an RGBA image into the float planes of its colour and (unless it is opaque) of its alpha as a second batch slot, the
forward runs them together, and one launch merges the result into the slot's 4-channel output buffer
(kernels.rgba_u8_split_f32 / rgb_u8_merge_rgba); 4 bytes per pixel cross the host link each way.
"""
import collections

import numpy as np
import torch

from . import kernels as K
from .image_utils import check_i420_frame, check_output_size, check_u8_image, i420_frame_bytes


class _Slot:
    """The staging buffers of one image in flight."""

    def __init__(self, device, copy_stream):
        self.device = device
        self.copy_stream = copy_stream
        self.pin, self.dev = {}, {}   # "in", "out" and (evaluate_stream only) "truth": the flat pinned / device buffers
        self.pin_record = self.dev_record = None   # evaluate_stream only
        self.pin_flag = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self.dev_flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.dev_flag.record_stream(copy_stream)
        self.h2d = torch.cuda.Event()
        self.fwd = torch.cuda.Event()
        self.done = torch.cuda.Event()
        self.out_shape = None
        self.d2h_issued = False

    def _grown(self, buf, n, pinned):
        if buf is not None and buf.numel() >= n:
            return buf
        n = -(-n // (1 << 20)) << 20   # whole MiB: a slightly larger image does not allocate again
        if pinned:
            return torch.empty(n, dtype=torch.uint8, pin_memory=True)
        buf = torch.empty(n, dtype=torch.uint8, device=self.device)
        buf.record_stream(self.copy_stream)
        # The block comes from the current (compute) stream's pool: it may be an activation a forward still in flight there
        # has just released, and the copy stream is the first to write an input buffer.  Once per growth.
        self.copy_stream.wait_stream(torch.cuda.current_stream())
        return buf

    def views(self, which, shape, host=True):
        """(pinned view, device view) at `shape` of the slot's `which` buffers, grown as needed; host=False: the device
        view alone (an input made on the device has no host side)."""
        n = int(np.prod(shape))
        if host:
            self.pin[which] = self._grown(self.pin.get(which), n, True)
        self.dev[which] = self._grown(self.dev.get(which), n, False)
        dev = self.dev[which][:n].view(shape)
        return (self.pin[which][:n].view(shape), dev) if host else dev

    def records(self, words):
        if self.dev_record is None:
            self.pin_record = torch.zeros(words, dtype=torch.int64, pin_memory=True)
            self.dev_record = torch.zeros(words, dtype=torch.int64, device=self.device)
            self.dev_record.record_stream(self.copy_stream)
        return self.pin_record, self.dev_record


def _check_image(a, who="upscale_stream", keep_alpha=False):
    check_u8_image(a, who, 3, also_rgba=keep_alpha)


def _check_frame(f, nbytes, width, height):
    check_i420_frame(f, "upscale_yuv_stream", nbytes, width, height)


def _check_target(output_size):
    """output_size as given -> None or (height, width); the ratio is checked per image, its size being known only then."""
    return None if output_size is None else check_output_size(output_size, 1, 1)


def _check_depth(depth, who):
    depth = int(depth)
    if depth < 1:
        raise ValueError("larvanet_amd: %s needs depth >= 1" % who)
    return depth


def _require_hip_model(model, who):
    if model.device.type != "cuda":
        raise RuntimeError("larvanet_amd: %s only runs on a HIP device (MI355X); there is no CPU fallback" % who)


class _Stage:
    """What _stream (the pipeline itself, below) asks about one kind of item, one subclass per public stream:
      admit(item) -> job            the item checked and sized, before anything of it is launched; job[0] is the array
      fill(slot, job) -> (copies, buffers)    the item written into the slot's pinned buffers: [(device view, pinned view)]
                                    to copy in on the copy stream, and the device views launch() works on
      launch(slot, job, *buffers)   the launches on the compute stream, through the plugin's composers (_infer_rgb,
                                    _infer_rgba, _infer_i420) with model._infer_u8_images as the forward; sets slot.out_shape
      outputs(slot) -> [(pinned view, device view)]    what the copy stream brings back
      result(slot)                  what the stream yields for the item, from the pinned buffers
    Written out here: one array in as a batch of one, and the slot's output buffer back (both upscaling streams)."""

    def fill(self, slot, job):
        pin_in, dev_in = slot.views("in", (1,) + tuple(job[0].shape))
        np.copyto(pin_in.numpy()[0], job[0])
        return [(dev_in, pin_in)], (dev_in,)

    def outputs(self, slot):
        return [slot.views("out", slot.out_shape)]

    def result(self, slot):
        return np.array(slot.views("out", slot.out_shape)[0].numpy()[0])


class _UpscaleStage(_Stage):
    """upscale_stream: uint8 (H, W, 3) images and, with keep_alpha, (H, W, 4) ones; with target every result has that size."""

    def __init__(self, model, target, keep_alpha):
        self.model, self.target, self.keep_alpha = model, target, keep_alpha

    def admit(self, image):
        _check_image(image, keep_alpha=self.keep_alpha)
        self.model._output_size(self.target, image.shape[0], image.shape[1])
        return (image,)

    def launch(self, slot, job, dev_in):
        m, target, image = self.model, self.target, job[0]
        slot.out_shape = (1,) + (target or tuple(m.scale * v for v in image.shape[:2])) + (image.shape[2],)
        dev_out = slot.views("out", slot.out_shape)[1]
        if image.shape[2] == 4:   # RGBA: split -> forward over colour (and alpha) -> merged into the slot's buffer
            m._infer_rgba(dev_in, [bool(image[..., 3].min() == 255)],
                          lambda planes: m._infer_rgb(planes, target, m._infer_u8_images), out=dev_out)
        else:   # (the x8 self-ensemble under --self_ensemble; resized, or else copied, straight into the slot's own buffer)
            m._infer_rgb(dev_in, target, m._infer_u8_images, out=dev_out)


class _VideoStage(_Stage):
    """upscale_yuv_stream: flat I420 frames of `size` = (width, height), or (frame, width, height) triples; a frame is a
    batch of one, [1][frame bytes], on the way in and on the way out."""

    def __init__(self, model, target, size, matrix, full_range):
        self.model, self.target, self.size, self.matrix, self.full_range = model, target, size, matrix, full_range

    def admit(self, item):
        frame, fw, fh = (item,) + self.size if self.size is not None else item
        fw, fh = int(fw), int(fh)
        _check_frame(frame, i420_frame_bytes(fw, fh), fw, fh)
        self.model._output_size(self.target, fh, fw)
        return frame, fw, fh

    def launch(self, slot, job, dev_in):   # frame -> float planes -> forward -> HR frame, written into the slot's own buffer
        m, (_, fw, fh) = self.model, job
        hr_h, hr_w = self.target or (m.scale * fh, m.scale * fw)
        slot.out_shape = (1, i420_frame_bytes(hr_w, hr_h))
        m._infer_i420(dev_in, fw, fh, self.matrix, self.full_range, self.target, m._infer_u8_images,
                      out=slot.views("out", slot.out_shape)[1])


class _EvaluateStage(_Stage):
    """evaluate_stream: (input, truth) pairs of uint8 (H, W, 3) images, the input None where it is made from the truth on
    the device; the 64-byte record comes back, and the image when `keep`."""

    def __init__(self, model, shave, channel, ssim, keep):
        self.model, self.shave, self.channel, self.ssim, self.keep = model, shave, channel, ssim, keep

    def admit(self, pair):
        image, truth = pair
        _check_image(truth, "evaluate_stream")
        if image is None:   # the input is made from the truth on the device
            in_shape = K.bicubic_down_size(truth.shape[0], truth.shape[1], self.model.scale) + (3,)
        else:
            _check_image(image, "evaluate_stream")
            in_shape = tuple(image.shape)
        K.metric_window((self.model.scale * in_shape[0], self.model.scale * in_shape[1]), truth.shape, self.shave, self.ssim)
        return image, truth, in_shape

    def fill(self, slot, job):
        image, truth, in_shape = job
        copies = []
        if image is None:
            dev_in = slot.views("in", (1,) + in_shape, host=False)
        else:
            pin_in, dev_in = slot.views("in", (1,) + in_shape)
            np.copyto(pin_in.numpy()[0], image)
            copies.append((dev_in, pin_in))
        pin_truth, dev_truth = slot.views("truth", tuple(truth.shape))
        np.copyto(pin_truth.numpy(), truth)
        copies.append((dev_truth, pin_truth))
        return copies, (dev_in, dev_truth)

    def launch(self, slot, job, dev_in, dev_truth):
        m = self.model
        if job[0] is None:
            K.bicubic_down_u8(dev_truth, m.scale, out=dev_in[0])
        out = m._infer_rgb(dev_in, None, m._infer_u8_images)
        slot.out_shape = tuple(out.shape)
        if self.keep:
            slot.views("out", slot.out_shape)[1].copy_(out)
        # (scored where the forward left it: nothing else runs on this stream in between)
        K.u8_metrics(out[0], dev_truth, self.shave, self.channel, self.ssim, result=slot.records(K.METRIC_RESULT_WORDS)[1])

    def outputs(self, slot):
        return (super().outputs(slot) if self.keep else []) + [(slot.pin_record, slot.dev_record)]

    def result(self, slot):
        result = K.metrics_from_record(slot.pin_record.numpy().copy())
        return (result, super().result(slot)) if self.keep else result


def upscale_stream(model, images, scale, depth=2, output_size=None, keep_alpha=False):
    """Generator: uint8 (H, W, 3) numpy images of any sizes -> their uint8 (sH, sW, 3) upscaled images, in input order;
    each result equals model.upscale_u8([image], scale)[0].  At most `depth` images are in flight (depth 1 = no overlap).
    keep_alpha=True: (H, W, 4) RGBA images are taken too, in any mix with RGB ones, and come back with 4 channels, each
    equal to model.upscale_rgba_u8([image], scale)[0]; the default refuses them as before.
    output_size = (height, width): every result is resized to it on the device and equals model.upscale_u8([image], scale,
    output_size=output_size)[0]; an image the size is out of range for raises ValueError before anything of it is launched.
    Under --precision fp16 an image whose activations overflow raises FloatingPointError when its turn to be yielded
    comes; the images before it have been yielded.  The yielded arrays are the caller's (copies of the pinned staging
    buffers)."""
    depth = _check_depth(depth, "upscale_stream")
    target = _check_target(output_size)
    model._check_scale(scale)
    _require_hip_model(model, "upscale_stream")
    return _stream(model, images, depth, _UpscaleStage(model, target, bool(keep_alpha)))


def evaluate_stream(model, pairs, scale, shave=None, channel="y", ssim=True, depth=2, keep_images=False):
    """Generator: (lr_uint8, truth_uint8) pairs of (H, W, 3) numpy images of any sizes -> per pair, in input order, the
    dict kernels.metrics_from_record gives for model.upscale_u8([lr], scale)[0] against the truth ({"psnr", "ssim", "sse",
    "n"}; see kernels.u8_metrics for shave / channel / ssim; shave=None shaves `scale` pixels), or with keep_images the
    tuple (dict, upscaled uint8 image).  upscale_stream's pipeline: the truth goes in beside the input, the metrics run
    behind the forward, the record (and the image only when kept) comes back.  A pair no metric is defined for (truth
    smaller than the output, window below 11 pixels with SSIM) raises ValueError before anything of it is launched; fp16
    overflow raises at the image's turn.  A pair (None, truth) is scored on lr = the bicubic decimation of the truth by
    `scale`, made on the device (kernels.bicubic_down_u8: the truth's top-left (H // scale) scale x (W // scale) scale
    pixels, the window the metrics crop to anyway); its result equals the pair (image_utils.bicubic_downscale_u8(truth,
    scale), truth)'s."""
    depth = _check_depth(depth, "evaluate_stream")
    model._check_scale(scale)
    if channel not in K.METRIC_CHANNELS:
        raise ValueError("larvanet_amd: channel must be 'y' or 'rgb', got %r" % (channel,))
    shave = model.scale if shave is None else int(shave)
    if shave < 0:
        raise ValueError("larvanet_amd: metrics need shave >= 0, got %d" % shave)
    _require_hip_model(model, "evaluate_stream")
    return _stream(model, pairs, depth, _EvaluateStage(model, shave, channel, bool(ssim), bool(keep_images)))


def upscale_yuv_stream(model, frames, scale, width=None, height=None, matrix="bt601", full_range=False, depth=2,
                       output_size=None):
    """Generator: uint8 1-D numpy I420 frames of width x height -> their uint8 1-D HR frames of (s width) x (s height), in
    input order; each equals model.upscale_yuv420([frame], scale, width, height, matrix, full_range)[0].  With width and
    height None the items are (frame, width, height) triples of any mix of sizes.  upscale_stream's pipeline: pinned
    staging slots, one copy stream, at most `depth` frames in flight; under --precision fp16 a frame whose activations
    overflow raises FloatingPointError when its turn to be yielded comes, the frames before it have been yielded.
    output_size = (height, width): the HR frames are of that size, as upscale_yuv420's with the same argument."""
    depth = _check_depth(depth, "upscale_yuv_stream")
    target = _check_target(output_size)
    if width is not None and height is not None:
        model._output_size(target, height, width)   # (one input size: the ratio is refused here, before any frame)
    if (width is None) != (height is None):
        raise ValueError("larvanet_amd: upscale_yuv_stream takes width and height, or neither (items are then "
                         "(frame, width, height) triples)")
    model._check_yuv_args(1 if width is None else width, 1 if height is None else height, matrix, full_range, scale)
    _require_hip_model(model, "upscale_yuv_stream")
    size = None if width is None else (int(width), int(height))
    return _stream(model, frames, depth, _VideoStage(model, target, size, matrix, bool(full_range)))


def _stream(model, items, depth, stage):
    """The pipeline itself, for the items and the work `stage` describes: the slots, the copy stream, the three events of
    a slot, and the order in which both streams are fed."""
    compute = torch.cuda.current_stream()
    copy = torch.cuda.Stream()
    free = [_Slot(model.device, copy) for _ in range(depth)]
    inflight = collections.deque()
    model_flag = model.overflow_flag()   # the fp16 launches' overflow flag; None at fp32
    fp16 = model_flag is not None

    def issue_d2h(slot):
        if slot.d2h_issued:
            return
        with torch.cuda.stream(copy):
            copy.wait_event(slot.fwd)
            for pinned, dev in stage.outputs(slot):
                pinned.copy_(dev, non_blocking=True)
            if fp16:
                slot.pin_flag.copy_(slot.dev_flag, non_blocking=True)
            slot.done.record(copy)
        slot.d2h_issued = True

    def retire(slot):
        issue_d2h(slot)
        slot.done.synchronize()
        if fp16 and int(slot.pin_flag[0]):
            raise model.overflow_error()
        result = stage.result(slot)
        free.append(slot)
        return result

    try:
        with torch.no_grad():
            if fp16:
                model_flag.zero_()
            for item in items:
                job = stage.admit(item)
                if len(inflight) == depth:
                    yield retire(inflight.popleft())
                slot = free.pop()
                copies, buffers = stage.fill(slot, job)
                with torch.cuda.stream(copy):
                    for dev, pinned in copies:
                        dev.copy_(pinned, non_blocking=True)
                    slot.h2d.record(copy)
                if inflight:   # the previous image's way back, queued behind this image's way in
                    issue_d2h(inflight[-1])
                compute.wait_event(slot.h2d)
                stage.launch(slot, job, *buffers)
                if fp16:   # this image's overflow verdict; the model's flag starts the next image clean
                    slot.dev_flag.copy_(model_flag)
                    model_flag.zero_()
                slot.fwd.record(compute)
                slot.d2h_issued = False
                inflight.append(slot)
            while inflight:
                yield retire(inflight.popleft())
    finally:
        # (an early exit or an error: the staging buffers are released only once no copy can still touch them)
        if inflight:
            copy.synchronize()
            compute.synchronize()
