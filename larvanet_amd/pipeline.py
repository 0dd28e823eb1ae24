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
the copy stream.  A slot is reused only after its device-to-host copy has been waited for, which orders every reuse.

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


class _Slot:
    """The staging buffers of one image in flight."""

    def __init__(self, device, copy_stream):
        self.device = device
        self.copy_stream = copy_stream
        self.pin_in = self.pin_out = self.dev_in = self.dev_out = None
        self.pin_truth = self.dev_truth = self.pin_record = self.dev_record = None   # evaluate_stream only
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
        return buf

    def views_in(self, shape):
        n = int(np.prod(shape))
        self.pin_in = self._grown(self.pin_in, n, True)
        self.dev_in = self._grown(self.dev_in, n, False)
        return self.pin_in[:n].view(shape), self.dev_in[:n].view(shape)

    def view_made_in(self, shape):
        """The device input buffer alone: an input made on the device has no host side."""
        n = int(np.prod(shape))
        self.dev_in = self._grown(self.dev_in, n, False)
        return self.dev_in[:n].view(shape)

    def views_truth(self, shape):
        n = int(np.prod(shape))
        self.pin_truth = self._grown(self.pin_truth, n, True)
        self.dev_truth = self._grown(self.dev_truth, n, False)
        return self.pin_truth[:n].view(shape), self.dev_truth[:n].view(shape)

    def records(self, words):
        if self.dev_record is None:
            self.pin_record = torch.zeros(words, dtype=torch.int64, pin_memory=True)
            self.dev_record = torch.zeros(words, dtype=torch.int64, device=self.device)
            self.dev_record.record_stream(self.copy_stream)
        return self.pin_record, self.dev_record

    def views_out(self, shape):
        n = int(np.prod(shape))
        self.pin_out = self._grown(self.pin_out, n, True)
        self.dev_out = self._grown(self.dev_out, n, False)
        return self.pin_out[:n].view(shape), self.dev_out[:n].view(shape)


def _check_image(a, who="upscale_stream", keep_alpha=False):
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise TypeError("larvanet_amd: %s takes uint8 numpy arrays (decoded images), got %s"
                        % (who, getattr(a, "dtype", type(a).__name__),))
    if keep_alpha and a.ndim == 3 and a.shape[2] == 4 and a.shape[0] >= 1 and a.shape[1] >= 1:
        return
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("larvanet_amd: %s takes (H, W, 3) images%s, got shape %s"
                         % (who, " and, with keep_alpha, (H, W, 4) ones" if keep_alpha else "", a.shape,))


def _check_target(output_size):
    """output_size as given -> None or (height, width); the ratio is checked per image, its size being known only then."""
    from .image_utils import check_output_size
    return None if output_size is None else check_output_size(output_size, 1, 1)


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
    depth = int(depth)
    if depth < 1:
        raise ValueError("larvanet_amd: upscale_stream needs depth >= 1")
    target = _check_target(output_size)
    if int(scale) != model.scale:
        raise ValueError("larvanet_amd: this model upscales by %d, not by %r" % (model.scale, scale))
    if model.device.type != "cuda":
        raise RuntimeError("larvanet_amd: upscale_stream only runs on a HIP device (MI355X); there is no CPU fallback")
    return _stream(model, images, depth, target=target, keep_alpha=bool(keep_alpha))


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
    from . import kernels as K
    depth = int(depth)
    if depth < 1:
        raise ValueError("larvanet_amd: evaluate_stream needs depth >= 1")
    if int(scale) != model.scale:
        raise ValueError("larvanet_amd: this model upscales by %d, not by %r" % (model.scale, scale))
    if channel not in K.METRIC_CHANNELS:
        raise ValueError("larvanet_amd: channel must be 'y' or 'rgb', got %r" % (channel,))
    shave = model.scale if shave is None else int(shave)
    if shave < 0:
        raise ValueError("larvanet_amd: metrics need shave >= 0, got %d" % shave)
    if model.device.type != "cuda":
        raise RuntimeError("larvanet_amd: evaluate_stream only runs on a HIP device (MI355X); there is no CPU fallback")
    return _stream(model, pairs, depth, {"shave": shave, "channel": channel, "ssim": bool(ssim), "keep": bool(keep_images)})


def _check_frame(f, nbytes, width, height):
    if not isinstance(f, np.ndarray) or f.dtype != np.uint8:
        raise TypeError("larvanet_amd: upscale_yuv_stream takes uint8 numpy frames, got %s"
                        % (getattr(f, "dtype", type(f).__name__),))
    if f.ndim != 1 or f.size != nbytes:
        raise ValueError("larvanet_amd: an I420 frame of %d x %d is a flat buffer of %d bytes, got shape %s"
                         % (width, height, nbytes, f.shape,))


def upscale_yuv_stream(model, frames, scale, width=None, height=None, matrix="bt601", full_range=False, depth=2,
                       output_size=None):
    """Generator: uint8 1-D numpy I420 frames of width x height -> their uint8 1-D HR frames of (s width) x (s height), in
    input order; each equals model.upscale_yuv420([frame], scale, width, height, matrix, full_range)[0].  With width and
    height None the items are (frame, width, height) triples of any mix of sizes.  upscale_stream's pipeline: pinned
    staging slots, one copy stream, at most `depth` frames in flight; under --precision fp16 a frame whose activations
    overflow raises FloatingPointError when its turn to be yielded comes, the frames before it have been yielded.
    output_size = (height, width): the HR frames are of that size, as upscale_yuv420's with the same argument."""
    depth = int(depth)
    if depth < 1:
        raise ValueError("larvanet_amd: upscale_yuv_stream needs depth >= 1")
    target = _check_target(output_size)
    if width is not None and height is not None:
        model._output_size(target, height, width)   # (one input size: the ratio is refused here, before any frame)
    if (width is None) != (height is None):
        raise ValueError("larvanet_amd: upscale_yuv_stream takes width and height, or neither (items are then "
                         "(frame, width, height) triples)")
    model._check_yuv_args(1 if width is None else width, 1 if height is None else height, matrix, full_range, scale)
    if model.device.type != "cuda":
        raise RuntimeError("larvanet_amd: upscale_yuv_stream only runs on a HIP device (MI355X); there is no CPU fallback")
    size = None if width is None else (int(width), int(height))
    return _stream(model, frames, depth, yuv={"size": size, "matrix": matrix, "full_range": bool(full_range)}, target=target)


def _stream(model, images, depth, score=None, yuv=None, target=None, keep_alpha=False):
    """The pipeline of upscale_stream; with `score` (evaluate_stream's settings) the items are (input, truth) pairs; with
    `yuv` (upscale_yuv_stream's settings) they are I420 frames, or (frame, width, height) triples; with `target` = (height,
    width) the two upscaling streams resize every result to it; with keep_alpha upscale_stream takes RGBA images too."""
    if score is not None or yuv is not None or target is not None or keep_alpha:
        from . import kernels as K
    if yuv is not None:
        from .image_utils import i420_frame_bytes
    keep = score is None or score["keep"]
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
            if keep:
                pin_out, dev_out = slot.views_out(slot.out_shape)
                pin_out.copy_(dev_out, non_blocking=True)
            if score is not None:
                slot.pin_record.copy_(slot.dev_record, non_blocking=True)
            if fp16:
                slot.pin_flag.copy_(slot.dev_flag, non_blocking=True)
            slot.done.record(copy)
        slot.d2h_issued = True

    def retire(slot):
        issue_d2h(slot)
        slot.done.synchronize()
        if fp16 and int(slot.pin_flag[0]):
            raise model.overflow_error()
        out = np.array(slot.views_out(slot.out_shape)[0].numpy()[0]) if keep else None
        if yuv is not None:
            out = out[0]   # (the frame itself, 1-D)
        result = None if score is None else K.metrics_from_record(slot.pin_record.numpy().copy())
        free.append(slot)
        if score is None:
            return out
        return (result, out) if keep else result

    try:
        with torch.no_grad():
            if fp16:
                model_flag.zero_()
            for image in images:
                if yuv is not None:
                    image, fw, fh = (image,) + yuv["size"] if yuv["size"] is not None else image
                    fw, fh = int(fw), int(fh)
                    _check_frame(image, i420_frame_bytes(fw, fh), fw, fh)
                    model._output_size(target, fh, fw)
                    image = image[None]   # (a batch of one frame: [1][frame bytes])
                elif score is None:
                    _check_image(image, keep_alpha=keep_alpha)
                    model._output_size(target, image.shape[0], image.shape[1])
                else:
                    image, truth = image
                    _check_image(truth, "evaluate_stream")
                    if image is None:   # the input is made from the truth on the device
                        in_shape = K.bicubic_down_size(truth.shape[0], truth.shape[1], model.scale) + (3,)
                    else:
                        _check_image(image, "evaluate_stream")
                        in_shape = tuple(image.shape)
                    K.metric_window((model.scale * in_shape[0], model.scale * in_shape[1]), truth.shape,
                                    score["shave"], score["ssim"])
                if len(inflight) == depth:
                    yield retire(inflight.popleft())
                slot = free.pop()
                made = score is not None and image is None
                shape = (1,) + (in_shape if made else tuple(image.shape))
                if made:
                    dev_in = slot.view_made_in(shape)
                else:
                    pin_in, dev_in = slot.views_in(shape)
                    np.copyto(pin_in.numpy()[0], image)
                if score is not None:
                    pin_truth, dev_truth = slot.views_truth(tuple(truth.shape))
                    np.copyto(pin_truth.numpy(), truth)
                with torch.cuda.stream(copy):
                    if not made:
                        dev_in.copy_(pin_in, non_blocking=True)
                    if score is not None:
                        dev_truth.copy_(pin_truth, non_blocking=True)
                    slot.h2d.record(copy)
                if inflight:   # the previous image's way back, queued behind this image's way in
                    issue_d2h(inflight[-1])
                compute.wait_event(slot.h2d)
                if made:
                    K.bicubic_down_u8(dev_truth, model.scale, out=dev_in[0])
                if yuv is not None:   # frame -> float planes -> forward -> HR frame, written into the slot's own buffer
                    x = K.i420_to_rgb_f32(dev_in[0], fw, fh, yuv["matrix"], yuv["full_range"])
                    out = model._infer_u8_images(x)
                    if target is not None:
                        out = K.resize_u8(out, target[0], target[1])
                    slot.out_shape = (1, 1, i420_frame_bytes(out.shape[2], out.shape[1]))
                    K.rgb_u8_to_i420(out, yuv["matrix"], yuv["full_range"], out=slot.views_out(slot.out_shape)[1][0])
                elif dev_in.shape[3] == 4:   # RGBA: split -> forward over colour (and alpha) -> merged into the slot's buffer
                    def infer(planes):
                        out = model._infer_u8_images(planes)
                        return out if target is None else K.resize_u8(out, target[0], target[1])
                    slot.out_shape = (1,) + (target or tuple(model.scale * v for v in image.shape[:2])) + (4,)
                    model._infer_rgba(dev_in, [bool(image[..., 3].min() == 255)], infer, out=slot.views_out(slot.out_shape)[1])
                else:
                    out = model._infer_u8_images(dev_in)   # (the x8 self-ensemble under --self_ensemble)
                    if target is not None:   # (upscale_stream only: resized straight into the slot's own buffer)
                        slot.out_shape = (1,) + target + (3,)
                        K.resize_u8(out, target[0], target[1], out=slot.views_out(slot.out_shape)[1])
                    else:
                        slot.out_shape = tuple(out.shape)
                        if keep:
                            slot.views_out(slot.out_shape)[1].copy_(out)
                if score is not None:   # (scored where the forward left it: nothing else runs on this stream in between)
                    K.u8_metrics(out[0], dev_truth, score["shave"], score["channel"], score["ssim"],
                                 result=slot.records(K.METRIC_RESULT_WORDS)[1])
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
