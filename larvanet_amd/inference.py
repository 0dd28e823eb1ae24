"""The grad-free half of the plugin class: the one eager-or-graph dispatch of the inference forward, the fp16 overflow
verdict, and every image-format entry point (float, uint8, RGBA, planar YUV 4:2:0, all exits) with its host-side argument
checks and its device-side composer.  A mixin without state of its own: models/LarvaNet.py's LarvaNet inherits it in front
of BaseModel and sets, in __init__ / prepare(), what it reads -- model, precision, device, scale, args, use_hip_graph,
strict_graph, dual_chain, batch_exit_legs and the four graph tables.  pipeline.py's streams run the same composers with
_infer_u8_images as the forward and a staging slot's buffer as the destination."""
import gc

import numpy as np
import torch

from . import kernels as K
from .autograd import HeadFn, StepScope, is_large_inference
from .image_utils import YUV_MATRICES, check_i420_frame, check_output_size, check_u8_image, i420_frame_bytes
from .infer_graphs import Form


def _require_hip(t):
    if not t.is_cuda:
        raise RuntimeError("larvanet_amd: the network only runs on a HIP device (MI355X); "
                           "got a %s tensor and there is no CPU fallback" % t.device)


def _require_u8_tensor(t, who):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise TypeError("larvanet_amd: %s takes a uint8 tensor, got %s" % (who, getattr(t, "dtype", type(t).__name__),))


class InferenceMixin:
    """Everything of the plugin that runs without gradients.  In front of BaseModel in the bases, so that its upscale wins."""

    def _infer_scope(self):
        """Inference forward inside a captured graph: the layer chain may run as two half-batch chains."""
        return StepScope(defer_wgrad=False, joint_input_grads=False, dual_chain=self.dual_chain,
                         lazy_chain_joins=(True, False))

    def _eager_or_graph(self, x, form):
        """The grad-free forward of the device batch `x` in `form`, eagerly or as a hipGraph: THE rule.  A shape seen for
        the second time is captured (launched one by one from Python the ~36 kernels of a 16 x 3 x 48 x 48 forward are
        host-bound: 0.70 ms against 0.5 ms of GPU time) and replayed from then on (infer_graphs.GraphTable; each table has
        its own limit, so each path captures exactly what it would without the others).  A replay returns the graph's
        output buffer: callers that keep it across calls copy it."""
        n = int(x.shape[0])
        h, w = (int(v) for v in (x.shape[1:3] if form.u8 and x.dtype == torch.uint8 else x.shape[2:4]))
        # A whole validation image is 36 launches of 60 us each: the host is ~2 ms ahead of the GPU after the first few,
        # and eager launches have no replay boundary and no copy into a static input: 2.162 against 2.178 ms per
        # 339 x 510 image (tools/infer_modes.py, round 5).  The capture pays where the launches are short.  The rule asks
        # about the forward's own batch (the ensemble: 8 N slots of a square image, 4 N otherwise) and also picks the head kernel.
        if not (self.use_hip_graph and x.is_cuda) or is_large_inference((8 if h == w else 4) * n if form.ensemble else n, h, w):
            return self._forward_nograd(x, *form, exits=form.exits)
        table, key = self._graph_table(form, x)
        return table.forward(key, x, capture=lambda x: self._capture_infer(x, form),
                             run=lambda x: self._forward_nograd(x, *form, exits=form.exits))

    def _graph_table(self, form, x):
        """-> (the table that holds `form`'s captured forwards, the key of x in it).  The self-ensemble's graph also
        holds its input launch and its merge launch, so it has a table (and a tag per form) of its own."""
        if form.ensemble:
            table, tag = self._infer_graphs_se, ("u8" if form.u8 else "f32", "se")
        elif form.u8:
            table, tag = self._infer_graphs_u8, ("u8",)
        else:
            table, tag = self._infer_graphs, ()
        if form.exits:
            table = self._infer_graphs_ex
        if form.u8 and x.dtype != torch.uint8:   # (the video and RGBA paths' u8 form takes float planes: _forward_nograd)
            tag += ("f32in",)
        return table, (tuple(x.shape), self.precision) + tag

    def _infer(self, x):
        """self.model(x); without gradients, by _eager_or_graph."""
        return self.model(x) if torch.is_grad_enabled() else self._eager_or_graph(x, Form())

    def _infer_u8_images(self, x_u8):
        """What the streams (pipeline.py) run on a uint8 device batch [N][H][W][3]: the uint8 form of _infer, or under
        --self_ensemble the ensemble.  The video and RGBA streams hand it float planes instead (see _forward_nograd)."""
        return self._eager_or_graph(x_u8, Form(True, self._self_ensemble()))

    def _capture_infer(self, x, form):
        """-> replay(x) of the captured forward of x's shape in `form`, or False if the capture failed."""
        static_x = x.clone()
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    with self._infer_scope():
                        self._forward_nograd(static_x, *form, exits=form.exits)
            torch.cuda.current_stream().wait_stream(side)
            # A plugin holds its captured graphs in reference cycles: one that was dropped lives until the collector
            # runs, and a graph freed while this capture is open calls into the HIP runtime and aborts the process.
            gc.collect()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                with self._infer_scope():
                    out = self._forward_nograd(static_x, *form, exits=form.exits)
        except Exception as e:   # an optimisation only
            if self.strict_graph:
                raise
            print("WARNING: hipGraph capture of the inference forward failed (%s: %s); running it eagerly"
                  % (type(e).__name__, e))
            torch.cuda.synchronize()
            return False

        def replay(x):
            self._refresh_inference_weights()   # weights restored / stepped since the capture: repack (outside the graph)
            static_x.copy_(x)
            graph.replay()
            return out
        return replay

    def _half(self):
        """The fp16 forward when the model runs at --precision fp16, else None: the one place precision is decided."""
        return self.model.half_forward() if self.precision == "fp16" else None

    def _self_ensemble(self):
        """Does this model run the x8 self-ensemble in its image entry points (--self_ensemble)?  The one place it is
        decided; grad-enabled calls, test, fwd_runtime and the validation of training never ask."""
        return bool(getattr(self.args, "self_ensemble", False))

    def _forward_ensemble(self, x, u8):
        """E(x) of image_utils.self_ensemble on the device (no graph): one launch builds the eight inputs as batch slots,
        the existing fp32 / fp16 forward runs them (one forward of 8 N for a square image, else one of 4 N per shape) and
        ends in fp32 HR images, one launch maps them back, averages and (u8) quantises.  A pixel's result does not depend
        on its batch slot, so this is the composition of eight plain calls bit for bit; the head kernel, whose two forms
        do differ, is chosen as the plain call of these N images would choose it."""
        n = int(x.shape[0])
        h, w = (int(v) for v in (x.shape[1:3] if x.dtype == torch.uint8 else x.shape[2:4]))
        half = self._half()
        run = half if half is not None else self.model
        with HeadFn.rule_batch_as(HeadFn.rule_batch or n):   # (a caller that runs slots of its own has named its images)
            if h == w:
                both = torch.empty((8 * n, 3, h, w), device=x.device, dtype=torch.float32)
                K.dihedral_inputs(x, out=(both[:4 * n], both[4 * n:]))
                out = run(both).contiguous()
                a, b = out[:4 * n], out[4 * n:]
            else:
                a, b = K.dihedral_inputs(x)
                a, b = run(a).contiguous(), run(b).contiguous()
        return K.dihedral_mean(a, b, u8=u8)

    def _forward_nograd(self, x, u8=False, ensemble=False, exits=False):
        """The inference forward at the model's precision (no graph).  u8: uint8 [N][H][W][3] -> uint8 [N][sH][sW][3],
        the float forward over the exactly converted image, then round half to even + clamp on the device (at fp16 the
        leg end's epilogue stores the bytes itself); a float32 [N][3][H][W] input (the video path: frames converted
        without a rounding to bytes) is taken as it is and leaves as uint8 the same way.  ensemble: the x8 self-ensemble of either form.  exits: every exit's
        image, [M] in front of the batch (fp32: one conversion launch over the M N images makes the uint8 form)."""
        if ensemble:
            return self._forward_ensemble(x.contiguous(), u8)
        half = self._half()
        if u8 and x.dtype == torch.uint8:
            x = K.u8_hwc_to_f32_chw(x)
        if exits:
            batched = True if self.batch_exit_legs is None else bool(self.batch_exit_legs)
            if half is not None:
                return half.exits(x, u8=u8, batched=batched)
            out = self.model.forward_exits(x, batched=batched)
            if not u8:
                return out
            m, n = int(out.shape[0]), int(out.shape[1])
            return K.f32_chw_to_u8_hwc(out.view((m * n,) + tuple(out.shape[2:]))).view(m, n, *out.shape[3:], 3)
        if half is not None:
            return half(x, u8=u8)
        out = self.model(x)
        return K.f32_chw_to_u8_hwc(out.contiguous()) if u8 else out

    def _refresh_inference_weights(self):
        """Repack the stale weight images of the active precision."""
        half = self._half()
        if half is not None:
            half.refresh()
        else:
            for pc in self.model.packed_convs():
                pc.refresh()

    def overflow_flag(self):
        """The device flag the fp16 launches set on overflow (int32 [1]), or None at --precision fp32."""
        half = self._half()
        return None if half is None else half.flag(self.device)

    @staticmethod
    def overflow_error():
        return FloatingPointError("larvanet_amd: an activation exceeded the fp16 range (|v| > 65504 or not finite) "
                                  "under --precision fp16; run this model with --precision fp32")

    def fp16_overflowed(self):
        """True if an fp16 inference forward (fwd_runtime included) overflowed since the last check; clears the flag.
        Always False at --precision fp32."""
        half = self._half()
        return half is not None and half.take_overflow()

    def _infer_checked(self, x, u8=False, ensemble=None, exits=False):
        """test and the image entry points, all under no_grad: an fp16 activation that left the fp16 range is an error,
        not a result.  ensemble None: as --self_ensemble says -- the one place the image entry points' form is decided."""
        half = self._half()
        if half is not None:
            half.clear_overflow()
        out = self._eager_or_graph(x, Form(u8, self._self_ensemble() if ensemble is None else ensemble, exits))
        if self.fp16_overflowed():
            raise self.overflow_error()
        return out

    def _to_input_tensor(self, input_list):
        arr = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.float32) for a in input_list]))
        return torch.from_numpy(arr).to(self.device)

    def upscale(self, input_list, scale):
        """list of CHW numpy images -> (N, 3, 4H, 4W) float32 numpy (models/LarvaNet.py:163-171)."""
        with torch.no_grad():
            return self._infer_checked(self._to_input_tensor(input_list)).detach().cpu().numpy()

    def upscale_tensor(self, input_list):
        """upscale() without the trip to the host: (N, 3, 4H, 4W) float32 on self.device."""
        with torch.no_grad():
            return self._infer_checked(self._to_input_tensor(input_list)).detach().clone()

    # ------------------------------------------------------------------ 8-bit images in, 8-bit images out
    def _check_scale(self, scale):
        """The one refusal of a scale this model was not prepared for."""
        if int(scale) != self.scale:
            raise ValueError("larvanet_amd: this model upscales by %d, not by %r" % (self.scale, scale))

    def _check_u8_images(self, input_list, scale, who="upscale_u8", channels=3):
        """Host-side argument checks of upscale_u8 and, with channels = 4, of upscale_rgba_u8 (before any device work) ->
        the (N, H, W, channels) uint8 batch."""
        self._check_scale(scale)
        if isinstance(input_list, np.ndarray) or not len(input_list):
            raise ValueError("larvanet_amd: %s takes a non-empty list of (H, W, %d) uint8 arrays" % (who, channels))
        for a in input_list:
            check_u8_image(a, who, channels)
            if a.shape != input_list[0].shape:
                raise ValueError("larvanet_amd: the images of one %s call must have one shape, got %s and %s"
                                 % (who, input_list[0].shape, a.shape))
        return np.ascontiguousarray(np.stack(input_list))

    def _check_u8_tensor(self, x_u8, who="upscale_u8_tensor", on_device=True, channels=3):
        _require_u8_tensor(x_u8, who)
        if x_u8.dim() != 4 or x_u8.shape[3] != channels or min(x_u8.shape) < 1:
            raise ValueError("larvanet_amd: %s takes [N][H][W][%d], got shape %s" % (who, channels, tuple(x_u8.shape),))
        if on_device:
            _require_hip(x_u8)
        return x_u8.contiguous()

    def _output_size(self, output_size, height, width):
        """The output_size argument of the image entry points for a height x width input -> None or (h, w), checked against
        the network's (s height) x (s width) result (image_utils.check_output_size) before any device work."""
        return check_output_size(output_size, self.scale * int(height), self.scale * int(width))

    def _infer_u8_checked(self, x):
        """The forward the image entry points hand to the composers below (the streams hand them _infer_u8_images)."""
        return self._infer_checked(x, u8=True)

    def _infer_rgb(self, x, size, infer, out=None):
        """uint8 [N][H][W][3] (or the float planes the video and RGBA paths make) -> uint8 [N][h][w][3]: infer(x), the
        uint8 forward; with size = (h, w) resized to it on the device (kernels.resize_u8: one eager launch on the forward's
        stream behind the replayed or eager forward) into `out` or a tensor of its own.  Without a size the result is the
        forward's own (a replayed graph's output buffer: callers that keep it copy it), copied into `out` if there is one."""
        rgb = infer(x)
        if size is not None:
            return K.resize_u8(rgb, size[0], size[1], out=out)
        return rgb if out is None else out.copy_(rgb)

    def upscale_u8(self, input_list, scale, output_size=None):
        """list of uint8 (H, W, 3) images of one shape -> uint8 (N, sH, sW, 3) numpy:
        image_to_uint8(upscale(...)) byte for byte, transposed for an image writer, with a quarter of the bytes crossing
        the host link and no pass over the image on the host.  output_size = (height, width): each image resized to it on
        the device before it leaves (image_utils.resize_u8 of today's result, byte for byte) -> (N, height, width, 3)."""
        batch = self._check_u8_images(input_list, scale)
        size = self._output_size(output_size, batch.shape[1], batch.shape[2])
        with torch.no_grad():
            x = torch.from_numpy(batch).to(self.device)
            _require_hip(x)
            return self._infer_rgb(x, size, self._infer_u8_checked).cpu().numpy()

    def upscale_u8_tensor(self, x_u8, output_size=None):
        """upscale_u8 without the trips to and from the host: uint8 [N][H][W][3] on self.device -> uint8 [N][sH][sW][3], or
        [N][height][width][3] with output_size = (height, width)."""
        x = self._check_u8_tensor(x_u8, on_device=False)
        size = self._output_size(output_size, x.shape[1], x.shape[2])
        _require_hip(x)
        with torch.no_grad():
            out = self._infer_rgb(x, size, self._infer_u8_checked)
            return out.clone() if size is None else out

    def _check_evaluate_args(self, who, x_u8, truth_u8, shave, channel, ssim):
        """Argument checks of `who` = evaluate_u8_tensor / evaluate_exits_u8_tensor -> (x, truth, shave)."""
        x = self._check_u8_tensor(x_u8, who, on_device=False)
        truth = self._check_u8_tensor(truth_u8, who, on_device=False)
        if truth.shape[0] != x.shape[0]:
            raise ValueError("larvanet_amd: %s takes as many truth images as inputs, got %d and %d"
                             % (who, truth.shape[0], x.shape[0]))
        if channel not in K.METRIC_CHANNELS:
            raise ValueError("larvanet_amd: channel must be 'y' or 'rgb', got %r" % (channel,))
        shave = self.scale if shave is None else int(shave)
        s = self.scale
        K.metric_window((s * x.shape[1], s * x.shape[2]), truth.shape[1:3], shave, ssim)   # refusals before any launch
        _require_hip(x)
        _require_hip(truth)
        return x, truth, shave

    def evaluate_u8_tensor(self, x_u8, truth_u8, shave=None, channel="y", ssim=True):
        """Upscale and score on the device: x_u8 uint8 [N][H][W][3] and truth_u8 uint8 [N][th][tw][3] (th >= sH, tw >= sW,
        cropped top-left) on self.device -> one {"psnr", "ssim", "sse", "n"} per image (kernels.u8_metrics on what
        upscale_u8_tensor returns).  shave=None shaves self.scale pixels; channel "y" (BT.601 luma) or "rgb"."""
        x, truth, shave = self._check_evaluate_args("evaluate_u8_tensor", x_u8, truth_u8, shave, channel, ssim)
        with torch.no_grad():
            out = self._infer_checked(x, u8=True)
            records = torch.stack([K.u8_metrics(out[n], truth[n], shave, channel, ssim) for n in range(out.shape[0])])
        return [K.metrics_from_record(r) for r in records.cpu().numpy()]

    # ------------------------------------------------------------------ transparency: RGBA images in and out
    def _infer_rgba(self, x_u8, opaque, infer, out=None):
        """uint8 [N][H][W][4] on the device -> uint8 [N][h][w][4]: one launch splits the batch into the float planes of
        N + K slots (image n's colour in slot n, the alpha plane of each of the K images that are not known to be opaque as
        a grey image of its own), infer(planes) -- the uint8 forward that takes float planes, as the video path's --
        returns the uint8 [N + K][h][w][3] result, and one launch merges it (alpha = the rounded mean of its slot's three
        channels, 255 for an opaque image) into `out` or a new tensor.  Both launches sit outside the forward's graph.  A
        pixel's result does not depend on its batch slot, and the head kernel is chosen as the RGB call of these N images
        would choose it, so the colour is upscale_u8's bit for bit."""
        n = int(x_u8.shape[0])
        slot, k = K.alpha_slot_table(opaque, x_u8.device)
        planes = K.rgba_u8_split_f32(x_u8, slot, k)
        with HeadFn.rule_batch_as(n):
            rgb = infer(planes)
        return K.rgb_u8_merge_rgba(rgb, slot, n, out=out)

    def upscale_rgba_u8(self, input_list, scale, output_size=None):
        """list of uint8 (H, W, 4) straight-alpha RGBA images of one shape -> uint8 (N, sH, sW, 4) numpy.  Channels 0..2 are
        upscale_u8 of the RGB part byte for byte; the alpha goes through the same network as a grey image and its three
        result channels are merged as (r + g + b + 1) // 3 (image_utils.rgba_merge_u8).  An opaque image (alpha 255
        everywhere, decided here on the host) keeps alpha 255 and costs what its RGB part costs.  output_size = (height,
        width): colour and alpha each go through image_utils.resize_u8 before the merge -> (N, height, width, 4)."""
        batch = self._check_u8_images(input_list, scale, "upscale_rgba_u8", 4)
        size = self._output_size(output_size, batch.shape[1], batch.shape[2])
        opaque = [bool(a[..., 3].min() == 255) for a in batch]
        with torch.no_grad():
            x = torch.from_numpy(batch).to(self.device)
            _require_hip(x)
            return self._infer_rgba(x, opaque, lambda planes: self._infer_rgb(planes, size, self._infer_u8_checked)).cpu().numpy()

    def upscale_rgba_u8_tensor(self, x_u8, opaque=None, output_size=None):
        """upscale_rgba_u8 without the trips to and from the host: uint8 [N][H][W][4] on self.device -> uint8
        [N][sH][sW][4], or [N][height][width][4] with output_size.  opaque: None (no image is known to be opaque: every
        alpha plane runs through the network) or N bools; the tensor is never read back to find out."""
        x = self._check_u8_tensor(x_u8, "upscale_rgba_u8_tensor", on_device=False, channels=4)
        n = int(x.shape[0])
        if opaque is None:
            opaque = [False] * n
        else:
            opaque = list(opaque)
            if len(opaque) != n or not all(isinstance(f, (bool, np.bool_)) for f in opaque):
                raise ValueError("larvanet_amd: opaque must be None or %d bools (one per image), got %r" % (n, opaque))
        size = self._output_size(output_size, x.shape[1], x.shape[2])
        _require_hip(x)
        with torch.no_grad():
            return self._infer_rgba(x, opaque, lambda planes: self._infer_rgb(planes, size, self._infer_u8_checked))

    # ------------------------------------------------------------------ video: planar YUV 4:2:0 frames in and out
    def _check_yuv_args(self, width, height, matrix, full_range, scale=None):
        """Host-side checks shared by the video entry points (before any device work) -> (W, H, LR frame bytes)."""
        if scale is not None:
            self._check_scale(scale)
        if matrix not in YUV_MATRICES:
            raise ValueError("larvanet_amd: matrix must be one of %s, got %r" % (sorted(YUV_MATRICES), matrix))
        if not isinstance(full_range, (bool, np.bool_)):
            raise TypeError("larvanet_amd: full_range must be True or False, got %r" % (full_range,))
        width, height = int(width), int(height)
        return width, height, i420_frame_bytes(width, height)

    def _infer_i420(self, buf_u8, width, height, matrix, full_range, size, infer, out=None):
        """uint8 [N][frame bytes] I420 frames of width x height on the device -> their uint8 [N][HR frame bytes] frames in
        `out` or a new tensor: frame -> float planes -> _infer_rgb(planes, size, infer) -> frame.  The two conversions are
        launches of their own, outside the forward's cached graph."""
        x = K.i420_to_rgb_f32(buf_u8, width, height, matrix, full_range)
        return K.rgb_u8_to_i420(self._infer_rgb(x, size, infer), matrix, full_range, out=out)

    def upscale_yuv420_tensor(self, buf_u8, width, height, matrix="bt601", full_range=False, output_size=None):
        """uint8 [N][frame bytes] on self.device, N I420 frames of width x height (image_utils.i420_frame_bytes) ->
        uint8 [N][HR frame bytes], the frames of (s width) x (s height).  Byte for byte
        rgb_u8_to_i420(f32_chw_to_u8_hwc(forward(i420_to_rgb_f32(frame)))) of image_utils, forward the inference at this
        model's precision (fp16 overflow raises FloatingPointError; --self_ensemble is honoured).  output_size = (height,
        width): the uint8 RGB image goes through image_utils.resize_u8 before rgb_u8_to_i420, and the frames are of that
        size (odd sizes included)."""
        width, height, nbytes = self._check_yuv_args(width, height, matrix, full_range)
        size = self._output_size(output_size, height, width)
        _require_u8_tensor(buf_u8, "upscale_yuv420_tensor")
        if buf_u8.dim() != 2 or buf_u8.shape[0] < 1 or buf_u8.shape[1] != nbytes:
            raise ValueError("larvanet_amd: upscale_yuv420_tensor takes [N][%d] (I420 frames of %d x %d), got shape %s"
                             % (nbytes, width, height, tuple(buf_u8.shape)))
        _require_hip(buf_u8)
        with torch.no_grad():
            return self._infer_i420(buf_u8.contiguous(), width, height, matrix, bool(full_range), size, self._infer_u8_checked)

    def upscale_yuv420(self, frames, scale, width, height, matrix="bt601", full_range=False, output_size=None):
        """list of uint8 1-D numpy I420 frames of width x height -> list of the uint8 1-D HR frames of (s width) x
        (s height), or of output_size = (height, width): upscale_yuv420_tensor with the trips over the host link, 1.5
        bytes per pixel each way."""
        width, height, nbytes = self._check_yuv_args(width, height, matrix, full_range, scale)
        self._output_size(output_size, height, width)
        if isinstance(frames, np.ndarray) or not len(frames):
            raise ValueError("larvanet_amd: upscale_yuv420 takes a non-empty list of 1-D uint8 frames")
        for f in frames:
            check_i420_frame(f, "upscale_yuv420", nbytes, width, height, one_size=True)
        buf = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(self.device)
        _require_hip(buf)
        return list(self.upscale_yuv420_tensor(buf, width, height, matrix, full_range, output_size).cpu().numpy())

    # ------------------------------------------------------------------ every exit's image from one forward pass
    def _check_exits(self):
        """Refusals of the all-exit entry points, before any device work: a route without per-body exits (ValueError
        naming the model) and --self_ensemble, which is not built for all exits."""
        self.model.exit_route()
        if self._self_ensemble():
            raise ValueError("larvanet_amd: --self_ensemble together with all-exit inference is not supported; run "
                             "one of the two")

    def upscale_exits(self, input_list, scale):
        """upscale() for every exit of the route: list of CHW numpy images -> (M, N, 3, sH, sW) float32 numpy, index 0
        the first exit.  Exit i is bit for bit upscale() of a LarvaLeg --leg=i+1 plugin with these weights; the head and
        the bodies run once."""
        self._check_exits()
        self._check_scale(scale)
        with torch.no_grad():
            return self._infer_checked(self._to_input_tensor(input_list), ensemble=False, exits=True).detach().cpu().numpy()

    def upscale_exits_tensor(self, input_list):
        """upscale_exits() without the trip to the host: (M, N, 3, sH, sW) float32 on self.device."""
        self._check_exits()
        with torch.no_grad():
            return self._infer_checked(self._to_input_tensor(input_list), ensemble=False, exits=True).detach().clone()

    def upscale_exits_u8(self, input_list, scale):
        """upscale_u8() for every exit: list of uint8 (H, W, 3) images of one shape -> uint8 (M, N, sH, sW, 3) numpy."""
        self._check_exits()
        batch = self._check_u8_images(input_list, scale)
        with torch.no_grad():
            x = torch.from_numpy(batch).to(self.device)
            _require_hip(x)
            return self._infer_checked(x, u8=True, ensemble=False, exits=True).cpu().numpy()

    def upscale_exits_u8_tensor(self, x_u8):
        """upscale_exits_u8 on the device: uint8 [N][H][W][3] -> uint8 [M][N][sH][sW][3]."""
        self._check_exits()
        x = self._check_u8_tensor(x_u8, "upscale_exits_u8_tensor")
        with torch.no_grad():
            return self._infer_checked(x, u8=True, ensemble=False, exits=True).clone()

    def evaluate_exits_u8_tensor(self, x_u8, truth_u8, shave=None, channel="y", ssim=True, return_images=False):
        """evaluate_u8_tensor() for every exit: per image a list of M {"psnr", "ssim", "sse", "n"} dicts, index 0 the
        first exit (kernels.u8_metrics per exit and image on what upscale_exits_u8_tensor returns).  return_images: ->
        (that list, the scored uint8 [M][N][sH][sW][3] images on the device)."""
        self._check_exits()
        x, truth, shave = self._check_evaluate_args("evaluate_exits_u8_tensor", x_u8, truth_u8, shave, channel, ssim)
        with torch.no_grad():
            out = self._infer_checked(x, u8=True, ensemble=False, exits=True)
            m_exits, n_images = int(out.shape[0]), int(out.shape[1])
            records = torch.stack([K.u8_metrics(out[i][n], truth[n], shave, channel, ssim)
                                   for n in range(n_images) for i in range(m_exits)])
            images = out.clone() if return_images else None
        recs = records.cpu().numpy()
        results = [[K.metrics_from_record(recs[n * m_exits + i]) for i in range(m_exits)] for n in range(n_images)]
        return (results, images) if return_images else results

    def test(self, input_list):
        if torch.is_grad_enabled():
            return self.model(self._to_input_tensor(input_list))
        return self._infer_checked(self._to_input_tensor(input_list), ensemble=False).clone()

    def fwd_runtime(self, input_tensor):
        """models/LarvaNet.py:200-202; under torch.no_grad() a repeated shape replays a captured graph and
        the result is that graph's output buffer (overwritten by the next call)."""
        return self._infer(input_tensor)
