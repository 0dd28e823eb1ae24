"""Every refusal of the image entry points and of the three streams, word for word: exception type and full message are
literals recorded before the checks were folded into shared ones, so a shared check cannot change what a caller reads or
which of two refusals wins.  Host only: nothing here launches; the plugin is told it sits on the CPU, so a call whose
arguments pass ends in the "only runs on a HIP device" refusal wherever the suite runs.  Likewise the refusals of the
autograd modules for an input whose gradient they do not compute (the image, a leg's base, a loss's truth)."""
import gc

import numpy as np
import torch

W, H, NBYTES = 8, 6, 72   # one I420 frame of 8 x 6: 48 luma + 2 x 12 chroma bytes


def _model(extra=()):
    from larvanet_amd.models import LarvaNet as L
    gc.collect()
    m = L.create_model()
    m.parse_args(["--num_modules=2", "--num_blocks=1,1"] + list(extra))
    m.prepare(is_training=False, scales=[4])
    m.device = torch.device("cpu")

    def no_device_work(*a, **k):
        raise AssertionError("device work was started before the arguments were checked")

    m._eager_or_graph = no_device_work
    return m


def _cases(m, se):
    """[(label, call)]: m a plain x4 model, se one with --self_ensemble."""
    from larvanet_amd import pipeline as P
    rgb, rgb2 = np.zeros((H, W, 3), np.uint8), np.zeros((8, 8, 3), np.uint8)
    rgba, rgba2 = np.zeros((H, W, 4), np.uint8), np.zeros((8, 8, 4), np.uint8)
    f32 = np.float32
    t3, t4 = torch.from_numpy(rgb[None]), torch.from_numpy(rgba[None])
    truth = torch.zeros(1, 4 * H, 4 * W, 3, dtype=torch.uint8)
    small = torch.zeros(1, 4 * H - 1, 4 * W, 3, dtype=torch.uint8)
    frame = np.zeros(NBYTES, np.uint8)
    buf = torch.from_numpy(frame[None])
    far = (5, 32)   # the 24 x 32 result would shrink by more than 4

    def lists(name, call, good, good2, other):
        """The list checks of upscale_u8 / upscale_rgba_u8 / upscale_exits_u8: call(input_list, scale, **kw)."""
        return [
            (name + ": wrong scale", lambda: call([good], 2)),
            (name + ": wrong scale, unparsable", lambda: call([good], 8)),
            (name + ": wrong scale beats an empty list", lambda: call([], 3)),
            (name + ": empty list", lambda: call([], 4)),
            (name + ": an array, not a list", lambda: call(good[None], 4)),
            (name + ": wrong dtype", lambda: call([good.astype(f32)], 4)),
            (name + ": not an array", lambda: call([[1, 2]], 4)),
            (name + ": wrong rank", lambda: call([good[..., 0]], 4)),
            (name + ": wrong channel count", lambda: call([other], 4)),
            (name + ": empty image", lambda: call([good[:0]], 4)),
            (name + ": mixed shapes", lambda: call([good, good2], 4)),
            (name + ": wrong dtype beats wrong shape", lambda: call([other.astype(f32)], 4)),
            (name + ": first bad image wins", lambda: call([good, other, good.astype(f32)], 4)),
        ]

    def sizes(name, call, every=False):
        """The output_size refusals: call(output_size); every: all that image_utils.check_output_size knows."""
        return [
            (name + ": output_size out of ratio", lambda: call(far)),
            (name + ": output_size not a pair", lambda: call((5,))),
        ] + ([
            (name + ": output_size a string", lambda: call("32x24")),
            (name + ": output_size fractional", lambda: call((20.5, 30))),
            (name + ": output_size below 1", lambda: call((0, 30))),
        ] if every else [])

    def tensors(name, call, good, other):
        """The tensor checks: call(x)."""
        return [
            (name + ": a numpy array", lambda: call(good.numpy())),
            (name + ": wrong dtype", lambda: call(good.float())),
            (name + ": wrong rank", lambda: call(good[0])),
            (name + ": wrong channel count", lambda: call(other)),
            (name + ": empty batch", lambda: call(good[:0])),
            (name + ": wrong dtype beats wrong shape", lambda: call(other.float())),
            (name + ": a host tensor", lambda: call(good)),
        ]

    def evaluates(name, call):
        """call(x, truth, **kw) of evaluate_u8_tensor / evaluate_exits_u8_tensor."""
        return [
            (name + ": input wrong dtype", lambda: call(t3.float(), truth)),
            (name + ": truth wrong dtype", lambda: call(t3, truth.float())),
            (name + ": truth a numpy array", lambda: call(t3, truth.numpy())),
            (name + ": input wrong channel count", lambda: call(t4, truth)),
            (name + ": truth wrong rank", lambda: call(t3, truth[0])),
            (name + ": input beats truth", lambda: call(t4, truth[0])),
            (name + ": truth count", lambda: call(t3, torch.cat([truth, truth]))),
            (name + ": bad channel", lambda: call(t3, truth, channel="luma")),
            (name + ": truth count beats bad channel", lambda: call(t3, torch.cat([truth, truth]), channel="luma")),
            (name + ": truth too small", lambda: call(t3, small)),
            (name + ": bad channel beats truth too small", lambda: call(t3, small, channel="Y")),
            (name + ": negative shave", lambda: call(t3, truth, shave=-1)),
            (name + ": window too small for ssim", lambda: call(t3, truth, shave=8)),
            (name + ": host tensors", lambda: call(t3, truth)),
            (name + ": host tensors, no ssim", lambda: call(t3, truth, shave=8, ssim=False)),
        ]

    def yuv_args(name, call):
        """call(**kw) with width / height / matrix / full_range / output_size; good defaults inside."""
        return [
            (name + ": bad matrix", lambda: call(matrix="bt2020")),
            (name + ": bad full_range", lambda: call(full_range=1)),
            (name + ": bad matrix beats bad full_range", lambda: call(matrix=None, full_range="full")),
            (name + ": bad frame size", lambda: call(width=0)),
            (name + ": bad full_range beats bad frame size", lambda: call(full_range=None, height=0)),
        ]

    cases = []
    # ---- upscale_u8 / upscale_u8_tensor / evaluate_u8_tensor
    cases += lists("upscale_u8", m.upscale_u8, rgb, rgb2, rgba)
    cases += sizes("upscale_u8", lambda s: m.upscale_u8([rgb], 4, output_size=s), every=True)
    cases += [("upscale_u8: bad list beats bad output_size", lambda: m.upscale_u8([rgba], 4, output_size=far)),
              ("upscale_u8: wrong scale beats bad output_size", lambda: m.upscale_u8([rgb], 2, output_size=far)),
              ("upscale_u8: a host model", lambda: m.upscale_u8([rgb], 4))]
    cases += tensors("upscale_u8_tensor", m.upscale_u8_tensor, t3, t4)
    cases += sizes("upscale_u8_tensor", lambda s: m.upscale_u8_tensor(t3, output_size=s))
    cases += [("upscale_u8_tensor: wrong shape beats bad output_size", lambda: m.upscale_u8_tensor(t4, output_size=far))]
    cases += evaluates("evaluate_u8_tensor", m.evaluate_u8_tensor)
    # ---- upscale_rgba_u8 / upscale_rgba_u8_tensor
    cases += lists("upscale_rgba_u8", m.upscale_rgba_u8, rgba, rgba2, rgb)
    cases += sizes("upscale_rgba_u8", lambda s: m.upscale_rgba_u8([rgba], 4, output_size=s))
    cases += [("upscale_rgba_u8: bad list beats bad output_size", lambda: m.upscale_rgba_u8([rgb], 4, output_size=far)),
              ("upscale_rgba_u8: a host model", lambda: m.upscale_rgba_u8([rgba], 4))]
    cases += tensors("upscale_rgba_u8_tensor", m.upscale_rgba_u8_tensor, t4, t3)
    cases += sizes("upscale_rgba_u8_tensor", lambda s: m.upscale_rgba_u8_tensor(t4, output_size=s))
    for i, bad in enumerate(([], [True, False], [1], "n", [None])):
        cases.append(("upscale_rgba_u8_tensor: bad opaque %d" % i, lambda bad=bad: m.upscale_rgba_u8_tensor(t4, opaque=bad)))
    cases += [("upscale_rgba_u8_tensor: wrong shape beats bad opaque", lambda: m.upscale_rgba_u8_tensor(t3, opaque=[1])),
              ("upscale_rgba_u8_tensor: bad opaque beats bad output_size",
               lambda: m.upscale_rgba_u8_tensor(t4, opaque=[], output_size=far)),
              ("upscale_rgba_u8_tensor: a host tensor, opaque given", lambda: m.upscale_rgba_u8_tensor(t4, opaque=[False]))]
    # ---- upscale_yuv420 / upscale_yuv420_tensor
    def yuv(frames=None, scale=4, width=W, height=H, **kw):
        return m.upscale_yuv420([frame] if frames is None else frames, scale, width, height, **kw)

    def yuv_t(x=buf, width=W, height=H, **kw):
        return m.upscale_yuv420_tensor(x, width, height, **kw)

    cases += [("upscale_yuv420: wrong scale", lambda: yuv(scale=2)),
              ("upscale_yuv420: wrong scale beats bad matrix", lambda: yuv(scale=3, matrix="bt2020"))]
    cases += yuv_args("upscale_yuv420", yuv)
    cases += sizes("upscale_yuv420", lambda s: yuv(output_size=s))
    cases += [
        ("upscale_yuv420: empty list", lambda: yuv(frames=[])),
        ("upscale_yuv420: an array, not a list", lambda: yuv(frames=frame[None])),
        ("upscale_yuv420: wrong dtype", lambda: yuv(frames=[frame.astype(f32)])),
        ("upscale_yuv420: not an array", lambda: yuv(frames=[b"\0" * NBYTES])),
        ("upscale_yuv420: wrong size", lambda: yuv(frames=[frame[:-1]])),
        ("upscale_yuv420: wrong rank", lambda: yuv(frames=[frame.reshape(9, 8)])),
        ("upscale_yuv420: mixed sizes", lambda: yuv(frames=[frame, np.zeros(NBYTES + 8, np.uint8)])),
        ("upscale_yuv420: wrong dtype beats wrong size", lambda: yuv(frames=[frame[:-1].astype(f32)])),
        ("upscale_yuv420: bad output_size beats an empty list", lambda: yuv(frames=[], output_size=far)),
        ("upscale_yuv420: bad frame size beats bad output_size", lambda: yuv(width=-1, output_size=far)),
        ("upscale_yuv420: a host model", lambda: yuv()),
    ]
    cases += yuv_args("upscale_yuv420_tensor", yuv_t)
    cases += sizes("upscale_yuv420_tensor", lambda s: yuv_t(output_size=s))
    cases += [
        ("upscale_yuv420_tensor: a numpy array", lambda: yuv_t(frame[None])),
        ("upscale_yuv420_tensor: wrong dtype", lambda: yuv_t(buf.float())),
        ("upscale_yuv420_tensor: wrong rank", lambda: yuv_t(buf[0])),
        ("upscale_yuv420_tensor: wrong size", lambda: yuv_t(buf[:, :-1])),
        ("upscale_yuv420_tensor: empty batch", lambda: yuv_t(buf[:0])),
        ("upscale_yuv420_tensor: bad output_size beats wrong dtype", lambda: yuv_t(buf.float(), output_size=far)),
        ("upscale_yuv420_tensor: a host tensor", lambda: yuv_t()),
    ]
    # ---- every exit
    chw = np.zeros((3, H, W), f32)
    cases += [
        ("upscale_exits: wrong scale", lambda: m.upscale_exits([chw], 2)),
        ("upscale_exits: --self_ensemble", lambda: se.upscale_exits([chw], 4)),
        ("upscale_exits: --self_ensemble beats wrong scale", lambda: se.upscale_exits([chw], 2)),
        ("upscale_exits_tensor: --self_ensemble", lambda: se.upscale_exits_tensor([chw])),
        ("upscale_exits_u8: --self_ensemble beats wrong scale", lambda: se.upscale_exits_u8([rgb], 2)),
        ("upscale_exits_u8: a host model", lambda: m.upscale_exits_u8([rgb], 4)),
        ("upscale_exits_u8_tensor: --self_ensemble beats wrong dtype", lambda: se.upscale_exits_u8_tensor(t3.float())),
        ("evaluate_exits_u8_tensor: --self_ensemble beats wrong dtype", lambda: se.evaluate_exits_u8_tensor(t3.float(), truth)),
    ]
    cases += lists("upscale_exits_u8", m.upscale_exits_u8, rgb, rgb2, rgba)
    cases += tensors("upscale_exits_u8_tensor", m.upscale_exits_u8_tensor, t3, t4)
    cases += evaluates("evaluate_exits_u8_tensor", m.evaluate_exits_u8_tensor)
    # ---- the streams: what they refuse when they are called ...
    cases += [
        ("upscale_stream: depth", lambda: P.upscale_stream(m, [rgb], 4, depth=0)),
        ("upscale_stream: depth beats wrong scale", lambda: P.upscale_stream(m, [rgb], 2, depth=0)),
        ("upscale_stream: wrong scale", lambda: P.upscale_stream(m, [rgb], 2)),
        ("upscale_stream: bad output_size beats wrong scale", lambda: P.upscale_stream(m, [rgb], 2, output_size=(5,))),
        ("upscale_stream: a host model", lambda: P.upscale_stream(m, [rgb], 4, output_size=far, keep_alpha=True)),
        ("evaluate_stream: depth", lambda: P.evaluate_stream(m, [], 4, depth=0)),
        ("evaluate_stream: wrong scale", lambda: P.evaluate_stream(m, [], 3)),
        ("evaluate_stream: wrong scale beats bad channel", lambda: P.evaluate_stream(m, [], 3, channel="luma")),
        ("evaluate_stream: bad channel", lambda: P.evaluate_stream(m, [], 4, channel="luma")),
        ("evaluate_stream: bad channel beats negative shave", lambda: P.evaluate_stream(m, [], 4, channel="luma", shave=-1)),
        ("evaluate_stream: negative shave", lambda: P.evaluate_stream(m, [], 4, shave=-1)),
        ("evaluate_stream: a host model", lambda: P.evaluate_stream(m, [], 4)),
        ("upscale_yuv_stream: depth", lambda: P.upscale_yuv_stream(m, [], 4, W, H, depth=0)),
        ("upscale_yuv_stream: output_size out of ratio", lambda: P.upscale_yuv_stream(m, [], 4, W, H, output_size=far)),
        ("upscale_yuv_stream: bad output_size beats width alone",
         lambda: P.upscale_yuv_stream(m, [], 4, W, None, output_size=(5,))),
        ("upscale_yuv_stream: width alone", lambda: P.upscale_yuv_stream(m, [], 4, width=W)),
        ("upscale_yuv_stream: height alone", lambda: P.upscale_yuv_stream(m, [], 4, height=H)),
        ("upscale_yuv_stream: width alone beats wrong scale", lambda: P.upscale_yuv_stream(m, [], 2, width=W)),
        ("upscale_yuv_stream: wrong scale", lambda: P.upscale_yuv_stream(m, [], 2, W, H)),
        ("upscale_yuv_stream: wrong scale beats bad matrix", lambda: P.upscale_yuv_stream(m, [], 2, W, H, matrix="x")),
        ("upscale_yuv_stream: bad matrix", lambda: P.upscale_yuv_stream(m, [], 4, W, H, matrix="x")),
        ("upscale_yuv_stream: bad matrix, sizes per frame", lambda: P.upscale_yuv_stream(m, [], 4, matrix="x")),
        ("upscale_yuv_stream: bad full_range", lambda: P.upscale_yuv_stream(m, [], 4, W, H, full_range=0)),
        ("upscale_yuv_stream: bad frame size", lambda: P.upscale_yuv_stream(m, [], 4, 0, H)),
        ("upscale_yuv_stream: a host model", lambda: P.upscale_yuv_stream(m, [], 4, W, H)),
        ("upscale_yuv_stream: a host model, sizes per frame", lambda: P.upscale_yuv_stream(m, [], 4)),
    ]
    # ---- ... and what they refuse item by item, before anything of the item is launched
    cases += [
        ("stream image: wrong dtype", lambda: P._check_image(rgb.astype(f32))),
        ("stream image: not an array", lambda: P._check_image([rgb])),
        ("stream image: four channels", lambda: P._check_image(rgba)),
        ("stream image: wrong rank", lambda: P._check_image(rgb[..., 0])),
        ("stream image: empty", lambda: P._check_image(rgb[:, :0])),
        ("stream image: evaluate_stream wrong dtype", lambda: P._check_image(rgb.astype(f32), "evaluate_stream")),
        ("stream image: evaluate_stream four channels", lambda: P._check_image(rgba, "evaluate_stream")),
        ("stream image: keep_alpha wrong dtype", lambda: P._check_image(rgba.astype(f32), keep_alpha=True)),
        ("stream image: keep_alpha two channels", lambda: P._check_image(rgba[..., :2], keep_alpha=True)),
        ("stream image: keep_alpha wrong rank", lambda: P._check_image(rgba[..., 0], keep_alpha=True)),
        ("stream image: keep_alpha empty", lambda: P._check_image(rgba[:0], keep_alpha=True)),
        ("stream frame: wrong dtype", lambda: P._check_frame(frame.astype(f32), NBYTES, W, H)),
        ("stream frame: not an array", lambda: P._check_frame(bytes(NBYTES), NBYTES, W, H)),
        ("stream frame: wrong size", lambda: P._check_frame(frame[:-1], NBYTES, W, H)),
        ("stream frame: wrong rank", lambda: P._check_frame(frame.reshape(9, 8), NBYTES, W, H)),
        ("stream frame: wrong dtype beats wrong size", lambda: P._check_frame(frame[:-1].astype(f32), NBYTES, W, H)),
    ]
    # ---- inputs whose gradient the autograd nodes do not compute: refused where torch would return one, never a silent
    # None; under no_grad the same tensors pass (and end, on the host, in the no-CPU-fallback refusal)
    from larvanet_amd.models import LarvaNet as L1, LarvaNetV2 as L2
    net, leg, tail = m.model, m.model.body_0.leg, L2.LarvaTail(2)
    xg = torch.zeros(1, 3, H, W, requires_grad=True)
    fea, hr = torch.zeros(1, 48, H, W), torch.zeros(1, 3, 4 * H, 4 * W)
    hrg = torch.zeros(1, 3, 4 * H, 4 * W, requires_grad=True)

    def no_grad(call):
        def run():
            with torch.no_grad():
                return call()
        return run

    needs = [
        ("head: the image needs a gradient", lambda: net.head(xg)),
        ("network: the image needs a gradient", lambda: net(xg)),
        ("all exits: the image needs a gradient", lambda: net.forward_exits(xg)),
        ("base: the image needs a gradient", lambda: net.base(xg)),
        ("leg: the base needs a gradient", lambda: leg(fea, hrg)),
        ("tail: the base needs a gradient", lambda: tail([fea, fea], hrg)),
        ("run_leg: the base needs a gradient", lambda: L1.run_leg(leg, fea, hrg, hr, 2)),
        ("run_leg: the truth needs a gradient", lambda: L1.run_leg(leg, fea, hr, hrg, 2)),
        ("run_leg: the base beats the truth", lambda: L1.run_leg(tail, [fea, fea], hrg, hrg)),
        ("batched exits: the base needs a gradient", lambda: m._all_exits([fea, fea], hrg, hr)),
        ("batched exits: the truth needs a gradient", lambda: m._all_exits([fea, fea], hr, hrg)),
        ("L1Loss: the truth needs a gradient", lambda: L1.L1Loss()(hr, hrg)),
    ]
    cases += needs
    # (run_leg and the batched exits are internal: they leave the device check to the modules that call them)
    cases += [(label + ", under no_grad", no_grad(call)) for label, call in needs
              if not label.startswith(("run_leg", "batched exits"))]
    return cases


V, T, R = ValueError, TypeError, RuntimeError
P_ = "larvanet_amd: "
NO_HIP = (R, P_ + "the network only runs on a HIP device (MI355X); got a cpu tensor and there is no CPU fallback")
NO_GRAD = P_ + "the gradient of %s is not computed by %s; detach() it, or call under torch.no_grad()"
RATIO = (V, P_ + "resizing shrinks an axis by at most 4, got 24 x 32 -> 5 x 32 (height x width)")
NOT_A_PAIR = (T, P_ + "output_size is (height, width) or None, got (5,)")
ENSEMBLE = (V, P_ + "--self_ensemble together with all-exit inference is not supported; run one of the two")
BY_2, BY_3, BY_8 = ((V, P_ + "this model upscales by 4, not by %d" % s) for s in (2, 3, 8))
LUMA = (V, P_ + "channel must be 'y' or 'rgb', got 'luma'")
TRIPLES = (V, P_ + "upscale_yuv_stream takes width and height, or neither (items are then (frame, width, height) triples)")

EXPECTED = {
    "upscale_u8: wrong scale": BY_2,
    "upscale_u8: wrong scale, unparsable": BY_8,
    "upscale_u8: wrong scale beats an empty list": BY_3,
    "upscale_u8: empty list": (V, P_ + "upscale_u8 takes a non-empty list of (H, W, 3) uint8 arrays"),
    "upscale_u8: an array, not a list": (V, P_ + "upscale_u8 takes a non-empty list of (H, W, 3) uint8 arrays"),
    "upscale_u8: wrong dtype": (T, P_ + "upscale_u8 takes uint8 numpy arrays (decoded images), got float32"),
    "upscale_u8: not an array": (T, P_ + "upscale_u8 takes uint8 numpy arrays (decoded images), got list"),
    "upscale_u8: wrong rank": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (6, 8)"),
    "upscale_u8: wrong channel count": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (6, 8, 4)"),
    "upscale_u8: empty image": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (0, 8, 3)"),
    "upscale_u8: mixed shapes":
        (V, P_ + "the images of one upscale_u8 call must have one shape, got (6, 8, 3) and (8, 8, 3)"),
    "upscale_u8: wrong dtype beats wrong shape":
        (T, P_ + "upscale_u8 takes uint8 numpy arrays (decoded images), got float32"),
    "upscale_u8: first bad image wins": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (6, 8, 4)"),
    "upscale_u8: output_size out of ratio": RATIO,
    "upscale_u8: output_size not a pair": NOT_A_PAIR,
    "upscale_u8: output_size a string": (T, P_ + "output_size is (height, width) or None, got '32x24'"),
    "upscale_u8: output_size fractional": (T, P_ + "output_size is (height, width) in whole pixels, got (20.5, 30)"),
    "upscale_u8: output_size below 1": (V, P_ + "resizing needs sizes >= 1, got 24 x 32 -> 0 x 30 (height x width)"),
    "upscale_u8: bad list beats bad output_size": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (6, 8, 4)"),
    "upscale_u8: wrong scale beats bad output_size": BY_2,
    "upscale_u8: a host model": NO_HIP,
    "upscale_u8_tensor: a numpy array": (T, P_ + "upscale_u8_tensor takes a uint8 tensor, got uint8"),
    "upscale_u8_tensor: wrong dtype": (T, P_ + "upscale_u8_tensor takes a uint8 tensor, got torch.float32"),
    "upscale_u8_tensor: wrong rank": (V, P_ + "upscale_u8_tensor takes [N][H][W][3], got shape (6, 8, 3)"),
    "upscale_u8_tensor: wrong channel count": (V, P_ + "upscale_u8_tensor takes [N][H][W][3], got shape (1, 6, 8, 4)"),
    "upscale_u8_tensor: empty batch": (V, P_ + "upscale_u8_tensor takes [N][H][W][3], got shape (0, 6, 8, 3)"),
    "upscale_u8_tensor: wrong dtype beats wrong shape":
        (T, P_ + "upscale_u8_tensor takes a uint8 tensor, got torch.float32"),
    "upscale_u8_tensor: a host tensor": NO_HIP,
    "upscale_u8_tensor: output_size out of ratio": RATIO,
    "upscale_u8_tensor: output_size not a pair": NOT_A_PAIR,
    "upscale_u8_tensor: wrong shape beats bad output_size":
        (V, P_ + "upscale_u8_tensor takes [N][H][W][3], got shape (1, 6, 8, 4)"),
    "evaluate_u8_tensor: input wrong dtype": (T, P_ + "evaluate_u8_tensor takes a uint8 tensor, got torch.float32"),
    "evaluate_u8_tensor: truth wrong dtype": (T, P_ + "evaluate_u8_tensor takes a uint8 tensor, got torch.float32"),
    "evaluate_u8_tensor: truth a numpy array": (T, P_ + "evaluate_u8_tensor takes a uint8 tensor, got uint8"),
    "evaluate_u8_tensor: input wrong channel count":
        (V, P_ + "evaluate_u8_tensor takes [N][H][W][3], got shape (1, 6, 8, 4)"),
    "evaluate_u8_tensor: truth wrong rank": (V, P_ + "evaluate_u8_tensor takes [N][H][W][3], got shape (24, 32, 3)"),
    "evaluate_u8_tensor: input beats truth": (V, P_ + "evaluate_u8_tensor takes [N][H][W][3], got shape (1, 6, 8, 4)"),
    "evaluate_u8_tensor: truth count":
        (V, P_ + "evaluate_u8_tensor takes as many truth images as inputs, got 2 and 1"),
    "evaluate_u8_tensor: bad channel": LUMA,
    "evaluate_u8_tensor: truth count beats bad channel":
        (V, P_ + "evaluate_u8_tensor takes as many truth images as inputs, got 2 and 1"),
    "evaluate_u8_tensor: truth too small": (V, P_ + "the truth image (23 x 32) is smaller than the output (24 x 32)"),
    "evaluate_u8_tensor: bad channel beats truth too small": (V, P_ + "channel must be 'y' or 'rgb', got 'Y'"),
    "evaluate_u8_tensor: negative shave": (V, P_ + "metrics need shave >= 0, got -1"),
    "evaluate_u8_tensor: window too small for ssim":
        (V, P_ + "SSIM needs a window of at least 11 x 11 pixels, got 8 x 16"),
    "evaluate_u8_tensor: host tensors": NO_HIP,
    "evaluate_u8_tensor: host tensors, no ssim": NO_HIP,
    "upscale_rgba_u8: wrong scale": BY_2,
    "upscale_rgba_u8: wrong scale, unparsable": BY_8,
    "upscale_rgba_u8: wrong scale beats an empty list": BY_3,
    "upscale_rgba_u8: empty list": (V, P_ + "upscale_rgba_u8 takes a non-empty list of (H, W, 4) uint8 arrays"),
    "upscale_rgba_u8: an array, not a list": (V, P_ + "upscale_rgba_u8 takes a non-empty list of (H, W, 4) uint8 arrays"),
    "upscale_rgba_u8: wrong dtype": (T, P_ + "upscale_rgba_u8 takes uint8 numpy arrays (decoded images), got float32"),
    "upscale_rgba_u8: not an array": (T, P_ + "upscale_rgba_u8 takes uint8 numpy arrays (decoded images), got list"),
    "upscale_rgba_u8: wrong rank": (V, P_ + "upscale_rgba_u8 takes (H, W, 4) images, got shape (6, 8)"),
    "upscale_rgba_u8: wrong channel count": (V, P_ + "upscale_rgba_u8 takes (H, W, 4) images, got shape (6, 8, 3)"),
    "upscale_rgba_u8: empty image": (V, P_ + "upscale_rgba_u8 takes (H, W, 4) images, got shape (0, 8, 4)"),
    "upscale_rgba_u8: mixed shapes":
        (V, P_ + "the images of one upscale_rgba_u8 call must have one shape, got (6, 8, 4) and (8, 8, 4)"),
    "upscale_rgba_u8: wrong dtype beats wrong shape":
        (T, P_ + "upscale_rgba_u8 takes uint8 numpy arrays (decoded images), got float32"),
    "upscale_rgba_u8: first bad image wins": (V, P_ + "upscale_rgba_u8 takes (H, W, 4) images, got shape (6, 8, 3)"),
    "upscale_rgba_u8: output_size out of ratio": RATIO,
    "upscale_rgba_u8: output_size not a pair": NOT_A_PAIR,
    "upscale_rgba_u8: bad list beats bad output_size":
        (V, P_ + "upscale_rgba_u8 takes (H, W, 4) images, got shape (6, 8, 3)"),
    "upscale_rgba_u8: a host model": NO_HIP,
    "upscale_rgba_u8_tensor: a numpy array": (T, P_ + "upscale_rgba_u8_tensor takes a uint8 tensor, got uint8"),
    "upscale_rgba_u8_tensor: wrong dtype": (T, P_ + "upscale_rgba_u8_tensor takes a uint8 tensor, got torch.float32"),
    "upscale_rgba_u8_tensor: wrong rank": (V, P_ + "upscale_rgba_u8_tensor takes [N][H][W][4], got shape (6, 8, 4)"),
    "upscale_rgba_u8_tensor: wrong channel count":
        (V, P_ + "upscale_rgba_u8_tensor takes [N][H][W][4], got shape (1, 6, 8, 3)"),
    "upscale_rgba_u8_tensor: empty batch": (V, P_ + "upscale_rgba_u8_tensor takes [N][H][W][4], got shape (0, 6, 8, 4)"),
    "upscale_rgba_u8_tensor: wrong dtype beats wrong shape":
        (T, P_ + "upscale_rgba_u8_tensor takes a uint8 tensor, got torch.float32"),
    "upscale_rgba_u8_tensor: a host tensor": NO_HIP,
    "upscale_rgba_u8_tensor: output_size out of ratio": RATIO,
    "upscale_rgba_u8_tensor: output_size not a pair": NOT_A_PAIR,
    "upscale_rgba_u8_tensor: bad opaque 0": (V, P_ + "opaque must be None or 1 bools (one per image), got []"),
    "upscale_rgba_u8_tensor: bad opaque 1": (V, P_ + "opaque must be None or 1 bools (one per image), got [True, False]"),
    "upscale_rgba_u8_tensor: bad opaque 2": (V, P_ + "opaque must be None or 1 bools (one per image), got [1]"),
    "upscale_rgba_u8_tensor: bad opaque 3": (V, P_ + "opaque must be None or 1 bools (one per image), got ['n']"),
    "upscale_rgba_u8_tensor: bad opaque 4": (V, P_ + "opaque must be None or 1 bools (one per image), got [None]"),
    "upscale_rgba_u8_tensor: wrong shape beats bad opaque":
        (V, P_ + "upscale_rgba_u8_tensor takes [N][H][W][4], got shape (1, 6, 8, 3)"),
    "upscale_rgba_u8_tensor: bad opaque beats bad output_size":
        (V, P_ + "opaque must be None or 1 bools (one per image), got []"),
    "upscale_rgba_u8_tensor: a host tensor, opaque given": NO_HIP,
    "upscale_yuv420: wrong scale": BY_2,
    "upscale_yuv420: wrong scale beats bad matrix": BY_3,
    "upscale_yuv420: bad matrix": (V, P_ + "matrix must be one of ['bt601', 'bt709'], got 'bt2020'"),
    "upscale_yuv420: bad full_range": (T, P_ + "full_range must be True or False, got 1"),
    "upscale_yuv420: bad matrix beats bad full_range": (V, P_ + "matrix must be one of ['bt601', 'bt709'], got None"),
    "upscale_yuv420: bad frame size": (V, P_ + "a frame needs width and height >= 1, got 0 x 6"),
    "upscale_yuv420: bad full_range beats bad frame size": (T, P_ + "full_range must be True or False, got None"),
    "upscale_yuv420: output_size out of ratio": RATIO,
    "upscale_yuv420: output_size not a pair": NOT_A_PAIR,
    "upscale_yuv420: empty list": (V, P_ + "upscale_yuv420 takes a non-empty list of 1-D uint8 frames"),
    "upscale_yuv420: an array, not a list": (V, P_ + "upscale_yuv420 takes a non-empty list of 1-D uint8 frames"),
    "upscale_yuv420: wrong dtype": (T, P_ + "upscale_yuv420 takes uint8 numpy frames, got float32"),
    "upscale_yuv420: not an array": (T, P_ + "upscale_yuv420 takes uint8 numpy frames, got bytes"),
    "upscale_yuv420: wrong size":
        (V, P_ + "an I420 frame of 8 x 6 is a flat buffer of 72 bytes (one size per call), got shape (71,)"),
    "upscale_yuv420: wrong rank":
        (V, P_ + "an I420 frame of 8 x 6 is a flat buffer of 72 bytes (one size per call), got shape (9, 8)"),
    "upscale_yuv420: mixed sizes":
        (V, P_ + "an I420 frame of 8 x 6 is a flat buffer of 72 bytes (one size per call), got shape (80,)"),
    "upscale_yuv420: wrong dtype beats wrong size": (T, P_ + "upscale_yuv420 takes uint8 numpy frames, got float32"),
    "upscale_yuv420: bad output_size beats an empty list": RATIO,
    "upscale_yuv420: bad frame size beats bad output_size": (V, P_ + "a frame needs width and height >= 1, got -1 x 6"),
    "upscale_yuv420: a host model": NO_HIP,
    "upscale_yuv420_tensor: bad matrix": (V, P_ + "matrix must be one of ['bt601', 'bt709'], got 'bt2020'"),
    "upscale_yuv420_tensor: bad full_range": (T, P_ + "full_range must be True or False, got 1"),
    "upscale_yuv420_tensor: bad matrix beats bad full_range":
        (V, P_ + "matrix must be one of ['bt601', 'bt709'], got None"),
    "upscale_yuv420_tensor: bad frame size": (V, P_ + "a frame needs width and height >= 1, got 0 x 6"),
    "upscale_yuv420_tensor: bad full_range beats bad frame size": (T, P_ + "full_range must be True or False, got None"),
    "upscale_yuv420_tensor: output_size out of ratio": RATIO,
    "upscale_yuv420_tensor: output_size not a pair": NOT_A_PAIR,
    "upscale_yuv420_tensor: a numpy array": (T, P_ + "upscale_yuv420_tensor takes a uint8 tensor, got uint8"),
    "upscale_yuv420_tensor: wrong dtype": (T, P_ + "upscale_yuv420_tensor takes a uint8 tensor, got torch.float32"),
    "upscale_yuv420_tensor: wrong rank":
        (V, P_ + "upscale_yuv420_tensor takes [N][72] (I420 frames of 8 x 6), got shape (72,)"),
    "upscale_yuv420_tensor: wrong size":
        (V, P_ + "upscale_yuv420_tensor takes [N][72] (I420 frames of 8 x 6), got shape (1, 71)"),
    "upscale_yuv420_tensor: empty batch":
        (V, P_ + "upscale_yuv420_tensor takes [N][72] (I420 frames of 8 x 6), got shape (0, 72)"),
    "upscale_yuv420_tensor: bad output_size beats wrong dtype": RATIO,
    "upscale_yuv420_tensor: a host tensor": NO_HIP,
    "upscale_exits: wrong scale": BY_2,
    "upscale_exits: --self_ensemble": ENSEMBLE,
    "upscale_exits: --self_ensemble beats wrong scale": ENSEMBLE,
    "upscale_exits_tensor: --self_ensemble": ENSEMBLE,
    "upscale_exits_u8: --self_ensemble beats wrong scale": ENSEMBLE,
    "upscale_exits_u8: a host model": NO_HIP,
    "upscale_exits_u8_tensor: --self_ensemble beats wrong dtype": ENSEMBLE,
    "evaluate_exits_u8_tensor: --self_ensemble beats wrong dtype": ENSEMBLE,
    # (upscale_exits_u8 shares upscale_u8's list check, and says so)
    "upscale_exits_u8: wrong scale": BY_2,
    "upscale_exits_u8: wrong scale, unparsable": BY_8,
    "upscale_exits_u8: wrong scale beats an empty list": BY_3,
    "upscale_exits_u8: empty list": (V, P_ + "upscale_u8 takes a non-empty list of (H, W, 3) uint8 arrays"),
    "upscale_exits_u8: an array, not a list": (V, P_ + "upscale_u8 takes a non-empty list of (H, W, 3) uint8 arrays"),
    "upscale_exits_u8: wrong dtype": (T, P_ + "upscale_u8 takes uint8 numpy arrays (decoded images), got float32"),
    "upscale_exits_u8: not an array": (T, P_ + "upscale_u8 takes uint8 numpy arrays (decoded images), got list"),
    "upscale_exits_u8: wrong rank": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (6, 8)"),
    "upscale_exits_u8: wrong channel count": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (6, 8, 4)"),
    "upscale_exits_u8: empty image": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (0, 8, 3)"),
    "upscale_exits_u8: mixed shapes":
        (V, P_ + "the images of one upscale_u8 call must have one shape, got (6, 8, 3) and (8, 8, 3)"),
    "upscale_exits_u8: wrong dtype beats wrong shape":
        (T, P_ + "upscale_u8 takes uint8 numpy arrays (decoded images), got float32"),
    "upscale_exits_u8: first bad image wins": (V, P_ + "upscale_u8 takes (H, W, 3) images, got shape (6, 8, 4)"),
    "upscale_exits_u8_tensor: a numpy array": (T, P_ + "upscale_exits_u8_tensor takes a uint8 tensor, got uint8"),
    "upscale_exits_u8_tensor: wrong dtype": (T, P_ + "upscale_exits_u8_tensor takes a uint8 tensor, got torch.float32"),
    "upscale_exits_u8_tensor: wrong rank": (V, P_ + "upscale_exits_u8_tensor takes [N][H][W][3], got shape (6, 8, 3)"),
    "upscale_exits_u8_tensor: wrong channel count":
        (V, P_ + "upscale_exits_u8_tensor takes [N][H][W][3], got shape (1, 6, 8, 4)"),
    "upscale_exits_u8_tensor: empty batch":
        (V, P_ + "upscale_exits_u8_tensor takes [N][H][W][3], got shape (0, 6, 8, 3)"),
    "upscale_exits_u8_tensor: wrong dtype beats wrong shape":
        (T, P_ + "upscale_exits_u8_tensor takes a uint8 tensor, got torch.float32"),
    "upscale_exits_u8_tensor: a host tensor": NO_HIP,
    "evaluate_exits_u8_tensor: input wrong dtype":
        (T, P_ + "evaluate_exits_u8_tensor takes a uint8 tensor, got torch.float32"),
    "evaluate_exits_u8_tensor: truth wrong dtype":
        (T, P_ + "evaluate_exits_u8_tensor takes a uint8 tensor, got torch.float32"),
    "evaluate_exits_u8_tensor: truth a numpy array": (T, P_ + "evaluate_exits_u8_tensor takes a uint8 tensor, got uint8"),
    "evaluate_exits_u8_tensor: input wrong channel count":
        (V, P_ + "evaluate_exits_u8_tensor takes [N][H][W][3], got shape (1, 6, 8, 4)"),
    "evaluate_exits_u8_tensor: truth wrong rank":
        (V, P_ + "evaluate_exits_u8_tensor takes [N][H][W][3], got shape (24, 32, 3)"),
    "evaluate_exits_u8_tensor: input beats truth":
        (V, P_ + "evaluate_exits_u8_tensor takes [N][H][W][3], got shape (1, 6, 8, 4)"),
    "evaluate_exits_u8_tensor: truth count":
        (V, P_ + "evaluate_exits_u8_tensor takes as many truth images as inputs, got 2 and 1"),
    "evaluate_exits_u8_tensor: bad channel": LUMA,
    "evaluate_exits_u8_tensor: truth count beats bad channel":
        (V, P_ + "evaluate_exits_u8_tensor takes as many truth images as inputs, got 2 and 1"),
    "evaluate_exits_u8_tensor: truth too small":
        (V, P_ + "the truth image (23 x 32) is smaller than the output (24 x 32)"),
    "evaluate_exits_u8_tensor: bad channel beats truth too small": (V, P_ + "channel must be 'y' or 'rgb', got 'Y'"),
    "evaluate_exits_u8_tensor: negative shave": (V, P_ + "metrics need shave >= 0, got -1"),
    "evaluate_exits_u8_tensor: window too small for ssim":
        (V, P_ + "SSIM needs a window of at least 11 x 11 pixels, got 8 x 16"),
    "evaluate_exits_u8_tensor: host tensors": NO_HIP,
    "evaluate_exits_u8_tensor: host tensors, no ssim": NO_HIP,
    "upscale_stream: depth": (V, P_ + "upscale_stream needs depth >= 1"),
    "upscale_stream: depth beats wrong scale": (V, P_ + "upscale_stream needs depth >= 1"),
    "upscale_stream: wrong scale": BY_2,
    "upscale_stream: bad output_size beats wrong scale": NOT_A_PAIR,
    "upscale_stream: a host model":
        (R, P_ + "upscale_stream only runs on a HIP device (MI355X); there is no CPU fallback"),
    "evaluate_stream: depth": (V, P_ + "evaluate_stream needs depth >= 1"),
    "evaluate_stream: wrong scale": BY_3,
    "evaluate_stream: wrong scale beats bad channel": BY_3,
    "evaluate_stream: bad channel": LUMA,
    "evaluate_stream: bad channel beats negative shave": LUMA,
    "evaluate_stream: negative shave": (V, P_ + "metrics need shave >= 0, got -1"),
    "evaluate_stream: a host model":
        (R, P_ + "evaluate_stream only runs on a HIP device (MI355X); there is no CPU fallback"),
    "upscale_yuv_stream: depth": (V, P_ + "upscale_yuv_stream needs depth >= 1"),
    "upscale_yuv_stream: output_size out of ratio": RATIO,
    "upscale_yuv_stream: bad output_size beats width alone": NOT_A_PAIR,
    "upscale_yuv_stream: width alone": TRIPLES,
    "upscale_yuv_stream: height alone": TRIPLES,
    "upscale_yuv_stream: width alone beats wrong scale": TRIPLES,
    "upscale_yuv_stream: wrong scale": BY_2,
    "upscale_yuv_stream: wrong scale beats bad matrix": BY_2,
    "upscale_yuv_stream: bad matrix": (V, P_ + "matrix must be one of ['bt601', 'bt709'], got 'x'"),
    "upscale_yuv_stream: bad matrix, sizes per frame": (V, P_ + "matrix must be one of ['bt601', 'bt709'], got 'x'"),
    "upscale_yuv_stream: bad full_range": (T, P_ + "full_range must be True or False, got 0"),
    "upscale_yuv_stream: bad frame size": (V, P_ + "a frame needs width and height >= 1, got 0 x 6"),
    "upscale_yuv_stream: a host model":
        (R, P_ + "upscale_yuv_stream only runs on a HIP device (MI355X); there is no CPU fallback"),
    "upscale_yuv_stream: a host model, sizes per frame":
        (R, P_ + "upscale_yuv_stream only runs on a HIP device (MI355X); there is no CPU fallback"),
    "stream image: wrong dtype": (T, P_ + "upscale_stream takes uint8 numpy arrays (decoded images), got float32"),
    "stream image: not an array": (T, P_ + "upscale_stream takes uint8 numpy arrays (decoded images), got list"),
    "stream image: four channels": (V, P_ + "upscale_stream takes (H, W, 3) images, got shape (6, 8, 4)"),
    "stream image: wrong rank": (V, P_ + "upscale_stream takes (H, W, 3) images, got shape (6, 8)"),
    "stream image: empty": (V, P_ + "upscale_stream takes (H, W, 3) images, got shape (6, 0, 3)"),
    "stream image: evaluate_stream wrong dtype":
        (T, P_ + "evaluate_stream takes uint8 numpy arrays (decoded images), got float32"),
    "stream image: evaluate_stream four channels": (V, P_ + "evaluate_stream takes (H, W, 3) images, got shape (6, 8, 4)"),
    "stream image: keep_alpha wrong dtype":
        (T, P_ + "upscale_stream takes uint8 numpy arrays (decoded images), got float32"),
    "stream image: keep_alpha two channels":
        (V, P_ + "upscale_stream takes (H, W, 3) images and, with keep_alpha, (H, W, 4) ones, got shape (6, 8, 2)"),
    "stream image: keep_alpha wrong rank":
        (V, P_ + "upscale_stream takes (H, W, 3) images and, with keep_alpha, (H, W, 4) ones, got shape (6, 8)"),
    "stream image: keep_alpha empty":
        (V, P_ + "upscale_stream takes (H, W, 3) images and, with keep_alpha, (H, W, 4) ones, got shape (0, 8, 4)"),
    "stream frame: wrong dtype": (T, P_ + "upscale_yuv_stream takes uint8 numpy frames, got float32"),
    "stream frame: not an array": (T, P_ + "upscale_yuv_stream takes uint8 numpy frames, got bytes"),
    "stream frame: wrong size": (V, P_ + "an I420 frame of 8 x 6 is a flat buffer of 72 bytes, got shape (71,)"),
    "stream frame: wrong rank": (V, P_ + "an I420 frame of 8 x 6 is a flat buffer of 72 bytes, got shape (9, 8)"),
    "stream frame: wrong dtype beats wrong size": (T, P_ + "upscale_yuv_stream takes uint8 numpy frames, got float32"),
    "head: the image needs a gradient": (R, NO_GRAD % ("the input image", "LarvaHead")),
    "network: the image needs a gradient": (R, NO_GRAD % ("the input image", "the network")),
    "all exits: the image needs a gradient": (R, NO_GRAD % ("the input image", "the base interpolation")),
    "base: the image needs a gradient": (R, NO_GRAD % ("the input image", "the base interpolation")),
    "leg: the base needs a gradient": (R, NO_GRAD % ("the base image", "LarvaLeg")),
    "tail: the base needs a gradient": (R, NO_GRAD % ("the base image", "LarvaTail")),
    "run_leg: the base needs a gradient": (R, NO_GRAD % ("the base image", "LarvaLeg")),
    "run_leg: the truth needs a gradient": (R, NO_GRAD % ("the truth", "an exit of LarvaLeg")),
    "run_leg: the base beats the truth": (R, NO_GRAD % ("the base image", "LarvaTail")),
    "batched exits: the base needs a gradient": (R, NO_GRAD % ("the base image", "the batched exits")),
    "batched exits: the truth needs a gradient": (R, NO_GRAD % ("the truth", "the batched exits")),
    "L1Loss: the truth needs a gradient": (R, NO_GRAD % ("the truth (the loss's target)", "L1Loss")),
}
EXPECTED.update({label + ", under no_grad": NO_HIP for label in list(EXPECTED)
                 if label.endswith("needs a gradient") and not label.startswith(("run_leg", "batched exits"))})


def _refusal(call):
    try:
        got = call()
    except AssertionError:
        raise
    except Exception as e:
        return type(e), str(e)
    return None, "no refusal: returned %s" % type(got).__name__


def test_every_refusal_keeps_its_type_and_its_text():
    cases = _cases(_model(), _model(["--self_ensemble"]))
    labels = [label for label, _ in cases]
    assert len(set(labels)) == len(labels) and set(labels) == set(EXPECTED)
    wrong = []
    for label, call in cases:
        got = _refusal(call)
        if got != EXPECTED[label]:
            wrong.append((label, got, EXPECTED[label]))
    assert not wrong, "\n".join("%s:\n  got  %s: %s\n  want %s: %s" % (l, g[0], g[1], w[0], w[1]) for l, g, w in wrong)


def test_v2_with_more_bodies_than_the_merge_conv_takes_is_refused_at_prepare():
    """LarvaNetV2 --num_modules=9: the tail's merge conv would have nine source tensors and the conv kernels take eight.
    Refused by prepare(), for training and inference alike, not by a RuntimeError inside the first forward."""
    import importlib
    nine = ["--num_modules=9", "--num_blocks=1,1,1,1,1,1,1,1,1"]
    text = P_ + ("%s merges the outputs of at most 8 bodies in its tail (one source tensor of the merge conv each), got "
                 "--num_modules=9%s")

    def prepare(name, training):
        m = importlib.import_module("larvanet_amd.models." + name).create_model()
        m.parse_args(nine)
        return _refusal(lambda: m.prepare(is_training=training, scales=[4]))

    for training in (False, True):
        assert prepare("LarvaNetV2", training) == (V, text % ("LarvaNetV2", ""))
    assert prepare("LarvaLegV2", True) == (V, text % ("LarvaLegV2", "; inference stops at --leg and prepares, training runs the tail"))
    assert prepare("LarvaLegV2", False)[0] is None   # (--leg=4 of nine: the tail is never on the route)
    assert prepare("LarvaNet", False)[0] is None     # (nine exits, no merge conv)


def test_passing_images_and_frames_are_not_refused():
    from larvanet_amd import pipeline as P
    rgb, rgba = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 4), np.uint8)
    assert P._check_image(rgb) is None and P._check_image(rgb, "evaluate_stream") is None
    assert P._check_image(rgb, keep_alpha=True) is None and P._check_image(rgba, keep_alpha=True) is None
    assert P._check_frame(np.zeros(NBYTES, np.uint8), NBYTES, W, H) is None
