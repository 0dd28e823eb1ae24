"""The x2 / x3 ends of the network as autograd Functions (a model prepared with scales=[2] or [3]).

At scale s the last conv of a leg (and of the V2 tail) has 3 s^2 = 12 / 27 outputs.  It runs as a plain-epilogue
32-output conv on zero-padded weight rows (PackedConv.cout_pad), and the kernels of csrc/larva_scale.hip map its
[N][32][H][W] output to the [N][3][sH][sW] image and back:
    forward    y = conv(h) ; out = PixelShuffle(s)(y) + base                       (pixel_shuffle_base)
    exit       partial sums of |out - truth| and the unshuffled sign gradient, one pass (shuffle_l1_partial_grad)
    backward   dh = dgrad(dyl) * [h > 0] on the 32 padded gradient channels (4 K chunks, zero weight rows),
               dW = the (32, 48) weight-gradient kernel, only the real 12 / 27 rows reach the parameters.
The x4 path (autograd.LegFn / ExitFn / ExitsFn with the conv kernel's shuffle epilogues) is not involved.
"""
import numpy as np
import torch

from . import kernels as K
from .autograd import StepScope, _lw, _splits, _targets, _wgrad


def padded_wgrad(dyl, h, pc, wshape):
    """Weight gradient of a padded-output conv from its padded output gradient dyl [N][cout_pad][H][W]: the
    (cout_pad, cin) kernel writes a padded image, and only its real rows and biases reach the gradients (copied into the
    bucket views when they exist) -> (dw, db), or (None, None) when written in place."""
    cp, cin, rows = pc.cout_pad, int(wshape[1]), int(wshape[0])
    dw = torch.empty((cp,) + tuple(wshape[1:]), device=dyl.device, dtype=torch.float32)
    db = torch.empty((cp,), device=dyl.device, dtype=torch.float32)
    K.conv3x3_wgrad([{"dy": dyl, "x": h, "dw": dw, "db": db, "cin_off": 0, "cin_valid": cin}], cp, cin,
                    _splits(1, cp, cin))
    tw, tb = _targets(pc)
    if tw is None:
        return dw[:rows], db[:rows]
    tw.copy_(dw[:rows])
    tb.copy_(db[:rows])
    return None, None


def _leg_backward(ctx, fea, h, dyl):
    pcs = ctx.pcs
    c = ctx.wshape[0]
    (_, bw1), = pcs[0].get()
    (_, bw2), = pcs[1].get()
    dh = K.conv3x3(dyl, bw2, c, mask=h)
    dfea = K.conv3x3(dh, bw1, c)
    inplace = _targets(pcs[0])[0] is not None
    ((dw1, db1),) = _wgrad([(dh, fea, ctx.wshape, 0, c) + _targets(pcs[0])], c, c, inplace=inplace)
    if inplace:
        dw1 = db1 = None
    dw2, db2 = padded_wgrad(dyl, h, pcs[1], ctx.wshape2)
    return dfea, dw1, db1, dw2, db2


def _leg_forward(fea, base, pcs, w1, b1, scale, lw=None):
    (f1, _), = pcs[0].get()
    (f2, _), = pcs[1].get()
    c = int(w1.shape[0])
    h = K.conv3x3(fea, f1, c, bias=b1.detach(), relu=True, logical_w=lw)
    y = K.conv3x3(h, f2, pcs[1].cout_pad, bias=pcs[1].padded_bias(), logical_w=lw)
    return h, y


class ScaledLegFn(torch.autograd.Function):
    """LarvaLeg.forward at scale 2 / 3: conv + ReLU, conv (3 s^2 outputs) -> PixelShuffle(s) -> + base."""

    @staticmethod
    def forward(ctx, fea, base, pcs, scale, w1, b1, w2, b2):
        h, y = _leg_forward(fea, base, pcs, w1, b1, scale, _lw())
        out = K.pixel_shuffle_base(y, base, scale, logical_w=_lw())
        ctx.save_for_backward(fea, h)
        ctx.pcs, ctx.scale = pcs, scale
        ctx.wshape, ctx.wshape2 = tuple(w1.shape), tuple(w2.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        fea, h = ctx.saved_tensors
        dyl = K.pixel_unshuffle(dout.contiguous(), ctx.scale, ctx.pcs[1].cout_pad)
        dfea, dw1, db1, dw2, db2 = _leg_backward(ctx, fea, h, dyl)
        return dfea, None, None, None, dw1, db1, dw2, db2


class ScaledExitFn(torch.autograd.Function):
    """One training exit at scale 2 / 3: the leg followed by nn.L1Loss against the truth.  Returns (exit image, loss
    term); with a divisor the term is the block partial sums of |out - truth| (LossTerm, prescaled: the 1/divisor of the
    mean over the exits is applied inside the gradient kernel).  When the seed of backward is known (the plugin's step)
    the gradient is written in the same pass as the partial sums, already unshuffled."""

    @staticmethod
    def forward(ctx, fea, base, truth, pcs, scale, divisor, w1, b1, w2, b2):
        h, y = _leg_forward(fea, base, pcs, w1, b1, scale)
        cpad = pcs[1].cout_pad
        ctx.gscale = 1.0 if divisor is None else float(np.float32(1.0) / np.float32(divisor))
        dyl = None
        if divisor is not None and StepScope.seed_grad is not None:
            term, _, dyl, out = K.shuffle_l1_partial_grad(y, base, truth, StepScope.seed_grad, ctx.gscale, scale)
        else:
            out = K.pixel_shuffle_base(y, base, scale)
            term = K.l1_fwd(out, truth) if divisor is None else K.l1_partial(out, truth)[0]
        ctx.have_dyl = dyl is not None
        ctx.save_for_backward(fea, h, *((dyl,) if dyl is not None else (out, truth)))
        ctx.pcs, ctx.scale, ctx.cpad = pcs, scale, cpad
        ctx.wshape, ctx.wshape2 = tuple(w1.shape), tuple(w2.shape)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return out, term

    @staticmethod
    def backward(ctx, _dout, gterm):
        if gterm is None:
            return (None,) * 10
        saved = ctx.saved_tensors
        fea, h = saved[:2]
        if ctx.have_dyl:
            dyl = saved[2]
        else:
            g0 = gterm.as_strided((), ()) if gterm.dim() else gterm.contiguous()
            dyl = K.l1_bwd_unshuffle(saved[2], saved[3], g0, ctx.scale, ctx.cpad, ctx.gscale)
        dfea, dw1, db1, dw2, db2 = _leg_backward(ctx, fea, h, dyl)
        return dfea, None, None, None, None, None, dw1, db1, dw2, db2
