"""fp16 inference forward (--precision fp16): the grad-free x4 network at 48 filters on the f16-MFMA kernels of
csrc/conv3x3_f16.hip, over the parameters of the existing module tree (head, bodies, the legs or the V2 tail).

Activations are fp16 channels-last [N][H][W][48]; every conv accumulates in fp32 and rounds its epilogue's result
(bias, ReLU, residual adds) once to fp16.  The image going in and the HR image coming out are fp32 NCHW, and the base
image is the fp32 path's own bicubic / bilinear kernel, so only the internal activations change precision.  The uint8
image path (upscale_u8) ends in the leg end's uint8 epilogue instead: the same fp32 values, stored as HWC bytes.  Training,
validate_for_train and every grad-enabled call stay on the fp32 path (the plugins only dispatch here without
gradients).

Every fp16-storing launch sets a device flag when a value leaves the fp16 range (or is not finite); the flag is sticky
until read (take_overflow).

HalfForward.exits returns every exit's image from one pass over the head and the bodies: the legs, which do not depend on
each other, go out as two job launches (K.f16_conv3x3_jobs, K.f16_conv3x3_shuffle_base_jobs)."""
import torch

from . import kernels as K


class HalfPack:
    """fp16 A-operand image of one conv weight in a persistent buffer, repacked by one launch when the weight's storage
    or version moves or after invalidate() -- PackedConv's staleness rules for inference.  The buffer keeps its address,
    so a captured graph that reads it sees the repacked image."""

    __slots__ = ("weight", "_key", "_buf")

    def __init__(self, weight):
        self.weight = weight
        self._key = None
        self._buf = None

    def invalidate(self):
        self._key = None

    def get(self):
        w = self.weight
        key = (w.data_ptr(), w._version, str(w.device))
        if key != self._key:
            buf = self._buf if self._buf is not None and self._buf.device == w.device else None
            self._buf = K.f16_pack_weights(w.detach(), out=buf)
            self._key = key
        return self._buf


class HalfForward:
    """The fp16 forward of one LarvaNetModule, along the module's own inference route (net.route(): how many bodies
    run and the LarvaLeg / LarvaTail that ends them, or None = the base image alone)."""

    def __init__(self, net):
        self.net = net
        self._packs = {}
        self._flag = None
        self._all_exits = False   # exits() has run: refresh() keeps every leg on the exit route packed, not only the end

    def _convs(self):
        bodies, end = self.net.route()
        out = []
        for body in self.net.bodies(bodies):
            for blk in body.res_blocks:
                out += [blk.body[0], blk.body[2]]
        if self._all_exits:
            for leg in self.net.exit_route()[1]:
                out += [leg.recon_block[0], leg.recon_block[2]]
        elif end is not None:
            out += ([end.merge_conv] if end.merges else []) + [end.recon_block[0], end.recon_block[2]]
        return out

    def _wpk(self, conv):
        p = self._packs.get(id(conv))
        if p is None or p.weight is not conv.weight:
            p = self._packs[id(conv)] = HalfPack(conv.weight)
        return p.get()

    def refresh(self):
        """Repack the stale weight images now (outside a graph, before a replay reads them)."""
        for c in self._convs():
            self._wpk(c)

    def invalidate(self):
        for p in self._packs.values():
            p.invalidate()

    def flag(self, device):
        if self._flag is None or self._flag.device != device:
            self._flag = torch.zeros(1, device=device, dtype=torch.int32)
        return self._flag

    def clear_overflow(self):
        if self._flag is not None:
            self._flag.zero_()

    def take_overflow(self):
        """True if an fp16 launch overflowed since the last call (host sync); clears the flag."""
        if self._flag is None:
            return False
        hit = bool(int(self._flag.item()))
        if hit:
            self._flag.zero_()
        return hit

    def _conv(self, conv, srcs, flag, **epi):
        return K.f16_conv3x3(srcs, self._wpk(conv), conv.bias.detach(), flag, **epi)

    def _body(self, body, x, flag):
        blocks = list(body.res_blocks)
        fea = x
        for j, blk in enumerate(blocks):
            h = self._conv(blk.body[0], fea, flag, relu=True)
            # the last block's second conv also adds the body's outer skip (models/LarvaNet.py:247)
            fea = self._conv(blk.body[2], h, flag, res0=fea, res1=x if j == len(blocks) - 1 else None)
        return fea

    def _leg_end(self, recon_block, fea, base, flag, u8=False):
        c1, c2 = recon_block[0], recon_block[2]
        h = self._conv(c1, fea, flag, relu=True)
        if u8:   # the same fp32 values, rounded and clamped to bytes in the conv's epilogue
            return K.f16_conv3x3_shuffle_base_u8(h, self._wpk(c2), c2.bias.detach(), base, flag)
        return K.f16_conv3x3_shuffle_base(h, self._wpk(c2), c2.bias.detach(), base)

    def _trunk(self, x, bodies, flag):
        """The head and the first `bodies` bodies -> every body's output."""
        net = self.net
        head = net.head.feature_extraction
        fea = K.f16_head(x, head.weight.detach(), head.bias.detach(), flag)
        feats = []
        for body in net.bodies(bodies):
            fea = self._body(body, fea, flag)
            feats.append(fea)
        return feats

    def exits(self, x, u8=False, batched=True):
        """Every exit of the module's exit route (net.exit_route()) from ONE pass over the head and the bodies: fp32
        [M][N][3][4H][4W], or with u8 uint8 [M][N][4H][4W][3]; index 0 is the first exit.  Exit i is bit for bit what
        __call__ returns on a module whose route ends at leg i.  batched: the M first convs are one job launch and the M
        leg ends against the shared base another (up to 8 legs per launch); False: one leg after the other."""
        net = self.net
        bodies, legs = net.exit_route()
        self._all_exits = True
        x = x.contiguous()
        base = net.base(x)
        flag = self.flag(x.device)
        feats = self._trunk(x, bodies, flag)
        M, (N, _, H, W) = len(legs), (int(v) for v in x.shape)
        if u8:
            out = torch.empty((M, N, 4 * H, 4 * W, 3), device=x.device, dtype=torch.uint8)
        else:
            out = torch.empty((M, N, 3, 4 * H, 4 * W), device=x.device, dtype=torch.float32)
        if not batched:
            for i, leg in enumerate(legs):
                out[i].copy_(self._leg_end(leg.recon_block, feats[i], base, flag, u8))
            return out
        for lo in range(0, M, K.F16_MAX_JOBS):
            part = legs[lo:lo + K.F16_MAX_JOBS]
            c1 = [leg.recon_block[0] for leg in part]
            c2 = [leg.recon_block[2] for leg in part]
            hs = K.f16_conv3x3_jobs(feats[lo:lo + len(part)], [self._wpk(c) for c in c1], [c.bias.detach() for c in c1],
                                    flag, relu=True)
            K.f16_conv3x3_shuffle_base_jobs(list(hs), [self._wpk(c) for c in c2], [c.bias.detach() for c in c2], base,
                                            flag, u8=u8, out=out[lo:lo + len(part)])
        return out

    def __call__(self, x, u8=False):
        """fp32 [N][3][H][W] -> the fp32 [N][3][4H][4W] image, or with u8 its uint8 [N][4H][4W][3] form
        (K.f32_chw_to_u8_hwc of the former, bit for bit)."""
        net = self.net
        bodies, end = net.route()
        x = x.contiguous()
        base = net.base(x)
        if end is None:
            return K.f32_chw_to_u8_hwc(base) if u8 else base
        flag = self.flag(x.device)
        feats = self._trunk(x, bodies, flag)
        fea = self._conv(end.merge_conv, feats, flag) if end.merges else feats[-1]
        return self._leg_end(end.recon_block, fea, base, flag, u8)
