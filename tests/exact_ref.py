"""Integer data and float64 references for tests/test_exact_integer.py (test helper, not a test).

Every matrix instruction of the library multiplies fp32 (v_mfma_f32_16x16x4f32) or fp16 (v_mfma_f32_16x16x32_f16)
operands into an fp32 accumulator.  On operands whose products and partial sums are integers below 2^24 every such sum
is exact whatever its order, so a kernel's result equals the integer sum bit for bit.  The generators below draw such
operands from a seed; the references compute the sums in float64 (exact far beyond 2^24) with torch's own conv2d and
numpy index maps, and hand back, next to the result, the values whose size decides whether equality may be asked
(`inter`): the reference's sums and a bound on every partial sum a kernel can form on the way,
max|x| * max_co sum|w[co]| + |bias| + |res0| + |res1|.  assert_exact_precondition checks them BEFORE a device result is
looked at, so a badly chosen range fails as a set-up error and never as a kernel failure."""
import numpy as np
import torch
import torch.nn.functional as F

LIMIT_F32 = 2 ** 24        # integers of smaller magnitude are exact in an fp32 accumulator
HALF_MAX = 65504           # the largest finite fp16


# ---------------------------------------------------------------- generators
def rng_of(*key):
    return np.random.default_rng([int(k) for k in key])


def ints(rng, shape, a, lo=None):
    """float32 integers in [-a, a] (or [lo, a])."""
    return rng.integers(-a if lo is None else lo, a + 1, size=shape).astype(np.float32)


def weights(rng, shape, b, nz=None):
    """float32 integer weights [cout][cin][3][3] in [-b, b] without zeros thinned out, or (nz given) sparse: about nz
    non-zero entries per output channel, each a non-zero integer in [-b, b]."""
    w = rng.integers(-b, b + 1, size=shape).astype(np.float32)
    if nz is not None:
        sign = rng.choice([-1.0, 1.0], size=shape)
        mag = rng.integers(1, b + 1, size=shape)
        per = int(np.prod(shape[1:]))
        w = np.where(rng.random(shape) < float(nz) / per, sign * mag, 0.0).astype(np.float32)
    return w


def masks(rng, shape):
    """ReLU-backward masks drawn from {-1, -0.0, +0.0, 1}: both zeros appear, and neither passes `mask > 0`."""
    return rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), size=shape).astype(np.float32)


def pad_pitch(a, pitch):
    """Rows of `a` [..., W] padded with zero columns to `pitch`."""
    out = np.zeros(a.shape[:-1] + (pitch,), a.dtype)
    out[..., :a.shape[-1]] = a
    return out


# ---------------------------------------------------------------- the two assertions
def assert_exact_precondition(ref_intermediates, limit=LIMIT_F32):
    """Every value the reference formed (arrays or scalars) is an integer of magnitude below `limit`: the condition that
    makes bitwise equality with a device result legitimate.  Raises a set-up error otherwise."""
    n = 0
    for v in ref_intermediates:
        v = np.asarray(v, np.float64)
        n += 1
        if v.size == 0:
            continue
        if not np.isfinite(v).all():
            raise AssertionError("test set-up: a reference intermediate is not finite")
        if not (v == np.rint(v)).all():
            raise AssertionError("test set-up: a reference intermediate is not an integer (first %r)"
                                 % float(v[v != np.rint(v)].ravel()[0]))
        big = float(np.abs(v).max())
        if not big < limit:
            raise AssertionError("test set-up: a reference intermediate reaches %.0f, not below %.0f" % (big, limit))
    if n == 0:
        raise AssertionError("test set-up: no reference intermediates were given")


def _np(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a)


def assert_bits_equal(got, ref, what):
    """Bitwise equality of `got` (device tensor or array: float32, float16, uint8 or an integer type) with `ref`
    (float64 or `got`'s type; cast to it -- exact for the integers of these tests).  On a mismatch: the count, the first
    four indices and got / expected at each of them."""
    g = _np(got)
    r = _np(ref)
    assert g.shape == r.shape, "%s: shape %s, expected %s" % (what, g.shape, r.shape)
    if r.dtype != g.dtype:
        with np.errstate(over="ignore", invalid="ignore"):
            r = r.astype(g.dtype)
    view = {4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}[g.dtype.itemsize]
    gb, rb = g.view(view), r.view(view)
    if np.array_equal(gb, rb):
        return
    bad = np.argwhere(gb != rb)
    lines = ["%s: %d of %d elements differ" % (what, len(bad), g.size)]
    for idx in bad[:4]:
        t = tuple(int(i) for i in idx)
        lines.append("  at %s got %r (0x%x) expected %r (0x%x)" % (list(t), g[t].item(), int(gb[t]), r[t].item(), int(rb[t])))
    raise AssertionError("\n".join(lines))


# ---------------------------------------------------------------- NaN / Inf (tests/test_nonfinite.py)
CLASS_NAMES = ("finite", "+Inf", "-Inf", "NaN")


def poison(a, positions, value):
    """A copy of `a` with `value` (NaN, +Inf or -Inf) at the listed index tuples."""
    v = float(value)
    if np.isfinite(v):
        raise AssertionError("test set-up: a poison is NaN, +Inf or -Inf, not %r" % (value,))
    out = np.array(a, copy=True)
    for pos in positions:
        out[tuple(int(i) for i in pos)] = v
    return out


def unpoisoned(a, positions):
    """The clean stand-in the exactness precondition is asserted on: `a` with its largest magnitude at `positions` (the
    finite outputs of the poisoned run are sums of a subset of the terms of this one, so its bound covers them)."""
    out = np.array(a, copy=True)
    big = np.abs(out[np.isfinite(out)]).max() if np.isfinite(out).any() else 0
    for pos in positions:
        out[tuple(int(i) for i in pos)] = big
    return out


def class_map(a):
    """uint8 per element: 0 finite, 1 +Inf, 2 -Inf, 3 NaN."""
    a = _np(a)
    with np.errstate(invalid="ignore"):
        return (np.isposinf(a) * 1 + np.isneginf(a) * 2 + np.isnan(a) * 3).astype(np.uint8)


def assert_equal_with_nonfinite(got, ref, what):
    """assert_bits_equal, except that where `ref` is NaN `got` must be a NaN of any payload and sign.  Everywhere else,
    +-Inf included, the bits must match.  On a mismatch: the count, got's and ref's elements per class (finite, +Inf,
    -Inf, NaN), the first four indices and got / expected at each of them."""
    g = _np(got)
    r = _np(ref)
    assert g.shape == r.shape, "%s: shape %s, expected %s" % (what, g.shape, r.shape)
    assert g.dtype.kind == "f", "%s: %s is not a float type" % (what, g.dtype)
    if r.dtype != g.dtype:
        with np.errstate(over="ignore", invalid="ignore"):
            r = r.astype(g.dtype)
    view = {4: np.uint32, 2: np.uint16, 8: np.uint64}[g.dtype.itemsize]
    gb, rb = g.view(view), r.view(view)
    rnan = np.isnan(r)
    wrong = np.where(rnan, ~np.isnan(g), gb != rb)
    if not wrong.any():
        return
    bad = np.argwhere(wrong)
    cg, cr = class_map(g), class_map(r)
    lines = ["%s: %d of %d elements differ" % (what, len(bad), g.size),
             "  got      " + ", ".join("%s %d" % (nm, int((cg == k).sum())) for k, nm in enumerate(CLASS_NAMES)),
             "  expected " + ", ".join("%s %d" % (nm, int((cr == k).sum())) for k, nm in enumerate(CLASS_NAMES))]
    for idx in bad[:4]:
        t = tuple(int(i) for i in idx)
        lines.append("  at %s got %r (0x%x) expected %r (0x%x)" % (list(t), g[t].item(), int(gb[t]), r[t].item(), int(rb[t])))
    raise AssertionError("\n".join(lines))


def mask_passes(mask):
    """ATen's threshold_backward predicate: the gradient passes wherever !(mask <= 0) -- NaN and +Inf pass."""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(mask) <= 0)


def conv_footprint(shape, positions, radius=1):
    """Boolean [N][H][W]: the pixels whose 3 x 3 neighbourhood holds one of `positions` ((n, c, y, x) tuples) -- the
    outputs of a 3 x 3 conv (any output channel) that depend on those elements."""
    n, h, w = shape
    fp = np.zeros((n, h, w), bool)
    for (i, _, y, x) in positions:
        fp[i, max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = True
    return fp


# ---------------------------------------------------------------- single operations (float64)
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def conv_sum_bound(xs, w, bias=None, res0=None, res1=None):
    """A bound on the magnitude of every partial sum of conv(cat(xs), w) + bias + res0 + res1, in any order."""
    amax = max(float(np.abs(x).max()) if np.size(x) else 0.0 for x in xs)
    wsum = float(np.abs(np.asarray(w, np.float64)).reshape(w.shape[0], -1).sum(1).max())
    extra = sum(float(np.abs(t).max()) for t in (bias, res0, res1) if t is not None and np.size(t))
    return amax * wsum + extra


def conv(xs, w, bias=None, relu=False, mask=None, res0=None, res1=None, nonfinite=False):
    """3x3 conv (stride 1, zero padding 1) over the channel concatenation of `xs` with the library's epilogue order
    + bias -> relu -> (mask > 0 ? v : 0) -> + res0 -> + res1 -> (float64 [N][cout][H][W], inter).
    nonfinite=True: operands may hold NaN / Inf, the rules are torch's (relu keeps NaN -- np.maximum does --, the mask
    passes where !(mask <= 0)) and `inter` is None: the precondition belongs to the clean operands (`unpoisoned`)."""
    if isinstance(xs, np.ndarray):
        xs = [xs]
    x = _t(np.concatenate(xs, axis=1))
    y = F.conv2d(x, _t(w), None if bias is None else _t(bias), padding=1).numpy()
    inter = None if nonfinite else [y.copy(), conv_sum_bound(xs, w, bias, res0, res1)]
    if relu:
        y = np.maximum(y, 0.0)
    if mask is not None and nonfinite:
        y = np.where(mask_passes(mask), y, 0.0)
    elif mask is not None:
        y = np.where(np.asarray(mask) > 0, y, 0.0)    # (a masked -x stays +0.0, as the kernel's select does)
    if res0 is not None:
        y = y + np.asarray(res0, np.float64)
    if res1 is not None:
        y = y + np.asarray(res1, np.float64)
    if inter is not None:
        inter.append(y)
    return y, inter


def dgrad(dy, w, mask=None, res0=None, res1=None, nonfinite=False):
    """Input gradient of the 3x3 conv: dx[n, ci] = sum_co corr(dy[n, co], w[co, ci] mirrored) -> (float64, inter); with
    the ReLU-backward mask and the skip gradients the library fuses into it.  nonfinite: as for conv()."""
    dx = F.conv_transpose2d(_t(dy), _t(w), padding=1).numpy()
    wt = np.asarray(w, np.float64).transpose(1, 0, 2, 3)
    inter = None if nonfinite else [dx.copy(), conv_sum_bound([dy], wt, None, res0, res1)]
    if mask is not None and nonfinite:
        dx = np.where(mask_passes(mask), dx, 0.0)
    elif mask is not None:
        dx = np.where(np.asarray(mask) > 0, dx, 0.0)
    if res0 is not None:
        dx = dx + np.asarray(res0, np.float64)
    if res1 is not None:
        dx = dx + np.asarray(res1, np.float64)
    if inter is not None:
        inter.append(dx)
    return dx, inter


def wgrad(dy, x):
    """Weight and bias gradient of the 3x3 conv -> (dw float64 [cout][cin][3][3], db float64 [cout], inter)."""
    dyt, xt = _t(dy), _t(x)
    cout, cin = dy.shape[1], x.shape[1]
    dw = torch.nn.grad.conv2d_weight(xt, (cout, cin, 3, 3), dyt, padding=1).numpy()
    db = dyt.sum((0, 2, 3)).numpy()
    n, _, h, wd = dy.shape
    bound = float(np.abs(dy).max()) * float(np.abs(x).max()) * n * h * wd
    return dw, db, [dw, db, bound, float(np.abs(dy).max()) * n * h * wd]


def pixel_shuffle(y, s):
    """nn.PixelShuffle(s): [N][C s^2][H][W] -> [N][C][sH][sW], out[n, c, s y + i, s x + j] = y[n, c s^2 + s i + j, y, x]."""
    n, cs, h, w = y.shape
    c = cs // (s * s)
    return np.ascontiguousarray(y.reshape(n, c, s, s, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(n, c, s * h, s * w))


def pixel_unshuffle(g, s):
    """Its inverse: [N][C][sH][sW] -> [N][C s^2][H][W]."""
    n, c, hh, ww = g.shape
    h, w = hh // s, ww // s
    return np.ascontiguousarray(g.reshape(n, c, h, s, w, s).transpose(0, 1, 3, 5, 2, 4).reshape(n, c * s * s, h, w))


def pad_channels(a, cpad):
    """[N][C][H][W] -> [N][cpad][H][W] with +0.0 in the padding channels."""
    out = np.zeros((a.shape[0], cpad) + a.shape[2:], a.dtype)
    out[:, :a.shape[1]] = a
    return out


def l1_sign_grad(out, truth, g):
    """sign(out - truth) * g with sign(0) = +0.0, float32; torch's sign on non-finite data: a NaN difference (NaN
    operand, Inf - Inf) gives +0.0, +-Inf differences give +-g."""
    with np.errstate(invalid="ignore"):
        d = np.asarray(out, np.float64) - np.asarray(truth, np.float64)
        return np.where(d > 0, np.float32(g), np.where(d < 0, np.float32(-g), np.float32(0.0))).astype(np.float32)


def f16_round(v):
    """float64 -> the float16 nearest to it (ties to even), as float64."""
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------- whole networks
def int_state_dict(shapes, seed, nz, bias_amp=2):
    """Sparse +-1 integer weights (about nz per output channel) and integer biases in [-bias_amp, bias_amp] for a
    state_dict's {key: shape}, float32 tensors."""
    rng = rng_of(seed, nz)
    sd = {}
    for k, shape in shapes.items():
        if k.endswith(".weight"):
            sd[k] = torch.from_numpy(weights(rng, tuple(shape), 1, nz=nz))
        else:
            sd[k] = torch.from_numpy(ints(rng, tuple(shape), bias_amp))
    return sd


class Net:
    """Float64 restatement of the inference forward of LarvaNet / LarvaNetV2 / LarvaLeg (x4, 48 filters) WITHOUT the base
    image: head -> bodies (residual blocks, outer skip) -> leg (conv + ReLU, conv, PixelShuffle(4)); V2: the tail over the
    concatenated body outputs.  half=True rounds to fp16 after every layer that stores fp16, as --precision fp16 does
    (the head, both convs of a block after their epilogue, the merge conv, the leg's first conv; the leg end stays
    fp32).  The precondition is asserted layer by layer on the whole arrays; `inter` keeps every layer's largest sum and
    partial-sum bound, `stored` the largest value each fp16 store sees."""

    def __init__(self, sd, blocks, half=False):
        self.sd = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float64)
                   for k, v in sd.items()}
        self.blocks = list(blocks)
        self.half = half
        self.inter = []
        self.stored = []

    def _store(self, v):
        if self.half:
            assert_exact_precondition([v], HALF_MAX + 1)   # (an integer of at most 65504: fp16 stores it finite)
            self.stored.append(float(np.abs(v).max()))
            return f16_round(v)
        return v

    def _conv(self, xs, prefix, **epi):
        y, inter = conv(xs, self.sd[prefix + ".weight"], self.sd[prefix + ".bias"], **epi)
        assert_exact_precondition(inter, LIMIT_F32)    # checked layer by layer, on the whole arrays; the maxima are kept
        self.inter += [float(np.abs(np.asarray(v)).max()) for v in inter]
        return y

    def _body(self, i, x):
        fea = x
        nb = self.blocks[i]
        for j in range(nb):
            p = "body_%d.res_blocks.%d.body" % (i, j)
            h = self._store(self._conv([fea], p + ".0", relu=True))
            fea = self._store(self._conv([h], p + ".2", res0=fea, res1=x if j == nb - 1 else None))
        return fea

    def _leg(self, prefix, fea):
        h = self._store(self._conv([fea], prefix + ".recon_block.0", relu=True))
        return pixel_shuffle(self._conv([h], prefix + ".recon_block.2"), 4)

    def features(self, x, bodies=None):
        fea = self._store(self._conv([np.asarray(x, np.float64)], "head.feature_extraction"))
        feats = []
        for i in range(len(self.blocks) if bodies is None else bodies):
            fea = self._body(i, fea)
            feats.append(fea)
        return feats

    def forward(self, x, exit_index=None):
        """The conv part of exit `exit_index` (default: the last one) -> float64 [N][3][4H][4W]."""
        e = len(self.blocks) - 1 if exit_index is None else exit_index
        return self._leg("body_%d.leg" % e, self.features(x, e + 1)[-1])

    def forward_v2(self, x):
        feats = self.features(x)
        fea = self._store(self._conv(feats, "tail.merge_conv"))
        return self._leg("tail", fea)

    def largest(self):
        return max(float(np.abs(np.asarray(v)).max()) for v in self.inter)
