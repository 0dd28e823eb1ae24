"""NaN and Inf through every float kernel: which outputs a poisoned element reaches, and torch's non-finite rules.

0 x NaN is NaN, so ONE poisoned input element marks exactly the outputs that consumed it -- also the ones that only
multiplied it by zero or added it into a lane they later discard (a halo pixel of the neighbouring image, a stale LDS
row, a tap outside the cubic support, the next layer's partial image in the flat weight-gradient grid).  That set is a
property of the operation, so it is compared with the plain float64 reference of tests/exact_ref.py on the integer draws
of tests/test_exact_integer.py: every finite output is exact, so the comparison is bitwise
(exact_ref.assert_equal_with_nonfinite: NaN against NaN by class) and no tolerance appears in the conv, weight-gradient
and L1 parts.  The exactness precondition is asserted on the clean operands with each poisoned element replaced by the
operand's largest magnitude: the finite outputs of a poisoned run are sums of a subset of those terms.

Weights are always finite; where an Inf is the poison they have no zeros, so Inf x w has a definite sign.  Poisons of
one tensor are at least 7 pixels apart (or in different images or launches): one footprint cannot hide another's leak."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
import placement
import test_exact_integer as E

gpu = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
SENTINEL = 12345.0          # what an output holds where a launch must not write


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _name(v):
    return "NaN" if v != v else ("+Inf" if v > 0 else "-Inf")


# =====================================================================================================================
# CPU part: the helpers and the reference rules
# =====================================================================================================================
def test_poison_class_map_and_the_clean_stand_in():
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4) - 7
    p = X.poison(a, [(0, 0, 0), (1, 2, 3)], NAN)
    assert np.isnan(p[0, 0, 0]) and np.isnan(p[1, 2, 3]) and int(np.isnan(p).sum()) == 2 and a[0, 0, 0] == -7
    q = X.poison(X.poison(p, [(0, 1, 1)], INF), [(0, 1, 2)], -INF)
    cm = X.class_map(q)
    assert cm.dtype == np.uint8 and cm[0, 0, 0] == 3 and cm[0, 1, 1] == 1 and cm[0, 1, 2] == 2 and int((cm == 0).sum()) == 20
    assert np.array_equal(X.class_map(torch.from_numpy(q)), cm)
    with pytest.raises(AssertionError, match="set-up"):
        X.poison(a, [(0, 0, 0)], 1.0)
    u = X.unpoisoned(q, [(0, 0, 0), (1, 2, 3), (0, 1, 1), (0, 1, 2)])
    assert np.isfinite(u).all() and u[0, 0, 0] == 15 and u[0, 1, 2] == 15 and u[1, 0, 0] == a[1, 0, 0]
    fp = X.conv_footprint((2, 5, 6), [(0, 9, 0, 0), (1, 0, 2, 5)])
    assert fp[0, :2, :2].all() and fp[1, 1:4, 4:6].all() and int(fp.sum()) == 4 + 6


def test_assert_equal_with_nonfinite_compares_nan_by_class_and_everything_else_by_bits():
    ref = np.array([[1.0, NAN], [INF, -INF], [0.0, -0.0]])
    good = ref.astype(np.float32)
    X.assert_equal_with_nonfinite(good, ref, "same")
    other_nan = good.copy()
    other_nan.view(np.uint32)[0, 1] = 0xFFC12345                      # negative, another payload
    X.assert_equal_with_nonfinite(torch.from_numpy(other_nan), ref, "any NaN")
    X.assert_equal_with_nonfinite(good.astype(np.float16), ref, "fp16")
    for bad, at in ((np.array([[1.0, 0.0], [INF, -INF], [0.0, -0.0]], np.float32), r"\[0, 1\]"),      # NaN lost
                    (np.array([[NAN, NAN], [INF, -INF], [0.0, -0.0]], np.float32), r"\[0, 0\]"),      # NaN where none belongs
                    (np.array([[1.0, NAN], [-INF, -INF], [0.0, -0.0]], np.float32), r"\[1, 0\]"),     # the Inf's sign
                    (np.array([[1.0, NAN], [INF, -INF], [-0.0, -0.0]], np.float32), r"\[2, 0\]")):    # the zero's sign
        with pytest.raises(AssertionError, match=r"1 of 6 elements differ\n  got .*finite \d+, \+Inf \d+, -Inf \d+, NaN \d+\n"
                                                 r"  expected +finite 3, \+Inf 1, -Inf 1, NaN 1\n  at " + at):
            X.assert_equal_with_nonfinite(bad, ref, "bad")
    with pytest.raises(AssertionError, match="shape"):
        X.assert_equal_with_nonfinite(good[:2], ref, "shape")


def test_reference_rules_are_torchs_rules():
    """relu(NaN) is NaN; the relu gradient at a NaN output is 1; sign(NaN) = 0; the L1Loss gradient at NaN and at
    Inf - Inf is 0 with a NaN loss -- torch on the CPU, against the numpy expressions the references use."""
    v = torch.tensor([NAN, INF, -INF, -0.0, 0.0, -2.0, 3.0])
    r = torch.relu(v)
    vn = v.numpy()
    with np.errstate(invalid="ignore"):
        X.assert_equal_with_nonfinite(np.where(vn < 0, np.float32(0), vn), r.numpy(), "the kernel's v < 0 ? 0 : v against torch.relu")
    keep = np.arange(7) != 3       # np.maximum, the references' ReLU, differs from both at -0.0 alone (it gives +0.0)
    X.assert_equal_with_nonfinite(np.maximum(vn, np.float32(0))[keep], r.numpy()[keep], "np.maximum against torch.relu")
    assert torch.isnan(r[0]) and r[1] == INF and r[2] == 0 and np.signbit(r.numpy()[3])
    x = v.clone().requires_grad_(True)
    torch.relu(x).backward(torch.full_like(x, 5.0))
    passes = X.mask_passes(torch.relu(v).numpy())          # the mask is the ReLU's output
    assert np.array_equal(x.grad.numpy(), np.where(passes, 5.0, 0.0)) and x.grad[0] == 5.0 and x.grad[1] == 5.0
    assert np.array_equal(X.mask_passes(np.array([NAN, INF, -INF, -0.0, 0.0, -1.0, 1.0], np.float32)),
                          [True, True, False, False, False, False, True])
    assert float(torch.sign(torch.tensor(NAN))) == 0.0
    out = torch.tensor([NAN, INF, INF, 1.0, 2.0, -INF, 4.0], requires_grad=True)
    truth = torch.tensor([1.0, INF, 1.0, INF, 2.0, 3.0, 1.0])
    loss = torch.nn.L1Loss()(out, truth)
    loss.backward()
    assert torch.isnan(loss)
    g = np.float32(1.0) / np.float32(7.0)
    want = X.l1_sign_grad(out.detach().numpy(), truth.numpy(), g)
    X.assert_bits_equal(out.grad.numpy(), want, "L1Loss gradient against l1_sign_grad")
    assert list(want) == [0, 0, g, -g, 0, -g, g]
    y, _ = X.conv([np.full((1, 8, 3, 3), 1.0, np.float32)], np.ones((8, 8, 3, 3), np.float32), nonfinite=True,
                  mask=np.full((1, 8, 3, 3), NAN, np.float32))
    assert (y > 0).all()                                   # a NaN mask passes; the integer tests' rule (mask > 0) does not
    y, _ = X.conv([np.full((1, 8, 3, 3), 1.0, np.float32)], np.ones((8, 8, 3, 3), np.float32),
                  mask=np.full((1, 8, 3, 3), NAN, np.float32))
    assert not y.any()


def _nine_tap(x, w):
    n, ci, h, wd = x.shape
    xp = np.zeros((n, ci, h + 2, wd + 2))
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, w.shape[0], h, wd))
    with np.errstate(invalid="ignore"):
        for ky in range(3):
            for kx in range(3):
                out += np.einsum("nchw,oc->nohw", xp[:, :, ky:ky + h, kx:kx + wd], w[:, :, ky, kx].astype(np.float64))
    return out


@pytest.mark.parametrize("dense", [False, True], ids=["weights-with-zeros", "dense-weights"])
def test_float64_conv2d_gives_the_class_map_of_a_nine_tap_sum(dense):
    """NaN, +Inf and -Inf at a corner, an edge and the interior of 1 x 8 x 6 x 7: F.conv2d in float64 marks the same
    elements finite / +Inf / -Inf / NaN as the direct sum, and the finite ones are equal."""
    rng = X.rng_of(8, 6, 7, int(dense))
    x = X.ints(rng, (1, 8, 6, 7), 8)
    w = _weights(rng, (8, 8, 3, 3), 4, dense)
    for k, (y0, x0) in enumerate(((0, 0), (5, 3), (3, 6), (2, 3))):
        for value in (NAN, INF, -INF):
            xp = X.poison(x, [(0, (3 * k + 1) % 8, y0, x0)], value)
            got, _ = X.conv([xp], w, nonfinite=True)
            want = _nine_tap(xp, w)
            assert np.array_equal(X.class_map(got), X.class_map(want)), (y0, x0, value)
            X.assert_equal_with_nonfinite(got, want, "conv2d against the nine-tap sum")
            nonfin = X.class_map(got).any(axis=1)
            assert np.array_equal(nonfin, X.conv_footprint((1, 6, 7), [(0, 0, y0, x0)])), (y0, x0, value)
            if value == value and dense:
                assert not np.isnan(got).any()             # a single Inf times non-zero weights: +-Inf, never NaN


# =====================================================================================================================
# shared set-up
# =====================================================================================================================
def _weights(rng, shape, b, dense):
    w = X.weights(rng, shape, b)
    if dense:
        redraw = rng.choice(np.array([-1.0, 1.0], np.float32), size=shape) * rng.integers(1, b + 1, size=shape)
        w = np.where(w == 0, redraw, w).astype(np.float32)
        assert (w != 0).all()
    return w


def _seam_pixels(h, w):
    """(y, x) on both sides of every tile seam of conv3x3_mfma.hip inside an h x w image -- 3-row and 4-row tiles (GeoWide
    3 x 48, 4 x 48), strip tiles of 5 and 4 rows in either order (16 columns), 16-column MFMA pixel groups and the
    48-column tile edge -- plus the four corners."""
    rows = sorted({r for step in (3, 4, 5) for s in range(step, h, step) for r in (s - 1, s)} | {s for s in (4, 5, 8) if s < h}
                  | {s - 1 for s in (4, 5) if s < h})
    cols = [c for c in (15, 16, 47, 48) if c < w] or [w // 2]
    px = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    for i, r in enumerate(rows):
        px.append((r, cols[i % len(cols)]))
    for i, c in enumerate(cols):
        px.append((rows[(2 * i + 1) % len(rows)] if rows else 0, c))
    return list(dict.fromkeys(px))


def _poison_sets(n, h, w, channels):
    """The seam pixels dealt over the images and packed into launches: within one launch two poisons of one image are at
    least 7 pixels apart (Chebyshev).  Image 0's last pixel and image 1's first pixel come first.  -> lists of
    (n, c, y, x); the channel cycles over `channels`."""
    px = [(h - 1, w - 1), (0, 0)] + _seam_pixels(h, w)
    sets = []
    for k, (y, x) in enumerate(px):
        img = 0 if k == 0 else (1 % n if k == 1 else k % n)
        c = channels[k % len(channels)]
        for s in sets:
            if all(q[0] != img or max(abs(q[2] - y), abs(q[3] - x)) >= 7 for q in s):
                s.append((img, c, y, x))
                break
        else:
            sets.append([(img, c, y, x)])
    return sets


def _source_positions(pos, cps):
    """(n, c, y, x) over the channel concatenation -> {source index: [(n, c within the source, y, x)]}."""
    out = {}
    for (n, c, y, x) in pos:
        out.setdefault(c // cps, []).append((n, c % cps, y, x))
    return out


def _poisoned_conv(shape, epi, pos, value, seed=0, operand="src"):
    """One conv problem of test_exact_integer with `value` at `pos` of `operand`: the clean problem's precondition on
    the stand-in operands, then the poisoned operands and their float64 reference with torch's rules."""
    cout, cps, nsrc, n, h, w, _ = shape
    dense = value == value                               # an Inf needs weights without zeros
    p = E._conv_problem(shape, epi, seed)
    if dense:
        p["w"] = _weights(X.rng_of(cout, cps, nsrc, 4242 + seed), p["w"].shape, 4, True)
    kw = {k: p[k] for k in ("mask", "res0", "res1") if k in p}
    kw["relu"] = epi == "relu"
    clean = dict(p)
    if operand == "src":
        by_src = _source_positions(pos, cps)
        clean["xs"] = [X.unpoisoned(x, by_src.get(i, [])) for i, x in enumerate(p["xs"])]
        p["xs"] = [X.poison(x, by_src.get(i, []), value) for i, x in enumerate(p["xs"])]
    else:
        clean[operand] = X.unpoisoned(p[operand], pos)
        p[operand] = X.poison(p[operand], pos, value)
        for k in ("mask", "res0", "res1"):
            if k in p:
                kw[k] = p[k]
    ckw = {k: clean[k] for k in ("mask", "res0", "res1") if k in clean and k != "mask"}
    if "mask" in clean:
        ckw["mask"] = np.ones_like(clean["mask"])        # (the bound: every element passes)
    _, inter = X.conv(clean["xs"], clean["w"], clean["bias"], relu=kw["relu"], **ckw)
    if "base" in clean:
        inter.append(X.pixel_shuffle(inter[-1], 4) + clean["base"])
    X.assert_exact_precondition(inter)
    ref, _ = X.conv(p["xs"], p["w"], p["bias"], nonfinite=True, **kw)
    if epi.startswith("shuffle"):
        ref = X.pixel_shuffle(ref, 4)
        if epi == "shuffle_base":
            with np.errstate(invalid="ignore"):
                ref = ref + p["base"]
    p["ref"] = ref
    return p


def _footprint_of_reference(p, shape, epi, pos, value):
    """The reference's own non-finite set IS the 3 x 3 footprint in every output channel of the poisoned image (mode 1:
    mapped through PixelShuffle), so the bitwise comparison with it pins the footprint and everything outside it."""
    cout, cps, nsrc, n, h, w, _ = shape
    fp = np.broadcast_to(X.conv_footprint((n, h, w), pos)[:, None], (n, cout, h, w))
    if epi.startswith("shuffle"):
        fp = X.pixel_shuffle(np.ascontiguousarray(fp), 4)
    nonfin = X.class_map(p["ref"]) != 0
    if epi == "relu" and value != value:
        assert np.array_equal(np.isnan(p["ref"]), fp)
    elif epi == "relu":
        assert not (nonfin & ~fp).any() and not np.isnan(p["ref"]).any()      # (-Inf under the ReLU is 0)
    elif value != value:
        assert np.array_equal(np.isnan(p["ref"]), fp)
    else:
        assert np.array_equal(nonfin, fp) and not np.isnan(p["ref"]).any()


def _conv_entry_points(K, dev, shape, epi):
    """(name, run(d) -> out [N][cout][H][P] or the HR image) for every launch family that applies at `shape`."""
    cout, cps, nsrc, n, h, w, pitch = shape
    P = pitch or w
    aligned = P % 4 == 0
    relu, shuffle = epi == "relu", epi.startswith("shuffle")

    def kw(d):
        return dict(bias=d["bias"], relu=relu, mask=d["mask"], res0=d["res0"], res1=d["res1"], shuffle=shuffle, base=d["base"],
                    logical_w=None if pitch is None else w)

    def fresh(d):
        shp = (n, cout // 16, 4 * h, 4 * w) if shuffle else (n, cout, h, P)
        return torch.full(shp, SENTINEL, device=dev)

    eps = [("wide tiles", lambda d: K.conv3x3(d["xs"], d["wpk"], cout, out=fresh(d), **kw(d))),
           ("3-row tiles", lambda d: K.conv3x3(d["xs"], d["wpk"], cout, out=fresh(d), tile_rows=3, **kw(d)))]
    if aligned and cout in (48, 32) and epi != "mask":
        eps.append(("4-row tiles", lambda d: K.conv3x3(d["xs"], d["wpk"], cout, out=fresh(d), tile_rows=4, **kw(d))))
    if E._strips_applicable(shape, K, dev):
        def strips(d, which):
            out = fresh(d)
            for lo in range(n):                          # image by image: each launch must leave the others alone
                K.conv3x3(d["xs"], d["wpk"], cout, out=out, images=(lo, lo + 1), strips=which, **kw(d))
            return out
        eps.append(("strips, 5 rows first, images one by one", lambda d: strips(d, 1)))
        eps.append(("strips, 4 rows first, images one by one", lambda d: strips(d, 2)))
    return eps


def _check_mode0_padding(out, shape, what):
    cout, cps, nsrc, n, h, w, pitch = shape
    if pitch is not None and out.shape[-1] == pitch:
        pad = out[..., w:].cpu().numpy()
        assert not pad.view(np.uint32).any(), what + ": columns [W, pitch) are not +0.0"


CONV_FOOTPRINT_SHAPES = [
    (48, 48, 1, 2, 9, 52, None),      # 16-byte staging; every row seam, columns 15/16 and 47/48
    (32, 32, 1, 2, 9, 52, None),
    (64, 64, 1, 2, 9, 52, None),
    (48, 48, 2, 2, 9, 52, None),      # two sources: the last channel of source 0, the first of source 1
    (48, 48, 1, 2, 9, 13, 16),        # 16-byte staging of a pitched 13-column image
    (48, 48, 1, 2, 9, 13, None),      # register-staged
    (32, 32, 1, 2, 9, 13, None),
    (64, 64, 2, 2, 9, 13, None),
]


def _channels(shape):
    cout, cps, nsrc, n, h, w, _ = shape
    ch = [7, 8, 0, cps * nsrc - 1]
    if nsrc > 1:
        ch = [cps - 1, cps, 7, 8, cps * nsrc - 1]
    return ch


# =====================================================================================================================
# B.1  fp32 forward conv: activation footprints
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("shape", CONV_FOOTPRINT_SHAPES, ids=E._conv_id)
def test_fp32_conv_activation_footprints(hip_device, shape):
    """One NaN at src[n, ci, y, x] gives NaN at out[n, :, y-1..y+1, x-1..x+1] clipped to the image and changes nothing
    else: every other element, the other image of the batch and the padding columns equal the float64 reference bit for
    bit.  Positions: both sides of every tile seam, the corners, the last pixel of image 0 and the first of image 1,
    channels 7 / 8 and the sources' seam; plain, ReLU and (48 outputs) the pixel-shuffle exits; every tiling; the batched
    launch with the poison in job 0 only.  One seam set again with +Inf and -Inf on dense weights."""
    from larvanet_amd import kernels as K
    E._threads()
    cout, cps, nsrc, n, h, w, pitch = shape
    sets = _poison_sets(n, h, w, _channels(shape))
    assert all(max(abs(a[2] - b[2]), abs(a[3] - b[3])) >= 7 for s in sets for a in s for b in s if a is not b and a[0] == b[0])
    runs = [(epi, s, NAN) for epi in ("plain", "relu") for s in sets]
    runs += [("plain", sets[0], INF), ("relu", sets[0], -INF), ("relu", sets[0], INF), ("plain", sets[-1], -INF)]
    if cout == 48:
        runs += [("shuffle", sets[0], NAN), ("shuffle_base", sets[-1], NAN), ("shuffle_base", sets[0], INF)]
    other = None
    for k, (epi, pos, value) in enumerate(runs):
        p = _poisoned_conv(shape, epi, pos, value)
        _footprint_of_reference(p, shape, epi, pos, value)
        want = E._expected(p, shape, epi)
        d = E._device_operands(p, pitch, hip_device, K)
        tag = "%s %s %s at %s: " % (E._conv_id(shape), epi, _name(value), pos)
        for name, run in _conv_entry_points(K, hip_device, shape, epi):
            out = run(d)
            X.assert_equal_with_nonfinite(out, want, tag + name)
            if not epi.startswith("shuffle"):
                _check_mode0_padding(out, shape, tag + name)
        if (pitch or w) % 4 == 0 and k % 2 == 0:
            # the batched launch: the poison is in job 0 only, job 1 (another draw) stays clean bit for bit
            q = E._conv_problem(shape, epi, seed=1)
            X.assert_exact_precondition(q["inter"])
            dq = E._device_operands(q, pitch, hip_device, K)
            jobs = [{kk: v for kk, v in dict(srcs=e["xs"], wpk=e["wpk"], bias=e["bias"], base=e["base"]).items() if v is not None}
                    for e in (d, dq)]
            outs = K.conv3x3_batch(jobs, cout, relu=epi == "relu", shuffle=epi.startswith("shuffle"),
                                   logical_w=None if pitch is None else w)
            X.assert_equal_with_nonfinite(outs[0], want, tag + "batched launch, the poisoned job")
            X.assert_bits_equal(outs[1], E._expected(q, shape, epi), tag + "batched launch, the clean job")


@gpu
@pytest.mark.parametrize("persist", ["persistent", "one-workgroup-per-tile"])
def test_fp32_conv_footprints_past_the_workgroup_slots(hip_device, monkeypatch, persist):
    """The smallest case of test_exact_integer.SLOT_CASES (32 channels, 2 x 200 x 200: more tiles than workgroup
    slots) under the ReLU: the persistent-tile launch and, with LARVA_PERSIST=0, one workgroup per tile."""
    from larvanet_amd import kernels as K
    E._threads()
    c, n, h, w = min({s[:4] for s in E.SLOT_CASES}, key=lambda s: s[0] * s[1] * s[2] * s[3])
    pitch = (w + 3) // 4 * 4
    shape = (c, c, 1, n, h, w, pitch)
    pos = [(0, 7, h - 1, w - 1), (1, 8, 0, 0), (0, 0, 2, 47), (1, 8, 3, 48), (1, 7, 3, 15), (1, c - 1, 4, 160), (0, 5, 101, 96),
           (1, 9, 199, 0), (0, 3, 0, 199), (1, 2, 150, 143), (0, 1, 152, 144)]
    p = _poisoned_conv(shape, "relu", pos, NAN)
    _footprint_of_reference(p, shape, "relu", pos, NAN)
    want = E._expected(p, shape, "relu")
    d = E._device_operands(p, pitch, hip_device, K)
    if persist == "persistent":
        monkeypatch.delenv("LARVA_PERSIST", raising=False)
    else:
        monkeypatch.setenv("LARVA_PERSIST", "0")
    for rows in (3, 0, 4):
        out = K.conv3x3(d["xs"], d["wpk"], c, bias=d["bias"], relu=True, logical_w=w, tile_rows=rows)
        X.assert_equal_with_nonfinite(out, want, "c%d %dx%dx%d relu %s tile_rows=%d" % (c, n, h, w, persist, rows))


@gpu
@pytest.mark.parametrize("n,h,w,pitch,cout", [(2, 9, 52, None, 48), (2, 9, 13, 16, 48), (2, 5, 7, None, 32), (2, 9, 13, None, 64)],
                         ids=lambda v: str(v))
def test_direct_head_conv_footprints(hip_device, n, h, w, pitch, cout):
    """larva_head_conv3_direct (the 4-pixel kernel and the one-pixel kernel): NaN, then +Inf on dense weights, in the raw
    3-channel image."""
    from larvanet_amd import kernels as K
    rng = X.rng_of(n, h, w, cout, 3)
    x, b = X.ints(rng, (n, 3, h, w), 255, lo=0), X.ints(rng, (cout,), 3)
    for value in (NAN, INF, -INF):
        wt = _weights(rng, (cout, 3, 3, 3), 4, value == value)
        for pos in _poison_sets(n, h, w, [0, 1, 2]):
            _, inter = X.conv([X.unpoisoned(x, pos)], wt, b)
            X.assert_exact_precondition(inter)
            ref, _ = X.conv([X.poison(x, pos, value)], wt, b, nonfinite=True)
            fp = np.broadcast_to(X.conv_footprint((n, h, w), pos)[:, None], ref.shape)
            assert np.array_equal(X.class_map(ref) != 0, fp) and (value != value or not np.isnan(ref).any())
            out = K.head_conv3_direct(_dev(X.poison(x, pos, value), hip_device), _dev(wt, hip_device), _dev(b, hip_device),
                                      pitch=pitch)
            X.assert_equal_with_nonfinite(out, X.pad_pitch(ref.astype(np.float32), pitch or w),
                                          "direct head %s %s at %s" % ((n, h, w, pitch, cout), _name(value), pos))


# =====================================================================================================================
# B.2  reads outside the image range of a launch
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("shape", [(48, 48, 1, 3, 9, 52, None), (48, 48, 2, 3, 9, 13, 16), (32, 32, 1, 3, 9, 13, None),
                                   (48, 16, 1, 3, 9, 24, None)], ids=E._conv_id)
def test_an_image_range_reads_nothing_outside_itself(hip_device, shape):
    """images=(1, 2) of a batch of three whose images 0 and 2 are all NaN in src, res0, res1 and mask: the range's output
    holds no NaN and equals the clean run, the output outside the range is untouched.  Again with every operand in a
    guarded buffer of 0xFF bytes (NaN as fp32) at 16-byte residue 0 and 4.  Padding columns are not poisoned (the contract
    wants zeros there); the 16-channel head input keeps its padded channels 3..15 zero in every image."""
    from larvanet_amd import kernels as K
    E._threads()
    cout, cps, nsrc, n, h, w, pitch = shape
    head = cps == 16
    for epi in ("relu", "mask", "res01"):
        p = E._conv_problem(shape, epi)
        if head:
            for x in p["xs"]:
                x[:, 3:] = 0
            p["ref"], p["inter"] = X.conv(p["xs"], p["w"], p["bias"], relu=epi == "relu",
                                          **{k: p[k] for k in ("mask", "res0", "res1") if k in p})
        X.assert_exact_precondition(p["inter"])
        want = np.full((n, cout, h, pitch or w), SENTINEL, np.float32)
        want[1] = E._expected(p, shape, epi)[1]

        def outside(a, channels=None):
            a = a.copy()
            for img in (0, 2):
                a[img, :channels, :, :w] = NAN
            return a
        q = dict(p, xs=[outside(x, 3 if head else None) for x in p["xs"]])
        for k in ("mask", "res0", "res1"):
            if k in p:
                q[k] = outside(p[k])
        d = E._device_operands(q, pitch, hip_device, K)
        kw = dict(bias=d["bias"], relu=epi == "relu", mask=d["mask"], res0=d["res0"], res1=d["res1"],
                  logical_w=None if pitch is None else w, images=(1, 2))
        tag = "%s %s images (1, 2) of 3: " % (E._conv_id(shape), epi)
        variants = [("wide tiles", {}), ("3-row tiles", {"tile_rows": 3})]
        if E._strips_applicable(shape, K, hip_device):
            variants += [("strips", {"strips": 1}), ("strips, 4 rows first", {"strips": 2})]
        for name, extra in variants:
            out = torch.full(want.shape, SENTINEL, device=hip_device)
            K.conv3x3(d["xs"], d["wpk"], cout, out=out, **kw, **extra)
            assert not bool(torch.isnan(out).any()), tag + name + ": a NaN from outside the range reached the output"
            X.assert_bits_equal(out, want, tag + name)
        for off in (0, 4):
            checks = []

            def put(a):
                v, chk = placement.placed(np.ascontiguousarray(a), torch.float32, hip_device, off, fill=0xFF)
                checks.append(chk)
                return v
            pd = {"xs": [put(x.cpu().numpy()) for x in d["xs"]], "wpk": put(d["wpk"].cpu().numpy())}
            for k in ("mask", "res0", "res1"):
                pd[k] = None if d[k] is None else put(d[k].cpu().numpy())
            out = put(np.full(want.shape, SENTINEL, np.float32))
            K.conv3x3(pd["xs"], pd["wpk"], cout, out=out, bias=d["bias"], relu=epi == "relu", mask=pd["mask"], res0=pd["res0"],
                      res1=pd["res1"], logical_w=None if pitch is None else w, images=(1, 2))
            X.assert_bits_equal(out, want, tag + "guarded 0xFF buffers at residue %d" % off)
            for chk in checks:
                chk()


# =====================================================================================================================
# B.3  epilogue operands
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("shape", [(48, 48, 1, 2, 9, 52, None), (48, 48, 1, 2, 9, 13, 16), (32, 32, 1, 2, 9, 13, None),
                                   (64, 64, 1, 2, 9, 52, None)], ids=E._conv_id)
def test_epilogue_operands_act_pointwise(hip_device, shape):
    """NaN, +Inf and -Inf at single elements of bias, res0, res1, base and mask: exactly that element (that channel for
    bias) changes, to what torch gives.  The ReLU keeps NaN and +Inf and turns -Inf into 0; the mask passes where
    !(mask <= 0): NaN and +Inf pass, -Inf and both zeros (in the draw) do not."""
    from larvanet_amd import kernels as K
    E._threads()
    cout, cps, nsrc, n, h, w, pitch = shape
    px = _seam_pixels(h, w)
    elems = [(k % n, (7, 8, 0, cout - 1, 16, 15)[k % 6], y, x) for k, (y, x) in enumerate(px)]
    cases = [("plain", "bias"), ("relu", "bias"), ("res0", "res0"), ("res01", "res0"), ("res01", "res1"), ("mask", "mask")]
    if cout == 48:
        cases.append(("shuffle_base", "base"))
    for epi, operand in cases:
        for value in (NAN, INF, -INF):
            if operand == "bias":
                pos = [(7,), (cout - 1,)] if value != value else [(8,)]
            elif operand == "base":
                pos = [(0, 2, 4 * h - 1, 4 * w - 1), (1, 0, 0, 0), (0, 1, 13, (4 * 15 + 3) % (4 * w))]
            else:
                pos = elems
            p = _poisoned_conv(shape, epi, pos, value, operand=operand)
            changed = X.class_map(p["ref"]) != 0
            if operand == "bias":
                hit = np.zeros(cout, bool)
                hit[[c for (c,) in pos]] = True
                exp = np.broadcast_to(hit[None, :, None, None], changed.shape)
                if epi == "relu" and value == -INF:
                    exp = np.zeros_like(changed)
            else:
                exp = np.zeros(changed.shape, bool)
                if operand != "mask":                    # (a mask element selects, it is never added)
                    for t in pos:
                        exp[t] = True
            assert np.array_equal(changed, exp), (epi, operand, value)
            if operand == "mask":                        # NaN and +Inf pass the conv's value, -Inf gives +0.0
                passed, _ = X.conv(p["xs"], p["w"], p["bias"])
                for t in pos:
                    assert p["ref"][t] == (passed[t] if value != value or value > 0 else 0.0)
            want = E._expected(p, shape, epi)
            d = E._device_operands(p, pitch, hip_device, K)
            tag = "%s %s with %s in %s: " % (E._conv_id(shape), epi, _name(value), operand)
            for name, run in _conv_entry_points(K, hip_device, shape, epi):
                out = run(d)
                X.assert_equal_with_nonfinite(out, want, tag + name)
                if not epi.startswith("shuffle"):
                    _check_mode0_padding(out, shape, tag + name)


# =====================================================================================================================
# B.4  the input-gradient pass
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("shape", [(48, 48, 1, 2, 9, 48, None), (48, 48, 1, 1, 5, 13, None), (48, 48, 1, 2, 9, 13, 16),
                                   (32, 32, 1, 2, 9, 48, None), (64, 64, 1, 2, 9, 52, None)], ids=E._conv_id)
def test_input_gradient_footprints(hip_device, shape):
    """The footprint test on the tap-mirrored, transposed weight image (wpk_bwd): one NaN (then +-Inf on dense weights)
    in dy reaches dx[n, :, y-1..y+1, x-1..x+1]; under the ReLU-backward mask only where !(mask <= 0); the skip gradients
    are added on top."""
    from larvanet_amd import kernels as K
    E._threads()
    c, _, _, n, h, w, pitch = shape
    rng = X.rng_of(c, n, h, w, 99)
    dy = X.ints(rng, (n, c, h, w), 8)
    mask, r0, r1 = X.masks(rng, (n, c, h, w)), X.ints(rng, (n, c, h, w), 8), X.ints(rng, (n, c, h, w), 8)
    pad = (lambda t: t) if pitch is None else (lambda t: X.pad_pitch(t, pitch))
    lw = None if pitch is None else w
    sets = _poison_sets(n, h, w, [7, 8, 0, c - 1])
    for value, use in ((NAN, sets), (INF, sets[:1]), (-INF, sets[-1:])):
        wt = _weights(rng, (c, c, 3, 3), 4, value == value)
        _, bwd = K.pack_weights(_dev(wt, hip_device))
        for pos in use:
            dyp = X.poison(dy, pos, value)
            dyd = _dev(pad(dyp), hip_device)
            for name, kw_ref in (("mask", {"mask": mask}), ("res0", {"res0": r0}), ("res01", {"res0": r0, "res1": r1})):
                _, inter = X.dgrad(X.unpoisoned(dy, pos), wt, **{k: (np.ones_like(v) if k == "mask" else v) for k, v in kw_ref.items()})
                X.assert_exact_precondition(inter)
                ref, _ = X.dgrad(dyp, wt, nonfinite=True, **kw_ref)
                fp = np.broadcast_to(X.conv_footprint((n, h, w), pos)[:, None], ref.shape)
                nonfin = X.class_map(ref) != 0
                assert np.array_equal(nonfin, fp & X.mask_passes(mask) if name == "mask" else fp)
                want = pad(ref.astype(np.float32))
                kw_dev = {k: _dev(pad(v), hip_device) for k, v in kw_ref.items()}
                tag = "dgrad %s %s %s at %s: " % (E._conv_id(shape), name, _name(value), pos)
                X.assert_equal_with_nonfinite(K.conv3x3(dyd, bwd, c, logical_w=lw, **kw_dev), want, tag + "wide tiles")
                X.assert_equal_with_nonfinite(K.conv3x3(dyd, bwd, c, logical_w=lw, tile_rows=3, **kw_dev), want, tag + "3-row tiles")
                if E._strips_applicable(shape, K, hip_device):
                    for which in (1, 2):
                        X.assert_equal_with_nonfinite(K.conv3x3(dyd, bwd, c, logical_w=lw, strips=which, **kw_dev), want,
                                                      tag + "strips %d" % which)
                if (pitch or w) % 4 == 0:
                    clean = _dev(pad(dy), hip_device)
                    outs = K.conv3x3_batch([dict(srcs=dyd, wpk=bwd, **kw_dev), dict(srcs=clean, wpk=bwd, **kw_dev)], c, logical_w=lw)
                    X.assert_equal_with_nonfinite(outs[0], want, tag + "batched, the poisoned job")
                    cref, _ = X.dgrad(dy, wt, **kw_ref)
                    X.assert_bits_equal(outs[1], pad(cref.astype(np.float32)), tag + "batched, the clean job")


# =====================================================================================================================
# B.5  weight and bias gradients
# =====================================================================================================================
def _wgrad_expected(clean_dw, clean_db, dy_pos, x_pos, valid):
    """dw / db of the clean operands with the rows (a NaN in dy[n, co]) and columns (a NaN in x[n, ci]) the poisons
    reach set to NaN.  Holds for poisons at 1 <= y <= H - 2, 1 <= x <= W - 2: all nine tap partners are in the image."""
    dw, db = clean_dw.copy(), clean_db.copy()
    for (_, co, _, _) in dy_pos:
        dw[co], db[co] = NAN, NAN
    for (_, ci, _, _) in x_pos:
        assert ci < valid
        dw[:, ci] = NAN
    return dw, db


def _wgrad_poisoned(case, job, dy_pos, x_pos):
    """The problem of test_exact_integer (precondition on the stand-in operands) with NaN at dy_pos / x_pos, the
    expected gradients, and torch's own float64 gradients of the poisoned operands agreeing with them by class."""
    cout, cin, valid, n, h, w, _ = case
    p = E._wgrad_problem(case, job)
    for (_, _, y, x) in list(dy_pos) + list(x_pos):
        assert 1 <= y <= h - 2 and 1 <= x <= w - 2
    _, _, inter = X.wgrad(X.unpoisoned(p["dy"], dy_pos), X.unpoisoned(p["x"], x_pos)[:, :valid])
    X.assert_exact_precondition(inter)
    q = dict(p, dy=X.poison(p["dy"], dy_pos, NAN) if dy_pos else p["dy"], x=X.poison(p["x"], x_pos, NAN) if x_pos else p["x"])
    q["dw"], q["db"] = _wgrad_expected(p["dw"], p["db"], dy_pos, x_pos, valid)
    tdw, tdb, _ = X.wgrad(q["dy"], q["x"][:, :valid])
    X.assert_equal_with_nonfinite(tdw, q["dw"], "torch's weight gradient of the poisoned operands")
    X.assert_equal_with_nonfinite(tdb, q["db"], "torch's bias gradient of the poisoned operands")
    return q


def _wgrad_device_jobs(probs, cout, valid, dev, wide):
    jobs = []
    wide_dw = torch.full((cout, valid * len(probs) + 5, 3, 3), SENTINEL, device=dev) if wide else None
    for j, p in enumerate(probs):
        job = {"dy": _dev(p["dy"], dev), "x": _dev(p["x"], dev), "db": torch.full((cout,), SENTINEL, device=dev), "cin_valid": valid}
        if wide:
            job["dw"], job["cin_off"] = wide_dw, 5 + valid * j
        else:
            job["dw"], job["cin_off"] = torch.full((cout, valid, 3, 3), SENTINEL, device=dev), 0
        jobs.append(job)
    return jobs, wide_dw


def _check_wgrad_nf(probs, jobs, wide_dw, what):
    for j, (p, job) in enumerate(zip(probs, jobs)):
        valid = job["cin_valid"]
        got = job["dw"] if wide_dw is None else wide_dw[:, job["cin_off"]:job["cin_off"] + valid].contiguous()
        X.assert_equal_with_nonfinite(got, p["dw"], "%s job %d dw" % (what, j))
        X.assert_equal_with_nonfinite(job["db"], p["db"], "%s job %d db" % (what, j))
    if wide_dw is not None:
        assert bool((wide_dw[:, :5] == SENTINEL).all()), what + ": channels outside the slices were written"


@gpu
@pytest.mark.parametrize("case", [(48, 48, 48, 2, 9, 48, 2), (48, 48, 48, 1, 5, 13, 2), (48, 16, 3, 2, 6, 48, 2), (48, 16, 3, 1, 7, 13, 2),
                                  (32, 32, 32, 2, 6, 48, 2), (64, 64, 64, 1, 6, 52, 2), (32, 48, 48, 1, 7, 13, 2)],
                         ids=lambda c: "%dx%d(valid %d)-N%d-%dx%d-%djobs" % c)
def test_weight_gradient_rows_and_columns_a_nan_reaches(hip_device, case):
    """A NaN in dy[n, co, y, x] makes all of dw[co] and db[co] NaN and nothing else; a NaN in x[n, ci, y, x] makes
    dw[:, ci] NaN, db and every other column stay exact.  The poison sits in job 0; job 1 of the same launch stays exact.

    The poisons sit at 1 <= y <= H - 2 and 1 <= x <= W - 2, where all nine tap partners are inside the image.  At the
    border a kernel that zero-fills a tile overhang (0 x NaN = NaN) and a reference that skips the tap may both be
    right; that is not what this test is for."""
    from larvanet_amd import kernels as K
    E._threads()
    cout, cin, valid, n, h, w, njobs = case
    rows = sorted({1, h - 2, min(3, h - 2), min(2, h - 2)})
    cols = sorted({1, w - 2, min(15, w - 2), min(16, w - 2)} | ({47, 48} & set(range(1, w - 1))))
    what = "wgrad %dx%d N%d %dx%d" % (cout, cin, n, h, w)
    layouts = []
    for k in range(3):
        y, x = rows[k % len(rows)], cols[(2 * k + 1) % len(cols)]
        layouts.append(([((n - 1) * (k % 2), (7, cout - 1, 16)[k], y, x)], []))
        layouts.append(([], [(0 if k else n - 1, (0, valid - 1, min(8, valid - 1))[k], rows[-1 - k % len(rows)], cols[k % len(cols)])]))
    for dy_pos, x_pos in layouts[:4] + [(layouts[4][0], layouts[5][1])]:
        probs = [_wgrad_poisoned(case, 0, dy_pos, x_pos), E._wgrad_problem(case, 1)]
        X.assert_exact_precondition(probs[1]["inter"])
        tag = "%s NaN at dy %s x %s" % (what, dy_pos, x_pos)
        for splits in (1, 3, 8):
            jobs, _ = _wgrad_device_jobs(probs, cout, valid, hip_device, False)
            K.conv3x3_wgrad(jobs, cout, cin, splits)
            _check_wgrad_nf(probs, jobs, None, "%s splits %d" % (tag, splits))
        jobs, wide = _wgrad_device_jobs(probs, cout, valid, hip_device, True)
        K.conv3x3_wgrad(jobs, cout, cin, 3)
        _check_wgrad_nf(probs, jobs, wide, tag + " slices of a wide gradient")
        jobs, _ = _wgrad_device_jobs(probs, cout, valid, hip_device, False)
        parts, used = K.conv3x3_wgrad_partial(jobs, cout, cin, 5)
        K.wgrad_reduce([dict(j, partial=p, splits=used, cout=cout, cin=cin) for j, p in zip(jobs, parts)])
        _check_wgrad_nf(probs, jobs, None, tag + " _partial + larva_wgrad_reduce")


@gpu
@pytest.mark.parametrize("njobs,nwg,n,h,w,head", [(5, 7, 2, 9, 48, False), (3, 64, 1, 6, 48, True)], ids=lambda v: str(v))
def test_flat_weight_gradient_grid_keeps_a_nan_in_its_layer(hip_device, njobs, nwg, n, h, w, head):
    """larva_conv3x3_wgrad_partial_flat / _flat_head: shares cross layer boundaries, so a workgroup holds the partial
    image of the poisoned layer and of its neighbour in turn.  The poison sits in ONE layer (each body layer in turn,
    then the head): its row / column is NaN, every other layer -- and the head when a body layer is poisoned, and the
    reverse -- is exact."""
    from larvanet_amd import kernels as K
    E._threads()
    c = 48
    rng = X.rng_of(njobs, nwg, n, h, w, 5)
    layers = [{"dy": X.ints(rng, (n, c, h, w), 2), "x": X.ints(rng, (n, c, h, w), 2)} for _ in range(njobs)]
    if head:
        x16 = np.zeros((n, 16, h, w), np.float32)
        x16[:, :3] = X.ints(rng, (n, 3, h, w), 2)
        layers.append({"dy": X.ints(rng, (n, 48, h, w), 2), "x": x16})
    clean = []
    for i, l in enumerate(layers):
        valid = 3 if head and i == njobs else c
        dw, db, inter = X.wgrad(l["dy"], l["x"][:, :valid])
        X.assert_exact_precondition(inter + [4.0 * n * h * w])       # (the poisoned stand-in is within the drawn range)
        clean.append((dw, db, valid))
    cols = [c_ for c_ in (1, 15, 16, 46) if c_ <= w - 2]
    for target in range(len(layers)):
        for kind in ("dy", "x"):
            valid = clean[target][2]
            pos = [((n - 1) * (target % 2), (7 + target) % (c if kind == "dy" else valid), 1 + target % (h - 2), cols[target % len(cols)])]
            ops = [dict(l) for l in layers]
            ops[target][kind] = X.poison(layers[target][kind], pos, NAN)
            dev = [{"dy": _dev(o["dy"], hip_device), "x": _dev(o["x"], hip_device),
                    "dw": torch.full((48, v, 3, 3), SENTINEL, device=hip_device), "db": torch.full((48,), SENTINEL, device=hip_device)}
                   for o, (_, _, v) in zip(ops, clean)]
            hd = dict(dev[-1], cin_off=0, cin_valid=3) if head else None
            body = dev[:njobs]
            res = K.conv3x3_wgrad_partial_flat(body, c, c, nwg, head=hd)
            assert res is not None, "the flat launch must apply at this shape"
            parts, splits = res
            rj = [dict(j, partial=p, splits=s, cout=c, cin=c) for j, p, s in zip(body, parts, splits)]
            if hd is not None:
                rj.append(dict(hd, partial=parts[-1], splits=splits[-1], cout=48, cin=16))
            K.wgrad_reduce(rj)
            for i, (j, (dw, db, v)) in enumerate(zip(dev, clean)):
                wdw, wdb = (dw, db) if i != target else _wgrad_expected(dw, db, pos if kind == "dy" else [], pos if kind == "x" else [], v)
                what = "flat grid %s NaN in %s of layer %d at %s: layer %d" % ((njobs, nwg, n, h, w, head), kind, target, pos, i)
                X.assert_equal_with_nonfinite(j["dw"], wdw, what + " dw")
                X.assert_equal_with_nonfinite(j["db"], wdb, what + " db")


# =====================================================================================================================
# B.6  exits and the loss tail
# =====================================================================================================================
def _block_sum(v):
    """The fixed order of loss_terms_block / l1_finish_kernel in numpy float32: 256 threads take the elements k, k + 256,
    ...; each 64-lane wave adds with the xor butterfly (32, 16, .., 1); then (w0 + w1) + (w2 + w3)."""
    v = np.asarray(v, np.float32).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        lanes = np.zeros(256, np.float32)
        for k in range(0, len(v), 256):
            chunk = v[k:k + 256]
            lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
        ws = lanes.reshape(4, 64).copy()
        for o in (32, 16, 8, 4, 2, 1):
            ws = ws + ws[:, np.arange(64) ^ o]
        return np.float32(np.float32(ws[0, 0] + ws[1, 0]) + np.float32(ws[2, 0] + ws[3, 0]))


def _loss_terms_ref(terms, scales, divisor):
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.float32(0)
        for t, s in zip(terms, scales):
            total = np.float32(total + np.float32(_block_sum(t) * np.float32(s)))
        return np.float32(total / np.float32(divisor))


def _same_scalar(got, want, what):
    X.assert_equal_with_nonfinite(np.asarray(float(got), np.float32).reshape(1), np.asarray(want, np.float32).reshape(1), what)


L1_VALUE_CASES = ("nan-in-out", "inf-minus-inf", "inf-out", "inf-truth")


def _l1_value_case(case, out, truth):
    """-> (out, truth, class of the loss) with the case's values at elements spread over planes, rows and a last column."""
    n, c, hh, ww = out.shape
    spots = [(0, 0, 0, 0), (n - 1, c - 1, hh - 1, ww - 1), (0, 1, hh // 2, ww // 2 + 1), (n - 1, 0, 5, ww - 1)]
    if case == "nan-in-out":
        return X.poison(out, spots, NAN), truth, "nan"
    if case == "inf-minus-inf":
        return X.poison(out, spots, INF), X.poison(truth, spots, INF), "nan"
    if case == "inf-out":
        return X.poison(out, spots[:2], INF), X.poison(truth, spots[2:], -INF), "inf"     # both differences are +Inf
    return X.poison(out, spots[2:], -INF), X.poison(truth, spots[:2], INF), "inf"         # both differences are -Inf


def _is_class(v, cls):
    v = float(v)
    return v != v if cls == "nan" else v == INF


@gpu
@pytest.mark.parametrize("case", L1_VALUE_CASES)
def test_l1_kernels_follow_torchs_sign_and_sum(hip_device, case):
    """larva_l1_fwd, _partial, _partial_grad, _partial_grad_batch, _l1_bwd, _l1_bwd_unshuffle4, _l1_bwd_unshuffle (x2, x3) and
    _shuffle_l1_partial_grad (x2, x3): the gradient is where(d > 0, g, where(d < 0, -g, 0)) bit for bit -- 0 at a NaN and
    at Inf - Inf, +-g at +-Inf --, the padded gradient channels stay +0.0, the partial sums hold the NaN / +Inf and the
    loss is NaN / +Inf, as nn.L1Loss gives."""
    from larvanet_amd import kernels as K
    dev = hip_device
    rng = X.rng_of(6, L1_VALUE_CASES.index(case))
    out0 = X.ints(rng, (2, 3, 24, 24), 255, lo=0)
    truth0 = (out0 + X.ints(rng, out0.shape, 3)).astype(np.float32)
    out, truth, cls = _l1_value_case(case, out0, truth0)
    numel = out.size
    t_out = torch.from_numpy(out).requires_grad_(True)
    t_loss = torch.nn.L1Loss()(t_out, torch.from_numpy(truth))
    (t_loss * 0.125).backward()
    assert _is_class(t_loss.detach(), cls)
    g = np.float32(0.125) * (np.float32(1.0) / np.float32(numel))      # (a power of two times 1 / numel: one rounding)
    sg = X.l1_sign_grad(out, truth, g)
    X.assert_bits_equal(t_out.grad.numpy(), sg, "l1_sign_grad against nn.L1Loss's gradient (%s)" % case)
    a, b = _dev(out, dev), _dev(truth, dev)
    gout = torch.tensor(0.25, device=dev)
    assert _is_class(K.l1_fwd(a, b), cls), "larva_l1_fwd " + case
    X.assert_bits_equal(K.l1_bwd(a, b, torch.tensor(0.125, device=dev)), sg, "larva_l1_bwd " + case)
    un4 = X.pixel_unshuffle(sg, 4)
    X.assert_bits_equal(K.l1_bwd_unshuffle4(a, b, gout, 0.5), un4, "larva_l1_bwd_unshuffle4 " + case)
    part, inv = K.l1_partial(a, b)
    pv = part.cpu().numpy()
    assert _is_class(pv.sum(), cls) and int((X.class_map(pv) != 0).sum()) <= 4, "larva_l1_partial " + case
    _same_scalar(K.loss_from_partials([part], [inv], 1.0), _loss_terms_ref([pv], [inv], 1.0), "loss of larva_l1_partial " + case)
    part2, _, grad2 = K.l1_partial_grad(a, b, 0.25, 0.5)
    X.assert_equal_with_nonfinite(part2, pv, "larva_l1_partial_grad partial sums " + case)
    X.assert_bits_equal(grad2, un4, "larva_l1_partial_grad gradient " + case)
    clean = _dev(out0, dev)
    pb, _, gb = K.l1_partial_grad_batch([clean, a, clean], b, 0.25, 0.5)
    # (one truth for all exits: the clean exits see the truth's own poison and nothing of the poisoned exit)
    X.assert_equal_with_nonfinite(pb[1], pv, "larva_l1_partial_grad_batch, the poisoned exit " + case)
    X.assert_bits_equal(gb[1], un4, "larva_l1_partial_grad_batch gradient " + case)
    X.assert_bits_equal(gb[0], X.pixel_unshuffle(X.l1_sign_grad(out0, truth, g), 4), "larva_l1_partial_grad_batch, a clean exit")
    X.assert_bits_equal(gb[2], gb[0].cpu().numpy(), "larva_l1_partial_grad_batch, the other clean exit")
    if case == "nan-in-out":
        assert np.isfinite(pb[0].cpu().numpy()).all() and np.isfinite(pb[2].cpu().numpy()).all()
    for s in (2, 3):
        cpad = 32
        gs = X.pad_channels(X.pixel_unshuffle(sg, s), cpad)
        got = K.l1_bwd_unshuffle(a, b, gout, s, cpad, 0.5)
        X.assert_bits_equal(got, gs, "larva_l1_bwd_unshuffle x%d %s" % (s, case))
        # the same image as PixelShuffle(s)(y) + base: y carries the conv part, the base the rest (and the Inf / NaN)
        h, w = 24 // s, 24 // s
        y = X.pad_channels(X.ints(rng, (2, 3 * s * s, h, w), 20), cpad)
        ys = X.pixel_shuffle(y[:, :3 * s * s], s)
        with np.errstate(invalid="ignore"):
            base = (out - ys).astype(np.float32)
            img = (ys + base).astype(np.float32)
        X.assert_equal_with_nonfinite(img, out, "set-up: y + base is the image")
        part3, inv3, grad3, image = K.shuffle_l1_partial_grad(_dev(y, dev), _dev(base, dev), b, 0.25, 0.5, s)
        X.assert_equal_with_nonfinite(image, out, "larva_shuffle_l1_partial_grad x%d image %s" % (s, case))
        X.assert_bits_equal(grad3, gs, "larva_shuffle_l1_partial_grad x%d gradient %s" % (s, case))
        assert not grad3[:, 3 * s * s:].cpu().numpy().view(np.uint32).any()
        assert _is_class(part3.cpu().numpy().sum(), cls)
        assert _is_class(K.loss_from_partials([part3], [inv3], 1.0), cls), "loss of larva_shuffle_l1_partial_grad x%d %s" % (s, case)


@gpu
@pytest.mark.parametrize("case", L1_VALUE_CASES)
def test_exits_scored_inside_the_conv_launch_with_nonfinite_values(hip_device, case):
    """larva_conv3x3_exit_l1_batch, three exits: a NaN in the SOURCE of exit 1 ("nan-in-out") is NaN over the 3 x 3
    footprint mapped through PixelShuffle, zero gradient there, NaN partial sums and loss for that exit only; the
    Inf cases sit in exit 1's base (and, shared by all exits, in the truth)."""
    from larvanet_amd import kernels as K
    E._threads()
    njobs, n, h, w = 3, 2, 9, 48
    shape = (48, 48, 1, n, h, w, None)
    probs = [E._conv_problem(shape, "shuffle_base", seed=20 + j) for j in range(njobs)]
    rng = X.rng_of(66, L1_VALUE_CASES.index(case))
    truth = (probs[0]["ref"] + X.ints(rng, probs[0]["ref"].shape, 3)).astype(np.float32)
    for p in probs:
        X.assert_exact_precondition(p["inter"])
    for p in probs[1:]:
        delta = X.ints(rng, p["ref"].shape, 3)
        p["base"] = (p["base"] + (truth - p["ref"]) + delta).astype(np.float32)
        p["ref"] = truth.astype(np.float64) + delta
        X.assert_exact_precondition([p["base"], p["ref"]])
    q = probs[1]
    if case == "nan-in-out":
        pos = [(0, 7, 2, 15), (1, 8, 3, 47), (0, 47, 8, 47), (1, 0, 0, 0)]
        clean, _ = X.conv([X.unpoisoned(q["xs"][0], pos)], q["w"], q["bias"])
        X.assert_exact_precondition([clean, X.conv_sum_bound([X.unpoisoned(q["xs"][0], pos)], q["w"], q["bias"])])
        q["xs"] = [X.poison(q["xs"][0], pos, NAN)]
        fp = X.pixel_shuffle(np.ascontiguousarray(np.broadcast_to(X.conv_footprint((n, h, w), pos)[:, None], (n, 48, h, w))), 4)
        q["ref"] = np.where(fp, NAN, q["ref"])
        y, _ = X.conv(q["xs"], q["w"], q["bias"], nonfinite=True)
        assert np.array_equal(np.isnan(X.pixel_shuffle(y, 4)), fp)
    else:
        img, truth, _ = _l1_value_case(case, q["ref"].astype(np.float32), truth)
        moved = X.class_map(img) != 0
        q["base"] = np.where(moved, img, q["base"]).astype(np.float32)
        q["ref"] = np.where(moved, img, q["ref"])
    cls = {"nan-in-out": "nan", "inf-minus-inf": "nan"}.get(case, "inf")
    jobs = []
    for p in probs:
        d = E._device_operands(p, None, hip_device, K)
        jobs.append({"srcs": d["xs"], "wpk": d["wpk"], "bias": d["bias"], "base": d["base"]})
    numel = truth.size
    gscale = float(np.float32(1.0) / np.float32(njobs))
    g = np.float32((np.float32(1.0) * np.float32(gscale)) * (np.float32(1.0) / np.float32(numel)))
    res = K.conv3x3_exit_l1_batch(jobs, 48, _dev(truth, hip_device), 1.0, gscale, [True] * njobs)
    assert res is not None, "the fused exit launch must apply at this shape"
    outs, parts, grads = res
    truth_poisoned = bool((X.class_map(truth) != 0).any())
    for j, p in enumerate(probs):
        what = "exit %d (%s)" % (j, case)
        X.assert_equal_with_nonfinite(outs[j], p["ref"], what + " image")
        X.assert_bits_equal(grads[j], X.pixel_unshuffle(X.l1_sign_grad(p["ref"], truth, g), 4), what + " gradient")
        pv = parts[j].cpu().numpy()
        loss = K.loss_from_partials([parts[j]], [1.0 / numel], 1.0)
        if j == 1 or truth_poisoned:
            want = cls if j == 1 else "inf"              # (a clean exit against a truth holding +Inf: |finite - Inf|)
            assert _is_class(pv.sum(), want) and _is_class(loss, want), (what, float(loss))
        else:
            assert np.isfinite(pv).all() and (pv == np.rint(pv)).all(), what + ": a clean exit's partial sums"
            with np.errstate(invalid="ignore"):
                exact = float(np.abs(p["ref"] - truth).sum())
            assert float(pv.astype(np.float64).sum()) == exact, what
    if not truth_poisoned:
        assert _is_class(K.loss_from_partials(parts, [1.0 / numel] * njobs, float(njobs)), cls)


@gpu
def test_scalar_loss_tail_with_nan_and_inf_terms(hip_device):
    """larva_loss_from_partials, larva_sum_scalars and larva_wgrad_reduce_with_loss with a NaN term, a +Inf term and
    both, against numpy float32 sums in the kernels' documented order; and a HostCell that receives 1.5, NaN, 2.5."""
    from larvanet_amd import kernels as K
    dev = hip_device
    rng = X.rng_of(61)
    vec = (rng.random(700) * 1000).astype(np.float32)
    small = (rng.random(37) * 10).astype(np.float32)
    lists = {"finite": [vec, small, np.float32([3.5])],
             "nan": [X.poison(vec, [(300,)], NAN), small, np.float32([3.5])],
             "inf": [vec, X.poison(small, [(36,)], INF), np.float32([3.5])],
             "inf-scalar": [vec, small, np.float32([INF])],
             "both": [X.poison(vec, [(0,)], INF), small, np.float32([NAN])],
             "inf-minus-inf": [X.poison(vec, [(699,)], INF), X.poison(small, [(1,)], -INF), np.float32([3.5])]}
    scales = [2.0 ** -13, 0.25, 1.0]        # (powers of two: a product fused into the running sum rounds the same)
    jobs = [{"dy": _dev(X.ints(rng, (1, 48, 6, 48), 2), dev), "x": _dev(X.ints(rng, (1, 48, 6, 48), 2), dev),
             "dw": torch.empty((48, 48, 3, 3), device=dev), "db": torch.empty(48, device=dev)}]
    parts, used = K.conv3x3_wgrad_partial(jobs, 48, 48, 2)
    rjobs = [dict(j, partial=p, splits=used, cout=48, cin=48) for j, p in zip(jobs, parts)]
    K.wgrad_reduce(rjobs)
    dw_ref = jobs[0]["dw"].clone()
    for name, terms in lists.items():
        want = _loss_terms_ref(terms, scales, 3.0)
        assert {"finite": np.isfinite(want), "nan": np.isnan(want), "inf": want == INF, "inf-scalar": want == INF,
                "both": np.isnan(want), "inf-minus-inf": np.isnan(want)}[name]
        td = [_dev(t, dev) if t.size > 1 else torch.tensor(float(t[0]), device=dev) for t in terms]
        _same_scalar(K.loss_from_partials(td, scales, 3.0), want, "larva_loss_from_partials, " + name)
        loss = torch.full((), SENTINEL, device=dev)
        jobs[0]["dw"].fill_(SENTINEL)
        K.wgrad_reduce(rjobs, loss=(td, scales, 3.0, loss))
        _same_scalar(loss, want, "larva_wgrad_reduce_with_loss, " + name)
        assert torch.equal(jobs[0]["dw"], dw_ref), "the gradient of the launch that carries a %s loss" % name
        sc = [np.float32(1.5), np.float32(terms[2][0]), np.float32(terms[1][-1])]
        with np.errstate(invalid="ignore"):
            ssum = np.float32(np.float32(np.float32(np.float32(0) + sc[0]) + sc[1]) + sc[2]) / np.float32(3.0)
        _same_scalar(K.sum_scalars([torch.tensor(float(v), device=dev) for v in sc], 3.0), ssum, "larva_sum_scalars, " + name)
    cell = K.HostCell()
    for k, v in enumerate((1.5, NAN, 2.5), 1):
        cell.expect()
        K.loss_from_partials([torch.tensor(v, device=dev)], [1.0], 1.0, host_cell=cell)
        torch.cuda.synchronize()
        got = cell.take()
        assert got is not None, "launch %d stored nothing into the host cell" % k
        assert (got != got) if v != v else got == v, (k, got)
        assert cell.sequence == k, (cell.sequence, k)


# =====================================================================================================================
# B.7  upsampling: the footprint is the tap set
# =====================================================================================================================
def _plane_poisons(shape):
    """One poison per plane of [N][C][H][W]: a corner, two edges, the interior."""
    n, c, h, w = shape
    spots = [(0, 0), (0, w // 2), (h // 2, w - 1), (h // 2, w // 2)]
    return [(k // c % n, k % c, y, x) for k, (y, x) in enumerate(spots)]


def _interp(x, s, mode, dtype):
    with np.errstate(invalid="ignore"):
        return F.interpolate(torch.from_numpy(x.astype(dtype)), scale_factor=s, mode=mode, align_corners=False).numpy()


def _check_upsample(got, x, s, mode, value, what):
    """The non-finite set against F.interpolate on the CPU in fp32 and in float64: where the two agree (always at the
    dyadic phases of x2 and x4) the kernel's set equals it; at x3 it lies between their intersection and their union.
    With an Inf poison (bilinear: weights of one sign) the classes agree as well.  The finite outputs at the existing
    upsample tests' bar."""
    got = got.cpu().numpy()
    r32, r64 = _interp(x, s, mode, np.float32), _interp(x, s, mode, np.float64)
    s32, s64, sg = X.class_map(r32) != 0, X.class_map(r64) != 0, X.class_map(got) != 0
    if s != 3:
        assert np.array_equal(s32, s64), what + ": set-up: fp32 and float64 tap sets differ at a dyadic phase"
    lo, hi = s32 & s64, s32 | s64
    miss, extra = np.argwhere(lo & ~sg), np.argwhere(sg & ~hi)
    assert not len(miss) and not len(extra), "%s: %d outputs lost the poison (first %s), %d gained it (first %s)" % (
        what, len(miss), miss[:1].tolist(), len(extra), extra[:1].tolist())
    if s == 3:
        print("%s: the kernel's set equals %s" % (what, "both" if np.array_equal(s32, s64) else
                                                   "the fp32 set" if np.array_equal(sg, s32) else
                                                   "the float64 set" if np.array_equal(sg, s64) else "neither (between them)"))
    if value == value:
        agree = lo & (X.class_map(r32) == X.class_map(r64))
        assert np.array_equal(X.class_map(got)[agree], X.class_map(r32)[agree]), what + ": class of an Inf output"
    fin = ~hi
    np.testing.assert_allclose(got[fin], r32[fin], rtol=1e-5, atol=3e-4, err_msg=what)


@gpu
@pytest.mark.parametrize("shape", [(2, 2, 5, 6), (2, 2, 9, 13)], ids=lambda s: "x".join(map(str, s)))
def test_upsample_footprints_are_the_tap_sets(hip_device, shape):
    """larva_upsample_fwd (x2, x3), larva_upsample4_fwd (both modes) and larva_bicubic4_fwd (both kernels: aligned and
    unaligned out): one NaN per plane (corner, two edges, interior; N C = 4 planes, so a leak across planes shows) marks
    the outputs whose taps hold it.  +-Inf for bilinear only: bicubic weights have both signs and the edge clamp repeats
    the pixel, so the class there depends on rounding."""
    from larvanet_amd import hip_lib, kernels as K
    lib = hip_lib.load()
    n, c, h, w = shape
    x0 = (np.random.default_rng([n, c, h, w, 7]).random(shape) * 255).astype(np.float32)
    pos = _plane_poisons(shape)
    for mode in ("bicubic", "bilinear"):
        for value in ((NAN,) if mode == "bicubic" else (NAN, INF, -INF)):
            x = X.poison(x0, pos, value)
            xd = _dev(x, hip_device)
            for s in (2, 3, 4):
                _check_upsample(K.upsample(xd, s, mode), x, s, mode, value, "upsample x%d %s %s %s" % (s, mode, _name(value), shape))
    x = X.poison(x0, pos, NAN)
    _check_upsample(K.bicubic4(_dev(x, hip_device)), x, 4, "bicubic", NAN, "bicubic4 %s" % (shape,))
    out, check = placement.placed((n, c, 4 * h, 4 * w), torch.float32, hip_device, 4)
    hip_lib.check(lib.larva_bicubic4_fwd(_dev(x, hip_device).data_ptr(), out.data_ptr(), n, c, h, w, K._stream()), "larva_bicubic4_fwd")
    _check_upsample(out, x, 4, "bicubic", NAN, "bicubic4 into an unaligned out %s" % (shape,))
    check()


@gpu
def test_step_prologue_copies_and_upsamples_a_nan_where_it_belongs(hip_device):
    """larva_step_prologue: x16[:, :3] is x with its NaN, the padded channels stay zero, and the base image holds NaN on
    the bicubic tap set of the poisoned pixels."""
    from larvanet_amd import kernels as K
    shape = (2, 3, 9, 13)
    n, c, h, w = shape
    x0 = (np.random.default_rng(12).random(shape) * 255).astype(np.float32)
    x = X.poison(x0, _plane_poisons(shape) + [(1, 2, h - 1, 0)], NAN)
    wt = _dev(X.ints(X.rng_of(3), (48, 3, 3, 3), 4), hip_device)
    job = (wt, torch.empty(K.packed_weight_floats(48, 16), device=hip_device), None, 48, 16, 0)
    x16 = torch.zeros((n, 16, h, w), device=hip_device)
    base = torch.full((n, c, 4 * h, 4 * w), SENTINEL, device=hip_device)
    K.step_prologue([job], _dev(x, hip_device), x16, base)
    X.assert_equal_with_nonfinite(x16[:, :3].contiguous(), x, "x16[:, :3]")
    assert not x16[:, 3:].cpu().numpy().view(np.uint32).any(), "the padded channels of x16"
    _check_upsample(base, x, 4, "bicubic", NAN, "the base image of larva_step_prologue")
    ref, _ = K.pack_weights(wt, cin_pad=16, want_bwd=False)
    assert torch.equal(job[1], ref)


# =====================================================================================================================
# B.8  fp16 inference kernels
# =====================================================================================================================
F16_SHAPE = (1, 5, 70)      # the smallest of test_exact_integer.F16_SHAPES with tile seams inside: 4-row x 64-column tiles


def _f16_pixels():
    n, h, w = F16_SHAPE
    px = [(3, 15), (4, 16), (3, 63), (4, 64), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    sets = []
    for k, (y, x) in enumerate(px):
        for s in sets:
            if all(max(abs(q[2] - y), abs(q[3] - x)) >= 7 for q in s):
                s.append((0, (7, 8, 0, 47)[k % 4], y, x))
                break
        else:
            sets.append([(0, (7, 8, 0, 47)[k % 4], y, x)])
    return sets


def _nhwc(pos):
    return [(n, y, x, c) for (n, c, y, x) in pos]


def _flag(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


@gpu
@pytest.mark.parametrize("value", [NAN, INF], ids=["NaN", "+Inf"])
def test_f16_conv_raises_its_flag_and_keeps_the_footprint(hip_device, value):
    """larva_f16_conv3x3 (plain, ReLU, + res0, + res0 + res1; one and two sources) with one NaN / +Inf activation at the
    seams of the 4 x 64 tiles and the 16-pixel N tiles: the flag is raised, every element outside the 3 x 3 x 48
    footprint is float16(exact sum), inside it the reference's class holds -- except under the ReLU, where the flag is
    the contract and the stored value is not asserted.  The clean launch leaves the flag at 0."""
    from larvanet_amd import kernels as K
    E._threads()
    n, h, w = F16_SHAPE
    h16 = lambda a: _dev(a.astype(np.float16), hip_device)   # noqa: E731
    for nsrc, epis in ((1, E.F16_EPIS), (2, ("plain", "res01"))):
        for epi in epis:
            p = E._f16_problem(F16_SHAPE, nsrc, epi)
            if value == value:
                p["w"] = _weights(X.rng_of(16, nsrc, 5), p["w"].shape, 2, True)
            res = {k: p[k] for k in ("res0", "res1") if k in p}
            wpk = K.f16_pack_weights(_dev(p["w"], hip_device))
            bias = _dev(p["bias"], hip_device)
            kw = {k: h16(v) for k, v in res.items()}
            kw_ref = {k: v.transpose(0, 3, 1, 2) for k, v in res.items()}
            clean, inter = X.conv([x.transpose(0, 3, 1, 2) for x in p["xs"]], p["w"], p["bias"], relu=epi == "relu", **kw_ref)
            X.assert_exact_precondition(inter)
            flag = _flag(hip_device)
            got = K.f16_conv3x3([h16(x) for x in p["xs"]], wpk, bias, flag, relu=epi == "relu", **kw)
            X.assert_bits_equal(got, clean.transpose(0, 2, 3, 1).astype(np.float16), "clean control %s %d sources" % (epi, nsrc))
            assert int(flag.item()) == 0, "the clean launch raised the flag"
            for pos in _f16_pixels():
                src = nsrc - 1                           # (the last source)
                xs = [x.copy() for x in p["xs"]]
                _, inter = X.conv([X.unpoisoned(x, _nhwc(pos) if i == src else []).transpose(0, 3, 1, 2) for i, x in enumerate(xs)],
                                  p["w"], p["bias"], relu=epi == "relu", **kw_ref)
                X.assert_exact_precondition(inter)
                X.assert_exact_precondition([inter[-1]], X.HALF_MAX + 1)
                xs[src] = X.poison(xs[src], _nhwc(pos), value)
                ref, _ = X.conv([x.transpose(0, 3, 1, 2) for x in xs], p["w"], p["bias"], relu=epi == "relu", nonfinite=True, **kw_ref)
                ref16 = np.ascontiguousarray(ref.transpose(0, 2, 3, 1)).astype(np.float16)
                fp = np.broadcast_to(X.conv_footprint((n, h, w), pos)[..., None], ref16.shape)
                if epi != "relu":
                    assert np.array_equal(X.class_map(ref16) != 0, fp)
                flag = _flag(hip_device)
                got = K.f16_conv3x3([h16(x) for x in xs], wpk, bias, flag, relu=epi == "relu", **kw)
                what = "larva_f16_conv3x3 %s %d sources %s at %s" % (epi, nsrc, _name(value), pos)
                assert int(flag.item()) == 1, what + ": the flag stayed 0"
                if epi == "relu":
                    g = got.cpu().numpy()
                    X.assert_bits_equal(np.where(fp, np.float16(0), g), np.where(fp, np.float16(0), ref16), what + " outside the footprint")
                else:
                    X.assert_equal_with_nonfinite(got, ref16, what)


@gpu
@pytest.mark.parametrize("nsrc,epi", [(1, "relu"), (2, "res01")], ids=["1-source-relu", "2-sources-res01"])
def test_f16_conv_reads_nothing_of_its_guards(hip_device, nsrc, epi):
    """larva_f16_conv3x3 with every fp16 operand and the output inside guarded buffers of 0xFF bytes (0xFFFF is an fp16
    NaN) at the only residue the launcher takes: the output is float16(exact sum), the flag stays 0, the guards are intact."""
    from larvanet_amd import kernels as K
    E._threads()
    p = E._f16_problem(F16_SHAPE, nsrc, epi)
    X.assert_exact_precondition(p["inter"])
    checks = []

    def put(a):
        v, chk = placement.placed(np.ascontiguousarray(a), torch.float16, hip_device, 0, fill=0xFF)
        checks.append(chk)
        return v
    wpk = put(K.f16_pack_weights(_dev(p["w"], hip_device)).cpu().numpy())
    kw = {k: put(p[k].astype(np.float16)) for k in ("res0", "res1") if k in p}
    out = put(np.full(p["ref"].shape, SENTINEL, np.float16))
    flag = _flag(hip_device)
    K.f16_conv3x3([put(x.astype(np.float16)) for x in p["xs"]], wpk, _dev(p["bias"], hip_device), flag, relu=epi == "relu", out=out, **kw)
    X.assert_bits_equal(out, p["ref"].astype(np.float16), "larva_f16_conv3x3 %s inside 0xFF guards" % epi)
    assert int(flag.item()) == 0, "a NaN of the guards reached the flag"
    for chk in checks:
        chk()


@gpu
@pytest.mark.parametrize("value", [NAN, INF], ids=["NaN", "+Inf"])
def test_f16_jobs_leg_ends_and_head_with_a_poisoned_source(hip_device, value):
    """larva_f16_conv3x3_jobs (three jobs, the poison in job 1's source: jobs 0 and 2 stay bit-exact), both leg ends
    (fp32 image by class and bits; uint8 image: flag raised, bytes exact outside the footprint) and larva_f16_head."""
    from larvanet_amd import kernels as K
    E._threads()
    n, h, w = F16_SHAPE
    dense = value == value
    rng = X.rng_of(n, h, w, 88, int(dense))
    h16 = lambda a: _dev(a.astype(np.float16), hip_device)   # noqa: E731
    srcs = [X.ints(rng, (n, h, w, 48), 4) for _ in range(3)]
    ws = [_weights(rng, (48, 48, 3, 3), 2, dense) for _ in range(3)]
    bs = [X.ints(rng, (48,), 3) for _ in range(3)]
    base = X.ints(rng, (n, 3, 4 * h, 4 * w), 400, lo=-150)
    wpks = [K.f16_pack_weights(_dev(wt, hip_device)) for wt in ws]
    bd = [_dev(b, hip_device) for b in bs]
    nchw = lambda a: a.transpose(0, 3, 1, 2)   # noqa: E731
    cleans = []
    for s, wt, b in zip(srcs, ws, bs):
        y, inter = X.conv([nchw(s)], wt, b)
        X.assert_exact_precondition(inter + [X.pixel_shuffle(y, 4) + base])
        cleans.append(y)
    for pos in _f16_pixels():
        _, inter = X.conv([nchw(X.unpoisoned(srcs[1], _nhwc(pos)))], ws[1], bs[1])
        X.assert_exact_precondition(inter)
        bad = X.poison(srcs[1], _nhwc(pos), value)
        ref, _ = X.conv([nchw(bad)], ws[1], bs[1], nonfinite=True)
        fp = np.broadcast_to(X.conv_footprint((n, h, w), pos)[:, None], ref.shape)
        assert np.array_equal(X.class_map(ref) != 0, fp)
        sd = [h16(srcs[0]), h16(bad), h16(srcs[2])]
        what = "%s at %s" % (_name(value), pos)
        for relu in (False, True):
            flag = _flag(hip_device)
            out = K.f16_conv3x3_jobs(sd, wpks, bd, flag, relu=relu)
            assert int(flag.item()) == 1, "larva_f16_conv3x3_jobs %s: the flag stayed 0" % what
            for j in (0, 2):
                want = np.maximum(cleans[j], 0) if relu else cleans[j]
                X.assert_bits_equal(out[j], want.transpose(0, 2, 3, 1).astype(np.float16), "larva_f16_conv3x3_jobs %s: clean job %d" % (what, j))
            r16 = np.ascontiguousarray((np.maximum(ref, 0) if relu else ref).transpose(0, 2, 3, 1)).astype(np.float16)
            f16fp = np.ascontiguousarray(fp.transpose(0, 2, 3, 1))
            if relu:
                X.assert_bits_equal(np.where(f16fp, np.float16(0), out[1].cpu().numpy()), np.where(f16fp, np.float16(0), r16),
                                    "larva_f16_conv3x3_jobs relu %s: outside the footprint" % what)
            else:
                X.assert_equal_with_nonfinite(out[1], r16, "larva_f16_conv3x3_jobs %s: the poisoned job" % what)
        with np.errstate(invalid="ignore"):
            img = X.pixel_shuffle(ref, 4) + base
        hrfp = X.class_map(img) != 0
        based = _dev(base, hip_device)
        X.assert_equal_with_nonfinite(K.f16_conv3x3_shuffle_base(sd[1], wpks[1], bd[1], based), img, "larva_f16_conv3x3_shuffle_base " + what)
        outs = K.f16_conv3x3_shuffle_base_jobs(sd, wpks, bd, based)
        X.assert_equal_with_nonfinite(outs[1], img, "larva_f16_conv3x3_shuffle_base_jobs, the poisoned job, " + what)
        for j in (0, 2):
            X.assert_bits_equal(outs[j], X.pixel_shuffle(cleans[j], 4) + base, "larva_f16_conv3x3_shuffle_base_jobs, clean job %d, %s" % (j, what))
        flag = _flag(hip_device)
        u8 = K.f16_conv3x3_shuffle_base_u8(sd[1], wpks[1], bd[1], based, flag).cpu().numpy()
        assert int(flag.item()) == 1, "larva_f16_conv3x3_shuffle_base_u8 %s: the flag stayed 0" % what
        with np.errstate(invalid="ignore"):
            want8 = np.clip(np.where(hrfp, 0, img), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
        keep = ~hrfp.transpose(0, 2, 3, 1)
        X.assert_bits_equal(np.where(keep, u8, 0), np.where(keep, want8, 0), "larva_f16_conv3x3_shuffle_base_u8 %s outside the footprint" % what)
    # the head: fp32 image in, fp16 out
    x = X.ints(rng, (n, 3, h, w), 15, lo=0)
    wt, b = _weights(rng, (48, 3, 3, 3), 2, dense), X.ints(rng, (48,), 3)
    flag = _flag(hip_device)
    y, inter = X.conv([x], wt, b)
    X.assert_exact_precondition(inter)
    X.assert_bits_equal(K.f16_head(_dev(x, hip_device), _dev(wt, hip_device), _dev(b, hip_device), flag),
                        y.transpose(0, 2, 3, 1).astype(np.float16), "larva_f16_head, clean control")
    assert int(flag.item()) == 0
    for pos in _f16_pixels():
        pos = [(i, c % 3, yy, xx) for (i, c, yy, xx) in pos]
        _, inter = X.conv([X.unpoisoned(x, pos)], wt, b)
        X.assert_exact_precondition(inter)
        ref, _ = X.conv([X.poison(x, pos, value)], wt, b, nonfinite=True)
        flag = _flag(hip_device)
        got = K.f16_head(_dev(X.poison(x, pos, value), hip_device), _dev(wt, hip_device), _dev(b, hip_device), flag)
        assert int(flag.item()) == 1, "larva_f16_head: the flag stayed 0"
        X.assert_equal_with_nonfinite(got, np.ascontiguousarray(ref.transpose(0, 2, 3, 1)).astype(np.float16),
                                      "larva_f16_head %s at %s" % (_name(value), pos))


# =====================================================================================================================
# B.9  AdamW over the whole fp32 range
# =====================================================================================================================
ADAMW = dict(lr=4e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
ADAMW_N, ADAMW_STEPS, ADAMW_TAIL = 40003, 5, 12


def _adamw_data():
    rng = X.rng_of(9, ADAMW_N)
    n = ADAMW_N
    p0 = (rng.standard_normal(n) * 0.05).astype(np.float32)
    grads = []
    for _ in range(ADAMW_STEPS):
        g = (10.0 ** rng.uniform(-30, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        g[:8] = np.float32([0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38, 1e-40, 1e-20])
        g[n - ADAMW_TAIL:] = np.float32([INF, -INF, NAN] * (ADAMW_TAIL // 3))
        grads.append(g)
    assert n % 4 != 0 and grads[0][2] == np.float32(2.0 ** -149) and np.signbit(grads[0][1])
    return p0, grads


def _adamw_torch(p0, grads):
    """torch.optim.AdamW on the CPU, the state after every step: (param, exp_avg, exp_avg_sq)."""
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([ref], lr=ADAMW["lr"], betas=(ADAMW["beta1"], ADAMW["beta2"]), eps=ADAMW["eps"], weight_decay=ADAMW["wd"])
    states = []
    for g in grads:
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[ref]
        states.append((ref.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return states


def _adamw_coefs(step, device_scalars):
    """The three per-step scalars as the launches compute them (csrc/larva_pointwise.hip): in double from the host's
    doubles (adamw_step_host), or from the fp32 lr and weight decay the device-scalar launch is given."""
    lr, wd = ADAMW["lr"], ADAMW["wd"]
    if device_scalars:
        lr, wd = float(np.float32(lr)), float(np.float32(wd))
    bc1, bc2 = 1.0 - ADAMW["beta1"] ** step, 1.0 - ADAMW["beta2"] ** step
    return float(np.float32(lr / bc1)), float(np.float32(np.sqrt(bc2))), float(np.float32(1.0 - lr * wd))


def _adamw_param_bound(p_prev, p_new, m, v, step, device_scalars, what):
    """|p_new - ref64| <= 2^-24 (2 |p| + 6 |update|), floor one fp32 subnormal spacing: ref64 is the documented update
    param * decay - step_size * m / (sqrt(v) / bc2_sqrt + eps) in float64 from the fp32 operands.  adamw_update rounds
    seven times: the product param * decay and the final sum (each at most 2^-24 |p| to first order), and on the update
    path sqrt, its division, + eps, the product step_size * m and the last division (five relative errors of 2^-24; the
    sixth allows for their second-order terms and the update's share of the final sum).  -> the largest error / bound."""
    step_size, bc2_sqrt, decay = _adamw_coefs(step, device_scalars)
    p64, m64, v64 = p_prev.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        update = -step_size * m64 / (np.sqrt(v64) / bc2_sqrt + float(np.float32(ADAMW["eps"])))
        ref = p64 * decay + update
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(p_new), ~fin), what + ": the parameters that are NaN are not those of a non-finite update"
        bound = np.maximum(2.0 ** -24 * (2 * np.abs(ref) + 6 * np.abs(update)), 2.0 ** -149)
        err = np.abs(p_new.astype(np.float64) - ref)
    worst = float((err[fin] / bound[fin]).max())
    assert worst <= 1.0, "%s: a parameter is %.3f of its rounding bound away from the float64 update" % (what, worst)
    return worst


def test_adamw_reference_stays_within_the_rounding_bound():
    """torch's own CPU AdamW against the float64 evaluation of the update, the bound the device is held to: the
    reference alone stays within it, subnormal second moments are kept (g = 1e-20 gives v = 9.9492e-44) and +-Inf / NaN
    gradients give NaN parameters."""
    p0, grads = _adamw_data()
    states = _adamw_torch(p0, grads)
    prev = p0
    for t, (p, m, v) in enumerate(states, 1):
        _adamw_param_bound(prev, p, m, v, t, False, "torch step %d" % t)
        prev = p
    p, m, v = states[0]
    assert v[7] == np.float32(9.9492e-44) and 0 < v[7] < np.float32(1.17549435e-38)
    assert np.isnan(p[-ADAMW_TAIL:]).all() and np.isfinite(p[:-ADAMW_TAIL]).all()
    sub = (np.abs(states[-1][2]) > 0) & (np.abs(states[-1][2]) < np.float32(1.17549435e-38))
    assert sub.sum() > 100, "too few subnormal second moments in the draw: %d" % sub.sum()


@gpu
@pytest.mark.parametrize("launch", ["adamw_step_host", "adamw_step"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
def test_adamw_over_the_whole_fp32_range(hip_device, launch, off):
    """Five steps on gradients from 1e-30 to 1e3, +-0, the smallest subnormal, FLT_MIN and a tail of +-Inf / NaN, n % 4 != 0:
    exp_avg and exp_avg_sq equal torch's on the CPU bit for bit (subnormals kept, NaN by class); the parameters stay
    within the rounding bound of the float64 update and are NaN exactly where torch's are."""
    from larvanet_amd import kernels as K
    p0, grads = _adamw_data()
    states = _adamw_torch(p0, grads)
    n = ADAMW_N
    prev = p0
    for t, (tp, tm, tv) in enumerate(states, 1):           # the reference first, on its own
        _adamw_param_bound(prev, tp, tm, tv, t, False, "torch step %d" % t)
        prev = tp
    buf = [torch.zeros(n + 4, device=hip_device) for _ in range(4)]
    p, g, m, v = (b[off:off + n] for b in buf)
    p.copy_(torch.from_numpy(p0))
    prev = p0
    same = []
    for t, gr in enumerate(grads, 1):
        g.copy_(torch.from_numpy(gr))
        if launch == "adamw_step_host":
            K.adamw_step_host(p, g, m, v, t, ADAMW["lr"], ADAMW["beta1"], ADAMW["beta2"], ADAMW["eps"], ADAMW["wd"])
        else:
            K.adamw_step(p, g, m, v, torch.tensor([float(t), ADAMW["lr"]], device=hip_device), ADAMW["beta1"], ADAMW["beta2"],
                         ADAMW["eps"], ADAMW["wd"])
        tp, tm, tv = states[t - 1]
        what = "%s at offset %d, step %d" % (launch, off, t)
        X.assert_equal_with_nonfinite(m, tm, what + ": exp_avg")
        X.assert_equal_with_nonfinite(v, tv, what + ": exp_avg_sq")
        pn = p.cpu().numpy()
        assert np.array_equal(np.isnan(pn), np.isnan(tp)), what + ": NaN parameters differ from torch's"
        _adamw_param_bound(prev, pn, tm, tv, t, launch == "adamw_step", what)
        fin = np.isfinite(tp)
        same.append(float((pn[fin].view(np.uint32) == tp[fin].view(np.uint32)).mean()))
        prev = pn
    assert np.isnan(prev[-ADAMW_TAIL:]).all() and np.isfinite(prev[:-ADAMW_TAIL]).all()
    for b in buf:
        assert not b[:off].any() and not b[off + n:].any(), "an element outside the view was written"
    print("%s offset %d vs torch CPU: fraction of bit-identical parameters after each step (each step from the device's own "
          "previous parameters): %s" % (launch, off, same))
