"""Per-kernel parity of the HIP path (through the C ABI) against the oracle, on a real MI355X.

Tolerances: conv outputs are sums of K = 9*Cin products of O(100)-scale activations with
O(0.01) weights; fp32 MFMA is an exact fma chain, so the only difference from the double-
accumulating C oracle is fp32 summation order: |err| <= ~K * 2^-24 * sum|a*b|.  We assert a
relative-to-scale bound of 2e-5 (measured errors are ~1e-6).  Index layouts (pixel shuffle /
unshuffle) are asserted bit-exact.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel_err(got, ref):
    scale = max(1.0, float(np.abs(ref).max()))
    return float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) / scale


def _report(name, got, ref, tol):
    err = _rel_err(got, ref)
    if not err <= tol:
        bad = np.argwhere(np.abs(got - ref) > tol * max(1.0, float(np.abs(ref).max())))
        raise AssertionError("%s: max rel-to-scale err %.3e > %.1e; %d bad; first bad idx %s got %r ref %r" % (
            name, err, tol, len(bad), bad[:4].tolist(),
            [float(got[tuple(b)]) for b in bad[:4]], [float(ref[tuple(b)]) for b in bad[:4]]))


def _rand(rng, shape, scale):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("N,C,H,W", [(2, 48, 9, 48), (1, 48, 7, 50), (1, 48, 5, 13), (2, 32, 6, 48), (1, 64, 6, 52),
                                     (1, 48, 3, 100)])
@pytest.mark.parametrize("epi", ["plain", "relu", "res1", "res2", "mask"])
def test_conv3x3_epilogues(hip_device, N, C, H, W, epi):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(N * 100003 + C * 1009 + H * 101 + W * 7 + len(epi))
    x = _rand(rng, (N, C, H, W), 20.0)
    w = _rand(rng, (C, C, 3, 3), 0.05)
    b = _rand(rng, (C,), 1.0)
    r0 = _rand(rng, (N, C, H, W), 20.0)
    r1 = _rand(rng, (N, C, H, W), 20.0)
    m = _rand(rng, (N, C, H, W), 1.0)
    ref = R.conv3x3(x, w, b)
    kw = {}
    if epi == "relu":
        ref = np.maximum(ref, 0)
        kw["relu"] = True
    elif epi == "res1":
        ref = ref + r0
        kw["res0"] = _dev(r0, hip_device)
    elif epi == "res2":
        ref = (ref + r0) + r1
        kw["res0"], kw["res1"] = _dev(r0, hip_device), _dev(r1, hip_device)
    elif epi == "mask":
        ref = np.where(m > 0, ref, 0).astype(np.float32)
        kw["mask"] = _dev(m, hip_device)
    wd = _dev(w, hip_device)
    fwd, bwd = K.pack_weights(wd)
    out = K.conv3x3(_dev(x, hip_device), fwd, C, bias=_dev(b, hip_device), **kw)
    torch.cuda.synchronize()
    _report("conv3x3[%s]" % epi, out.cpu().numpy(), ref, 2e-5)


@pytest.mark.parametrize("N,H,W", [(2, 6, 48), (1, 5, 20), (1, 4, 49)])
@pytest.mark.parametrize("with_base", [True, False])
def test_conv3x3_pixel_shuffle_tail(hip_device, N, H, W, with_base):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(N * 1000 + H * 10 + W)
    x = _rand(rng, (N, 48, H, W), 20.0)
    w = _rand(rng, (48, 48, 3, 3), 0.05)
    b = _rand(rng, (48,), 1.0)
    base = _rand(rng, (N, 3, 4 * H, 4 * W), 50.0)
    ref = R.pixel_shuffle(R.conv3x3(x, w, b), 4)
    if with_base:
        ref = ref + base
    fwd, _ = K.pack_weights(_dev(w, hip_device))
    out = K.conv3x3(_dev(x, hip_device), fwd, 48, bias=_dev(b, hip_device), shuffle=True,
                    base=_dev(base, hip_device) if with_base else None)
    torch.cuda.synchronize()
    _report("tail", out.cpu().numpy(), ref, 2e-5)


def test_pixel_shuffle_store_is_bit_exact_index_map(hip_device, golden):
    """Identity-like conv (centre tap = 1 on the diagonal) turns the tail kernel into a pure
    PixelShuffle(4): the integer fixture F3 from the reference must come out bit for bit."""
    from larvanet_amd import kernels as K
    g = golden("f3_pixel_shuffle.npz")
    inp = g["inp"].astype(np.float32)  # integers < 2^24: exact in fp32
    w = np.zeros((48, 48, 3, 3), np.float32)
    for c in range(48):
        w[c, c, 1, 1] = 1.0
    fwd, _ = K.pack_weights(_dev(w, hip_device))
    out = K.conv3x3(_dev(inp, hip_device), fwd, 48, shuffle=True)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().astype(np.int32), g["out"])
    back = K.pixel_unshuffle4(out)
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy().astype(np.int32), g["inp"])


@pytest.mark.parametrize("N,C,H,W", [(2, 48, 9, 48), (1, 48, 5, 13), (1, 32, 6, 48), (1, 64, 6, 52)])
def test_conv3x3_dgrad(hip_device, N, C, H, W):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(N + C + H + W)
    dy = _rand(rng, (N, C, H, W), 1e-3)
    w = _rand(rng, (C, C, 3, 3), 0.05)
    ref = R.conv3x3_dgrad(dy, w)
    _, bwd = K.pack_weights(_dev(w, hip_device))
    out = K.conv3x3(_dev(dy, hip_device), bwd, C)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
    assert err < 2e-5, err


def test_multi_source_concat_conv(hip_device):
    """torch.cat(features, 1) + merge_conv (models/LarvaNetV2.py:328-330) without the concat."""
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(9)
    feats = [_rand(rng, (2, 48, 6, 48), 20.0) for _ in range(3)]
    w = _rand(rng, (48, 144, 3, 3), 0.03)
    b = _rand(rng, (48,), 1.0)
    ref = R.conv3x3(np.concatenate(feats, 1), w, b)
    fwd, _ = K.pack_weights(_dev(w, hip_device), want_bwd=False)
    out = K.conv3x3([_dev(f, hip_device) for f in feats], fwd, 48, bias=_dev(b, hip_device))
    torch.cuda.synchronize()
    _report("merge", out.cpu().numpy(), ref, 2e-5)
    # per-source dgrad slices
    dy = _rand(rng, (2, 48, 6, 48), 1e-3)
    full = R.conv3x3_dgrad(dy, w)
    for i in range(3):
        _, bwd = K.pack_weights(_dev(w, hip_device), cin_off=48 * i, cin=48)
        d = K.conv3x3(_dev(dy, hip_device), bwd, 48)
        torch.cuda.synchronize()
        r = full[:, 48 * i:48 * i + 48]
        assert float(np.abs(d.cpu().numpy() - r).max()) / float(np.abs(r).max()) < 2e-5


@pytest.mark.parametrize("N,Cout,Cin,H,W,splits", [(2, 48, 48, 9, 48, 4), (1, 48, 48, 5, 13, 1), (3, 48, 48, 7, 50, 7),
                                                   (2, 32, 32, 6, 48, 3), (1, 64, 64, 6, 52, 2), (2, 48, 16, 6, 48, 4)])
def test_conv3x3_wgrad(hip_device, N, Cout, Cin, H, W, splits):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(N * 7 + Cout + Cin + H + W)
    dy = _rand(rng, (N, Cout, H, W), 1e-3)
    x = _rand(rng, (N, Cin, H, W), 20.0)
    cin_valid = 3 if Cin == 16 else Cin
    if Cin == 16:
        x[:, 3:] = 0
    dw_ref, db_ref = R.conv3x3_wgrad(dy, x[:, :cin_valid])
    dw = torch.full((Cout, cin_valid, 3, 3), float("nan"), device=hip_device)
    db = torch.full((Cout,), float("nan"), device=hip_device)
    K.conv3x3_wgrad([{"dy": _dev(dy, hip_device), "x": _dev(x, hip_device), "dw": dw, "db": db,
                      "cin_off": 0, "cin_valid": cin_valid}], Cout, Cin, splits)
    torch.cuda.synchronize()
    _report("dw", dw.cpu().numpy(), dw_ref, 3e-5)
    _report("db", db.cpu().numpy(), db_ref, 3e-5)


def test_wgrad_batched_jobs_and_slices(hip_device):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(77)
    jobs, refs = [], []
    dw_wide = torch.zeros((48, 96, 3, 3), device=hip_device)
    for i in range(3):
        dy = _rand(rng, (2, 48, 6, 48), 1e-3)
        x = _rand(rng, (2, 48, 6, 48), 20.0)
        refs.append(R.conv3x3_wgrad(dy, x))
        if i < 2:  # two jobs write channel slices of one wide gradient (merge conv)
            jobs.append({"dy": _dev(dy, hip_device), "x": _dev(x, hip_device), "dw": dw_wide,
                         "db": torch.empty(48, device=hip_device), "cin_off": 48 * i, "cin_valid": 48})
        else:
            jobs.append({"dy": _dev(dy, hip_device), "x": _dev(x, hip_device),
                         "dw": torch.empty((48, 48, 3, 3), device=hip_device), "db": torch.empty(48, device=hip_device)})
    K.conv3x3_wgrad(jobs, 48, 48, 5)
    torch.cuda.synchronize()
    wide = dw_wide.cpu().numpy()
    _report("slice0", wide[:, :48], refs[0][0], 3e-5)
    _report("slice1", wide[:, 48:], refs[1][0], 3e-5)
    _report("job2", jobs[2]["dw"].cpu().numpy(), refs[2][0], 3e-5)
    _report("job2.db", jobs[2]["db"].cpu().numpy(), refs[2][1], 3e-5)


@pytest.mark.parametrize("njobs,kind", [(2, "relu"), (4, "mask"), (3, "res2"), (2, "shuffle")])
def test_batched_conv_launch_equals_separate_launches(hip_device, njobs, kind):
    """Independent convs in one launch (blockIdx.y = job) are the same arithmetic as one launch each."""
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(91)
    N, C, H, W = 2, 48, 9, 52
    jobs = []
    for _ in range(njobs):
        w = _dev(_rand(rng, (C, C, 3, 3), 0.05), hip_device)
        fwd, _ = K.pack_weights(w)
        j = {"srcs": _dev(_rand(rng, (N, C, H, W), 20.0), hip_device), "wpk": fwd,
             "bias": _dev(_rand(rng, (C,), 1.0), hip_device)}
        if kind == "mask":
            j["mask"] = _dev(_rand(rng, (N, C, H, W), 1.0), hip_device)
        if kind == "res2":
            j["res0"] = _dev(_rand(rng, (N, C, H, W), 5.0), hip_device)
            j["res1"] = _dev(_rand(rng, (N, C, H, W), 5.0), hip_device)
        if kind == "shuffle":
            j["base"] = _dev(_rand(rng, (N, C // 16, 4 * H, 4 * W), 100.0), hip_device)
        jobs.append(j)
    outs = K.conv3x3_batch(jobs, C, relu=kind == "relu", shuffle=kind == "shuffle")
    for j, o in zip(jobs, outs):
        ref = K.conv3x3(j["srcs"], j["wpk"], C, bias=j["bias"], relu=kind == "relu", mask=j.get("mask"),
                        res0=j.get("res0"), res1=j.get("res1"), shuffle=kind == "shuffle", base=j.get("base"))
        assert torch.equal(o, ref)
    # unaligned width: the batched entry declines, the wrapper issues the jobs one by one
    odd = [{"srcs": _dev(_rand(rng, (1, C, 5, 7), 20.0), hip_device), "wpk": jobs[0]["wpk"]} for _ in range(2)]
    for j, o in zip(odd, K.conv3x3_batch(odd, C, relu=True)):
        assert torch.equal(o, K.conv3x3(j["srcs"], j["wpk"], C, relu=True))


def test_wgrad_split_phases_match_the_fused_call(hip_device):
    """partial launches with different split counts + ONE reduce launch == per-batch fused calls."""
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(31)
    groups = []
    for njobs, splits in ((3, 4), (1, 16), (2, 1000)):  # 1000 > tiles: clamped by the library
        jobs = [{"dy": _dev(_rand(rng, (2, 48, 9, 52), 1e-3), hip_device),
                 "x": _dev(_rand(rng, (2, 48, 9, 52), 20.0), hip_device)} for _ in range(njobs)]
        groups.append((jobs, splits))
    fused, queued = [], []
    for jobs, splits in groups:
        ref = [dict(j, dw=torch.empty((48, 48, 3, 3), device=hip_device), db=torch.empty(48, device=hip_device))
               for j in jobs]
        K.conv3x3_wgrad(ref, 48, 48, splits)
        fused += ref
        parts, used = K.conv3x3_wgrad_partial(jobs, 48, 48, splits)
        assert 1 <= used <= splits
        queued += [{"partial": p, "splits": used, "dw": torch.empty((48, 48, 3, 3), device=hip_device),
                    "db": torch.empty(48, device=hip_device)} for p in parts]
    K.wgrad_reduce(queued, 48, 48)
    torch.cuda.synchronize()
    for a, b in zip(fused, queued):
        assert torch.equal(a["dw"], b["dw"]) and torch.equal(a["db"], b["db"])


def test_wgrad_is_deterministic(hip_device):
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(5)
    dy = _dev(_rand(rng, (4, 48, 12, 48), 1e-3), hip_device)
    x = _dev(_rand(rng, (4, 48, 12, 48), 20.0), hip_device)
    outs = []
    for _ in range(2):
        dw = torch.empty((48, 48, 3, 3), device=hip_device)
        K.conv3x3_wgrad([{"dy": dy, "x": x, "dw": dw, "db": None}], 48, 48, 16)
        torch.cuda.synchronize()
        outs.append(dw.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])


def test_bicubic4(hip_device, golden):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    g = golden("f4_bicubic.npz")
    out = K.bicubic4(_dev(g["inp"], hip_device))
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), g["out"], rtol=1e-5, atol=3e-4)
    rng = np.random.default_rng(3)
    x = (rng.random((2, 3, 17, 23)) * 255).astype(np.float32)
    out = K.bicubic4(_dev(x, hip_device))
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), R.bicubic_up(x, 4), rtol=1e-5, atol=3e-4)


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_upsample4_modes_match_f_interpolate(hip_device, mode):
    """The two modes with which the reference's F.interpolate(..., align_corners=False) call works
    (models/LarvaNet.py:57,283-285) against F.interpolate itself on the CPU, within fp32 rounding on the 0-255
    scale; borders, a 1-pixel-wide and a 1-pixel-high image included."""
    import torch.nn.functional as F
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(31)
    for shape in ((2, 3, 17, 23), (1, 3, 1, 9), (1, 2, 6, 1), (16, 3, 48, 48)):
        x = torch.from_numpy((rng.random(shape) * 255).astype(np.float32))
        ref = F.interpolate(x, scale_factor=4, mode=mode, align_corners=False)
        out = K.upsample4(x.to(hip_device), mode).cpu()
        np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-5, atol=3e-4, err_msg="%s %s" % (mode, shape))
    with pytest.raises(RuntimeError):
        K.upsample4(x.to(hip_device), "nearest")


@pytest.mark.parametrize("numel_shape", [(2, 3, 16, 20), (1, 3, 7, 9), (16, 3, 192, 192)])
def test_l1_forward_backward(hip_device, numel_shape):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(11)
    a = (rng.random(numel_shape) * 255).astype(np.float32)
    b = (rng.random(numel_shape) * 255).astype(np.float32)
    b.ravel()[::7] = a.ravel()[::7]  # exact ties: sign(0) = 0
    ad, bd = _dev(a, hip_device), _dev(b, hip_device)
    loss = K.l1_fwd(ad, bd)
    g = torch.tensor(0.25, device=hip_device)
    ga = K.l1_bwd(ad, bd, g)
    torch.cuda.synchronize()
    assert abs(float(loss) - R.l1_mean(a, b)) < 2e-6 * R.l1_mean(a, b) + 1e-6
    assert np.array_equal(ga.cpu().numpy(), R.l1_grad(a, b, 0.25))


def test_adamw_flat(hip_device):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(2)
    n = 100003
    p = rng.standard_normal(n).astype(np.float32) * 0.05
    g = rng.standard_normal(n).astype(np.float32) * 1e-3
    pd, md, vd = _dev(p, hip_device), torch.zeros(n, device=hip_device), torch.zeros(n, device=hip_device)
    pr, mr, vr = p.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step in (1, 2, 3):
        sl = torch.tensor([float(step), 4e-4], device=hip_device)
        K.adamw_step(pd, _dev(g * step, hip_device), md, vd, sl, 0.9, 0.999, 1e-8, 0.01)
        pr, mr, vr = R.adamw(pr, g * step, mr, vr, step)
    torch.cuda.synchronize()
    np.testing.assert_allclose(pd.cpu().numpy(), pr, rtol=2e-6, atol=1e-8)
    np.testing.assert_allclose(vd.cpu().numpy(), vr, rtol=2e-6, atol=1e-12)


def test_canonical_layer_properties(hip_device):
    """BASELINE size (16x48x48x48): linearity in the input and agreement with the torch CPU
    operator on a sample -- size-independent checks where the C oracle would take too long."""
    from larvanet_amd import kernels as K
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(0)
    x1 = torch.randn(16, 48, 48, 48, generator=gen) * 20
    x2 = torch.randn(16, 48, 48, 48, generator=gen) * 20
    w = torch.randn(48, 48, 3, 3, generator=gen) * 0.05
    fwd, _ = K.pack_weights(w.to(hip_device))
    y1 = K.conv3x3(x1.to(hip_device), fwd, 48)
    y2 = K.conv3x3(x2.to(hip_device), fwd, 48)
    y12 = K.conv3x3((x1 + x2).to(hip_device), fwd, 48)
    torch.cuda.synchronize()
    lin = float((y12 - (y1 + y2)).abs().max()) / float(y12.abs().max())
    assert lin < 1e-5, lin
    ref = F.conv2d(x1, w, padding=1)
    err = float((y1.cpu() - ref).abs().max()) / float(ref.abs().max())
    assert err < 1e-5, err


def test_invalid_arguments_are_rejected(hip_device):
    from larvanet_amd import kernels as K
    x = torch.zeros(1, 48, 4, 4, device=hip_device)
    w = torch.zeros(48, 48, 3, 3, device=hip_device)
    fwd, _ = K.pack_weights(w)
    with pytest.raises(RuntimeError):
        K.conv3x3(x.cpu(), fwd, 48)  # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        K.conv3x3(x, fwd, 40)  # unsupported channel count
    with pytest.raises(RuntimeError):
        K.conv3x3(x, fwd, 48, relu=True, res0=x)  # fusion that is not compiled
    with pytest.raises(RuntimeError):
        K.conv3x3(x[:, :, :, ::2], fwd, 48)  # non-contiguous


def test_l1_bwd_unshuffle_and_sum_scalars(hip_device):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(21)
    a = (rng.random((2, 3, 24, 32)) * 255).astype(np.float32)
    b = (rng.random((2, 3, 24, 32)) * 255).astype(np.float32)
    b.ravel()[::5] = a.ravel()[::5]
    g = torch.tensor(0.25, device=hip_device)
    got = K.l1_bwd_unshuffle4(_dev(a, hip_device), _dev(b, hip_device), g)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), R.pixel_unshuffle(R.l1_grad(a, b, 0.25), 4))
    terms = [torch.tensor(v, device=hip_device) for v in (1.5, 2.25, 3.0)]
    s = K.sum_scalars(terms, 3.0)
    torch.cuda.synchronize()
    assert float(s) == np.float32(np.float32(np.float32(1.5) + np.float32(2.25)) + np.float32(3.0)) / np.float32(3.0)
    x, y = _dev(a, hip_device), _dev(b, hip_device)
    vals = [float(K.l1_fwd(x, y)) for _ in range(5)]
    assert len(set(vals)) == 1 and abs(vals[0] - R.l1_mean(a, b)) < 1e-5 * R.l1_mean(a, b)
    # the fused loss tail: partial sums finished together with other terms == finishing each L1
    # on its own and adding the scalars (bit for bit), and the gradient scale rides in the kernel
    part, inv = K.l1_partial(x, y)
    assert part.dim() == 1 and inv == 1.0 / a.size
    three = torch.tensor(3.0, device=hip_device)
    fused = K.loss_from_partials([part, three, part], [inv, 1.0, inv], 3.0)
    l1 = K.l1_fwd(x, y)
    assert float(fused) == float(K.sum_scalars([l1, three, l1], 3.0))
    part2, inv2, grad2 = K.l1_partial_grad(x, y, 0.25, 0.5)
    assert torch.equal(part2, part) and inv2 == inv
    assert torch.equal(grad2, K.l1_bwd_unshuffle4(x, y, g, 0.5))  # one sweep == the two kernels
    pb, invb, gb = K.l1_partial_grad_batch([x, y, x], y, 0.25, 0.5)  # three "exits" against truth y
    assert invb == inv and torch.equal(pb[0], part) and torch.equal(gb[0], grad2) and torch.equal(pb[2], part)
    assert float(pb[1].sum()) == 0.0 and float(gb[1].abs().sum()) == 0.0
    half = K.l1_bwd_unshuffle4(x, y, g, 0.5)
    assert torch.equal(half, K.l1_bwd_unshuffle4(x, y, torch.tensor(0.125, device=hip_device)))


def test_gather_patches_matches_numpy_crop_rot_flip(hip_device):
    """Device-resident sampler: every (k, flip) combination against np.rot90 / [::-1]."""
    from larvanet_amd.dataloaders import device_patch_loader as D
    ld = D.create_loader()
    ld.parse_args(["--device_source=synthetic_loader", "--synthetic_images=3", "--synthetic_lr_size=20", "--data_seed=4"])
    ld.prepare([4])
    p = 8
    draws = []
    for img in range(3):
        for k in (1, 2, 3, 4):
            for flip in (0, 1):
                h, w = ld.shapes[img]
                draws.append((img, (img * 3 + k) % (w - p), (k * 2 + flip) % (h - p), k, flip))
    draws = np.array(draws, np.int32)
    x, y = ld.get_device_batch(len(draws), 4, p, draws=draws)
    torch.cuda.synchronize()
    x, y = x.cpu().numpy(), y.cpu().numpy()
    for b, d in enumerate(draws):
        lr, hr, _ = ld.get_image_pair(int(d[0]), 4)
        a_ref, b_ref = D.apply_draw_numpy(d, lr, hr, 4, p)
        assert np.array_equal(x[b], a_ref), d
        assert np.array_equal(y[b], b_ref), d
    # seeded draw streams reproduce, and feed train-shaped batches
    x1, y1 = ld.get_device_batch(4, 4, p)
    assert tuple(x1.shape) == (4, 3, p, p) and tuple(y1.shape) == (4, 3, 4 * p, 4 * p) and x1.dtype == torch.float32
    # in-place production into caller-owned buffers (the captured step's inputs)
    bx, by = torch.empty_like(x1), torch.empty_like(y1)
    ox, oy = ld.get_device_batch(4, 4, p, draws=draws[:4], out=(bx, by))
    assert ox.data_ptr() == bx.data_ptr() and oy.data_ptr() == by.data_ptr()
    rx, ry = ld.get_device_batch(4, 4, p, draws=draws[:4])
    assert torch.equal(bx, rx) and torch.equal(by, ry)


@pytest.mark.parametrize("W,P", [(13, 16), (50, 52), (26, 28), (47, 48)])
def test_conv3x3_row_pitch(hip_device, W, P):
    """Rows padded to a pitch (columns [W, P) zero): same result as the unpadded conv, and the
    pad columns of the output are written as zeros so that layers can be chained."""
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(W * 7 + P)
    N, C, H = 2, 48, 7
    x = _rand(rng, (N, C, H, W), 20.0)
    w = _rand(rng, (C, C, 3, 3), 0.05)
    b = _rand(rng, (C,), 1.0)
    r0 = _rand(rng, (N, C, H, W), 20.0)
    ref1 = np.maximum(R.conv3x3(x, w, b), 0)
    ref2 = R.conv3x3(ref1, w, b) + r0

    def pad(a):
        out = np.zeros(a.shape[:-1] + (P,), np.float32)
        out[..., :W] = a
        return out

    fwd, _ = K.pack_weights(_dev(w, hip_device))
    bd = _dev(b, hip_device)
    h = K.conv3x3(_dev(pad(x), hip_device), fwd, C, bias=bd, relu=True, logical_w=W)
    y = K.conv3x3(h, fwd, C, bias=bd, res0=_dev(pad(r0), hip_device), logical_w=W)
    torch.cuda.synchronize()
    hn, yn = h.cpu().numpy(), y.cpu().numpy()
    assert not hn[..., W:].any() and not yn[..., W:].any()
    _report("pitched conv+relu", hn[..., :W], ref1, 2e-5)
    _report("pitched chained conv+res", yn[..., :W], ref2, 2e-5)
    base = _rand(rng, (N, 3, 4 * H, 4 * W), 50.0)
    t = K.conv3x3(h, fwd, C, bias=bd, shuffle=True, base=_dev(base, hip_device), logical_w=W)
    torch.cuda.synchronize()
    _report("pitched tail", t.cpu().numpy(), R.pixel_shuffle(R.conv3x3(ref1, w, b), 4) + base, 2e-5)


def test_device_psnr_matches_validate_protocol(hip_device, golden):
    from larvanet_amd import kernels as K, metrics
    g = golden("f7_validate_helpers.npz")
    # the .5 / clip cases of the fixture, as a 3x2x4 "image" against an arbitrary uint8 truth
    img = g["img"]
    truth = np.random.RandomState(1).randint(0, 256, size=(3, 5, 6)).astype(np.uint8)
    got = K.psnr_u8(_dev(img, hip_device), torch.from_numpy(truth).to(hip_device))
    o8 = metrics.image_to_uint8(img)
    ref = float(metrics.image_psnr(o8, metrics.fit_truth_image_size(o8, truth)))
    assert abs(got - ref) < 1e-4, (got, ref)
    o = g["o_img"].astype(np.float32) + 0.25
    got2 = K.psnr_u8(_dev(o, hip_device), torch.from_numpy(g["t_big"]).to(hip_device))
    assert abs(got2 - float(g["psnr"])) < 1e-4


@pytest.mark.parametrize("H,W", [(1, 1), (1, 4), (2, 3), (3, 1), (4, 16), (1, 97)])
def test_conv3x3_tiny_and_thin_images(hip_device, H, W):
    """Images smaller than one tile / one pixel group: every tap but the centre may be padding."""
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(H * 100 + W)
    x = _rand(rng, (2, 48, H, W), 20.0)
    w = _rand(rng, (48, 48, 3, 3), 0.05)
    b = _rand(rng, (48,), 1.0)
    fwd, bwd = K.pack_weights(_dev(w, hip_device))
    out = K.conv3x3(_dev(x, hip_device), fwd, 48, bias=_dev(b, hip_device), relu=True)
    t = K.conv3x3(_dev(x, hip_device), fwd, 48, bias=_dev(b, hip_device), shuffle=True)
    d = K.conv3x3(_dev(x, hip_device), bwd, 48)
    torch.cuda.synchronize()
    ref = R.conv3x3(x, w, b)
    _report("tiny relu", out.cpu().numpy(), np.maximum(ref, 0), 2e-5)
    _report("tiny tail", t.cpu().numpy(), R.pixel_shuffle(ref, 4), 2e-5)
    _report("tiny dgrad", d.cpu().numpy(), R.conv3x3_dgrad(x, w), 2e-5)
    dw = torch.empty((48, 48, 3, 3), device=hip_device)
    db = torch.empty(48, device=hip_device)
    K.conv3x3_wgrad([{"dy": _dev(x * 1e-3, hip_device), "x": _dev(x, hip_device), "dw": dw, "db": db}], 48, 48, 3)
    torch.cuda.synchronize()
    dw_ref, db_ref = R.conv3x3_wgrad(x * 1e-3, x)
    _report("tiny dw", dw.cpu().numpy(), dw_ref, 3e-5)
    _report("tiny db", db.cpu().numpy(), db_ref, 3e-5)


def test_conv3x3_full_image_against_torch_cpu(hip_device):
    """A DIV2K-val-sized LR plane set (339 x 510, width not a multiple of 4) through both staging
    paths: plain (scalar fallback) and row-pitched (LDS-DMA)."""
    from larvanet_amd import kernels as K
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(1, 48, 339, 510, generator=gen) * 20
    w = torch.randn(48, 48, 3, 3, generator=gen) * 0.05
    b = torch.randn(48, generator=gen)
    ref = F.relu(F.conv2d(x, w, b, padding=1))
    fwd, _ = K.pack_weights(w.to(hip_device))
    plain = K.conv3x3(x.to(hip_device), fwd, 48, bias=b.to(hip_device), relu=True)
    xp = torch.zeros(1, 48, 339, 512)
    xp[..., :510] = x
    pitched = K.conv3x3(xp.to(hip_device), fwd, 48, bias=b.to(hip_device), relu=True, logical_w=510)
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    assert float((plain.cpu() - ref).abs().max()) / scale < 1e-5
    assert float((pitched.cpu()[..., :510] - ref).abs().max()) / scale < 1e-5
    assert not pitched.cpu()[..., 510:].any()


def test_conv3x3_seeded_shape_fuzz(hip_device):
    """40 seeded random problems through the conv entry point: batch, height, width (aligned and
    not), 1..3 channel-concatenated sources of 8..48 channels, every epilogue, single and batched
    launches -- against the C oracle.  Guards the staging paths (buffer-descriptor LDS-DMA with
    zero fill by range check, loader wave, register staging) at shapes the fixed cases do not hit."""
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(20261003)
    for case in range(40):
        N = int(rng.integers(1, 4))
        H = int(rng.integers(1, 23))
        W = int(rng.choice([4, 8, 16, 20, 44, 48, 52, 96, 100, int(rng.integers(1, 70))]))
        nsrc = int(rng.integers(1, 4))
        cps = int(rng.choice([8, 16, 24, 48]))
        cout = int(rng.choice([32, 48, 64])) if case % 4 == 0 else 48
        epi = ["plain", "relu", "res1", "res2", "mask", "shuffle", "shuffle_base"][case % 7]
        srcs = [_rand(rng, (N, cps, H, W), 10.0) for _ in range(nsrc)]
        w = _rand(rng, (cout, cps * nsrc, 3, 3), 0.05)
        b = _rand(rng, (cout,), 1.0)
        ref = R.conv3x3(np.concatenate(srcs, axis=1), w, b)
        kw = {}
        r0, r1, m = (_rand(rng, ref.shape, 5.0) for _ in range(3))
        if epi == "relu":
            ref, kw["relu"] = np.maximum(ref, 0), True
        elif epi == "res1":
            ref, kw["res0"] = ref + r0, _dev(r0, hip_device)
        elif epi == "res2":
            ref = (ref + r0) + r1
            kw["res0"], kw["res1"] = _dev(r0, hip_device), _dev(r1, hip_device)
        elif epi == "mask":
            ref, kw["mask"] = np.where(m > 0, ref, 0).astype(np.float32), _dev(m, hip_device)
        elif epi.startswith("shuffle"):
            ref, kw["shuffle"] = R.pixel_shuffle(ref, 4), True
            if epi == "shuffle_base":
                base = _rand(rng, ref.shape, 50.0)
                ref, kw["base"] = ref + base, _dev(base, hip_device)
        fwd, _ = K.pack_weights(_dev(w, hip_device))
        dsrcs = [_dev(s, hip_device) for s in srcs]
        out = K.conv3x3(dsrcs, fwd, cout, bias=_dev(b, hip_device), **kw)
        torch.cuda.synchronize()
        tag = "case %d N%d H%d W%d %dx%d->%d %s" % (case, N, H, W, nsrc, cps, cout, epi)
        _report(tag, out.cpu().numpy(), ref, 3e-5)
        if case % 3 == 0:  # the same problem twice in one batched launch
            job = dict(srcs=dsrcs, wpk=fwd, bias=_dev(b, hip_device),
                       **{k: v for k, v in kw.items() if k in ("res0", "res1", "mask", "base")})
            o2 = K.conv3x3_batch([job, dict(job)], cout, relu=kw.get("relu", False), shuffle=kw.get("shuffle", False))
            assert torch.equal(o2[0], out) and torch.equal(o2[1], out), tag


def test_wgrad_seeded_shape_fuzz(hip_device):
    """24 seeded random weight-gradient problems (batch, height, width aligned and not, 1..5 layers
    per launch, split counts from 1 to more than there are tiles; 48x48 / 32x32 / 48x16 channels and, round 4, the
    shapes of the 32- and 64-filter networks: 64x64 and 48x64 run as two passes over 32 input channels, 64x16 and
    48x32 on the pipelined kernel's operand runs) against the C oracle: both the pipelined kernel and the
    register-staged one (unaligned widths)."""
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(77001)
    for case in range(24):
        N = int(rng.integers(1, 4))
        H = int(rng.integers(1, 20))
        W = int(rng.choice([4, 16, 48, 52, 96, int(rng.integers(1, 60))]))
        cout, cin, valid = [(48, 48, 48), (64, 64, 64), (32, 32, 32), (48, 16, 3), (48, 64, 64), (48, 48, 48), (64, 16, 3),
                            (48, 32, 32)][case % 8]
        njobs = int(rng.integers(1, 6))
        splits = int(rng.choice([1, 2, 5, 16, 400]))
        jobs, refs = [], []
        for _ in range(njobs):
            dy = _rand(rng, (N, cout, H, W), 1e-2)
            x = np.zeros((N, cin, H, W), np.float32)
            x[:, :valid] = _rand(rng, (N, valid, H, W), 10.0)
            refs.append(R.conv3x3_wgrad(dy, x[:, :valid]))
            jobs.append({"dy": _dev(dy, hip_device), "x": _dev(x, hip_device),
                         "dw": torch.empty((cout, valid, 3, 3), device=hip_device),
                         "db": torch.empty(cout, device=hip_device), "cin_valid": valid})
        K.conv3x3_wgrad(jobs, cout, cin, splits)
        torch.cuda.synchronize()
        for i, (j, (dw_ref, db_ref)) in enumerate(zip(jobs, refs)):
            tag = "case %d job %d N%d H%d W%d %dx%d splits %d" % (case, i, N, H, W, cout, cin, splits)
            _report(tag + " dw", j["dw"].cpu().numpy(), dw_ref, 5e-5)
            _report(tag + " db", j["db"].cpu().numpy(), db_ref, 5e-5)


@pytest.mark.parametrize("N,H,W,kind,images", [(4, 48, 48, "relu", None), (4, 48, 48, "res2", (1, 3)),
                                                (3, 13, 20, "mask", (0, 2)), (2, 17, 36, "shuffle", None),
                                                (5, 9, 52, "res1", (2, 5)), (2, 48, 48, "k96", None),
                                                (16, 48, 48, "relu", (8, 16)), (2, 8, 16, "plain", None),
                                                # round 3: the mask / residual operands reach the epilogue through LDS
                                                # (streamed by the loader wave during the last two K chunks): every such
                                                # epilogue at the canonical size and both table phases, K = 16 (two chunks:
                                                # both turns of the loader are past-the-end turns) and K = 8 (one chunk: the
                                                # strip launch is refused and the call runs the wide tiles)
                                                (16, 48, 48, "mask", (0, 8)), (16, 48, 48, "res1", (8, 16)),
                                                (16, 48, 48, "res2", None), (16, 48, 48, "k96", (8, 16)),
                                                (3, 13, 20, "cin16_res2", (1, 3)), (3, 13, 20, "cin16_mask", None),
                                                (2, 9, 36, "cin8_res2", None)])
def test_strip_tiles_and_image_ranges_match_the_wide_tiles_bit_for_bit(hip_device, N, H, W, kind, images):
    """larva_conv3x3_fwd_strips (5 x 16 / 4 x 16 tiles, what the two half-batch chains of the training
    step run) against the 3 x 48 tiles: the K loop of every output runs in the same order, so the
    results are identical bit for bit; an image range leaves the other images of `out` untouched."""
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(N * 100 + H + W)
    C = 48
    n_src = 2 if kind == "k96" else 1
    cin = 16 if kind.startswith("cin16") else (8 if kind.startswith("cin8") else C)
    kind = kind.split("_")[-1]
    xs = [_dev(_rand(rng, (N, cin, H, W), 20.0), hip_device) for _ in range(n_src)]
    w = _dev(_rand(rng, (C, cin * n_src, 3, 3), 0.05), hip_device)
    b = _dev(_rand(rng, (C,), 1.0), hip_device)
    fwd, _ = K.pack_weights(w, want_bwd=False)
    kw = {"bias": b}
    if kind == "relu":
        kw["relu"] = True
    elif kind == "mask":
        kw["mask"] = _dev(_rand(rng, (N, C, H, W), 1.0), hip_device)
    elif kind in ("res1", "res2", "k96"):
        kw["res0"] = _dev(_rand(rng, (N, C, H, W), 5.0), hip_device)
        if kind != "res1":
            kw["res1"] = _dev(_rand(rng, (N, C, H, W), 5.0), hip_device)
    elif kind == "shuffle":
        kw["shuffle"] = True
        kw["base"] = _dev(_rand(rng, (N, 3, 4 * H, 4 * W), 50.0), hip_device)
    assert K.strip_tile_table(H, W, hip_device) is not None
    ref = K.conv3x3(xs, fwd, C, **kw)
    shape = ref.shape
    out = torch.full(shape, -7.0, device=hip_device)
    K.conv3x3(xs, fwd, C, out=out, images=images, strips=True, **kw)
    torch.cuda.synchronize()
    lo, hi = images or (0, N)
    assert torch.equal(out[lo:hi], ref[lo:hi])
    if kind != "shuffle":   # the other table phase (the second chain's launches) and plain stores
        outp = torch.full(shape, -7.0, device=hip_device)
        K.conv3x3(xs, fwd, C, out=outp, images=images, strips=2, plain_stores=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(outp, out)
    if lo > 0:
        assert bool((out[:lo] == -7.0).all())
    if hi < N:
        assert bool((out[hi:] == -7.0).all())
    # the same image range on the regular tiles
    out2 = torch.full(shape, -7.0, device=hip_device)
    K.conv3x3(xs, fwd, C, out=out2, images=images, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out2, out)


@pytest.mark.parametrize("njobs,N,H,W", [(4, 2, 9, 48), (2, 3, 7, 20), (3, 16, 48, 48)])
def test_exits_scored_inside_the_conv_launch(hip_device, njobs, N, H, W):
    """larva_conv3x3_exit_l1_batch (conv -> PixelShuffle(4) -> + base -> L1 against the truth, all in
    the conv's epilogue) against the separate launches it replaces: images and the pixel-unshuffled
    sign gradient bit for bit (sign(0) = 0 included), the |out - truth| sum to fp32 rounding (another
    grouping of the same addends) and against a float64 sum."""
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(njobs * 1000 + H)
    jobs = []
    for _ in range(njobs):
        w = _dev(_rand(rng, (48, 48, 3, 3), 0.05), hip_device)
        jobs.append({"srcs": _dev(_rand(rng, (N, 48, H, W), 20.0), hip_device), "wpk": K.pack_weights(w, want_bwd=False)[0],
                     "bias": _dev(_rand(rng, (48,), 1.0), hip_device), "base": _dev(_rand(rng, (N, 3, 4 * H, 4 * W), 50.0), hip_device)})
    imgs = K.conv3x3_batch(jobs, 48, shuffle=True)
    truth = _dev(_rand(rng, (N, 3, 4 * H, 4 * W), 60.0), hip_device)
    truth[:, :, ::5, ::3] = imgs[0][:, :, ::5, ::3]          # exact ties for exit 0: gradient 0 there
    gvalue, gscale = 1.0, float(np.float32(1.0) / np.float32(njobs))
    ref_parts, _, ref_grads = K.l1_partial_grad_batch(imgs, truth, gvalue, gscale)
    want = [j == njobs - 1 for j in range(njobs)]
    res = K.conv3x3_exit_l1_batch(jobs, 48, truth, gvalue, gscale, want)
    assert res is not None
    outs, parts, grads = res
    torch.cuda.synchronize()
    assert outs[0] is None and torch.equal(outs[-1], imgs[-1])
    t64 = truth.double()
    for j in range(njobs):
        assert torch.equal(grads[j], ref_grads[j]), j
        exact = float((imgs[j].double() - t64).abs().sum())
        got, old = float(parts[j].double().sum()), float(ref_parts[j].double().sum())
        assert abs(got - exact) <= 2e-6 * exact and abs(got - old) <= 2e-6 * exact, (j, got, old, exact)
    assert int((grads[0] == 0).sum()) >= int(truth[:, :, ::5, ::3].numel())
    # run to run: the same bits
    res2 = K.conv3x3_exit_l1_batch(jobs, 48, truth, gvalue, gscale, want)
    torch.cuda.synchronize()
    for j in range(njobs):
        assert torch.equal(res2[1][j], parts[j])


@pytest.mark.parametrize("N,H,W,pitch,cout", [(16, 48, 48, None, 48), (1, 9, 13, 16, 48), (2, 5, 7, None, 48), (1, 339, 510, 512, 48),
                                              (1, 7, 18, 20, 48), (2, 33, 50, 64, 32), (1, 20, 95, 96, 64), (3, 1, 16, None, 48),
                                              (1, 2, 40, 48, 48)])
def test_direct_head_conv_against_oracle_and_mfma_path(hip_device, N, H, W, pitch, cout):
    """larva_head_conv3_direct (LarvaHead, K = 27) against the C oracle and against the same layer on
    the MFMA conv kernel (image zero-padded to 16 channels); padding columns of a pitched output are zero.  The entry point
    picks the 4-pixel direct kernel (pitch % 4 == 0) or the scalar one: both are covered, at 32 / 48 / 64 channels, at image
    borders, with padding columns (up to 8 of them), one-row and two-row images."""
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(H * 31 + W + cout)
    x = _rand(rng, (N, 3, H, W), 70.0)
    w = _rand(rng, (cout, 3, 3, 3), 0.1)
    b = _rand(rng, (cout,), 1.0)
    out = K.head_conv3_direct(_dev(x, hip_device), _dev(w, hip_device), _dev(b, hip_device), pitch=pitch)
    torch.cuda.synchronize()
    P = pitch or W
    assert tuple(out.shape) == (N, cout, H, P)
    got = out.cpu().numpy()
    if P > W:
        assert not got[..., W:].any()
    if N * H * W <= 16 * 48 * 48:
        _report("head", got[..., :W], R.conv3x3(x, w, b), 2e-5)
    if P % 4 == 0:
        x16 = torch.zeros((N, 16, H, P), device=hip_device)
        x16[:, :3, :, :W] = _dev(x, hip_device)
        fwd, _ = K.pack_weights(_dev(w, hip_device), cin_pad=16, want_bwd=False)
        ref = K.conv3x3(x16, fwd, cout, bias=_dev(b, hip_device), logical_w=W if P > W else None)
        torch.cuda.synchronize()
        scale = float(ref.abs().max())
        assert float((out - ref).abs().max()) <= 1e-5 * scale


def test_head_conv_kernels_agree_bit_for_bit(hip_device):
    """The two kernels behind larva_head_conv3_direct compute every output as the same fmaf chain in tap order from the
    bias: the 4-pixel kernel (pitch % 4 == 0) and the one-pixel kernel (any pitch) produce identical bits."""
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(11)
    N, H, W = 2, 37, 90
    x = _dev(_rand(rng, (N, 3, H, W), 70.0), hip_device)
    w = _dev(_rand(rng, (48, 3, 3, 3), 0.1), hip_device)
    b = _dev(_rand(rng, (48,), 1.0), hip_device)
    direct4 = K.head_conv3_direct(x, w, b, pitch=92)  # 4 pixels x 8 channels per thread
    scalar = K.head_conv3_direct(x, w, b, pitch=91)   # one pixel per thread
    torch.cuda.synchronize()
    assert torch.equal(direct4[..., :W], scalar[..., :W])


def test_step_prologue_equals_its_three_launches(hip_device):
    """larva_step_prologue (weight images of all layers + the head's padded input + the bicubic base in
    one launch) against pack_weights_batch, the padded copy and bicubic4: identical bits."""
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(3)
    ws = [_dev(_rand(rng, (48, 48, 3, 3), 0.05), hip_device) for _ in range(5)] + [_dev(_rand(rng, (48, 3, 3, 3), 0.1), hip_device)]
    def bufs():
        out = []
        for w in ws:
            cin_k = 16 if w.shape[1] == 3 else 48
            f = torch.full((K.packed_weight_floats(48, cin_k),), -1.0, device=hip_device)
            b = None if w.shape[1] == 3 else torch.full((K.packed_weight_floats(cin_k, 48),), -1.0, device=hip_device)
            out.append((w, f, b, 48, cin_k, 0))
        return out
    ref_jobs, got_jobs = bufs(), bufs()
    x = _dev(_rand(rng, (5, 3, 13, 20), 80.0), hip_device)
    K.pack_weights_batch(ref_jobs)
    ref_base = K.bicubic4(x)
    x16 = torch.zeros((5, 16, 13, 20), device=hip_device)
    base = torch.empty_like(ref_base)
    K.step_prologue(got_jobs, x, x16, base)
    torch.cuda.synchronize()
    for (_, f0, b0, *_), (_, f1, b1, *_) in zip(ref_jobs, got_jobs):
        assert torch.equal(f0, f1) and (b0 is None or torch.equal(b0, b1))
    assert torch.equal(base, ref_base)
    assert torch.equal(x16[:, :3], x) and not bool(x16[:, 3:].any())


@pytest.mark.parametrize("njobs,nwg,N,H,W,C", [(5, 7, 2, 9, 48, 48), (3, 64, 1, 6, 48, 48), (6, 4, 2, 7, 52, 48), (1, 3, 2, 9, 48, 48),
                                                (40, 256, 4, 12, 48, 48),
                                                # round 3: the pipelined kernel at (32,32) -- 8-10 MFMAs per k-step, the
                                                # k-step's fillers dealt two to a gap -- per layer and as the flat grid
                                                (5, 7, 2, 9, 48, 32), (6, 4, 2, 7, 52, 32), (40, 256, 4, 12, 48, 32),
                                                (8, 256, 16, 48, 48, 32),
                                                # round 4: (64, 64) as two (64, 32) passes per workgroup and layer into one
                                                # partial image
                                                (5, 7, 2, 9, 48, 64), (6, 4, 2, 7, 52, 64), (8, 256, 16, 48, 48, 64)])
def test_flat_wgrad_grid_over_all_layers(hip_device, njobs, nwg, N, H, W, C):
    """larva_conv3x3_wgrad_partial_flat: one grid over the tiles of all layers (a workgroup's share may
    cross layer boundaries, more workgroups than tiles, several layers per workgroup) + the fixed-order
    reduction, against the C oracle / torch per layer; and run to run the same bits."""
    from larvanet_amd import kernels as K
    gen = torch.Generator().manual_seed(njobs * 100 + nwg)
    jobs = []
    for _ in range(njobs):
        dy = (torch.randn(N, C, H, W, generator=gen) * 1e-3).to(hip_device)
        x = (torch.randn(N, C, H, W, generator=gen) * 20).to(hip_device)
        jobs.append({"dy": dy, "x": x, "dw": torch.full((C, C, 3, 3), float("nan"), device=hip_device),
                     "db": torch.full((C,), float("nan"), device=hip_device)})
    res = K.conv3x3_wgrad_partial_flat(jobs, C, C, nwg)
    assert res is not None
    parts, splits = res
    tiles = N * ((H + 2) // 3) * ((W + 47) // 48)
    assert all(1 <= s <= min(nwg, tiles) + 1 for s in splits)
    K.wgrad_reduce([dict(j, partial=p, splits=s, cout=C, cin=C) for j, p, s in zip(jobs, parts, splits)])
    torch.cuda.synchronize()
    for j in jobs:
        dw_ref = torch.nn.grad.conv2d_weight(j["x"].double().cpu(), (C, C, 3, 3), j["dy"].double().cpu(), padding=1)
        db_ref = j["dy"].double().cpu().sum((0, 2, 3))
        dw, db = j["dw"].cpu().double(), j["db"].cpu().double()
        assert float((dw - dw_ref).abs().max()) <= 3e-5 * float(dw_ref.abs().max())
        assert float((db - db_ref).abs().max()) <= 3e-5 * float(db_ref.abs().max()) + 1e-9
    first = [j["dw"].clone() for j in jobs]
    res2 = K.conv3x3_wgrad_partial_flat(jobs, C, C, nwg)
    K.wgrad_reduce([dict(j, partial=p, splits=s, cout=C, cin=C) for j, p, s in zip(jobs, *res2)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, j["dw"]) for a, j in zip(first, jobs))


@pytest.mark.parametrize("njobs,nwg,N,H,W", [(5, 7, 2, 9, 48), (1, 3, 2, 9, 48), (3, 64, 1, 6, 48), (8, 256, 16, 48, 48),
                                              (2, 5, 3, 10, 52)])
def test_flat_wgrad_grid_with_the_head_as_its_tail(hip_device, njobs, nwg, N, H, W):
    """larva_conv3x3_wgrad_partial_flat_head: the 3 -> 48 head's weight gradient (a (48, 16) layer on the
    zero-padded input) taken by the last workgroups of the flat grid -- every layer and the head against torch in
    float64 (the head makes the sequence longer, so the 48 -> 48 layers' shares differ from the head-less grid's
    and only the tolerance is asserted); run to run the same bits."""
    from larvanet_amd import kernels as K
    gen = torch.Generator().manual_seed(njobs * 1000 + nwg)
    jobs = []
    for _ in range(njobs):
        jobs.append({"dy": (torch.randn(N, 48, H, W, generator=gen) * 1e-3).to(hip_device),
                     "x": (torch.randn(N, 48, H, W, generator=gen) * 20).to(hip_device),
                     "dw": torch.full((48, 48, 3, 3), float("nan"), device=hip_device),
                     "db": torch.full((48,), float("nan"), device=hip_device)})
    x3 = (torch.rand(N, 3, H, W, generator=gen) * 255).to(hip_device)
    x16 = torch.zeros(N, 16, H, W, device=hip_device)
    x16[:, :3] = x3
    head = {"dy": (torch.randn(N, 48, H, W, generator=gen) * 1e-3).to(hip_device), "x": x16,
            "dw": torch.full((48, 3, 3, 3), float("nan"), device=hip_device),
            "db": torch.full((48,), float("nan"), device=hip_device), "cin_off": 0, "cin_valid": 3}

    def run():
        res = K.conv3x3_wgrad_partial_flat(jobs, 48, 48, nwg, head=head)
        assert res is not None
        parts, splits = res
        rj = [dict(j, partial=p, splits=s, cout=48, cin=48) for j, p, s in zip(jobs, parts, splits)]
        rj.append(dict(head, partial=parts[-1], splits=splits[-1], cout=48, cin=16))
        K.wgrad_reduce(rj)
        torch.cuda.synchronize()
        return splits

    splits = run()
    assert len(splits) == njobs + 1 and splits[-1] >= 1
    for j, cin_x in [(j, j["x"]) for j in jobs] + [(head, x3)]:
        dw_ref = torch.nn.grad.conv2d_weight(cin_x.double().cpu(), tuple(j["dw"].shape), j["dy"].double().cpu(), padding=1)
        db_ref = j["dy"].double().cpu().sum((0, 2, 3))
        dw, db = j["dw"].cpu().double(), j["db"].cpu().double()
        assert float((dw - dw_ref).abs().max()) <= 3e-5 * float(dw_ref.abs().max())
        assert float((db - db_ref).abs().max()) <= 3e-5 * float(db_ref.abs().max()) + 1e-9
    first = [j["dw"].clone() for j in jobs + [head]]
    for j in jobs + [head]:
        j["dw"].fill_(float("nan"))
    run()
    assert all(torch.equal(a, j["dw"]) for a, j in zip(first, jobs + [head]))


@pytest.mark.parametrize("njobs,nwg,N,H,W,with_head", [(32, 256, 64, 48, 48, False), (32, 200, 64, 48, 48, False),
                                                        (8, 256, 16, 96, 96, True)])
def test_flat_wgrad_grid_with_large_shares(hip_device, njobs, nwg, N, H, W, with_head):
    """The flat weight-gradient grid at training batches past the headline: a workgroup's share holds 128-164 tiles
    (32 layers of 64 x 48 x 48 over 256 / 200 workgroups: shares on and across the layer boundaries) or 32+ tiles with
    the head as the grid's tail (8 layers of 16 x 96 x 96).  Against torch in float64 for the first and the last layer,
    two layers whose first share starts inside the layer before (where there are such) and the head; run to run the
    same bits for every layer."""
    from larvanet_amd import kernels as K
    gen = torch.Generator(device=hip_device).manual_seed(njobs * 1000 + nwg)
    jobs = []
    for _ in range(njobs):
        jobs.append({"dy": torch.randn(N, 48, H, W, generator=gen, device=hip_device) * 1e-3,
                     "x": torch.randn(N, 48, H, W, generator=gen, device=hip_device) * 20,
                     "dw": torch.full((48, 48, 3, 3), float("nan"), device=hip_device),
                     "db": torch.full((48,), float("nan"), device=hip_device)})
    head = None
    if with_head:
        x16 = torch.zeros(N, 16, H, W, device=hip_device)
        x16[:, :3] = torch.rand(N, 3, H, W, generator=gen, device=hip_device) * 255
        head = {"dy": torch.randn(N, 48, H, W, generator=gen, device=hip_device) * 1e-3, "x": x16,
                "dw": torch.full((48, 3, 3, 3), float("nan"), device=hip_device),
                "db": torch.full((48,), float("nan"), device=hip_device), "cin_off": 0, "cin_valid": 3}

    def run():
        parts, splits = K.conv3x3_wgrad_partial_flat(jobs, 48, 48, nwg, head=head)
        rj = [dict(j, partial=p, splits=s, cout=48, cin=48) for j, p, s in zip(jobs, parts, splits)]
        if head is not None:
            rj.append(dict(head, partial=parts[-1], splits=splits[-1], cout=48, cin=16))
        K.wgrad_reduce(rj)
        torch.cuda.synchronize()
        return splits

    splits = run()
    tiles = N * ((H + 2) // 3) * ((W + 47) // 48)
    assert len(splits) == njobs + (head is not None)
    # layers whose first tile is not the first of a share (the share of workgroup w is [G w / nwg, G (w + 1) / nwg));
    # without the head G is the tile count, with it the head's units lengthen the sequence: check every layer then
    starts = {njobs * tiles * w // nwg for w in range(nwg)}
    crossing = [i for i in range(1, njobs) if i * tiles not in starts]
    check = sorted({0, njobs - 1, *crossing[len(crossing) // 2:len(crossing) // 2 + 2]}) if head is None else range(njobs)
    if head is None and nwg == 200:
        assert len(crossing) >= 2 and all(s >= 2 for s in splits)
    for j, cin_x in [(jobs[i], jobs[i]["x"]) for i in check] + ([(head, head["x"][:, :3])] if head is not None else []):
        dw_ref = torch.nn.grad.conv2d_weight(cin_x.double().cpu(), tuple(j["dw"].shape), j["dy"].double().cpu(), padding=1)
        db_ref = j["dy"].double().cpu().sum((0, 2, 3))
        dw, db = j["dw"].cpu().double(), j["db"].cpu().double()
        assert float((dw - dw_ref).abs().max()) <= 3e-5 * float(dw_ref.abs().max())
        assert float((db - db_ref).abs().max()) <= 3e-5 * float(db_ref.abs().max()) + 1e-9
    every = jobs + ([head] if head is not None else [])
    first = [j["dw"].clone() for j in every] + [j["db"].clone() for j in every]
    for j in every:
        j["dw"].fill_(float("nan"))
        j["db"].fill_(float("nan"))
    assert run() == splits
    assert all(torch.equal(a, b) for a, b in zip(first, [j["dw"] for j in every] + [j["db"] for j in every]))


def test_reduce_launch_carries_the_loss_and_adamw_launch_the_copy(hip_device):
    """larva_wgrad_reduce_with_loss == larva_wgrad_reduce + larva_loss_from_partials (same bits), and
    larva_adamw_step_host_copy == larva_adamw_step_host + a 4-byte copy."""
    from larvanet_amd import kernels as K
    gen = torch.Generator().manual_seed(77)
    jobs = []
    for _ in range(3):
        jobs.append({"dy": (torch.randn(2, 48, 9, 48, generator=gen) * 1e-3).to(hip_device),
                     "x": (torch.randn(2, 48, 9, 48, generator=gen) * 20).to(hip_device),
                     "dw": torch.empty((48, 48, 3, 3), device=hip_device), "db": torch.empty(48, device=hip_device)})
    parts, used = K.conv3x3_wgrad_partial(jobs, 48, 48, 4)
    rjobs = [dict(j, partial=p, splits=used, cout=48, cin=48) for j, p in zip(jobs, parts)]
    terms = [(torch.rand(1024, generator=gen) * 1e4).to(hip_device), (torch.rand(37, generator=gen) * 1e4).to(hip_device),
             torch.tensor(3.5, device=hip_device)]
    scales = [1.0 / 7.0e6, 1.0 / 7.0e6, 1.0]
    K.wgrad_reduce(rjobs)
    ref_dw = [j["dw"].clone() for j in jobs]
    ref_loss = K.loss_from_partials(terms, scales, 3.0)
    for j in jobs:
        j["dw"].fill_(float("nan"))
    out = torch.full((), float("nan"), device=hip_device)
    K.wgrad_reduce(rjobs, loss=(terms, scales, 3.0, out))
    torch.cuda.synchronize()
    assert all(torch.equal(a, j["dw"]) for a, j in zip(ref_dw, jobs)) and torch.equal(out, ref_loss)
    n = 1000
    p0, g = torch.randn(n, generator=gen).to(hip_device), torch.randn(n, generator=gen).to(hip_device)
    res = []
    for copy in (None, (ref_loss, torch.zeros((), device=hip_device))):
        p, m, v = p0.clone(), torch.zeros(n, device=hip_device), torch.zeros(n, device=hip_device)
        K.adamw_step_host(p, g, m, v, 1, 4e-4, 0.9, 0.999, 1e-8, 0.01, 1.0, copy=copy)
        res.append(p)
    torch.cuda.synchronize()
    assert torch.equal(res[0], res[1]) and torch.equal(copy[1], ref_loss)


def test_adamw_host_scalars_match_torch_and_unaligned_views(hip_device):
    """larva_adamw_step_host: 16-byte-per-lane walk + a tail (n % 4 != 0), against torch.optim.AdamW on the CPU over 5
    steps; buffers that start 4 bytes off a 16-byte boundary take the element-wise walk and give the same bits."""
    from larvanet_amd import kernels as K
    gen = torch.Generator().manual_seed(5)
    n = 40007
    p0 = torch.randn(n, generator=gen) * 0.05
    grads = [torch.randn(n, generator=gen) * 1e-3 for _ in range(5)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    outs = []
    for off in (0, 1):
        buf = [torch.zeros(n + 4, device=hip_device) for _ in range(4)]
        p, g, m, v = (b[off:off + n] for b in buf)
        p.copy_(p0)
        for t, gr in enumerate(grads, 1):
            g.copy_(gr)
            K.adamw_step_host(p, g, m, v, t, 4e-4, 0.9, 0.999, 1e-8, 0.01)
        outs.append((p.clone(), m.clone(), v.clone()))
    for gr in grads:
        ref.grad = gr.clone()
        opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    np.testing.assert_allclose(outs[0][0].cpu().numpy(), ref.detach().numpy(), rtol=2e-6, atol=2e-8)
    # The kernel follows torch.optim.AdamW's single-tensor step operation by operation (lerp as an fma, the second
    # moment as mul + fused addcmul, sqrt / bias_correction2_sqrt then + eps, addcdiv) with torch's double-precision
    # scalars (1 - beta2 = 0.001f, not 1.f - 0.999f): against ATen's CPU kernels (AVX2 build) both moments come out bit
    # for bit after five steps and the parameters on ~98 % of the elements (the rest 1 ulp, 4e-9: the correctly rounded
    # device sqrt / division against ATen's vectorised ones).
    st = opt.state[ref]
    same = [float((a.cpu() == b).float().mean()) for a, b in ((outs[0][0], ref.detach()), (outs[0][1], st["exp_avg"]),
                                                               (outs[0][2], st["exp_avg_sq"]))]
    print("AdamW vs torch CPU after 5 steps, fraction of bit-identical elements (param, exp_avg, exp_avg_sq):", same)
    assert same[1] == 1.0 and same[2] == 1.0 and same[0] > 0.97, same
    assert float((outs[0][0].cpu() - ref.detach()).abs().max()) < 3e-8   # (<= 2 ulp of a 0.1-sized weight)


def test_strip_tiles_seeded_shape_fuzz(hip_device):
    """24 seeded random problems (batch, height, width % 4 == 0, 1-2 sources, every mode-0 epilogue and the
    pixel-shuffle ones, image sub-ranges, both table phases and store policies): strip tiles == 3 x 48 tiles
    bit for bit wherever a height can be cut into 5s and 4s."""
    from larvanet_amd import kernels as K
    rng = np.random.default_rng(2025)
    done = 0
    while done < 24:
        N, H, W = int(rng.integers(1, 5)), int(rng.integers(4, 40)), 4 * int(rng.integers(1, 17))
        if K.strip_tile_table(H, W, hip_device) is None:
            continue
        done += 1
        n_src = int(rng.integers(1, 3))
        kind = ["plain", "relu", "mask", "res1", "res2", "shuffle", "shuffle_base"][int(rng.integers(0, 7))]
        xs = [_dev(_rand(rng, (N, 48, H, W), 20.0), hip_device) for _ in range(n_src)]
        fwd, _ = K.pack_weights(_dev(_rand(rng, (48, 48 * n_src, 3, 3), 0.05), hip_device), want_bwd=False)
        kw = {"bias": _dev(_rand(rng, (48,), 1.0), hip_device)}
        if kind == "relu":
            kw["relu"] = True
        if kind == "mask":
            kw["mask"] = _dev(_rand(rng, (N, 48, H, W), 1.0), hip_device)
        if kind in ("res1", "res2"):
            kw["res0"] = _dev(_rand(rng, (N, 48, H, W), 5.0), hip_device)
        if kind == "res2":
            kw["res1"] = _dev(_rand(rng, (N, 48, H, W), 5.0), hip_device)
        if kind.startswith("shuffle"):
            kw["shuffle"] = True
        if kind == "shuffle_base":
            kw["base"] = _dev(_rand(rng, (N, 3, 4 * H, 4 * W), 50.0), hip_device)
        lo = int(rng.integers(0, N))
        hi = int(rng.integers(lo + 1, N + 1))
        ref = K.conv3x3(xs, fwd, 48, **kw)
        out = torch.full(ref.shape, 3.0, device=hip_device)
        K.conv3x3(xs, fwd, 48, out=out, images=(lo, hi), strips=1 + done % 2, plain_stores=bool(done % 3), **kw)
        torch.cuda.synchronize()
        assert torch.equal(out[lo:hi], ref[lo:hi]), (N, H, W, n_src, kind, lo, hi)
        assert bool((out[:lo] == 3.0).all()) and bool((out[hi:] == 3.0).all()), (N, H, W, kind, lo, hi)


@pytest.mark.parametrize("kind", ["relu", "res2", "mask", "plain"])
@pytest.mark.parametrize("C", [32, 64])
def test_strip_tiles_at_32_and_64_channels(hip_device, kind, C):
    """Strip tiles at 32 output channels (waves 3/3/2/2 and 2/2/2/2) and at 64 (5/5/5/5 and 4/4/4/4; round 3: the weight
    rows of these widths are staged unpadded with odd rows swizzled, which is what lets two 64-channel strip workgroups
    share a CU) == the 3 x 48 tiles bit for bit, and the C oracle (BASELINE's "32ch" / "64ch" configurations have no
    reference counterpart: SURVEY 8a N1)."""
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    rng = np.random.default_rng(C)
    N, H, W = 3, 13, 20
    x = _rand(rng, (N, C, H, W), 20.0)
    w = _rand(rng, (C, C, 3, 3), 0.05)
    b = _rand(rng, (C,), 1.0)
    fwd, _ = K.pack_weights(_dev(w, hip_device), want_bwd=False)
    kw = {"bias": _dev(b, hip_device)}
    aux = [_rand(rng, (N, C, H, W), 5.0) for _ in range(2)]
    ref = R.conv3x3(x, w, b)
    if kind == "relu":
        kw["relu"] = True
        ref = np.maximum(ref, 0)
    elif kind == "mask":
        kw["mask"] = _dev(aux[0], hip_device)
        ref = np.where(aux[0] > 0, ref, 0).astype(np.float32)
    elif kind == "res2":
        kw["res0"], kw["res1"] = _dev(aux[0], hip_device), _dev(aux[1], hip_device)
        ref = (ref + aux[0]) + aux[1]
    wide = K.conv3x3(_dev(x, hip_device), fwd, C, **kw)
    out = torch.full(wide.shape, -1.0, device=hip_device)
    K.conv3x3(_dev(x, hip_device), fwd, C, out=out, images=(1, 3), strips=2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out[1:], wide[1:]) and bool((out[0] == -1.0).all())
    _report("c%d strips[%s]" % (C, kind), wide.cpu().numpy(), ref, 2e-5)


@pytest.fixture(scope="module")
def canonical_wide_case():
    """16 x C x 48 x 48 operands for C in (32, 64) with their CPU references (torch's own operators: conv2d,
    conv2d_input, conv2d_weight -- float64 for the weight gradient, whose K is 36 864), computed once."""
    import torch.nn.functional as F
    torch.set_num_threads(8)
    cases = {}
    for C in (32, 64):
        gen = torch.Generator().manual_seed(3200 + C)
        x = torch.randn(16, C, 48, 48, generator=gen) * 20           # N(0,1) * 20 activations
        w = torch.randn(C, C, 3, 3, generator=gen) * 0.05
        b = torch.randn(C, generator=gen)
        dy = torch.randn(16, C, 48, 48, generator=gen) * 1e-3
        r0 = torch.randn(16, C, 48, 48, generator=gen) * 20
        r1 = torch.randn(16, C, 48, 48, generator=gen) * 20
        y = F.conv2d(x, w, b, padding=1)
        dx = torch.nn.grad.conv2d_input(x.shape, w, dy, padding=1)
        dw = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), padding=1).float()
        db = dy.double().sum((0, 2, 3)).float()
        cases[C] = dict(x=x, w=w, b=b, dy=dy, r0=r0, r1=r1, y=y, dx=dx, dw=dw, db=db)
    return cases


@pytest.mark.parametrize("C", [32, 64])
def test_canonical_batch_at_32_and_64_channels(hip_device, canonical_wide_case, C):
    """BASELINE configs 2 / 5 name 32- and 64-channel bodies; bench.py times roofline_c32 / _c64 and
    roofline_wgrad_c32 / _c64 at 16 x C x 48 x 48.  The launches exactly as they are timed -- 256-workgroup wide
    grid, XCD remap, the strip tables of the two half-batch chains, the 8-way split weight gradient -- checked by
    value at that size against torch's CPU operators: conv + bias + ReLU, the residual and mask epilogues, dgrad
    (tap-mirrored weight image), wgrad + bias gradient."""
    from larvanet_amd import kernels as K
    c = canonical_wide_case[C]
    d = {k: v.to(hip_device) for k, v in c.items() if k in ("x", "w", "b", "dy", "r0", "r1")}
    fwd, bwd = K.pack_weights(d["w"])
    scale = float(c["y"].abs().max())

    def close(got, ref, tol, what):
        err = float((got.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        assert err < tol, (what, C, err)

    # wide tiles: conv + bias + ReLU, both residual operands, the ReLU-backward mask
    relu_wide = K.conv3x3(d["x"], fwd, C, bias=d["b"], relu=True)
    close(relu_wide, c["y"].clamp_min(0), 1e-5, "conv+ReLU wide")
    res2 = K.conv3x3(d["x"], fwd, C, bias=d["b"], res0=d["r0"], res1=d["r1"])
    close(res2, (c["y"] + c["r0"]) + c["r1"], 1e-5, "conv+res0+res1 wide")
    # dgrad of the layer (+ the mask epilogue the residual blocks' backward uses)
    dx = K.conv3x3(d["dy"], bwd, C)
    close(dx, c["dx"], 2e-5, "dgrad wide")
    dxm = K.conv3x3(d["dy"], bwd, C, mask=relu_wide)
    close(dxm, c["dx"] * (c["y"].clamp_min(0) > 0), 2e-5, "dgrad+mask wide")
    # the two half-batch chains' launches (strip tables of both phases where the width has them; at 64 channels the
    # call runs the wide tiles over the image range): bit-identical to the full-batch wide launch
    for kw, ref in ((dict(bias=d["b"], relu=True), relu_wide), (dict(bias=d["b"], res0=d["r0"], res1=d["r1"]), res2)):
        out = torch.full_like(ref, float("nan"))
        K.conv3x3(d["x"], fwd, C, out=out, images=(0, 8), strips=True, **kw)
        K.conv3x3(d["x"], fwd, C, out=out, images=(8, 16), strips=2, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), ("half-batch strips", C, sorted(kw))
    # weight + bias gradient, 8-way split (256 workgroups per layer at the canonical size would be splits = 256;
    # 8 is the step's launch shape) and a single split
    for splits in (8, 1):
        dw = torch.full((C, C, 3, 3), float("nan"), device=hip_device)
        db = torch.full((C,), float("nan"), device=hip_device)
        K.conv3x3_wgrad([{"dy": d["dy"], "x": d["x"], "dw": dw, "db": db}], C, C, splits)
        torch.cuda.synchronize()
        close(dw, c["dw"], 3e-5, "wgrad splits=%d" % splits)
        close(db, c["db"], 3e-5, "bias grad splits=%d" % splits)
    assert scale > 10   # (the activations really are at the 0-255 scale's order of magnitude)


@pytest.mark.parametrize("N,C,H,W", [(1, 48, 23, 100), (2, 48, 9, 48), (1, 32, 14, 52), (1, 48, 5, 20)])
@pytest.mark.parametrize("epi", ["plain", "relu", "res1", "res2", "shuffle", "shuffle_base", "two_sources"])
def test_four_row_tiles_equal_three_row_tiles_bit_for_bit(hip_device, N, C, H, W, epi):
    """Round 4: whole-tensor launches may run on 4 x 48 tiles (fewer rounds of resident workgroups on large images, 9
    MFMAs per k-step per wave).  An output pixel's K loop does not depend on the tile it sits in: the two tile heights
    give the same bits for every epilogue the 4-row tiles exist for, heights that are not a multiple of 4, row-padded
    widths and concatenated sources; and the library's own choice (tile_rows = 0) is one of the two."""
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    if epi.startswith("shuffle") and C != 48:
        pytest.skip("pixel-shuffle exits have 48 output channels")
    rng = np.random.default_rng(N * 31 + C + H * 7 + W + len(epi))
    two = epi == "two_sources"
    x = _rand(rng, (N, C, H, W), 20.0)
    x2 = _rand(rng, (N, C, H, W), 20.0)
    w = _rand(rng, (C, 2 * C if two else C, 3, 3), 0.05)
    b = _rand(rng, (C,), 1.0)
    kw = {"bias": _dev(b, hip_device)}
    if epi == "relu":
        kw["relu"] = True
    if epi in ("res1", "res2"):
        kw["res0"] = _dev(_rand(rng, (N, C, H, W), 20.0), hip_device)
    if epi == "res2":
        kw["res1"] = _dev(_rand(rng, (N, C, H, W), 20.0), hip_device)
    if epi.startswith("shuffle"):
        kw["shuffle"] = True
    if epi == "shuffle_base":
        kw["base"] = _dev(_rand(rng, (N, 3, 4 * H, 4 * W), 50.0), hip_device)
    fwd, _ = K.pack_weights(_dev(w, hip_device))
    srcs = [_dev(x, hip_device), _dev(x2, hip_device)] if two else _dev(x, hip_device)
    outs = {r: K.conv3x3(srcs, fwd, C, tile_rows=r, **kw) for r in (3, 4, 0)}
    torch.cuda.synchronize()
    assert torch.equal(outs[3], outs[4]) and torch.equal(outs[0], outs[3])
    if epi == "plain":
        _report("conv3x3 on 4-row tiles", outs[4].cpu().numpy(), R.conv3x3(x, w, b), 2e-5)


def test_four_row_tiles_are_refused_where_they_do_not_exist(hip_device):
    from larvanet_amd import kernels as K
    x = torch.zeros(1, 48, 8, 16, device=hip_device)
    fwd, _ = K.pack_weights(torch.zeros(48, 48, 3, 3, device=hip_device))
    with pytest.raises(RuntimeError, match="hip error 801"):
        K.conv3x3(x, fwd, 48, mask=torch.ones_like(x), tile_rows=4)      # (no ReLU-backward epilogue on 4-row tiles)
    x13 = torch.zeros(1, 48, 5, 13, device=hip_device)                   # register-staged path
    with pytest.raises(RuntimeError, match="hip error 801"):
        K.conv3x3(x13, fwd, 48, tile_rows=4)


@pytest.mark.parametrize("N,C,H,W", [(1, 48, 339, 510), (5, 64, 100, 150), (2, 32, 200, 200), (3, 48, 120, 196)])
@pytest.mark.parametrize("epi", ["plain", "relu", "res1", "res2", "shuffle", "shuffle_base", "two_sources"])
def test_persistent_tiles_equal_one_workgroup_per_tile_bit_for_bit(hip_device, monkeypatch, N, C, H, W, epi):
    """Round 5: a whole-tensor launch with more tiles than the chip has workgroup slots (a full validation image:
    validate.py:94-102 / models/LarvaNet.py:283-293 of the reference) runs as ONE persistent workgroup per slot that walks
    its tiles behind a loader wave streaming the flattened (tile, chunk) sequence (conv3x3_mfma_persist_kernel).  Same
    bits as one workgroup per tile (LARVA_PERSIST=0) for every epilogue of the inference forward, 32 / 48 / 64 channels,
    row-padded widths, several images and concatenated sources."""
    from larvanet_amd import kernels as K
    if epi.startswith("shuffle") and C != 48:
        pytest.skip("pixel-shuffle exits have 48 output channels")
    P = (W + 3) // 4 * 4
    slots = 2 * torch.cuda.get_device_properties(hip_device).multi_processor_count   # (kWgPerCu workgroups per CU: conv_slots())
    assert N * ((H + 2) // 3) * ((P + 47) // 48) > slots, "the case must exceed the device's %d workgroup slots" % slots
    rng = np.random.default_rng(N * 31 + C + H * 7 + W + len(epi))
    two = epi == "two_sources"

    def padded(shape, scale):
        t = torch.zeros(shape[:-1] + (P,), device=hip_device)
        t[..., :W] = _dev(_rand(rng, shape, scale), hip_device)
        return t

    x, x2 = padded((N, C, H, W), 20.0), padded((N, C, H, W), 20.0)
    w = _rand(rng, (C, 2 * C if two else C, 3, 3), 0.05)
    kw = {"bias": _dev(_rand(rng, (C,), 1.0), hip_device), "logical_w": W, "tile_rows": 3}
    if epi == "relu":
        kw["relu"] = True
    if epi in ("res1", "res2"):
        kw["res0"] = padded((N, C, H, W), 20.0)
    if epi == "res2":
        kw["res1"] = padded((N, C, H, W), 20.0)
    if epi.startswith("shuffle"):
        kw["shuffle"] = True
    if epi == "shuffle_base":
        kw["base"] = _dev(_rand(rng, (N, 3, 4 * H, 4 * W), 50.0), hip_device)
    fwd, _ = K.pack_weights(_dev(w, hip_device))
    srcs = [x, x2] if two else x
    monkeypatch.delenv("LARVA_PERSIST", raising=False)
    persistent = K.conv3x3(srcs, fwd, C, **kw)
    monkeypatch.setenv("LARVA_PERSIST", "0")
    per_tile = K.conv3x3(srcs, fwd, C, **kw)
    torch.cuda.synchronize()
    assert torch.equal(persistent, per_tile)
    assert float(persistent.abs().max()) > 1.0   # (something was computed)


@pytest.mark.parametrize("C,H,P,strips", [(48, 3345, 3344, True), (32, 4100, 4096, False)])
def test_images_whose_cout_planes_exceed_2gib_take_the_per_tile_launch(hip_device, monkeypatch, C, H, P, strips):
    """csrc/conv3x3_mfma.hip launch_persist / strips_dispatch: the strip and persistent kernels fetch their residual /
    mask operands by buffer loads with 32-BIT byte offsets inside one image, so an image whose cout planes reach 2 GiB is
    refused (hipErrorNotSupported, before anything is launched) and the one-workgroup-per-tile launch -- 64-bit
    addressing -- takes over: kernels.conv3x3's `code == 801` fall-through for strips, conv_dispatch's own for persistent
    tiles.  Checked on a REAL tensor of that size (cout * H * pitch * 4 >= 2^31): the strip entry point returns 801 and
    leaves the output untouched; conv3x3(strips=True) and the default whole-tensor launch (more tiles than workgroup
    slots) then produce the same bits as LARVA_PERSIST=0, and windows at the image's first and LAST bytes (where a 32-bit
    offset would have wrapped) match the C oracle, residual operand included.  (32 channels: strip tables end at 4095 rows /
    columns, so 2 GiB of 32 planes is out of the strips' reach; the whole-tensor launches -- 4-row tiles by default,
    persistent 3-row tiles when asked for -- are checked the same way.)"""
    from larvanet_amd import hip_lib, kernels as K
    from oracle import larva_ref as R
    assert C * H * P * 4 >= 2 ** 31 and 8 * H * P * 4 < 2 ** 31
    gen = torch.Generator(device=hip_device).manual_seed(C + H)
    x = torch.randn(1, C, H, P, device=hip_device, generator=gen) * 20
    r0 = torch.randn(1, C, H, P, device=hip_device, generator=gen) * 20
    rng = np.random.default_rng(7)
    w, b = _rand(rng, (C, C, 3, 3), 0.05), _rand(rng, (C,), 1.0)
    fwd, _ = K.pack_weights(_dev(w, hip_device))
    bias = _dev(b, hip_device)
    lib = hip_lib.load()
    seen = []
    real = lib.larva_conv3x3_fwd_strips
    out_s = torch.full((1, C, H, P), float("nan"), device=hip_device)

    def spy(*a):
        rc = real(*a)
        torch.cuda.synchronize()
        seen.append((rc, bool(torch.isnan(out_s).all())))   # refused -> nothing may have been launched on `out`
        return rc
    monkeypatch.setattr(lib, "larva_conv3x3_fwd_strips", spy)
    assert (K.strip_tile_table(H, P, hip_device) is not None) == strips   # (48: a shape the strips themselves accept)
    K.conv3x3(x, fwd, C, bias=bias, res0=r0, out=out_s, strips=True)
    torch.cuda.synchronize()
    assert seen == ([(801, True)] if strips else []), seen    # hipErrorNotSupported, output untouched at that point
    slots = 2 * torch.cuda.get_device_properties(hip_device).multi_processor_count
    assert ((H + 2) // 3) * ((P + 47) // 48) > slots           # the default launch would pick persistent tiles
    out_p = K.conv3x3(x, fwd, C, bias=bias, res0=r0)           # persistent refused inside conv_dispatch -> per-tile
    out_3 = K.conv3x3(x, fwd, C, bias=bias, res0=r0, tile_rows=3)
    monkeypatch.setenv("LARVA_PERSIST", "0")
    out_t = K.conv3x3(x, fwd, C, bias=bias, res0=r0, tile_rows=3)
    torch.cuda.synchronize()
    assert torch.equal(out_s, out_t) and torch.equal(out_p, out_t) and torch.equal(out_3, out_t)
    del out_s, out_p, out_3
    # windows against the oracle: first bytes, the middle, and the last rows / columns / channels of the image
    for (ya, yb, xa, xb) in ((0, 24, 0, 40), (H // 2 - 12, H // 2 + 12, P // 2 - 20, P // 2 + 20), (H - 24, H, P - 40, P)):
        xc, rc_ = x[:, :, ya:yb, xa:xb].cpu().numpy(), r0[:, :, ya:yb, xa:xb].cpu().numpy()
        ref = R.conv3x3(xc, w, b) + rc_
        got = out_t[:, :, ya:yb, xa:xb].cpu().numpy()
        # the crop's own zero padding is the image's only at the image border: drop the crop's inner edges
        ys = slice(0 if ya == 0 else 1, (yb - ya) if yb == H else (yb - ya) - 1)
        xs = slice(0 if xa == 0 else 1, (xb - xa) if xb == P else (xb - xa) - 1)
        _report("conv3x3 over 2 GiB window (%d, %d)" % (ya, xa), got[:, :, ys, xs], ref[:, :, ys, xs], 2e-5)
