"""x2 / x3 networks (prepare(scales=[2]) / [3]): the legs' last conv has 3 s^2 outputs before PixelShuffle(s), the base
image is F.interpolate(x, scale_factor=s).  The truth is a functional restatement of the network at scale s over torch
CPU operators (pinned at s = 4 against oracle/larva_torch.py bit for bit) and the C oracle's scale-generic pieces."""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import larva_torch as T



# ---------------------------------------------------------------- restatement at scale s
def _leg(sd, prefix, fea, base, s):
    h = F.relu(F.conv2d(fea, sd[prefix + ".recon_block.0.weight"], sd[prefix + ".recon_block.0.bias"], padding=1))
    return F.pixel_shuffle(F.conv2d(h, sd[prefix + ".recon_block.2.weight"], sd[prefix + ".recon_block.2.bias"],
                                    padding=1), s) + base


def forward_exits(sd, x, blocks, s, mode="bicubic"):
    fea = T.head(sd, x)
    base = F.interpolate(x, scale_factor=s, mode=mode, align_corners=False)
    outs, feats = [], []
    for i, nb in enumerate(blocks):
        fea = T.body(sd, i, fea, nb)
        feats.append(fea)
        outs.append(_leg(sd, "body_%d.leg" % i, fea, base, s))
    return outs, feats, base


def _tail(sd, feats, base, s):
    fea = F.conv2d(torch.cat(feats, dim=1), sd["tail.merge_conv.weight"], sd["tail.merge_conv.bias"], padding=1)
    return _leg(sd, "tail", fea, base, s)


def multi_exit_loss(sd, x, truth, blocks, s, v2=False):
    outs, feats, base = forward_exits(sd, x, blocks, s)
    loss = 0
    for o in outs:
        loss = loss + F.l1_loss(o, truth)
    if v2:
        return (loss + F.l1_loss(_tail(sd, feats, base, s), truth)) / (len(blocks) + 1)
    return loss / len(blocks)


def train_steps(sd, x, truth, blocks, s, steps=1, lr=4e-4, v2=False):
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=lr)
    losses, grads = [], None
    for _ in range(steps):
        loss = multi_exit_loss(params, x, truth, blocks, s, v2=v2)
        opt.zero_grad()
        loss.backward()
        grads = {k: v.grad.detach().clone() for k, v in params.items()}
        opt.step()
        losses.append(float(loss.item()))
    for k in sd:
        sd[k] = params[k].detach()
    return losses, grads


def test_restatement_at_x4_is_the_oracle_bit_for_bit():
    blocks = [1, 1]
    sd = T.init_state_dict(blocks, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 8, 12, generator=g) * 255
    truth = torch.rand(2, 3, 32, 48, generator=g) * 255
    a, _, _ = forward_exits(sd, x, blocks, 4)
    b, _, _ = T.forward_exits(sd, x, blocks)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    sd1, sd2 = dict(sd), dict(sd)
    la, ga = train_steps(sd1, x, truth, blocks, 4, steps=2)
    lb, gb = T.train_steps(sd2, x, truth, blocks, steps=2)
    assert la == lb and all(torch.equal(ga[k], gb[k]) and torch.equal(sd1[k], sd2[k]) for k in sd)


# ---------------------------------------------------------------- models (CPU)
def _model(name, scale, extra=(), training=False):
    import importlib
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=2", "--num_blocks=1,1"] + list(extra))
    m.prepare(is_training=training, scales=[scale])
    return m


MODELS = [("LarvaNet", ()), ("LarvaNetV2", ()), ("LarvaLeg", ("--leg=2",)), ("LarvaLegV2", ("--leg=2",))]


@pytest.mark.parametrize("name,extra", MODELS)
def test_last_convs_and_shuffle_follow_the_scale(name, extra):
    ref = _model(name, 4, extra).model
    keys4 = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert keys4["body_0.leg.recon_block.2.weight"] == (48, 48, 3, 3)
    for s in (2, 3):
        net = _model(name, s, extra).model
        sd = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        assert list(sd) == list(keys4)
        for k, shape in sd.items():
            if re.search(r"recon_block\.2\.(weight|bias)$", k):
                assert shape == (3 * s * s,) + keys4[k][1:], (k, shape)
            else:
                assert shape == keys4[k], k
        legs = [getattr(net, "body_%d" % i).leg for i in range(2)] + ([net.tail] if hasattr(net, "tail") else [])
        for leg in legs:
            assert isinstance(leg.upsample, torch.nn.PixelShuffle) and leg.upsample.upscale_factor == s


@pytest.mark.parametrize("name", ["LarvaNet", "LarvaNetV2"])
def test_save_restore_round_trip_at_x2_x3(name, tmp_path):
    for s in (2, 3):
        a = _model(name, s)
        path = a.save(str(tmp_path))
        b = _model(name, s)
        b.restore(path)
        for k, v in a.model.state_dict().items():
            assert torch.equal(v.cpu(), b.model.state_dict()[k].cpu()), k
        os.unlink(path)


@pytest.mark.parametrize("nf,s", [(32, 2), (64, 2), (32, 3), (64, 3)])
def test_other_widths_are_refused_at_x2_x3(nf, s):
    with pytest.raises(ValueError, match="num_filters %d at x%d" % (nf, s)):
        _model("LarvaNet", s, ("--num_filters=%d" % nf,))


# ---------------------------------------------------------------- kernels (GPU)
def _rand(shape, seed):
    return (np.random.default_rng(seed).random(shape) * 255).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
def test_base_image(hip_device, s, mode):
    from larvanet_amd import kernels as K
    from oracle import larva_ref as R
    for h, w in ((1, 1), (2, 5), (5, 2), (48, 67), (67, 48), (5, 67)):
        x = _rand((2, 3, h, w), h * 100 + w)
        out = K.upsample(torch.from_numpy(x).to(hip_device), s, mode).cpu().numpy()
        # against F.interpolate in float64: exact source coordinates, as the kernel's constant phases (in float32 ATen's
        # x3 coordinates carry the rounding of (float)(1/3), csrc/larva_scale.hip)
        ref = F.interpolate(torch.from_numpy(x).double(), scale_factor=s, mode=mode, align_corners=False).numpy()
        np.testing.assert_allclose(out, ref, rtol=1e-5, atol=3e-4, err_msg="%s x%d %s" % (mode, s, (h, w)))
        if mode == "bicubic":
            np.testing.assert_allclose(out, R.bicubic_up(x, s), rtol=1e-5, atol=3e-4)


def _padded_leg_conv(s, seed):
    """Leg conv2 at scale s: weights [3 s^2][48], their packed padded 32-row image, bias."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(3 * s * s, 48, 3, 3, generator=g) * 0.05
    b = torch.randn(3 * s * s, generator=g)
    return w, b


@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 3])
def test_leg_conv2_shuffle_l1_and_unshuffled_gradient(hip_device, s):
    """The plain 32-output conv on zero-padded rows + shuffle(s) + base, the fused L1 partials and the unshuffled
    gradient against the C oracle: the 16-byte path (W % 4 == 0), the row-pitch path (logical_w) and the register path
    (odd width, no pitch).  Padding channels of the gradient are exactly zero."""
    from larvanet_amd import kernels as K
    from larvanet_amd.autograd import PackedConv
    from oracle import larva_ref as R
    w, b = _padded_leg_conv(s, s)
    wd, bd = w.to(hip_device), b.to(hip_device)
    pc = PackedConv(wd, bd, cout_pad=32)
    pc.refresh()
    (fwd, bwd), = pc.get()
    for (N, H, W, pitch) in ((2, 12, 16, None), (2, 9, 13, 16), (1, 7, 13, None)):
        h = np.maximum(_rand((N, 48, H, W), W) - 128, 0) / 64
        base = _rand((N, 3, s * H, s * W), H)
        truth = _rand((N, 3, s * H, s * W), H + 1)
        y_ref = R.pixel_shuffle(R.conv3x3(h, w.numpy(), b.numpy()), s)
        out_ref = y_ref + base
        hd = torch.from_numpy(h).to(hip_device)
        if pitch is not None:
            hp = torch.zeros((N, 48, H, pitch), device=hip_device)
            hp[..., :W] = hd
            y = K.conv3x3(hp, fwd, 32, bias=pc.padded_bias(), logical_w=W)
            out = K.pixel_shuffle_base(y, torch.from_numpy(base).to(hip_device), s, logical_w=W)
            np.testing.assert_allclose(out.cpu().numpy(), out_ref, rtol=1e-4, atol=2e-3)
            continue
        y = K.conv3x3(hd, fwd, 32, bias=pc.padded_bias())
        out = K.pixel_shuffle_base(y, torch.from_numpy(base).to(hip_device), s)
        np.testing.assert_allclose(out.cpu().numpy(), out_ref, rtol=1e-4, atol=2e-3)
        td = torch.from_numpy(truth).to(hip_device)
        part, inv, grad, img = K.shuffle_l1_partial_grad(y, torch.from_numpy(base).to(hip_device), td, 1.0, 0.5, s)
        assert torch.equal(img, out)
        l1 = float(part.double().sum()) * inv
        assert abs(l1 - float(np.abs(out.cpu().numpy().astype(np.float64) - truth).mean())) < 1e-5 * l1
        gref = R.pixel_unshuffle(R.l1_grad(out.cpu().numpy(), truth, 0.5), s)
        gd = grad.cpu().numpy()
        np.testing.assert_allclose(gd[:, :3 * s * s], gref, rtol=1e-6, atol=0)
        assert not gd[:, 3 * s * s:].any()
        g2 = K.l1_bwd_unshuffle(out, td, torch.tensor(1.0, device=hip_device), s, 32, 0.5)
        assert torch.equal(g2, grad)
        un = K.pixel_unshuffle(out, s, 32).cpu().numpy()
        np.testing.assert_array_equal(un[:, :3 * s * s], R.pixel_unshuffle(out.cpu().numpy(), s))
        assert not un[:, 3 * s * s:].any()
        # dgrad of the padded gradient (4 K chunks, zero weight rows) with the ReLU mask, and the (32, 48) weight gradient
        dh = K.conv3x3(grad, bwd, 48, mask=hd).cpu().numpy()
        dref = R.conv3x3_dgrad(gref, w.numpy()) * (h > 0)
        np.testing.assert_allclose(dh, dref, rtol=1e-4, atol=1e-4 * float(np.abs(dref).max()))
        from larvanet_amd.autograd import padded_wgrad
        pc.grad_inplace = False
        dw, db = padded_wgrad(grad, hd, pc, tuple(w.shape))
        dw_ref, db_ref = R.conv3x3_wgrad(gref, h)
        np.testing.assert_allclose(dw.cpu().numpy(), dw_ref, rtol=1e-4, atol=1e-4 * float(np.abs(dw_ref).max()))
        np.testing.assert_allclose(db.cpu().numpy(), db_ref, rtol=1e-4, atol=1e-4 * float(np.abs(db_ref).max()))


# ---------------------------------------------------------------- training step (GPU)
class _NoVal:
    def get_num_images(self):
        return 0


def _train_model(name, s, blocks, use_graph, sd=None):
    import importlib
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks))])
    torch.manual_seed(0)
    m.prepare(is_training=True, scales=[s])
    m.use_hip_graph = use_graph
    m.strict_graph = True
    if sd is not None:
        with torch.no_grad():
            for k, p in m.model.state_dict().items():
                p.copy_(sd[k])
        m.model.invalidate_packed_weights()
    return m


def _batch(n, h, w, s, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, h, w, generator=g) * 255, torch.rand(n, 3, s * h, s * w, generator=g) * 255


CASES = [("LarvaNet", 2, [2, 2], (16, 48, 48)), ("LarvaNet", 3, [2, 2], (16, 48, 48)),
         ("LarvaNet", 2, [4, 4, 4, 4], (16, 48, 48)), ("LarvaNet", 3, [4, 4, 4, 4], (16, 48, 48)),
         ("LarvaNet", 3, [2, 2], (12, 40, 56)), ("LarvaNetV2", 2, [4, 4, 4, 4], (16, 48, 48))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,s,blocks,shape", CASES)
def test_training_step_against_float64_and_graph_equals_eager(hip_device, name, s, blocks, shape):
    v2 = name == "LarvaNetV2"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    mg = _train_model(name, s, blocks, True)
    sd = {k: v.detach().cpu().clone() for k, v in mg.model.state_dict().items()}
    me = _train_model(name, s, blocks, False, sd)
    x, truth = _batch(*shape, s, seed=s * 10 + len(blocks))
    ref_losses, ref_grads = train_steps({k: v.double() for k, v in sd.items()}, x.double(), truth.double(), blocks, s,
                                        v2=v2)
    args = types.SimpleNamespace(train_path="/tmp")
    xd, td = x.to(hip_device), truth.to(hip_device)
    steps = 1 if v2 else 3
    lg, le = [], []
    for step in range(steps):
        lg.append(mg.train_step_larva(args, _NoVal(), xd, td, None))
        le.append(me.train_step_larva(args, _NoVal(), xd, td, None))
        if step == 0:
            assert abs(lg[0] - ref_losses[0]) <= 2e-5 * abs(ref_losses[0])
            named = dict(mg.model.named_parameters())
            assert len(named) == (82 if len(blocks) == 4 and not v2 else len(named))
            for k, p in named.items():
                got, ref = p.grad.detach().cpu().double(), ref_grads[k]
                d = float((got - ref).abs().max())
                # 1e-3 of the tensor's maximum: the x4 bar is 2e-4, but an exit element whose output and truth agree
                # to fp32 rounding gets the opposite sign gradient in float64, and with a 4x / 1.8x smaller HR image one
                # such element weighs that much more (measured up to 3.6x the x4 bar at M4B4 x3, in the deepest body)
                bar = 1e-3 * max(float(ref.abs().max()), 1e-30)
                if k.endswith("recon_block.2.bias"):
                    # a sum of +-g over the HR pixels of one sub-pixel channel (g = 1 / (terms * numel)) that cancels
                    # down to a few hundred g: two such near-tie elements of opposite sign are allowed
                    bar += 4.0 / ((len(blocks) + (1 if v2 else 0)) * truth.numel())
                assert d <= bar, (k, d, bar)
                assert torch.equal(p.grad, dict(me.model.named_parameters())[k].grad), ("graph != eager", k)
    assert mg.use_hip_graph and mg.hip_graph_fell_back is None
    assert lg == le
    for k, v in mg.model.state_dict().items():
        assert torch.equal(v, me.model.state_dict()[k]), k


@pytest.mark.gpu
def test_wrong_truth_shape_is_refused_before_any_launch(hip_device):
    m = _train_model("LarvaNet", 2, [1, 1], True)
    x, _ = _batch(2, 12, 12, 2, 0)
    bad = torch.zeros(2, 3, 48, 48)
    with pytest.raises(ValueError, match="truth"):
        m.train_step_larva(types.SimpleNamespace(train_path="/tmp"), _NoVal(), x.to(hip_device), bad.to(hip_device))
    assert m.global_step == 0


# ---------------------------------------------------------------- inference (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("s", [2, 3])
def test_upscale_whole_images_and_bands(hip_device, s):
    from larvanet_amd import image_utils
    m = _model("LarvaNet", s)
    sd = {k: v.detach().cpu().double() for k, v in m.model.state_dict().items()}
    for (h, w) in ((67, 93), (339, 510)):
        x = _rand((3, h, w), h)
        out = m.upscale([x], s)
        assert out.shape == (1, 3, s * h, s * w)
        with torch.no_grad():
            ref = forward_exits(sd, torch.from_numpy(x)[None].double(), [1, 1], s)[0][-1].numpy()
        np.testing.assert_allclose(out, ref, rtol=1e-4, atol=2e-3)
    x = _rand((3, 67, 93), 5)
    whole = m.upscale([x], s)[0]
    bands = [image_utils.upscale_band(m, x, s, r0, r1, m.receptive_halo()) for r0, r1 in ((0, 22), (22, 45), (45, 67))]
    assert np.array_equal(np.concatenate(bands, axis=1), whole)


@pytest.mark.gpu
def test_larvaleg_exit_2_at_x3(hip_device):
    m = _model("LarvaLeg", 3, ("--leg=2",))
    sd = {k: v.detach().cpu().double() for k, v in m.model.state_dict().items()}
    x = _rand((3, 20, 28), 9)
    out = m.upscale([x], 3)
    with torch.no_grad():
        ref = forward_exits(sd, torch.from_numpy(x)[None].double(), [1, 1], 3)[0][1].numpy()
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=2e-3)


# ---------------------------------------------------------------- drivers (GPU)
@pytest.mark.gpu
def test_train_larva_at_x2_validates_at_x2(hip_device, tmp_path, capsys):
    from larvanet_amd import train_larva
    model = train_larva.main([
        "--model=LarvaNet", "--dataloader=synthetic_loader", "--val_dataloader=synthetic_loader", "--scales=2",
        "--train_path", str(tmp_path), "--max_steps=3", "--batch_size=4", "--input_patch_size=12",
        "--num_modules=2", "--num_blocks=1,1", "--synthetic_images=3", "--synthetic_lr_size=20"])
    out = capsys.readouterr().out
    assert model.global_step == 3 and model.model.scale == 2
    psnr = [float(v) for v in re.findall(r"psnr=([-0-9.naif]+)", out)]
    assert psnr and all(np.isfinite(psnr))
