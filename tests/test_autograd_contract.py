"""The autograd nodes OUTSIDE the plugin's fused step, against float64.

larvanet_amd/autograd.py wires the HIP kernels into torch as HeadFn, BodyFn, LegFn, ExitFn, ExitsFn, MergeFn, L1LossFn
and MeanTermsFn.  Inside the fused step (StepScope(seed_grad=1), a GradBucket that owns every gradient, deferred weight
gradients, the stock L1Loss) the rest of the suite pins them.  This file pins what else the code supports: model(x)
under grad, a replaced loss_fn, gradients handed back to autograd, an upstream gradient that is not 1, exits whose term
is not used, more than 8 loss terms, inputs whose gradient is not computed, parameters frozen after prepare().

Reference: oracle/larva_torch.py in float64 on the same state_dict, at x2 / x3 the scale-generic restatement of
tests/test_scales.py, and `multi_exit` below for a loss that is not L1 (pinned bit for bit against both on the CPU).

Bars (the project's, tests/test_train_regimes.py::test_training_step_regime_against_the_float64_oracle): per gradient
tensor max(3 * max|g_fp32cpu - g_fp64|, floor * max|g_fp64|) with floor 1e-4 at 48 filters and 5e-4 at 32 / 64; loss
values 2e-5 relative; images on the 0..255 scale 2e-3 absolute.  The CPU tests at the end of the harness section show
that torch's own fp32 run stays inside every bar on every input used here, and that the bars reject a float64 run with
one dropped conv tap, with a base image shifted by one pixel, and with every quantity wrong by 5 bars.

Every GPU test prints its worst ratio to its bar."""
import functools
import importlib
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import larva_torch as T

import test_scales as S
from test_train_regimes import GRAD_BAR, LOSS_BAR, _rel

LOSS_REL = 2e-5      # loss values, relative
IMAGE_ABS = 2e-3     # images on the 0..255 scale
FP32_MULT = 3        # x the distance of torch's fp32 CPU run from float64 ...
FLOOR = {48: 1e-4, 32: 5e-4, 64: 5e-4}   # ... or this share of the tensor's largest element, whichever is larger

SHAPES = [(2, 8, 12), (1, 7, 9), (3, 6, 8)]   # N, LR height, LR width: aligned; odd width (register-staged); three images


# ================================================================ harness
def multi_exit(sd, x, truth, blocks, loss, weights=None, v2=False, s=4):
    """sum_i weights[i] * loss(out_i, truth) / n_terms over the exits (and, v2, the tail) at scale s."""
    outs, feats, base = S.forward_exits(sd, x, blocks, s)
    if v2:
        outs = outs + [S._tail(sd, feats, base, s)]
    total = 0
    for i, o in enumerate(outs):
        term = loss(o, truth)
        total = total + (term if weights is None else weights[i] * term)
    return total / len(outs)


def _route(sd, x, blocks, s, name, extra=()):
    """What model(x) returns: the last exit (LarvaNet), exit k (LarvaLeg --leg=k) or the tail (LarvaNetV2)."""
    outs, feats, base = S.forward_exits(sd, x, blocks, s)
    if name == "LarvaNetV2":
        return S._tail(sd, feats, base, s)
    leg = [int(e.split("=")[1]) for e in extra if e.startswith("--leg=")]
    return outs[leg[0] - 1] if leg else outs[-1]


def _model(name, blocks, s=4, nf=48, training=False, extra=(), seed=5):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(["--num_modules=%d" % len(blocks), "--num_blocks=" + ",".join(map(str, blocks)),
                  "--num_filters=%d" % nf] + list(extra))
    torch.manual_seed(seed)
    m.prepare(is_training=training, scales=[s])
    m.strict_graph = True
    return m


@functools.lru_cache(maxsize=None)
def _spec_sd(name, blocks, s=4, nf=48, extra=()):
    """The weights of a case: the model's own initial draw, with non-zero biases (the reference initialises them to 0)."""
    sd = {k: v.detach().cpu().clone() for k, v in _model(name, blocks, s, nf, False, extra).model.state_dict().items()}
    g = torch.Generator().manual_seed(17)
    for k in sd:
        if k.endswith(".bias"):
            sd[k] = torch.rand(sd[k].shape, generator=g) - 0.5
    return sd


def _load(m, sd):
    with torch.no_grad():
        for k, p in m.model.state_dict().items():
            p.copy_(sd[k])
    m.model.invalidate_packed_weights()
    return m


def _inputs(shape, s, seed=0):
    """Uniform images on 0..255 -> (x, truth)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(100 * n + 10 * h + w + seed)
    return torch.rand(n, 3, h, w, generator=g) * 255, torch.rand(n, 3, s * h, s * w, generator=g) * 255


def _coeff(shape, s):
    """The fixed, signed, non-constant c of loss = (out * c).sum(): dout = c exactly, no L1 sign can flip."""
    n, h, w = shape
    g = torch.Generator().manual_seed(7000 + 100 * n + 10 * h + w)
    return torch.rand(n, 3, s * h, s * w, generator=g) * 2 - 1


def _exit_inputs(shape, s, nf=48, count=1):
    """Body outputs, a base image and a truth for exits run on their own."""
    n, h, w = shape
    g = torch.Generator().manual_seed(9000 + 100 * n + 10 * h + w + s)
    feas = [torch.randn(n, nf, h, w, generator=g) * 20 for _ in range(count)]
    return feas, torch.rand(n, 3, s * h, s * w, generator=g) * 255, torch.rand(n, 3, s * h, s * w, generator=g) * 255


def _leaf(sd, dtype, only=None):
    return {k: v.detach().to(dtype, copy=True).requires_grad_(True) for k, v in sd.items() if only is None or only(k)}


def _grads(named):
    return {k: None if v.grad is None else v.grad.detach().double() for k, v in named.items()}


class Ref:
    """fn(dtype) -> {"value": float or None, "image": tensor or None, "grads": {name: tensor or None}}, run in float64
    (the truth) and in float32 (torch's CPU operators: what fp32 itself costs on these inputs)."""

    def __init__(self, fn, nf=48):
        self.r64, self.r32 = fn(torch.float64), fn(torch.float32)
        self.floor = FLOOR[nf]

    def bar(self, k):
        g64, g32 = self.r64["grads"][k], self.r32["grads"][k]
        return max(FP32_MULT * float((g32 - g64).abs().max()), self.floor * max(float(g64.abs().max()), 1e-30))

    def ratios(self, got):
        """{check: distance from float64 / its bar}; a gradient that float64 does not have must be None or zero."""
        out = {}
        if self.r64.get("value") is not None:
            out["value"] = abs(got["value"] - self.r64["value"]) / (LOSS_REL * abs(self.r64["value"]))
        if self.r64.get("image") is not None:
            out["image"] = float((got["image"].double() - self.r64["image"]).abs().max()) / IMAGE_ABS
        for k, g64 in self.r64["grads"].items():
            g = got["grads"][k]
            if g64 is None:
                out["grad " + k] = 0.0 if g is None or not bool(g.any()) else float("inf")
            elif g is None:
                out["grad " + k] = float("inf")
            else:
                out["grad " + k] = float((g.double() - g64).abs().max()) / self.bar(k)
        return out

    def check(self, label, got):
        r = self.ratios(got)
        worst = max(r, key=r.get)
        print("\nautograd contract %s: worst %.3f of its bar (%s)" % (label, r[worst], worst))
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        assert not bad, (label, bad)
        return r[worst]


@functools.lru_cache(maxsize=None)
def linear_ref(name, blocks, extra, s, nf, shape):
    sd = _spec_sd(name, blocks, s, nf, extra)
    x, c = _inputs(shape, s)[0], _coeff(shape, s)

    def fn(dtype):
        p = _leaf(sd, dtype)
        out = _route(p, x.to(dtype), list(blocks), s, name, extra)
        (out * c.to(dtype)).sum().backward()
        return {"image": out.detach().double(), "grads": _grads(p)}
    return Ref(fn, nf)


LOSSES = {"mse": F.mse_loss, "l1": F.l1_loss}


@functools.lru_cache(maxsize=None)
def loss_ref(name, blocks, loss, shape, s=4, nf=48):
    """The plugin's step: mean over the exits (and V2's tail) of a loss; loss None = T.multi_exit_loss itself."""
    v2 = name == "LarvaNetV2"
    sd = _spec_sd(name, blocks, s, nf)
    x, truth = _inputs(shape, s)

    def fn(dtype):
        p = _leaf(sd, dtype)
        if loss is None:
            val = T.multi_exit_loss(p, x.to(dtype), truth.to(dtype), list(blocks), v2=v2)
        else:
            val = multi_exit(p, x.to(dtype), truth.to(dtype), list(blocks), LOSSES[loss], v2=v2, s=s)
        val.backward()
        with torch.no_grad():
            img = _route(p, x.to(dtype), list(blocks), s, name)
        return {"value": float(val.detach()), "image": img.double(), "grads": _grads(p)}
    return Ref(fn, nf)


LEG = "body_0.leg"


@functools.lru_cache(maxsize=None)
def exit_ref(s, shape, divisor):
    """One exit on its own: value l1(leg(fea, base), truth); gradients of 0.37 * value [/ divisor]."""
    sd = _spec_sd("LarvaNet", (1, 1), s)
    (fea,), base, truth = _exit_inputs(shape, s)

    def fn(dtype):
        p = _leaf(sd, dtype, lambda k: k.startswith(LEG))
        p["fea"] = fea.to(dtype).requires_grad_(True)
        out = S._leg(p, LEG, p["fea"], base.to(dtype), s)
        val = F.l1_loss(out, truth.to(dtype))
        (0.37 * val / (divisor or 1)).backward()
        return {"value": float(val.detach()), "image": out.detach().double(), "grads": _grads(p)}
    return Ref(fn)


def exit_weights(M, subset):
    """{exit: weight}: the first and the last exit with 0.5 and 2, or every exit with its own weight."""
    return {0: 0.5, M - 1: 2.0} if subset == "ends" else {i: 0.5 + 0.25 * i for i in range(M)}


@functools.lru_cache(maxsize=None)
def exits_ref(M, subset, shape):
    """All exits as one node: value sum_i w_i l1_i over the live exits; the node applies the 1 / M of the mean in its
    backward, so the gradients are those of value / M.  The image is the last exit's."""
    sd = _spec_sd("LarvaNet", (1,) * M)
    feas, base, truth = _exit_inputs(shape, 4, count=M)
    w = exit_weights(M, subset)

    def fn(dtype):
        p = _leaf(sd, dtype)
        for i in range(M):
            p["fea_%d" % i] = feas[i].to(dtype).requires_grad_(True)
        val = 0
        for i in sorted(w):
            val = val + w[i] * F.l1_loss(S._leg(p, "body_%d.leg" % i, p["fea_%d" % i], base.to(dtype), 4), truth.to(dtype))
        (val / M).backward()
        with torch.no_grad():
            last = S._leg(p, "body_%d.leg" % (M - 1), p["fea_%d" % (M - 1)], base.to(dtype), 4)
        return {"value": float(val.detach()), "image": last.double(), "grads": _grads(p)}
    return Ref(fn)


# ---------------------------------------------------------------- the cases of the GPU tests (the CPU tests walk them too)
ROUTES = [("LarvaNet", (2, 1), ()), ("LarvaNetV2", (1, 2), ()), ("LarvaLeg", (2, 1), ("--leg=1",)), ("LarvaNet", (0, 1), ())]
A_CASES = [(name, blocks, extra, s, 48) for name, blocks, extra in ROUTES for s in (2, 3, 4)] + \
          [(name, blocks, extra, 4, nf) for name, blocks, extra in ROUTES[:2] for nf in (32, 64)]
A_IDS = ["%s-%s%s-x%d-nf%d" % (n, "".join(map(str, b)), "".join(e), s, nf) for n, b, e, s, nf in A_CASES]
B_CASES = [("LarvaNet", (2, 1)), ("LarvaNetV2", (1, 2))]
NINE = ("LarvaNetV2", (1,) * 8)


def _all_refs():
    """(label, Ref) of every float64 reference the GPU tests use."""
    for case, cid in zip(A_CASES, A_IDS):
        for shape in SHAPES:
            yield "a %s %s" % (cid, shape), linear_ref(*case, shape)
    for name, blocks in B_CASES:
        for shape in SHAPES[:2]:
            yield "b %s %s" % (name, shape), loss_ref(name, blocks, "mse", shape)
    for s in (2, 3, 4):
        for divisor in (None, 3):
            for shape in SHAPES:
                yield "c x%d /%s %s" % (s, divisor, shape), exit_ref(s, shape, divisor)
    for M in (3, 5, 9):
        for subset in ("ends", "all"):
            for shape in SHAPES:
                yield "d M%d %s %s" % (M, subset, shape), exits_ref(M, subset, shape)
    for shape in SHAPES[:2]:
        yield "f %s" % (shape,), loss_ref(*NINE, None, shape)


# ---------------------------------------------------------------- CPU tests of the harness
def test_multi_exit_with_l1_is_the_oracle_bit_for_bit():
    for v2, blocks, s in ((False, [2, 1], 4), (True, [1, 2], 4), (True, [1, 1], 3)):
        sd = _spec_sd("LarvaNetV2" if v2 else "LarvaNet", tuple(blocks), s)
        x, truth = _inputs(SHAPES[0], s)
        fns = [lambda p: multi_exit(p, x, truth, blocks, F.l1_loss, v2=v2, s=s),
               lambda p: multi_exit(p, x, truth, blocks, F.l1_loss, weights=[1.0] * (len(blocks) + v2), v2=v2, s=s),
               lambda p: S.multi_exit_loss(p, x, truth, blocks, s, v2=v2)]
        if s == 4:   # (the oracle itself is x4 only)
            fns.append(lambda p: T.multi_exit_loss(p, x, truth, blocks, v2=v2))
        runs = []
        for fn in fns:
            p = _leaf(sd, torch.float32)
            val = fn(p)
            val.backward()
            runs.append((val.detach(), _grads(p)))
        for val, grads in runs[1:]:
            assert torch.equal(val, runs[0][0])
            assert all(torch.equal(grads[k], runs[0][1][k]) for k in grads)


def test_multi_exit_weights_and_loss_are_applied():
    sd = _spec_sd("LarvaNet", (2, 1))
    x, truth = _inputs(SHAPES[0], 4)
    outs, _, _ = T.forward_exits({k: v.double() for k, v in sd.items()}, x.double(), [2, 1])
    want = (0.5 * F.mse_loss(outs[0], truth.double()) + 2.0 * F.mse_loss(outs[1], truth.double())) / 2
    got = multi_exit({k: v.double() for k, v in sd.items()}, x.double(), truth.double(), [2, 1], F.mse_loss, weights=[0.5, 2.0])
    assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))


def test_fp32_cpu_run_stays_inside_every_bar():
    """The bars are not tight for the reference itself: torch's fp32 CPU run passes every check of every case."""
    worst, n = ("", 0.0), 0
    for label, ref in _all_refs():
        r = ref.ratios(ref.r32)
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        assert not bad, (label, bad)
        k = max(r, key=r.get)
        worst, n = max(worst, (label + " " + k, r[k]), key=lambda t: t[1]), n + 1
    print("\nautograd contract: fp32 CPU inside every bar of %d references, worst %.3f (%s)" % (n, worst[1], worst[0]))


def _faulty(kind, linear):
    """A float64 run of LarvaNet [2,1] at x4 with one defect: a leg conv with one of its nine taps dropped, or a base
    image shifted by one pixel.  linear: under (out * c).sum(), else under the mean L1 of the exits."""
    blocks, shape = [2, 1], SHAPES[0]
    sd = _spec_sd("LarvaNet", (2, 1))
    x, truth = (t.double() for t in _inputs(shape, 4))
    c = _coeff(shape, 4).double()
    p = _leaf(sd, torch.float64)
    used, delta = dict(p), 0.0
    if kind == "tap":
        mask = torch.ones(1, 1, 3, 3, dtype=torch.float64)
        mask[..., 0, 0] = 0
        used["body_1.leg.recon_block.0.weight"] = p["body_1.leg.recon_block.0.weight"] * mask
    else:
        base = T.base_image(x)
        delta = torch.roll(base, 1, -1) - base
    if linear:
        out = _route(used, x, blocks, 4, "LarvaNet") + delta
        (out * c).sum().backward()
        return {"image": out.detach(), "grads": _grads(p)}
    val = multi_exit(used, x, truth, blocks, lambda o, t: F.l1_loss(o + delta, t))
    val.backward()
    with torch.no_grad():
        img = _route(used, x, blocks, 4, "LarvaNet") + delta
    return {"value": float(val.detach()), "image": img, "grads": _grads(p)}


@pytest.mark.parametrize("kind", ["tap", "shift"])
def test_bars_reject_a_defective_float64_run(kind):
    """Fault sensitivity of the harness on the smallest shape used: what the checks of case a (image + gradients) and of
    the loss cases (value + image + gradients) say about a run with one defect."""
    lin = linear_ref("LarvaNet", (2, 1), (), 4, 48, SHAPES[0]).ratios(_faulty(kind, True))
    l1 = loss_ref("LarvaNet", (2, 1), "l1", SHAPES[0]).ratios(_faulty(kind, False))
    print("\nautograd contract defect %s: linear image %.1f, worst gradient %.1f; L1 value %.1f, image %.1f, worst gradient %.1f"
          % (kind, lin["image"], max(v for k, v in lin.items() if k.startswith("grad")), l1["value"], l1["image"],
             max(v for k, v in l1.items() if k.startswith("grad"))))
    assert lin["image"] > 1.0 and l1["image"] > 1.0 and l1["value"] > 1.0
    assert max(v for k, v in l1.items() if k.startswith("grad")) > 1.0
    if kind == "tap":   # (a shifted base leaves the gradients of a linear functional as they are: the image check sees it)
        assert lin["grad body_1.leg.recon_block.0.weight"] > 1.0
        assert sum(v > 1.0 for k, v in lin.items() if k.startswith("grad")) >= 8   # the leg and everything before it


def test_bars_reject_an_error_of_five_bars_and_no_less():
    """How tight the bars are, in their own units: a run whose loss is off by 1e-4 relative, whose image by 1e-2 and
    whose every gradient tensor by 5e-4 of itself is rejected by the loss check, by the image check and by every
    gradient tensor whose fp32 distance lies under the floor (most of them); ten times wider bars would let all of it pass."""
    ref = loss_ref("LarvaNet", (2, 1), "l1", SHAPES[0])
    r64 = ref.r64
    wrong = {"value": r64["value"] * (1 + 1e-4), "image": r64["image"] + 1e-2,   # (literals: the errors do not follow the bars)
             "grads": {k: g * (1 + 5e-4) for k, g in r64["grads"].items()}}
    r = ref.ratios(wrong)
    floor_bound = [k for k in r64["grads"] if ref.bar(k) <= 1.0001 * ref.floor * float(r64["grads"][k].abs().max())]
    assert r["value"] > 1.0 and r["image"] > 1.0
    assert len(floor_bound) >= len(r64["grads"]) // 2 and all(r["grad " + k] > 1.0 for k in floor_bound)
    print("\nautograd contract five bars: value %.2f image %.2f gradients %.2f..%.2f (%d of %d tensors at the floor)"
          % (r["value"], r["image"], min(r["grad " + k] for k in floor_bound), max(r["grad " + k] for k in floor_bound),
             len(floor_bound), len(r64["grads"])))


def test_a_frozen_parameter_ends_the_gradient_bucket():
    from larvanet_amd.autograd import GradBucket
    net = _model("LarvaNet", (1, 1)).model
    bucket = GradBucket(net, net.packed_convs())
    assert bucket.intact() and all(pc.grad_inplace for pc in net.packed_convs())
    net.body_0.res_blocks[0].body[0].bias.requires_grad_(False)
    assert not bucket.intact()
    net.body_0.res_blocks[0].body[0].bias.requires_grad_(True)
    assert bucket.intact()
    net.head.feature_extraction.weight.grad = None
    assert not bucket.intact()


# ================================================================ GPU
def _param_grads(net):
    return {k: None if p.grad is None else p.grad.detach().double().cpu() for k, p in net.named_parameters()}


def _clear(m):
    """Before a backward: the bucket zeroed where one owns the gradients, else every .grad dropped."""
    if m.grad_bucket is not None:
        assert m.grad_bucket.intact()
        m.grad_bucket.flat.zero_()
    else:
        for p in m.model.parameters():
            p.grad = None


def _outside_any_scope():
    from larvanet_amd.autograd import DeferredWgrad, StepScope
    assert StepScope.depth == 0 and StepScope.seed_grad is None and not DeferredWgrad.active


def _run_linear(m, x, c, dev, clear=True):
    if clear:
        _clear(m)
    out = m.model(x.to(dev))
    (out * c.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return {"image": out.detach().double().cpu(), "grads": _param_grads(m.model)}


@pytest.mark.gpu
@pytest.mark.parametrize("training", [False, True], ids=["autograd", "bucket"])
@pytest.mark.parametrize("case", A_CASES, ids=A_IDS)
def test_model_under_grad_with_a_linear_functional(hip_device, case, training):
    """2a: model(x) under grad, loss = (out * c).sum(): image and every parameter gradient, handed back to autograd
    (prepared for inference: no bucket) and written into the bucket views (prepared for training, no scope open)."""
    name, blocks, extra, s, nf = case
    m = _load(_model(name, blocks, s, nf, training, extra), _spec_sd(name, blocks, s, nf, extra))
    assert (m.grad_bucket is not None) == training
    _outside_any_scope()
    worst = 0.0
    for shape in SHAPES:
        got = _run_linear(m, _inputs(shape, s)[0], _coeff(shape, s), hip_device)
        worst = max(worst, linear_ref(*case, shape).check("a %s %s %s" % (A_IDS[A_CASES.index(case)],
                                                                           "bucket" if training else "autograd", shape), got))
    print("autograd contract a: worst of the three shapes %.3f" % worst)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [3, 4])
def test_autograd_accumulates_and_the_bucket_overwrites(hip_device, s):
    """Two backwards without zeroing: handed back to autograd they leave exactly 2 g (g + g is exact and the weight
    gradients are deterministic), written into the bucket they leave g (GradBucket's contract)."""
    case = ("LarvaNetV2", (1, 2), (), s, 48)
    x, c = _inputs(SHAPES[0], s)[0], _coeff(SHAPES[0], s)
    for training in (False, True):
        m = _load(_model(*case[:2], s, 48, training), _spec_sd(*case[:2], s, 48))
        once = _run_linear(m, x, c, hip_device)["grads"]
        twice = _run_linear(m, x, c, hip_device, clear=False)["grads"]
        assert sum(g is not None and bool(g.any()) for g in once.values()) == 20   # head, 3 blocks, merge conv, the tail's two
        for k in once:
            if once[k] is None:   # (the legs of the bodies are not on V2's inference route)
                assert twice[k] is None, k
            else:
                assert torch.equal(twice[k], once[k] if training else 2 * once[k]), (k, training)


def _plugin_step(m, xd, td, graph):
    m.use_hip_graph = graph
    loss, out = m._forward_backward(xd, td)
    m._finish_backward()
    torch.cuda.synchronize()
    assert m.use_hip_graph == graph and m.hip_graph_fell_back is None
    return {"value": float(loss.detach()), "image": out.detach().double().cpu(), "grads": _param_grads(m.model)}


def _eager_and_captured(m, ref, label, shape, dev):
    """One _forward_backward eagerly and as a captured step against float64, and the two against each other."""
    x, truth = _inputs(shape, 4)
    xd, td = x.to(dev), truth.to(dev)
    eager = _plugin_step(m, xd, td, False)
    ref.check(label + " eager %s" % (shape,), eager)
    _plugin_step(m, xd, td, True)              # (warm-ups, the capture, a replay)
    graph = _plugin_step(m, xd, td, True)      # a replay alone
    ref.check(label + " captured %s" % (shape,), graph)
    gl = abs(graph["value"] - eager["value"]) / abs(eager["value"])
    gg = {k: _rel(graph["grads"][k], eager["grads"][k]) for k in eager["grads"]}
    print("autograd contract %s %s: captured vs eager loss %.2e, gradients %.2e" % (label, shape, gl, max(gg.values())))
    assert gl <= LOSS_BAR and all(v <= GRAD_BAR for v in gg.values()), (label, gl, gg)


@pytest.mark.gpu
@pytest.mark.parametrize("name,blocks", B_CASES)
def test_replaced_loss_through_the_plugin(hip_device, name, blocks):
    """2b: m.loss_fn = MSELoss(): every exit is leg() + loss_fn (LegFn with torch's own gradient flowing in)."""
    m = _load(_model(name, blocks, training=True), _spec_sd(name, blocks))
    m.loss_fn = torch.nn.MSELoss()
    for shape in SHAPES[:2]:
        _eager_and_captured(m, loss_ref(name, blocks, "mse", shape), "b %s" % name, shape, hip_device)


@pytest.mark.gpu
@pytest.mark.parametrize("divisor", [None, 3])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_one_exit_unfused_with_a_seed_that_is_not_one(hip_device, s, divisor):
    """2c: run_leg(leg, fea, base, truth, divisor) outside any scope, backward seeded with 0.37.  Without a divisor the
    term is the finished L1; with one it is partial sums, finished here by torch's operators, and the node applies the
    1 / divisor in its backward."""
    from larvanet_amd.models import LarvaNet as L
    m = _load(_model("LarvaNet", (1, 1), s), _spec_sd("LarvaNet", (1, 1), s))
    leg = m.model.body_0.leg
    _outside_any_scope()
    for shape in SHAPES:
        (fea,), base, truth = _exit_inputs(shape, s)
        fd = fea.to(hip_device).requires_grad_(True)
        _clear(m)
        out, term = L.run_leg(leg, fd, base.to(hip_device), truth.to(hip_device), divisor)
        assert (term.dim() == 0) == (divisor is None)
        value = term if divisor is None else term.sum() * (1.0 / out.numel())
        value.backward(torch.tensor(0.37, device=hip_device))
        torch.cuda.synchronize()
        grads = {k: v for k, v in _param_grads(m.model).items() if k.startswith(LEG)}
        grads["fea"] = fd.grad.detach().double().cpu()
        exit_ref(s, shape, divisor).check("c x%d divisor %s %s" % (s, divisor, shape),
                                          {"value": float(value.detach()), "image": out.detach().double().cpu(), "grads": grads})


@pytest.mark.gpu
@pytest.mark.parametrize("training", [False, True], ids=["autograd", "bucket"])
@pytest.mark.parametrize("subset", ["ends", "all"])
@pytest.mark.parametrize("M", [3, 5, 9])
def test_all_exits_without_a_seed_and_with_dead_exits(hip_device, M, subset, training):
    """2d: m._all_exits outside a scope (no seed: the L1 gradient is made in backward from what autograd hands in), the
    loss built from some of the terms with unequal weights.  A dead exit gets no gradient at all: None, or the zero the
    test put into the bucket; neither do the head and the bodies, which this graph does not contain."""
    m = _load(_model("LarvaNet", (1,) * M, training=training), _spec_sd("LarvaNet", (1,) * M))
    w = exit_weights(M, subset)
    _outside_any_scope()
    for shape in SHAPES:
        feas, base, truth = _exit_inputs(shape, 4, count=M)
        fds = [f.to(hip_device).requires_grad_(True) for f in feas]
        _clear(m)
        last, terms = m._all_exits(fds, base.to(hip_device), truth.to(hip_device))
        assert len(terms) == M and all(t.prescaled for t in terms)
        value = sum(w[i] * terms[i].tensor.sum() * terms[i].scale for i in sorted(w))
        value.backward()
        torch.cuda.synchronize()
        grads = _param_grads(m.model)
        for i, f in enumerate(fds):
            assert (f.grad is None) == (i not in w), i
            grads["fea_%d" % i] = None if f.grad is None else f.grad.detach().double().cpu()
        if not training:
            dead = [k for k, g in grads.items() if g is not None and not any(k.startswith("body_%d.leg" % i) or k == "fea_%d" % i for i in w)]
            assert not dead, dead
        exits_ref(M, subset, shape).check("d M=%d %s %s %s" % (M, subset, "bucket" if training else "autograd", shape),
                                          {"value": float(value.detach()), "image": last.detach().double().cpu(), "grads": grads})


@pytest.mark.gpu
def test_l1_loss_with_a_negative_seed_and_a_sliced_output(hip_device):
    """2e: L1Loss on a non-contiguous view, backward seeded with -2.5.  The gradient is sign * g / numel: the kernel
    multiplies g by fl(1 / numel), which is g / numel rounded once when numel is a power of two (the first shape) and
    within one rounding of it otherwise (the second, a 3-channel image)."""
    from larvanet_amd.models import LarvaNet as L
    for shape, cut in (((2, 4, 16, 40), slice(4, 36)), ((1, 3, 28, 44), slice(4, 40))):
        g = torch.Generator().manual_seed(shape[1])
        big, truth = torch.rand(shape, generator=g) * 255, torch.rand(shape, generator=g)[..., cut] * 255
        bd = big.to(hip_device).requires_grad_(True)
        out = bd[..., cut]
        assert not out.is_contiguous()
        loss = L.L1Loss()(out, truth.to(hip_device))
        loss.backward(torch.tensor(-2.5, device=hip_device))
        b64 = big.double().requires_grad_(True)
        ref = F.l1_loss(b64[..., cut], truth.double())
        ref.backward(torch.tensor(-2.5, dtype=torch.float64))
        rel = abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach())
        numel = out.numel()
        got = bd.grad.cpu()
        kernel = torch.sign(b64.grad).float() * (np.float32(2.5) * (np.float32(1.0) / np.float32(numel)))
        once = b64.grad.float()
        ulp = float(np.spacing(np.float32(2.5 / numel)))
        print("\nautograd contract e %s: loss %.2e relative, gradient %.2f ulp from float64's" %
              (shape, rel, float((got - once).abs().max()) / ulp))
        assert rel <= LOSS_REL
        assert torch.equal(got, kernel)
        assert not got[..., :4].any() and not got[..., cut.stop:].any()
        if numel & (numel - 1) == 0:
            assert torch.equal(got, once)
        else:
            assert float((got - once).abs().max()) <= ulp


@pytest.mark.gpu
@pytest.mark.parametrize("batch_exits", [True, False], ids=["batched", "one_by_one"])
def test_v2_with_nine_loss_terms(hip_device, batch_exits):
    """2f: LarvaNetV2 --num_modules=8: nine loss terms, the mean's grouped-sum branch, eight prescaled partial-sum terms
    and the tail's finished scalar in one mean; with batch_exits off every exit goes through ExitFn."""
    m = _load(_model(*NINE, training=True), _spec_sd(*NINE))
    m.batch_exits = batch_exits
    for shape in SHAPES[:2]:
        _eager_and_captured(m, loss_ref(*NINE, None, shape), "f %s" % ("batched" if batch_exits else "one by one"),
                            shape, hip_device)


@pytest.mark.gpu
def test_inputs_that_need_a_gradient_are_refused_and_pass_under_no_grad(hip_device):
    """Section 3 on the device: under grad the refusal, under no_grad the same bits as for a plain tensor."""
    m = _load(_model("LarvaNet", (1, 1)), _spec_sd("LarvaNet", (1, 1)))
    x = _inputs(SHAPES[0], 4)[0].to(hip_device)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="^larvanet_amd: the gradient of the input image"):
        m.model(xg)
    with torch.no_grad():
        assert torch.equal(m.model(xg), m.model(x))
    assert xg.grad is None


# ---------------------------------------------------------------- parameters frozen after prepare(is_training=True)
def _frozen_reference(sd, x, truth, blocks, frozen, steps, lr):
    """float64: `steps` steps of torch.optim.AdamW over the parameters that are not frozen -> (losses, first gradients, sd)."""
    p = {k: v.double().clone().requires_grad_(k not in frozen) for k, v in sd.items()}
    opt = torch.optim.AdamW([v for k, v in p.items() if k not in frozen], lr=lr)
    losses, first = [], None
    for step in range(steps):
        loss = T.multi_exit_loss(p, x.double(), truth.double(), blocks)
        opt.zero_grad()
        loss.backward()
        first = first or {k: v.grad.detach().clone() for k, v in p.items() if k not in frozen}
        opt.step()
        losses.append(float(loss.detach()))
    return losses, first, {k: v.detach() for k, v in p.items()}


FROZEN = {"head": ("head.feature_extraction.weight", "head.feature_extraction.bias"),
          "one_bias": ("body_0.res_blocks.1.body.0.bias",)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(FROZEN))
def test_parameters_frozen_after_prepare_are_not_trained(hip_device, which):
    """Section 4, three eager steps.  The frozen tensors keep their bits.  Everything else against float64 AdamW over the
    same trainable set: losses 2e-5 relative and the first step's gradients within 1e-3 of each tensor's maximum (+ the
    near-tie allowance of an exit's last bias), the bars of test_scales' training step; the weights after the third step
    as test_model_parity compares trained weights: no element further than 2.1 lr from float64 (AdamW moves an element
    by about lr per step whatever the gradient's size, so an element whose gradient is within rounding of zero may go
    the other way once) and fewer than 2 in 1000 further than 2e-5."""
    blocks, shape, frozen = (2, 1), SHAPES[0], FROZEN[which]
    sd = _spec_sd("LarvaNet", blocks)
    m = _load(_model("LarvaNet", blocks, training=True), sd)
    m.use_hip_graph = False
    named = dict(m.model.named_parameters())
    for k in frozen:
        named[k].requires_grad_(False)
    x, truth = _inputs(shape, 4)
    xd, td = x.to(hip_device), truth.to(hip_device)
    lr = m.get_lr()
    ref_losses, ref_first, ref_sd = _frozen_reference(sd, x, truth, list(blocks), frozen, 3, lr)
    args = types.SimpleNamespace(train_path="/tmp")
    losses, worst = [], 0.0
    for step in range(3):
        losses.append(m.train_step_larva(args, S._NoVal(), xd, td, None))
        if step == 0:
            for k, p in named.items():
                if k in frozen:
                    assert p.grad is None, k
                    continue
                d = float((p.grad.detach().double().cpu() - ref_first[k]).abs().max())
                bar = 1e-3 * max(float(ref_first[k].abs().max()), 1e-30)
                if k.endswith("recon_block.2.bias"):
                    bar += 4.0 / (len(blocks) * truth.numel())
                worst = max(worst, d / bar)
                assert d <= bar, (k, d, bar)
    assert m.grad_bucket is None and not m.use_hip_graph
    state = {k: v.detach().cpu() for k, v in m.model.state_dict().items()}
    for k in frozen:
        assert torch.equal(state[k], sd[k]), "frozen %s moved by %g" % (k, float((state[k] - sd[k]).abs().max()))
    rel = max(abs(a - b) / abs(b) for a, b in zip(losses, ref_losses))
    far = total = 0
    dmax = 0.0
    for k in state:
        if k in frozen:
            continue
        d = (state[k].double() - ref_sd[k]).abs()
        moved = float((ref_sd[k] - sd[k].double()).abs().max())
        assert float(d.max()) <= 2.1 * lr, (k, float(d.max()), moved)
        far, total, dmax = far + int((d > 2e-5).sum()), total + d.numel(), max(dmax, float(d.max()))
    print("\nautograd contract frozen %s: losses %.2e relative, first gradients %.3f of their bar, weights after 3 steps "
          "max %.2e (lr %.1e), %d of %d further than 2e-5" % (which, rel, worst, dmax, lr, far, total))
    assert rel <= LOSS_REL, (losses, ref_losses)
    assert far < 2e-3 * total, (far, total)
