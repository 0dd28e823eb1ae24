"""The training step at batch and patch sizes past the 16 x 48 x 48 of the headline, one case per launch regime.

Which kernels a step launches depends on its shape (DualChain.wants, the persistent / 4 x 48 / per-tile choice of the
library's conv_dispatch, the batched exit-L1 launch, the flat weight-gradient grid).  Against a float64 oracle a wrong
3 x 48 tile in one of ~500 moves a weight gradient by ~0.2 %, about as much as fp32's own sign flips of near-zero ReLU
inputs and L1 differences at these sizes; so these cases are checked EXACTLY, by linearity:

* every conv tiling gives each image the same bits (strips, 3 x 48, 4 x 48, persistent: test_hip_kernels.py), so each
  image has the same activations, ReLU masks and L1 signs in whichever regime its batch lands;
* the loss of N images is the sum over sub-batches of (n_i / N) * loss_i, and so are the gradients.

Each case runs its whole batch eagerly in the regime it names and its sub-batches in the dual-chain regime that the
headline tests cover; the two agree to the summation order of the weight gradients.  The captured step on the whole
batch must agree with the eager one to the same bar.  Spies on the launch wrappers assert that the whole batch reached
the regime its case names, with the expectations derived from DualChain.max_workgroups and the device's slot count (2 x
CUs), so that a threshold change fails here instead of quietly testing another regime.  The smaller cases are also
compared with oracle/larva_torch.py in float64.

Bars, set from the measured residuals with >= 3x headroom: loss 1e-6 relative (largest measured 1.3e-7), every gradient
tensor 3e-5 of its largest element (largest measured 8.2e-6, an exit's bias gradient: sums of +-g that nearly cancel).
The captured step measured bit-identical to the eager one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_BAR = 1e-6
GRAD_BAR = 3e-5


class Case:
    def __init__(self, cid, name, blocks, n, p, parts, chains, past_slots, nf=48, aligned=True):
        self.cid, self.name, self.blocks, self.n, self.p, self.parts = cid, name, blocks, n, p, parts
        self.chains, self.past_slots, self.nf, self.aligned = chains, past_slots, nf, aligned
        assert sum(parts) == n

    @property
    def v2(self):
        return self.name == "LarvaNetV2"

    def oracle(self):
        """fp64 oracle comparison: at most ~80 k LR pixels and 2 modules (CPU time)."""
        return self.n * self.p * self.p <= 80000 and len(self.blocks) <= 2


# chains: the whole batch runs as two half-batch strip chains; past_slots: whole-batch launches of more 3 x 48 tiles than
# workgroup slots (persistent forward tiles -- 4 x 48 tiles at 32 channels -- and per-tile mask / exit / two-source launches)
CASES = [
    Case("chain_boundary", "LarvaNet", [4, 4, 4, 4], 32, 48, [16, 16], chains=True, past_slots=False),
    Case("just_past", "LarvaNet", [4, 4, 4, 4], 33, 48, [11, 11, 11], chains=False, past_slots=True),
    Case("two_rounds", "LarvaNet", [2, 1], 64, 48, [16, 16, 16, 16], chains=False, past_slots=True),
    Case("big_patch", "LarvaNet", [1, 2, 1], 16, 64, [8, 8], chains=False, past_slots=True),
    Case("bigger_patch", "LarvaNet", [2, 1], 16, 96, [8, 8], chains=False, past_slots=True),
    Case("unaligned_width", "LarvaNet", [2, 1], 12, 50, [6, 6], chains=False, past_slots=False, aligned=False),
    Case("odd_halves", "LarvaNet", [2, 1], 7, 48, [3, 4], chains=True, past_slots=False),
    Case("v2_just_past", "LarvaNetV2", [2, 1, 1], 33, 48, [11, 11, 11], chains=False, past_slots=True),
    Case("v2_big_patch", "LarvaNetV2", [2, 1, 1], 16, 64, [8, 8], chains=False, past_slots=True),
    Case("nf32_two_rounds", "LarvaNet", [2, 1], 64, 48, [16, 16, 16, 16], chains=False, past_slots=True, nf=32),
    Case("nf64_just_past", "LarvaNet", [2, 1], 33, 48, [11, 11, 11], chains=False, past_slots=True, nf=64),
]


def tiles_per_image(p):
    return ((p + 2) // 3) * ((p + 47) // 48)


def slots():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def expects_chains(n, p):
    """DualChain.wants restated from its thresholds (the strip table exists for every height used here)."""
    from larvanet_amd.autograd import DualChain
    return n >= 2 and p % 4 == 0 and n * tiles_per_image(p) <= DualChain.max_workgroups


class Spies:
    """Records every call of the launch wrappers a training step chooses between (patched on the modules the step
    reads them from, restored on exit).  `defect`: optional hooks (scratch sensitivity runs) called with a record and
    the result, which they may alter."""

    def __init__(self, defect=None):
        self.calls = []
        self.defect = defect or {}

    def __enter__(self):
        from larvanet_amd import kernels as K
        from larvanet_amd.autograd import DualChain
        self._saved = [(K, k, getattr(K, k)) for k in ("conv3x3", "conv3x3_batch", "conv3x3_exit_l1_batch",
                                                       "conv3x3_wgrad_partial_flat")]
        self._saved.append((DualChain, "conv", DualChain.__dict__["conv"]))
        conv, batch, exits, flat = (s[2] for s in self._saved[:4])
        dual = DualChain.conv

        def rec(kind, **kw):
            r = dict(kind=kind, **kw)
            self.calls.append(r)
            return r

        def first(srcs):
            return srcs if isinstance(srcs, torch.Tensor) else srcs[0]

        def conv3x3(srcs, wpk, cout, **kw):
            out = conv(srcs, wpk, cout, **kw)
            r = rec("conv", shape=tuple(first(srcs).shape), cout=cout, images=kw.get("images"),
                    strips=bool(kw.get("strips")), mask=kw.get("mask") is not None, shuffle=bool(kw.get("shuffle")),
                    nsrc=1 if isinstance(srcs, torch.Tensor) else len(srcs))
            if "conv" in self.defect:
                self.defect["conv"](r, out)
            return out

        def conv3x3_batch(jobs, cout, **kw):
            rec("batch", shape=tuple(first(jobs[0]["srcs"]).shape), cout=cout, njobs=len(jobs),
                mask=jobs[0].get("mask") is not None)
            return batch(jobs, cout, **kw)

        def conv3x3_exit_l1_batch(jobs, cout, *a, **kw):
            res = exits(jobs, cout, *a, **kw)
            r = rec("exits", shape=tuple(first(jobs[0]["srcs"]).shape), cout=cout, njobs=len(jobs), none=res is None)
            if "exits" in self.defect and res is not None:
                self.defect["exits"](r, res)
            return res

        def conv3x3_wgrad_partial_flat(jobs, cout, cin, nwg, head=None):
            res = flat(jobs, cout, cin, nwg, head=head)
            rec("flat", shape=tuple(jobs[0]["dy"].shape), cout=cout, cin=cin, njobs=len(jobs), head=head is not None,
                none=res is None)
            return res

        def dual_conv(cls, srcs, wpk, cout, forward=False, **kw):
            n, _, h, p = (int(v) for v in first(srcs).shape)
            rec("dual", shape=(n, h, p), wants=cls.wants(n, h, p), mask=kw.get("mask") is not None)
            return dual(srcs, wpk, cout, forward=forward, **kw)

        K.conv3x3, K.conv3x3_batch = conv3x3, conv3x3_batch
        K.conv3x3_exit_l1_batch, K.conv3x3_wgrad_partial_flat = conv3x3_exit_l1_batch, conv3x3_wgrad_partial_flat
        DualChain.conv = classmethod(dual_conv)
        return self

    def __exit__(self, *exc):
        for owner, k, v in self._saved:
            setattr(owner, k, v)
        return False

    def of(self, kind, **match):
        return [c for c in self.calls if c["kind"] == kind and all(c.get(k) == v for k, v in match.items())]


def _model(case, seed=0):
    import importlib
    m = importlib.import_module("larvanet_amd.models." + case.name).create_model()
    m.parse_args(["--num_modules=%d" % len(case.blocks), "--num_blocks=%s" % ",".join(map(str, case.blocks)),
                  "--num_filters=%d" % case.nf])
    torch.manual_seed(seed)
    m.prepare(is_training=True, scales=[4])
    return m


def _batch(case):
    g = torch.Generator().manual_seed(1000 + case.n * 7 + case.p)
    x = torch.rand(case.n, 3, case.p, case.p, generator=g) * 255
    truth = torch.rand(case.n, 3, 4 * case.p, 4 * case.p, generator=g) * 255
    return x, truth


def _step(m, x, truth, graph=False):
    """(loss, {name: grad}) of one forward + backward, float64 copies on the host."""
    m.use_hip_graph = graph
    loss, _ = m._forward_backward(x, truth)
    m._finish_backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu() for k, p in m.model.named_parameters()}
    return float(loss.detach()), grads


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def check_regime(case, spies, n):
    """What the case's label says about the step on `n` images, asserted from the recorded launches."""
    p, tiles = case.p, n * tiles_per_image(case.p)
    chains = expects_chains(n, p)
    dual = spies.of("dual")
    assert dual and all(c["wants"] == chains for c in dual), (case.cid, n, "DualChain.wants disagrees with its thresholds")
    strips = [c for c in spies.of("conv") if c["strips"]]
    if chains:
        half = n // 2
        assert strips, (case.cid, n, "no strip launch")
        assert {c["images"] for c in strips} == {(0, half), (half, n)}, (case.cid, n)
    else:
        assert not strips and all(c["images"] is None for c in spies.of("conv")), (case.cid, n, "a strip / range launch")
        whole_mask = spies.of("conv", mask=True, images=None)
        assert [c for c in whole_mask if c["shape"][0] == n], (case.cid, n, "no whole-batch mask launch")
        if tiles > slots():
            assert any(c["shape"][0] * tiles_per_image(p) > slots() for c in whole_mask)
    if case.v2:   # the tail's merge conv over the M body outputs as one multi-source launch on the whole batch
        assert spies.of("conv", nsrc=len(case.blocks), images=None), (case.cid, n, "no merge launch")
    # the flat grid exists for the square body shapes (the head riding on a 48-channel grid); the others go per layer
    flat = [c for c in spies.of("flat") if c["cout"] == c["cin"] == case.nf]
    assert flat, (case.cid, n, "no flat weight-gradient call")
    assert all(c["none"] == (not case.aligned) for c in flat), (case.cid, n, [c["none"] for c in flat])
    if case.nf == 48:
        assert any(c["head"] and not c["none"] for c in flat) == case.aligned, (case.cid, n, "the head's ride on the flat grid")
    exits = spies.of("exits")
    if case.nf == 48:
        assert exits and all(c["none"] == (not case.aligned) for c in exits), (case.cid, n, exits)


@pytest.mark.parametrize("case", CASES, ids=[c.cid for c in CASES])
def test_training_step_regime_decomposes_into_dual_chain_sub_batches(hip_device, case):
    """The whole batch in the regime the case names vs the n_i / N-weighted sum of its sub-batches (eager), and the
    captured step on the whole batch vs the eager one: loss and every gradient element."""
    from larvanet_amd.autograd import DualChain
    tiles = case.n * tiles_per_image(case.p)
    # the labels against the thresholds they were written for: a changed threshold fails here, loudly
    assert expects_chains(case.n, case.p) == case.chains, (case.cid, tiles, DualChain.max_workgroups)
    assert (tiles > slots() and not case.chains) == case.past_slots, (case.cid, tiles, slots())
    assert (case.p % 4 == 0) == case.aligned
    assert all(expects_chains(k, case.p) == case.aligned for k in case.parts), "sub-batches of an aligned case run as two chains"

    m = _model(case)
    x, truth = _batch(case)
    x, truth = x.to(hip_device), truth.to(hip_device)
    with Spies() as spies:
        loss, grads = _step(m, x, truth)
    check_regime(case, spies, case.n)

    sum_loss, sum_grads, lo = 0.0, {k: torch.zeros_like(v) for k, v in grads.items()}, 0
    for k in case.parts:
        with Spies() as sub:
            li, gi = _step(m, x[lo:lo + k].contiguous(), truth[lo:lo + k].contiguous())
        check_regime(case, sub, k)
        w = k / case.n
        sum_loss += w * li
        for name in sum_grads:
            sum_grads[name] += w * gi[name]
        lo += k

    _step(m, x, truth, graph=True)            # capture (two eager warm-ups, the capture, a replay) ...
    g_loss, g_grads = _step(m, x, truth, graph=True)   # ... and a replay of the captured step alone
    assert m.use_hip_graph and m.hip_graph_fell_back is None

    dec = {k: _rel(sum_grads[k], grads[k]) for k in grads}
    gra = {k: _rel(g_grads[k], grads[k]) for k in grads}
    dl, gl = abs(sum_loss - loss) / abs(loss), abs(g_loss - loss) / abs(loss)
    worst_d, worst_g = max(dec, key=dec.get), max(gra, key=gra.get)
    print("\nregime %s n=%d p=%d tiles=%d: decomposition loss %.2e grad %.2e (%s); graph loss %.2e grad %.2e (%s)"
          % (case.cid, case.n, case.p, tiles, dl, dec[worst_d], worst_d, gl, gra[worst_g], worst_g))
    assert dl <= LOSS_BAR, (case.cid, loss, sum_loss)
    assert gl <= LOSS_BAR, (case.cid, loss, g_loss)
    for k in grads:
        assert dec[k] <= GRAD_BAR, (case.cid, "decomposition", k, dec[k])
        assert gra[k] <= GRAD_BAR, (case.cid, "graph vs eager", k, gra[k])


ORACLE_CASES = [c for c in CASES if c.oracle()]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.cid for c in ORACLE_CASES])
def test_training_step_regime_against_the_float64_oracle(hip_device, case):
    """Loss (2e-5 relative) and every gradient against oracle/larva_torch.py in float64: per tensor within 3x the
    distance of torch's own fp32 CPU run from float64, with a floor of 1e-4 of the tensor's maximum at 48 channels and
    5e-4 at 32 / 64 (the bar test_headline_parity.py uses at those widths).  A ReLU input or an L1 difference within
    fp32 rounding of zero, on one side of it in one run and on the other in the other, moves one row of that layer's
    weight gradient and, through the input gradient, every layer before it: at 64 channels two leg-mask rows and one
    L1-sign row put this run 3.3e-4 of a maximum from float64, while torch's fp32 run met fewer such flips.  The exact
    check of these regimes is the decomposition above.  upscale() of the batch against the oracle forward within 2e-3."""
    from oracle import larva_torch as T
    m = _model(case)
    sd = {k: v.detach().cpu().clone() for k, v in m.model.state_dict().items()}
    x, truth = _batch(case)
    loss, grads = _step(m, x.to(hip_device), truth.to(hip_device))
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))

    def cpu(dtype):
        sdr = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        ref = T.multi_exit_loss(sdr, x.to(dtype), truth.to(dtype), case.blocks, v2=case.v2)
        ref.backward()
        return float(ref.detach()), {k: v.grad.double() for k, v in sdr.items()}

    l64, g64 = cpu(torch.float64)
    _, g32 = cpu(torch.float32)
    assert abs(loss - l64) <= 2e-5 * abs(l64), (case.cid, loss, l64)
    worst = 0.0
    for k in g64:
        scale = max(float(g64[k].abs().max()), 1e-30)
        bar = max(3 * float((g32[k] - g64[k]).abs().max()), (1e-4 if case.nf == 48 else 5e-4) * scale)
        d = float((grads[k] - g64[k]).abs().max())
        worst = max(worst, d / bar)
        assert d <= bar, (case.cid, k, d, bar)
    got = m.upscale([im.numpy() for im in x], 4)
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        ref = (T.forward_v2(sd64, x.double(), case.blocks) if case.v2 else T.forward(sd64, x.double(), case.blocks)).numpy()
    fwd = float(np.abs(got - ref).max())
    print("\noracle %s: loss %.2e rel, worst gradient %.2f of its bar, forward %.2e" % (case.cid, abs(loss - l64) / abs(l64),
                                                                                      worst, fwd))
    assert fwd <= 2e-3, (case.cid, fwd)
