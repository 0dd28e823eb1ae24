"""Networks and launches past the per-launch job caps, the default depth (--num_blocks=16,16) included.

Caps: 64 jobs per larva_pack_weights_batch / larva_step_prologue / larva_conv3x3_wgrad[_partial[_flat[_head]]] /
larva_wgrad_reduce[_with_loss] launch, 8 jobs per fp16 job launch, 8 terms per loss launch, 2..4 jobs per batched conv
or exit launch.  The Python side chunks around them (kernels.pack_weights_batch, autograd.step_prologue,
DeferredWgrad._launches / _issue, half.HalfForward.exits, LarvaNetModule.forward_exits); every other file of the suite
stays below every cap.  Section A fills the 64-entry argument tables of the entry points and goes one past them,
section B trains tiny steps of networks whose depth is past the caps, section C runs nine exits.

Bars, where each comes from, and the largest residual measured on the MI355X:

* section A: none.  Integer data (tests/exact_ref.py): every result equals the float64 sum bit for bit, a chunked call
  equals the small calls bit for bit.
* section B, first reference = the same plugin with per-node weight gradients (defer_wgrad off: at most 16 layers per
  launch, no cap is met).  Step 1 starts from the same weights, and step 2 of the reference starts from the weights the
  deferred run holds after its first AdamW step, so activations, masks and L1 signs are the same bits in both runs:
  the loss must be EQUAL; every gradient tensor within GRAD_BAR = 3e-5 of its own largest element
  (tests/test_train_regimes.py: summation order of the weight gradients); no tensor all zero or non-finite.
  Measured: the loss equal in all 12 cases and both steps; at (2, 8, 8) the worst tensor 0.008 .. 0.011 of GRAD_BAR
  (3.3e-7 of its largest element: LarvaNet 32,32, body_1.res_blocks.23.body.2.weight); at (1, 7, 9) every gradient
  EQUAL (three tiles per layer: both paths cut them into the same partial images).  GRAD_BAR holds at this depth with
  90x headroom, so it is not re-derived.  The weights after the second AdamW step: the two runs' moments differ by
  the step-1 gradients' summation order, so the bar is the one tests/test_autograd_contract.py and
  tests/test_model_parity.py use for trained weights: no element further than 2.1 lr, fewer than 2 in 1000 further
  than 2e-5.  Measured: at most 0.007 of 2.1 lr, no element further than 2e-5.
* the captured step against the eager one: EQUAL (loss, gradients, weights after two steps), the project's rule.
  Measured: equal in all 12 cases.
* the split flush (jobs_per_launch = 32) against the same two references with the same bars.  Measured: the loss equal,
  the worst tensor 0.007 of GRAD_BAR (the head's weight, which rides on another grid than in the reference), the
  weights 0.007 of 2.1 lr.
* section B, second reference = oracle/larva_torch.py in float64 with torch's AdamW between the steps, bars of
  tests/test_autograd_contract.py: loss 2e-5 relative; per gradient tensor max(3 |fp32 CPU - fp64|, 1e-4 max|g64|);
  the weights as above.  The CPU tests show that torch's own fp32 run stays inside every bar on these inputs (worst
  0.178 of a bar) and that the bars reject a float64 run whose layers past the 64th have no gradient (every such
  tensor at 10 000 bars).  Measured on the device: step 1 at most 0.014 of a bar, step 2 at most 0.254 (LarvaNet 15,15
  at (1, 7, 9), body_1.res_blocks.9.body.0.weight; the default depth 0.089), the weights 0.014 of 2.1 lr and no
  element further than 2e-5.
* inference at the default depth: float images 2e-3 on the 0..255 scale, uint8 at most one level on at most 0.1 % of
  the bytes (tests/test_interleaved_shapes.py); measured 4.4e-5 (0.022 of the bar) and 0 of 16 848 bytes, both models;
  torch's fp32 CPU run 4.3e-5 and 0 bytes.  fp16: the quality bar of tests/test_half_infer.py (|dPSNR| <= 0.02 dB,
  max |d| <= 0.25, mean |d| <= 0.03 against the fp32 run of the same trained weights); measured at most 0.085 of it
  (LarvaNet 12 x 24: 0.0017 dB, max |d| 0.0103, mean |d| 0.0019).
* section C: every exit EQUAL to its LarvaLeg --leg=k plugin (tests/test_all_exits.py).  Measured: equal.

Every GPU test prints its worst ratio to its bar.  On one MI355X the 99 tests of the file take 28 s, the longest 1.4 s."""
import ctypes
import functools
import gc
import importlib

import numpy as np
import pytest
import torch

from oracle import larva_torch as T

import exact_ref as X
import test_autograd_contract as AC
from test_train_regimes import GRAD_BAR, LOSS_BAR, _rel

gpu = pytest.mark.gpu

PACK_CAP = 64        # kMaxPackJobs (larva_pack_weights_batch, larva_step_prologue)
REDUCE_CAP = 64      # kMaxReduceJobs (larva_wgrad_reduce, larva_wgrad_reduce_with_loss)
INVALID = 1          # hipErrorInvalidValue


# A plugin holds its captured graphs in reference cycles, and a graph freed by the collector while another one is being
# captured aborts the process (tests/test_interleaved_shapes.py): the collector runs between the tests of this file only.
@pytest.fixture(scope="module", autouse=True)
def _nothing_dropped_earlier_is_left():
    gc.collect()
    yield


@pytest.fixture(autouse=True)
def _the_collector_runs_between_tests_only(_nothing_dropped_earlier_is_left):
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        gc.collect()
        if was:
            gc.enable()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pattern(shape, dev, value=-7.0):
    return torch.full(shape, value, device=dev, dtype=torch.float32)


def _untouched(t, value=-7.0):
    return bool((t == value).all())


class LibSpy:
    """Counts the calls of one entry point of the library object (kernels._launch looks it up on every call) and keeps
    the value of one integer argument of each."""

    def __init__(self, monkeypatch, name, arg):
        from larvanet_amd import hip_lib
        lib = hip_lib.load()
        real = getattr(lib, name)
        self.seen = []

        def spy(*args):
            self.seen.append(int(args[arg]))
            return real(*args)
        monkeypatch.setattr(lib, name, spy, raising=False)


# =====================================================================================================================
# A. kernel entry points at the cap and one past it (integer data, bit for bit)
# =====================================================================================================================
# (cout, channels of the slice, cin_total, cin_off, cin_pad): square shapes, slices of a merge conv's weight, the padded
# heads, the legs' last conv at 32 / 64 filters
PACK_KINDS = [(48, 48, 48, 0, None), (48, 48, 144, 48, None), (32, 32, 32, 0, None), (64, 64, 64, 0, None), (48, 3, 3, 0, 16),
              (48, 48, 432, 384, None), (48, 32, 32, 0, None), (48, 48, 96, 0, None), (64, 3, 3, 0, 16), (48, 64, 64, 0, None),
              (32, 32, 96, 64, None)]


def _pack_jobs(n, dev, seed=0):
    """n pack jobs over PACK_KINDS with integer weights; both images of every job pre-filled with a pattern."""
    from larvanet_amd import kernels as K
    rng = X.rng_of(n, seed)
    jobs = []
    for j in range(n):
        cout, cin, total, off, pad = PACK_KINDS[j % len(PACK_KINDS)]
        w = _dev(X.ints(rng, (cout, total, 3, 3), 1000), dev)
        cin_k = pad or cin
        fwd = _pattern((K.packed_weight_floats(cout, cin_k),), dev)
        bwd = None if pad is not None else _pattern((K.packed_weight_floats(cin_k, cout),), dev)
        jobs.append((w, fwd, bwd, cout, cin_k, off))
    return jobs


def _pack_one_by_one(jobs):
    """larva_pack_weights (the entry point of kernels.pack_weights) on every job, into pre-filled images of its own."""
    from larvanet_amd import kernels as K
    out = []
    for (w, fwd, bwd, cout, cin_k, off) in jobs:
        f, b = _pattern(fwd.shape, w.device), None if bwd is None else _pattern(bwd.shape, w.device)
        K._launch("larva_pack_weights", w.data_ptr(), f.data_ptr(), None if b is None else b.data_ptr(), cout, cin_k,
                  int(w.shape[1]), off)
        out.append((f, b))
    return out


def _assert_packed(jobs, refs, what):
    for j, ((_, fwd, bwd, *_), (f, b)) in enumerate(zip(jobs, refs)):
        assert not _untouched(f), "%s: the reference of job %d was not written" % (what, j)
        X.assert_bits_equal(fwd, f, "%s job %d forward image" % (what, j))
        if bwd is not None:
            X.assert_bits_equal(bwd, b, "%s job %d backward image" % (what, j))


@gpu
@pytest.mark.parametrize("njobs", [64, 65, 128, 130])
def test_pack_weights_batch_at_and_past_64_jobs_equals_pack_weights(hip_device, monkeypatch, njobs):
    """kernels.pack_weights_batch: one launch per 64 jobs (64 -> 1, 65 and 128 -> 2, 130 -> 3), every image of every
    job the one larva_pack_weights makes of that job."""
    from larvanet_amd import kernels as K
    jobs = _pack_jobs(njobs, hip_device)
    spy = LibSpy(monkeypatch, "larva_pack_weights_batch", 7)
    K.pack_weights_batch(jobs)
    torch.cuda.synchronize()
    want = [min(PACK_CAP, njobs - i) for i in range(0, njobs, PACK_CAP)]
    assert spy.seen == want, (spy.seen, want)
    _assert_packed(jobs, _pack_one_by_one(jobs), "pack_weights_batch of %d jobs" % njobs)
    print("\njob caps: pack_weights_batch %d jobs in launches of %s, every image equal (0 of its bar: exact)" % (njobs, spy.seen))


@gpu
def test_pack_entry_point_refuses_65_jobs_and_writes_nothing(hip_device):
    from larvanet_amd import hip_lib, kernels as K
    jobs = _pack_jobs(PACK_CAP + 1, hip_device)
    code = hip_lib.load().larva_pack_weights_batch(*K._pack_job_args(jobs), K._stream())
    torch.cuda.synchronize()
    assert code == INVALID, code
    assert all(_untouched(f) and (b is None or _untouched(b)) for (_, f, b, *_) in jobs)
    x = _dev(X.ints(X.rng_of(3), (2, 3, 8, 8), 255, lo=0), hip_device)
    x16, base = _pattern((2, 16, 8, 8), hip_device), _pattern((2, 3, 32, 32), hip_device)
    code = hip_lib.load().larva_step_prologue(*K._pack_job_args(jobs), x.data_ptr(), x16.data_ptr(), base.data_ptr(), 2, 3, 8, 8,
                                              K._stream())
    torch.cuda.synchronize()
    assert code == INVALID, code
    assert _untouched(x16) and _untouched(base) and all(_untouched(f) for (_, f, *_) in jobs)
    with pytest.raises(RuntimeError, match="at most 64 pack jobs"):
        K.step_prologue(jobs, x, x16, base)
    assert _untouched(x16) and _untouched(base)


@gpu
@pytest.mark.parametrize("shape", [(2, 8, 8), (1, 7, 9)], ids=["2x8x8", "1x7x9"])
def test_step_prologue_with_64_jobs_equals_its_three_launches(hip_device, monkeypatch, shape):
    """larva_step_prologue with a full job table against pack_weights_batch, the padded copy and bicubic4."""
    from larvanet_amd import kernels as K
    n, h, w = shape
    got_jobs, ref_jobs = _pack_jobs(PACK_CAP, hip_device, seed=1), _pack_jobs(PACK_CAP, hip_device, seed=1)
    x = _dev(X.ints(X.rng_of(n, h, w), (n, 3, h, w), 255, lo=0), hip_device)
    x16 = torch.zeros((n, 16, h, w), device=hip_device)
    base = _pattern((n, 3, 4 * h, 4 * w), hip_device)
    spy = LibSpy(monkeypatch, "larva_step_prologue", 7)
    K.step_prologue(got_jobs, x, x16, base)
    K.pack_weights_batch(ref_jobs)
    ref_base = K.bicubic4(x)
    torch.cuda.synchronize()
    assert spy.seen == [PACK_CAP]
    _assert_packed(got_jobs, [(f, b) for (_, f, b, *_) in ref_jobs], "step_prologue of 64 jobs")
    _assert_packed(got_jobs, _pack_one_by_one(got_jobs), "step_prologue of 64 jobs against larva_pack_weights")
    X.assert_bits_equal(base, ref_base, "the base image of the prologue")
    X.assert_bits_equal(x16[:, :3].contiguous(), x, "the padded input of the prologue")
    assert not bool(x16[:, 3:].any())
    print("\njob caps: step_prologue 64 jobs %s equal to its three launches (exact)" % (shape,))


# ---------------------------------------------------------------- weight gradients
def _wgrad_layers(njobs, n, cout, cin, valid, h, w, dev, seed=0):
    """njobs layers drawn on the device: integers in [-2, 2]; x has `cin` channels of which the first `valid` are
    non-zero (the head: 3 of 16); dw / db pre-filled with NaN."""
    gen = torch.Generator(device=dev).manual_seed(1000 * njobs + 100 * cout + 10 * h + w + seed)

    def draw(*shape):
        return torch.randint(-2, 3, shape, generator=gen, device=dev).float()
    jobs = []
    for _ in range(njobs):
        x = torch.zeros(n, cin, h, w, device=dev)
        x[:, :valid] = draw(n, valid, h, w)
        jobs.append({"dy": draw(n, cout, h, w), "x": x, "dw": torch.full((cout, valid, 3, 3), float("nan"), device=dev),
                     "db": torch.full((cout,), float("nan"), device=dev), "cin_off": 0, "cin_valid": valid})
    return jobs


def _check_layers(jobs, what):
    """dw and db of every layer against the float64 sums, bit for bit (preconditions first)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for i, j in enumerate(jobs):
        valid = int(j["cin_valid"])
        dw, db, inter = X.wgrad(j["dy"].cpu().numpy(), j["x"][:, :valid].cpu().numpy())
        X.assert_exact_precondition(inter)
        X.assert_bits_equal(j["dw"], dw, "%s layer %d dw" % (what, i))
        X.assert_bits_equal(j["db"], db, "%s layer %d db" % (what, i))


def _refill(jobs):
    for j in jobs:
        j["dw"].fill_(float("nan"))
        j["db"].fill_(float("nan"))


FLAT_CASES = [(48, 256, False, (2, 8, 8)), (48, 256, True, (2, 8, 8)), (48, 7, False, (2, 8, 8)), (48, 7, True, (2, 8, 8)),
              (32, 256, False, (2, 8, 8)), (32, 7, False, (2, 8, 8)), (64, 256, False, (2, 8, 8)), (64, 7, False, (2, 8, 8)),
              (48, 256, True, (1, 4, 48)), (48, 7, True, (1, 7, 48))]


@gpu
@pytest.mark.parametrize("c,nwg,head,shape", FLAT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_flat_weight_gradient_grid_with_64_layers(hip_device, c, nwg, head, shape):
    """larva_conv3x3_wgrad_partial_flat[_head] with njobs = 64 (every entry of WgradBatch::job and first_wg filled):
    nwg = 256 gives shares of one or two tiles, nwg = 7 one share over about ten layers; every layer's dw and db, the
    head's included, equal the float64 sums; splits_out stays within larva_wgrad_flat_max_splits."""
    from larvanet_amd import hip_lib, kernels as K
    n, h, w = shape
    jobs = _wgrad_layers(64, n, c, c, c, h, w, hip_device)
    hd = _wgrad_layers(1, n, 48, 16, 3, h, w, hip_device, seed=5)[0] if head else None
    res = K.conv3x3_wgrad_partial_flat(jobs, c, c, nwg, head=hd)
    assert res is not None, "the flat launch must apply at this shape"
    parts, splits = res
    tiles = n * ((h + 2) // 3) * ((w + 47) // 48)
    cap = int(hip_lib.load().larva_wgrad_flat_max_splits(64, nwg, tiles))
    assert len(splits) == 64 + bool(head) and all(1 <= s <= cap for s in splits[:64]), (splits, cap)
    if head:
        assert 1 <= splits[-1] <= int(hip_lib.load().larva_wgrad_flat_head_splits(64, nwg, tiles))
    rj = [dict(j, partial=p, splits=s, cout=c, cin=c) for j, p, s in zip(jobs, parts, splits)]
    K.wgrad_reduce(rj)                                         # 64 reduce jobs: the cap
    if head:
        K.wgrad_reduce([dict(hd, partial=parts[-1], splits=splits[-1], cout=48, cin=16)])
    torch.cuda.synchronize()
    _check_layers(jobs + ([hd] if head else []), "flat grid %s" % ((c, nwg, head, shape),))
    print("\njob caps: flat grid c=%d nwg=%d head=%s %s: 64 layers exact, splits %d..%d (cap %d)"
          % (c, nwg, head, shape, min(splits[:64]), max(splits[:64]), cap))


@gpu
@pytest.mark.parametrize("head", [False, True])
def test_flat_entry_points_refuse_65_layers_before_any_launch(hip_device, head):
    from larvanet_amd import hip_lib, kernels as K
    lib = hip_lib.load()
    n, h, w, njobs = 2, 8, 8, 65
    jobs = _wgrad_layers(2, n, 48, 48, 48, h, w, hip_device)
    nfl = K.wgrad_partial_floats(48, 48, int(lib.larva_wgrad_flat_max_splits(njobs, 256, 6)))
    parts = [_pattern((nfl,), hip_device) for _ in range(2)]
    dys = hip_lib.ptr_array([jobs[i % 2]["dy"].data_ptr() for i in range(njobs)])
    xs = hip_lib.ptr_array([jobs[i % 2]["x"].data_ptr() for i in range(njobs)])
    ps = hip_lib.ptr_array([parts[i % 2].data_ptr() for i in range(njobs)])
    used = (ctypes.c_int * njobs)(*([-5] * njobs))
    if head:
        hd = _wgrad_layers(1, n, 48, 16, 3, h, w, hip_device)[0]
        hpart, hused = _pattern((K.wgrad_partial_floats(48, 16, 64),), hip_device), ctypes.c_int(-5)
        code = lib.larva_conv3x3_wgrad_partial_flat_head(dys, xs, ps, njobs, hd["dy"].data_ptr(), hd["x"].data_ptr(),
                                                         hpart.data_ptr(), 256, n, h, w, used, ctypes.byref(hused), K._stream())
        assert hused.value == -5 and _untouched(hpart)
    else:
        code = lib.larva_conv3x3_wgrad_partial_flat(dys, xs, ps, njobs, 256, n, 48, 48, h, w, used, K._stream())
    torch.cuda.synchronize()
    assert code == INVALID, code
    assert list(used) == [-5] * njobs and all(_untouched(p) for p in parts)
    # the wrapper: no flat launch for 65 layers (the caller would go per layer, which refuses them too)
    many = [jobs[i % 2] for i in range(njobs)]
    assert K.conv3x3_wgrad_partial_flat(many, 48, 48, 256) is None


WGRAD_CASES = [(48, 48, 48, (2, 8, 8)), (48, 48, 48, (1, 7, 9)), (48, 16, 3, (1, 7, 9)), (32, 32, 32, (2, 5, 6))]


@gpu
@pytest.mark.parametrize("cout,cin,valid,shape", WGRAD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_wgrad_and_wgrad_partial_with_64_jobs(hip_device, cout, cin, valid, shape):
    """larva_conv3x3_wgrad and larva_conv3x3_wgrad_partial + larva_wgrad_reduce with 64 jobs each, W % 4 == 0 and the
    narrow walk (W = 9, W = 6): every layer exact.  65 jobs are refused by the wrappers and by the entry points."""
    from larvanet_amd import hip_lib, kernels as K
    n, h, w = shape
    jobs = _wgrad_layers(K.max_wgrad_jobs(), n, cout, cin, valid, h, w, hip_device)
    assert len(jobs) == 64
    K.conv3x3_wgrad(jobs, cout, cin, 3)
    torch.cuda.synchronize()
    _check_layers(jobs, "conv3x3_wgrad of 64 jobs %s" % ((cout, cin, shape),))
    _refill(jobs)
    parts, used = K.conv3x3_wgrad_partial(jobs, cout, cin, 2)
    assert 1 <= used <= 2
    K.wgrad_reduce([dict(j, partial=p, splits=used, cout=cout, cin=cin) for j, p in zip(jobs, parts)])
    torch.cuda.synchronize()
    _check_layers(jobs, "conv3x3_wgrad_partial of 64 jobs + reduce %s" % ((cout, cin, shape),))
    # one past
    _refill(jobs)
    many = jobs + jobs[:1]
    with pytest.raises(RuntimeError, match="wgrad jobs per call"):
        K.conv3x3_wgrad(many, cout, cin, 3)
    with pytest.raises(RuntimeError, match="wgrad jobs per call"):
        K.conv3x3_wgrad_partial(many, cout, cin, 2)
    lib = hip_lib.load()
    nfl = K.wgrad_partial_floats(cout, cin, 2)
    scratch = [_pattern((nfl,), hip_device) for _ in many]
    dys, xs = hip_lib.ptr_array([j["dy"].data_ptr() for j in many]), hip_lib.ptr_array([j["x"].data_ptr() for j in many])
    ps = hip_lib.ptr_array([p.data_ptr() for p in scratch])
    seen = ctypes.c_int(-5)
    code = lib.larva_conv3x3_wgrad_partial(dys, xs, ps, 65, 2, n, cout, cin, h, w, ctypes.byref(seen), K._stream())
    assert code == INVALID and seen.value == -5, (code, seen.value)
    code = lib.larva_conv3x3_wgrad(dys, xs, ps, hip_lib.ptr_array([j["dw"].data_ptr() for j in many]),
                                   hip_lib.ptr_array([j["db"].data_ptr() for j in many]), hip_lib.int_array([0] * 65),
                                   hip_lib.int_array([valid] * 65), hip_lib.int_array([valid] * 65), 65, 2, n, cout, cin, h, w,
                                   K._stream())
    torch.cuda.synchronize()
    assert code == INVALID, code
    assert all(_untouched(p) for p in scratch)
    assert all(bool(torch.isnan(j["dw"]).all()) and bool(torch.isnan(j["db"]).all()) for j in jobs)
    print("\njob caps: wgrad / wgrad_partial 64 jobs %s exact, 65 refused" % ((cout, cin, valid, shape),))


# groups of the mixed reduction: (cout, cin, valid, layers, splits asked)
REDUCE_GROUPS = [(48, 48, 48, 24, 4), (48, 48, 48, 16, 1), (48, 16, 3, 1, 2), (32, 32, 32, 12, 3), (64, 64, 64, 11, 2)]


def _mixed_reduce_jobs(dev):
    """64 reduce jobs of mixed kernel shapes and split counts in an interleaved order, their partial images made by
    larva_conv3x3_wgrad_partial, and a second set of destinations for the small calls."""
    from larvanet_amd import kernels as K
    n, h, w = 2, 8, 8
    jobs = []
    for g, (cout, cin, valid, count, splits) in enumerate(REDUCE_GROUPS):
        layers = _wgrad_layers(count, n, cout, cin, valid, h, w, dev, seed=g)
        parts, used = K.conv3x3_wgrad_partial(layers, cout, cin, splits)
        assert used == splits
        jobs += [dict(j, partial=p, splits=used, cout=cout, cin=cin) for j, p in zip(layers, parts)]
    assert len(jobs) == REDUCE_CAP
    order = np.random.default_rng(11).permutation(len(jobs))
    jobs = [jobs[i] for i in order]
    twin = [dict(j, dw=torch.full_like(j["dw"], float("nan")), db=torch.full_like(j["db"], float("nan"))) for j in jobs]
    return jobs, twin


def _loss_terms(dev):
    """Eight terms (the cap of a loss launch): partial-sum vectors of integers and two scalars, scales powers of two."""
    terms = [_dev(X.ints(X.rng_of(7, i), (64 - 5 * i,), 1000, lo=0), dev) for i in range(6)]
    terms += [torch.tensor(3.0, device=dev), torch.tensor(40.0, device=dev)]
    return terms, [0.25, 0.5, 1.0, 0.25, 0.5, 1.0, 1.0, 2.0], 8.0


@gpu
@pytest.mark.parametrize("with_loss", [False, True], ids=["plain", "with_loss"])
def test_wgrad_reduce_with_64_mixed_jobs_equals_small_calls(hip_device, with_loss):
    """larva_wgrad_reduce[_with_loss] over 64 jobs of four kernel shapes ((48, 16) included) and four split counts
    against the same partial images reduced in calls of 7 jobs, and against the float64 sums; the loss of the launch
    against loss_from_partials.  All bit for bit."""
    from larvanet_amd import kernels as K
    jobs, twin = _mixed_reduce_jobs(hip_device)
    loss = None
    if with_loss:
        terms, scales, divisor = _loss_terms(hip_device)
        loss = torch.full((), float("nan"), device=hip_device)
        K.wgrad_reduce(jobs, loss=(terms, scales, divisor, loss))
    else:
        K.wgrad_reduce(jobs)
    for i in range(0, len(twin), 7):
        K.wgrad_reduce(twin[i:i + 7])
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(jobs, twin)):
        X.assert_bits_equal(a["dw"], b["dw"].cpu().numpy(), "64-job reduce against small calls, job %d dw" % i)
        X.assert_bits_equal(a["db"], b["db"].cpu().numpy(), "64-job reduce against small calls, job %d db" % i)
    _check_layers(jobs, "64-job reduce")
    if with_loss:
        want = K.loss_from_partials(terms, scales, divisor)
        X.assert_bits_equal(loss, want.cpu().numpy(), "the loss of the 64-job reduce launch")
        exact = sum(s * float(t.double().sum()) for t, s in zip(terms, scales)) / divisor
        assert float(loss) == exact, (float(loss), exact)       # (integers times powers of two: exact in fp32)
    print("\njob caps: wgrad_reduce 64 mixed jobs %s: equal to the small calls and to float64 (exact)"
          % ("with the loss" if with_loss else "without a loss"))


@gpu
def test_wgrad_reduce_refuses_65_jobs_and_writes_nothing(hip_device):
    from larvanet_amd import hip_lib, kernels as K
    jobs, _ = _mixed_reduce_jobs(hip_device)
    many = jobs + [dict(jobs[0], dw=torch.full_like(jobs[0]["dw"], float("nan")), db=torch.full_like(jobs[0]["db"], float("nan")))]
    loss = torch.full((), float("nan"), device=hip_device)
    terms, scales, divisor = _loss_terms(hip_device)
    with pytest.raises(RuntimeError, match="reduce jobs per call"):
        K.wgrad_reduce(many)
    with pytest.raises(RuntimeError, match="reduce jobs per call"):
        K.wgrad_reduce(many, loss=(terms, scales, divisor, loss))
    lib = hip_lib.load()
    valid = [int(j["cin_valid"]) for j in many]
    common = (hip_lib.ptr_array([j["partial"].data_ptr() for j in many]), hip_lib.ptr_array([j["dw"].data_ptr() for j in many]),
              hip_lib.ptr_array([j["db"].data_ptr() for j in many]), hip_lib.int_array([0] * 65), hip_lib.int_array(valid),
              hip_lib.int_array(valid), hip_lib.int_array([int(j["splits"]) for j in many]),
              hip_lib.int_array([int(j["cout"]) for j in many]), hip_lib.int_array([int(j["cin"]) for j in many]), 65)
    assert lib.larva_wgrad_reduce(*common, K._stream()) == INVALID
    assert lib.larva_wgrad_reduce_with_loss(*common, *K._loss_terms(terms, scales), len(terms), divisor, loss.data_ptr(),
                                            K._stream()) == INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss)) and all(bool(torch.isnan(j["dw"]).all()) and bool(torch.isnan(j["db"]).all()) for j in many)


# =====================================================================================================================
# B. networks past the caps, as tiny steps
# =====================================================================================================================
DEPTHS = {"15_15": ("--num_modules=2", "--num_blocks=15,15"), "default": (), "32_32": ("--num_modules=2", "--num_blocks=32,32")}
ORACLE_DEPTHS = ("15_15", "default")
NAMES = ("LarvaNet", "LarvaNetV2")
STEP_SHAPES = [(2, 8, 8), (1, 7, 9)]    # aligned: dual chain, flat grid; odd width: register-staged, no flat grid
INPUT_SEED = 0                          # (of AC._inputs: the CPU tests show that fp32 passes every bar with it)
B_CASES = [(name, depth, shape) for name in NAMES for depth in DEPTHS for shape in STEP_SHAPES]
B_IDS = ["%s-%s-%s" % (n, d, "x".join(map(str, s))) for n, d, s in B_CASES]
O_CASES = [c for c in B_CASES if c[1] in ORACLE_DEPTHS]
O_IDS = [i for c, i in zip(B_CASES, B_IDS) if c[1] in ORACLE_DEPTHS]


def _plugin(name, depth, training=False, extra=(), seed=5):
    """AC._model with the depth's own flags: none at all for the default depth."""
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(list(DEPTHS[depth]) + list(extra))
    if depth == "default":   # the subject of this file is whatever a user gets without depth flags: follow it
        assert (m.args.num_modules, m.args.num_blocks) == (2, "16,16"), "the default depth changed: update the header and DESIGN.md"
    torch.manual_seed(seed)
    m.prepare(is_training=training, scales=[4])
    m.strict_graph = True
    return m


def _blocks(m):
    from larvanet_amd.models.LarvaNet import parse_num_blocks
    return parse_num_blocks(m.args)


@functools.lru_cache(maxsize=None)
def _spec(name, depth):
    """(blocks, lr, state_dict on the host): the model's own initial draw with non-zero biases, as AC._spec_sd."""
    m = _plugin(name, depth)
    sd = {k: v.detach().cpu().clone() for k, v in m.model.state_dict().items()}
    g = torch.Generator().manual_seed(17)
    for k in sd:
        if k.endswith(".bias"):
            sd[k] = torch.rand(sd[k].shape, generator=g) - 0.5
    return tuple(_blocks(m)), float(m.args.lr), sd


def _inputs(shape):
    return AC._inputs(shape, 4, seed=INPUT_SEED)


def job_counts(net):
    """What the launches of a step see, derived from packed_convs(): pack jobs (a sliced conv packs its whole forward
    image and every slice), weight-gradient layers per kernel shape (a sliced conv has one per slice; the head runs on
    its padded input), reduce jobs (one per layer)."""
    pack, layers = 0, {}
    for pc in net.packed_convs():
        cout, cin = (int(v) for v in pc.weight.shape[:2])
        if pc.slices is not None:
            pack += 1 + len(pc.slices)
            for _, c in pc.slices:
                layers[(cout, c)] = layers.get((cout, c), 0) + 1
        else:
            pack += 1
            key = (cout, cin if pc.cin_pad is None else pc.cin_pad)
            layers[key] = layers.get(key, 0) + 1
    return {"pack": pack, "layers": layers, "reduce": sum(layers.values())}


def _chunks(n, cap):
    return [min(cap, n - i) for i in range(0, n, cap)]


def test_job_counts_of_the_depths_are_past_the_caps():
    """The counts the GPU tests expect, from packed_convs() on the host: 15,15 is 64 (48, 48) layers exactly with 65 pack
    and 65 reduce jobs; the default depth is past 64 of every kind; 32,32 is three chunks of every kind."""
    from larvanet_amd import kernels as K
    from larvanet_amd.autograd import DeferredWgrad
    cap = K.max_wgrad_jobs()
    assert cap == 64 and DeferredWgrad.jobs_per_launch == 32
    got = {(name, depth): job_counts(_plugin(name, depth).model) for name in NAMES for depth in DEPTHS}
    c = got[("LarvaNet", "15_15")]
    assert c["layers"] == {(48, 16): 1, (48, 48): cap} and c["pack"] == PACK_CAP + 1 and c["reduce"] == REDUCE_CAP + 1, c
    c = got[("LarvaNet", "default")]
    assert c["layers"][(48, 48)] == 68 and c["pack"] == 69 and c["reduce"] == 69, c
    for name in NAMES:
        for depth in DEPTHS:
            c = got[(name, depth)]
            want = 3 if depth == "32_32" else 2
            assert len(_chunks(c["pack"], PACK_CAP)) == want and len(_chunks(c["reduce"], REDUCE_CAP)) == want, (name, depth, c)
            if (name, depth) != ("LarvaNet", "15_15"):
                assert len(_chunks(c["layers"][(48, 48)], cap)) == want, (name, depth, c)
            assert set(c["layers"]) == {(48, 16), (48, 48)} and c["layers"][(48, 16)] == 1
    v2 = got[("LarvaNetV2", "default")]   # the merge conv: its forward image and two slices; two (48, 48) layers
    assert v2["pack"] == 69 + 3 + 2 and v2["layers"][(48, 48)] == 68 + 2 + 2, v2


# ---------------------------------------------------------------- the float64 oracle (host)
@functools.lru_cache(maxsize=None)
def _oracle_run(name, depth, shape, dtype):
    """Two steps of oracle/larva_torch.py with torch's AdamW in `dtype` -> per step (loss, gradients), and the weights
    after the second step."""
    blocks, lr, sd = _spec(name, depth)
    x, truth = (t.to(dtype) for t in _inputs(shape))
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.AdamW(list(p.values()), lr=lr)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)   # (images this small: torch's CPU operators are much slower on many threads)
    steps = []
    try:
        for _ in range(2):
            loss = T.multi_exit_loss(p, x, truth, list(blocks), v2=name == "LarvaNetV2")
            opt.zero_grad()
            loss.backward()
            steps.append({"value": float(loss.detach()), "grads": {k: v.grad.detach().double().clone() for k, v in p.items()}})
            opt.step()
    finally:
        torch.set_num_threads(threads)
    return steps, {k: v.detach().double().clone() for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _oracle_ref(name, depth, shape, step):
    return AC.Ref(lambda dtype: _oracle_run(name, depth, shape, dtype)[0][step - 1])


def weight_distance(got, want, lr):
    """The trained-weights bar of tests/test_autograd_contract.py: (largest distance / (2.1 lr), share of the elements
    further than 2e-5 / 2e-3); both must be <= 1."""
    far = total = 0
    dmax = 0.0
    for k in want:
        d = (got[k].double() - want[k].double()).abs()
        far, total, dmax = far + int((d > 2e-5).sum()), total + d.numel(), max(dmax, float(d.max()))
    return dmax / (2.1 * lr), far / (2e-3 * total)


def past_the_64th(sd):
    """The parameter names of every conv layer after the 64th, in the order of the state_dict."""
    convs = [k[:-len(".weight")] for k in sd if k.endswith(".weight")]
    return [c + s for c in convs[64:] for s in (".weight", ".bias")]


@pytest.mark.parametrize("name,depth,shape", O_CASES, ids=O_IDS)
def test_fp32_cpu_run_stays_inside_every_bar_at_these_depths(name, depth, shape):
    """torch's own fp32 run of both steps passes the loss bar, every gradient bar and the weight bar on the very inputs
    and seeds of the GPU tests (a ReLU input that changes sign between fp32 and float64 is the hazard at this depth)."""
    _, lr, _ = _spec(name, depth)
    worst = 0.0
    for step in (1, 2):
        ref = _oracle_ref(name, depth, shape, step)
        r = ref.ratios(ref.r32)
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        assert not bad, (name, depth, shape, step, bad)
        worst = max(worst, max(r.values()))
    w = weight_distance(_oracle_run(name, depth, shape, torch.float32)[1], _oracle_run(name, depth, shape, torch.float64)[1], lr)
    print("\njob caps %s %s %s: fp32 CPU worst %.3f of its bar, weights %.3f / %.3f of theirs" % (name, depth, shape, worst, *w))
    assert max(w) <= 1.0, w


@pytest.mark.parametrize("name,depth,shape", O_CASES, ids=O_IDS)
def test_bars_reject_a_run_without_the_layers_past_the_64th(name, depth, shape):
    """A float64 run in which the gradients of every layer past the 64th are zero (a dropped chunk) fails the bar of
    every one of those tensors, in both steps."""
    _, _, sd = _spec(name, depth)
    lost = past_the_64th(sd)
    assert lost and len(lost) == 2 * (len(sd) // 2 - 64)
    for step in (1, 2):
        ref = _oracle_ref(name, depth, shape, step)
        wrong = dict(ref.r64, grads={k: (torch.zeros_like(g) if k in lost else g) for k, g in ref.r64["grads"].items()})
        r = ref.ratios(wrong)
        assert all(r["grad " + k] > 1.0 for k in lost), {k: r["grad " + k] for k in lost}
        assert all(v == 0.0 for k, v in r.items() if k.startswith("grad ") and k[5:] not in lost)
    print("\njob caps %s %s %s: %d tensors past the 64th layer, smallest ratio of a zeroed one %.1f"
          % (name, depth, shape, len(lost), min(r["grad " + k] for k in lost)))


# ---------------------------------------------------------------- spies
class CapSpies:
    """Records the launch wrappers a step chooses between at the caps (patched where the step reads them, restored on
    exit).  DESIGN.md 7r lists the deliberate defects, one per cap, that these records and the references rejected."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        from larvanet_amd import kernels as K
        from larvanet_amd.autograd import DeferredWgrad, DualChain
        from larvanet_amd.models import LarvaNet as V1
        names = ("pack_weights_batch", "step_prologue", "conv3x3_wgrad", "conv3x3_wgrad_partial", "conv3x3_wgrad_partial_flat",
                 "wgrad_reduce")
        self._saved = [(K, k, getattr(K, k)) for k in names]
        self._saved.append((V1, "autograd_step_prologue", V1.autograd_step_prologue))
        self._saved.append((DeferredWgrad, "flush", DeferredWgrad.__dict__["flush"]))
        self._saved.append((DualChain, "conv", DualChain.__dict__["conv"]))
        pack, prologue, wgrad, partial, flat, reduce_ = (s[2] for s in self._saved[:6])
        fused, flush, dual = V1.autograd_step_prologue, DeferredWgrad.__dict__["flush"].__func__, DualChain.conv

        def rec(kind, **kw):
            self.calls.append(dict(kind=kind, **kw))

        def pack_weights_batch(jobs):
            rec("pack", njobs=len(jobs))
            return pack(jobs)

        def step_prologue(jobs, *a):
            rec("prologue_launch", njobs=len(jobs))
            return prologue(jobs, *a)

        def autograd_step_prologue(pcs, x):
            res = fused(pcs, x)
            rec("prologue", none=res is None)
            return res

        def conv3x3_wgrad(jobs, cout, cin, splits):
            rec("wgrad", njobs=len(jobs), cout=cout, cin=cin)
            return wgrad(jobs, cout, cin, splits)

        def conv3x3_wgrad_partial(jobs, cout, cin, splits):
            rec("partial", njobs=len(jobs), cout=cout, cin=cin)
            return partial(jobs, cout, cin, splits)

        def conv3x3_wgrad_partial_flat(jobs, cout, cin, nwg, head=None):
            res = flat(jobs, cout, cin, nwg, head=head)
            rec("flat", njobs=len(jobs), cout=cout, cin=cin, head=head is not None, none=res is None)
            return res

        def wgrad_reduce(jobs, cout=None, cin=None, loss=None):
            rec("reduce", njobs=len(jobs), loss=loss is not None)
            return reduce_(jobs, cout=cout, cin=cin, loss=loss)

        def flush_(cls, split=False):
            res = flush(cls, split)
            rec("flush", split=split, early=None if res is None else list(res), late=list(cls.late_targets()))
            return res

        K.pack_weights_batch, K.step_prologue, K.conv3x3_wgrad = pack_weights_batch, step_prologue, conv3x3_wgrad
        K.conv3x3_wgrad_partial, K.conv3x3_wgrad_partial_flat, K.wgrad_reduce = conv3x3_wgrad_partial, conv3x3_wgrad_partial_flat, wgrad_reduce
        def dual_conv(cls, srcs, wpk, cout, forward=False, **kw):   # (as test_train_regimes.Spies records it)
            first = srcs if isinstance(srcs, torch.Tensor) else srcs[0]
            n, _, h, p = (int(v) for v in first.shape)
            rec("dual", wants=cls.wants(n, h, p))
            return dual(srcs, wpk, cout, forward=forward, **kw)

        V1.autograd_step_prologue = autograd_step_prologue
        DeferredWgrad.flush = classmethod(flush_)
        DualChain.conv = classmethod(dual_conv)
        return self

    def __exit__(self, *exc):
        for owner, k, v in self._saved:
            setattr(owner, k, v)
        return False

    def of(self, kind, **match):
        return [c for c in self.calls if c["kind"] == kind and all(c.get(k) == v for k, v in match.items())]


def check_deferred_step(spies, counts, aligned, what):
    """One eager step with deferred weight gradients, not split: what was launched, against the counts of packed_convs()."""
    from larvanet_amd import kernels as K
    cap, n48 = K.max_wgrad_jobs(), counts["layers"][(48, 48)]
    # the fused prologue gave up and the caller packed in launches of 64
    assert [c["none"] for c in spies.of("prologue")] == [True], (what, spies.of("prologue"))
    assert not spies.of("prologue_launch"), what
    packs = [c["njobs"] for c in spies.of("pack")]
    assert packs and packs[0] == counts["pack"] > PACK_CAP, (what, packs, counts)
    # the (48, 48) layers: full launches of max_wgrad_jobs() and the rest
    want = _chunks(n48, cap)
    flats = spies.of("flat", cout=48, cin=48)
    assert [c["njobs"] for c in flats] == want, (what, flats, want)
    partial48 = [c["njobs"] for c in spies.of("partial", cout=48, cin=48)]
    partial16 = [c["njobs"] for c in spies.of("partial", cout=48, cin=16)]
    if aligned:     # every launch a flat grid, the head riding on the last one
        assert all(not c["none"] for c in flats) and [c["head"] for c in flats] == [False] * (len(want) - 1) + [True], (what, flats)
        assert not partial48 and not partial16, (what, partial48, partial16)
    else:           # no flat grid at this width: the same chunks through conv3x3_wgrad_partial, the head on its own
        assert all(c["none"] for c in flats), (what, flats)
        assert partial48 == want and partial16 == [1], (what, partial48, partial16, want)
    assert not spies.of("wgrad"), what
    # one reduction per 64 layers, the loss on the last one only
    reduces = spies.of("reduce")
    assert [c["njobs"] for c in reduces] == _chunks(counts["reduce"], REDUCE_CAP) and len(reduces) > 1, (what, reduces)
    assert [c["loss"] for c in reduces] == [False] * (len(reduces) - 1) + [True], (what, reduces)
    assert [c["split"] for c in spies.of("flush")] == [False], what
    # (2, 8, 8) runs the body convs as the two half-batch chains, (1, 7, 9) cannot
    dual = spies.of("dual")
    assert dual and all(c["wants"] == aligned for c in dual), (what, "DualChain.wants", [c["wants"] for c in dual][:4])


def check_per_node_step(spies, what):
    """The reference step: per-node launches of at most 16 layers, no deferred launch, no reduction of its own."""
    assert spies.of("wgrad") and max(c["njobs"] for c in spies.of("wgrad")) <= 16, what
    assert not spies.of("flat") and not spies.of("partial") and not spies.of("reduce"), what


# ---------------------------------------------------------------- the runs (device), shared by the tests of a case
def _one_step(m, xd, td, before_finish=None):
    """loss (0-d host tensor) and every gradient (host) of one forward + backward; the bucket zeroed before it, so a
    tensor nobody wrote stays zero."""
    if m.grad_bucket is not None:
        assert m.grad_bucket.intact()
        m.grad_bucket.flat.zero_()
    loss, _ = m._forward_backward(xd, td)
    if before_finish is not None:
        before_finish()
    m._finish_backward()
    torch.cuda.synchronize()
    assert m.hip_graph_fell_back is None
    return {"loss": loss.detach().cpu().clone(), "grads": {k: p.grad.detach().cpu().clone() for k, p in m.model.named_parameters()}}


def _adamw(m):
    m.optim.step()
    m.model.invalidate_packed_weights()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.model.state_dict().items()}


def _training_plugin(name, depth, dev, graph=False):
    m = AC._load(_plugin(name, depth, training=True), _spec(name, depth)[2])
    m.use_hip_graph = graph
    assert m.defer_wgrad and not m._split_backward()
    return m


_RUNS = {}


def _runs(name, depth, shape, dev):
    """The deferred eager run (two steps, AdamW between and after them) and its per-node reference: step 1 from the same
    weights, step 2 of the reference from the weights the deferred run holds after its first AdamW step."""
    key = (name, depth, shape)
    if key in _RUNS:
        return _RUNS[key]
    x, truth = _inputs(shape)
    xd, td = x.to(dev), truth.to(dev)
    D, R = _training_plugin(name, depth, dev), _training_plugin(name, depth, dev)
    R.defer_wgrad = False
    out = {"counts": job_counts(D.model), "lr": float(D.args.lr)}
    with CapSpies() as s:
        out["d1"] = _one_step(D, xd, td)
    out["spies1"] = s
    with CapSpies() as s:
        out["r1"] = _one_step(R, xd, td)
    out["spies_r"] = s
    out["weights1"] = _adamw(D)
    _adamw(R)
    AC._load(R, out["weights1"])
    with CapSpies() as s:
        out["d2"] = _one_step(D, xd, td)
    out["spies2"] = s
    out["r2"] = _one_step(R, xd, td)
    out["weights2"], out["weights2_r"] = _adamw(D), _adamw(R)
    _RUNS[key] = out
    return out


def compare_with_reference(got, ref, what):
    """The exact reference's rule: the loss EQUAL, every gradient tensor within GRAD_BAR of its own largest element,
    none all zero or non-finite -> the worst ratio to GRAD_BAR."""
    assert torch.equal(got["loss"], ref["loss"]), (what, float(got["loss"]), float(ref["loss"]))
    worst = ("", 0.0)
    for k, g in got["grads"].items():
        assert bool(torch.isfinite(g).all()), (what, k, "not finite")
        assert bool(g.any()), (what, k, "all zero: nobody wrote it")
        r = _rel(g.double(), ref["grads"][k].double()) / GRAD_BAR
        worst = max(worst, (k, r), key=lambda t: t[1])
    print("job caps %s: loss equal, worst gradient %.3f of GRAD_BAR (%s)" % (what, worst[1], worst[0]))
    bad = {k: _rel(g.double(), ref["grads"][k].double()) for k, g in got["grads"].items()
           if not _rel(g.double(), ref["grads"][k].double()) <= GRAD_BAR}
    assert not bad, (what, bad)
    return worst[1]


def assert_same_bits(a, b, what):
    assert torch.equal(a["loss"], b["loss"]), (what, float(a["loss"]), float(b["loss"]))
    diff = {k: _rel(g.double(), b["grads"][k].double()) for k, g in a["grads"].items() if not torch.equal(g, b["grads"][k])}
    assert not diff, (what, diff)


@gpu
@pytest.mark.parametrize("name,depth,shape", B_CASES, ids=B_IDS)
def test_eager_steps_past_the_caps_against_per_node_weight_gradients(hip_device, name, depth, shape):
    """Two eager steps with AdamW between them: the second reads weights the first one's optimizer moved, so a conv past
    the 64th whose packed image was not refreshed shows in its loss.  What was launched is asserted from the spies."""
    r = _runs(name, depth, shape, hip_device)
    aligned = shape[2] % 4 == 0
    what = "%s %s %s" % (name, depth, shape)
    assert r["counts"] == job_counts(_plugin(name, depth).model)
    check_deferred_step(r["spies1"], r["counts"], aligned, what + " step 1")
    check_deferred_step(r["spies2"], r["counts"], aligned, what + " step 2")
    check_per_node_step(r["spies_r"], what)
    print()
    compare_with_reference(r["d1"], r["r1"], what + " step 1")
    compare_with_reference(r["d2"], r["r2"], what + " step 2")
    assert not torch.equal(r["d1"]["loss"], r["d2"]["loss"])          # (the optimizer did move the weights)
    moved = [k for k, v in r["weights1"].items() if not torch.equal(v, _spec(name, depth)[2][k])]
    assert len(moved) == len(r["weights1"]), "a tensor the first AdamW step left alone"
    w = weight_distance(r["weights2"], r["weights2_r"], r["lr"])
    print("job caps %s: weights after step 2 %.3f / %.3f of their bars" % (what, *w))
    assert max(w) <= 1.0, (what, w)


@gpu
@pytest.mark.parametrize("name,depth,shape", B_CASES, ids=B_IDS)
def test_captured_steps_past_the_caps_equal_the_eager_ones(hip_device, name, depth, shape):
    """use_hip_graph on: both replayed steps and the weights after them equal the eager run bit for bit."""
    r = _runs(name, depth, shape, hip_device)
    x, truth = _inputs(shape)
    xd, td = x.to(hip_device), truth.to(hip_device)
    G = _training_plugin(name, depth, hip_device, graph=True)
    g1 = _one_step(G, xd, td)          # (warm-ups, the capture, a replay)
    assert G.use_hip_graph and G._step is not None
    _adamw(G)
    g2 = _one_step(G, xd, td)          # a replay alone, on the moved weights
    weights = _adamw(G)
    what = "%s %s %s captured" % (name, depth, shape)
    print("\njob caps %s: step 1 loss %.2e gradients %.2e, step 2 loss %.2e gradients %.2e from the eager run (bar: 0)"
          % (what, abs(float(g1["loss"]) - float(r["d1"]["loss"])), max(_rel(g.double(), r["d1"]["grads"][k].double()) for k, g in g1["grads"].items()),
             abs(float(g2["loss"]) - float(r["d2"]["loss"])), max(_rel(g.double(), r["d2"]["grads"][k].double()) for k, g in g2["grads"].items())))
    assert_same_bits(g1, r["d1"], what + " step 1")
    assert_same_bits(g2, r["d2"], what + " step 2")
    assert all(torch.equal(weights[k], r["weights2"][k]) for k in weights), what


@gpu
@pytest.mark.parametrize("name,depth,shape", B_CASES, ids=B_IDS)
def test_split_flush_past_the_caps(hip_device, name, depth, shape):
    """force_split_backward with overlap_allreduce: weight-gradient launches of jobs_per_launch = 32 layers, the second
    half held back for flush_late.  Same references, same bars; early_targets and late_targets cover the bucket; the
    late half is still unwritten before _late runs and every gradient is complete after it."""
    from larvanet_amd import kernels as K
    from larvanet_amd.autograd import DeferredWgrad
    r = _runs(name, depth, shape, hip_device)
    x, truth = _inputs(shape)
    xd, td = x.to(hip_device), truth.to(hip_device)
    S = _training_plugin(name, depth, hip_device)
    S.force_split_backward, S.overlap_allreduce = True, True
    assert S._split_backward() and DeferredWgrad.jobs_per_launch == 32
    what = "%s %s %s split" % (name, depth, shape)
    seen = {}

    def before_finish():
        torch.cuda.synchronize()
        assert S._late is not None and DeferredWgrad.has_late(), what
        early = {t.data_ptr() for t in spies.of("flush")[0]["early"]}
        late = [t for t in DeferredWgrad.late_targets() if t.data_ptr() not in early]   # (slices of one dw may fall apart)
        seen["late_unwritten"] = sum(not bool(t.any()) for t in late)
        seen["late"] = len(late)

    with CapSpies() as spies:
        s1 = _one_step(S, xd, td, before_finish)
    assert not DeferredWgrad.has_late() and S._late is None
    # the late half was really held back: its tensors were still the zeros put there before the step
    assert seen["late"] > 0 and seen["late_unwritten"] == seen["late"], (what, seen)
    # early and late targets together are the whole bucket, element for element
    (flush,) = spies.of("flush")
    assert flush["split"] and flush["early"] and flush["late"]
    flat = S.grad_bucket.flat
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for t in flush["early"] + flush["late"]:
        off = (t.data_ptr() - flat.data_ptr()) // 4
        assert 0 <= off and off + t.numel() <= flat.numel()
        covered[off:off + t.numel()] = True
    assert bool(covered.all()), (what, int((~covered).sum()), "bucket elements no launch writes")
    # launches of at most jobs_per_launch layers: the (48, 48) layers as full launches of 32 and the rest
    cap = min(DeferredWgrad.jobs_per_launch, K.max_wgrad_jobs())
    aligned = shape[2] % 4 == 0
    n48 = r["counts"]["layers"][(48, 48)]
    sizes = [c["njobs"] for c in (spies.of("flat", cout=48, cin=48) if aligned else spies.of("partial", cout=48, cin=48))]
    assert sorted(sizes, reverse=True) == _chunks(n48, cap) and len(sizes) >= 2, (what, sizes)
    if aligned:
        assert all(not c["none"] for c in spies.of("flat", cout=48, cin=48)), what
    reduces = spies.of("reduce")
    assert sum(c["njobs"] for c in reduces) == r["counts"]["reduce"] and len(reduces) >= 2, (what, reduces)
    assert sum(c["loss"] for c in reduces) == 1 and all(c["njobs"] <= REDUCE_CAP for c in reduces), (what, reduces)
    # what each of the two _issue calls did: the flush record is written when the early one has returned
    cut = next(i for i, c in enumerate(spies.calls) if c is flush)
    early, late = spies.calls[:cut], spies.calls[cut + 1:]

    def of(calls, kind, **match):
        return [c for c in calls if c["kind"] == kind and all(c.get(k) == v for k, v in match.items())]
    # the loss rides on the LAST reduction of the early half (the scope's loss is due when the scope ends), never later
    assert [c["loss"] for c in of(early, "reduce")] == [False] * (len(of(early, "reduce")) - 1) + [True], (what, of(early, "reduce"))
    assert of(late, "reduce") and not any(c["loss"] for c in of(late, "reduce")), (what, of(late, "reduce"))
    # the head (the lowest address of the bucket) is in the late half; where a flat grid applies it rides on the last
    # (48, 48) grid of that half, else it goes per layer there
    assert not of(early, "flat", head=True) and not of(early, "partial", cout=48, cin=16), what
    if aligned:
        hosts = of(late, "flat", cout=48, cin=48)
        assert hosts and [c["head"] for c in hosts] == [False] * (len(hosts) - 1) + [True], (what, hosts)
        assert not of(late, "partial", cout=48, cin=16), what
    else:
        assert [c["njobs"] for c in of(late, "partial", cout=48, cin=16)] == [1], what
    print()
    compare_with_reference(s1, r["r1"], what + " step 1")
    weights1 = _adamw(S)
    # step 2 starts from the split run's own weights, which the step-1 gradients' order moved by a rounding: the
    # reference takes them over, as in _runs
    R = _training_plugin(name, depth, hip_device)
    R.defer_wgrad = False
    AC._load(R, weights1)
    s2 = _one_step(S, xd, td)
    compare_with_reference(s2, _one_step(R, xd, td), what + " step 2")
    w = weight_distance(_adamw(S), r["weights2_r"], r["lr"])
    print("job caps %s: weights after step 2 %.3f / %.3f of their bars" % (what, *w))
    assert max(w) <= 1.0, (what, w)


@gpu
@pytest.mark.parametrize("name,depth,shape", O_CASES, ids=O_IDS)
def test_steps_past_the_caps_against_the_float64_oracle(hip_device, name, depth, shape):
    """Both steps of the eager run (loss and every gradient tensor) and the weights after the second AdamW step against
    oracle/larva_torch.py in float64 with torch's AdamW."""
    r = _runs(name, depth, shape, hip_device)
    what = "%s %s %s" % (name, depth, shape)
    for step in (1, 2):
        d = r["d%d" % step]
        _oracle_ref(name, depth, shape, step).check("job caps %s step %d" % (what, step),
                                                    {"value": float(d["loss"]), "grads": {k: g.double() for k, g in d["grads"].items()}})
    w = weight_distance(r["weights2"], _oracle_run(name, depth, shape, torch.float64)[1], r["lr"])
    print("job caps %s: weights after step 2 %.3f / %.3f of their bars" % (what, *w))
    assert max(w) <= 1.0, (what, w)


# ---------------------------------------------------------------- inference at the default depth
INFER_SHAPES = [(7, 9), (12, 24)]
FLOAT_BAR = 2e-3     # tests/test_interleaved_shapes.py
U8_SHARE = 1e-3


def _infer_image(h, w):
    """uint8 (h, w, 3) noise on 64..255 (tests/test_interleaved_shapes.py: no clamp at 0 in the way)."""
    return np.random.default_rng([h, w, 77]).integers(64, 256, (h, w, 3), dtype=np.uint8)


def _chw(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, -3)).astype(np.float32)


def _q(y):
    return np.ascontiguousarray(np.moveaxis(np.clip(np.rint(y), 0, 255).astype(np.uint8), -3, -1))


@functools.lru_cache(maxsize=None)
def _oracle_forward(name, h, w, dtype):
    blocks, _, sd = _spec(name, "default")
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    x = torch.from_numpy(_chw(_infer_image(h, w))).to(dtype)[None]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            return (T.forward_v2 if name == "LarvaNetV2" else T.forward)(sdd, x, list(blocks))[0].numpy()
    finally:
        torch.set_num_threads(threads)


def _byte_distance(got, want):
    """(levels of the worst byte, bytes that differ, bytes)."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), int((d > 0).sum()), int(d.size)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_rounds_like_float64_on_the_inference_images(name):
    """The oracle's own fp32 run on the two images: within FLOAT_BAR of float64, no byte more than a level off and at
    most 0.1 % of the bytes off at all."""
    off = total = 0
    worst = 0.0
    for h, w in INFER_SHAPES:
        y32, y64 = _oracle_forward(name, h, w, torch.float32), _oracle_forward(name, h, w, torch.float64)
        worst = max(worst, float(np.abs(y32 - y64).max()))
        levels, n, size = _byte_distance(_q(y32), _q(y64))
        assert levels <= 1
        off, total = off + n, total + size
    print("\njob caps inference %s: fp32 CPU %.2e from float64 (bar %.0e), %d of %d bytes a level off" % (name, worst, FLOAT_BAR, off, total))
    assert worst <= FLOAT_BAR and off <= U8_SHARE * total


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_upscale_at_the_default_depth_against_float64(hip_device, name):
    """upscale / upscale_u8 of a 7 x 9 and a 12 x 24 image at --num_blocks=16,16 against the float64 oracle; the second
    call at a shape is captured, the third replays: both equal the eager one bit for bit."""
    m = AC._load(_plugin(name, "default"), _spec(name, "default")[2])
    off = total = 0
    worst = 0.0
    for h, w in INFER_SHAPES:
        img = _infer_image(h, w)
        y64 = _oracle_forward(name, h, w, torch.float64)
        calls = [m.upscale([_chw(img)], 4)[0] for _ in range(3)]
        calls8 = [m.upscale_u8([img], 4)[0] for _ in range(3)]
        key = ((1, 3, h, w), "fp32")
        assert m._infer_graphs.get(key) not in (None, False), "the float forward of %s was not captured" % (key,)
        assert any(k[0] == (1, h, w, 3) and m._infer_graphs_u8[k] is not False for k in m._infer_graphs_u8), list(m._infer_graphs_u8)
        for k, (a, b) in enumerate(zip(calls[1:], calls8[1:])):
            X.assert_bits_equal(a, calls[0], "%s %dx%d float call %d against the eager one" % (name, h, w, k + 2))
            X.assert_bits_equal(b, calls8[0], "%s %dx%d uint8 call %d against the eager one" % (name, h, w, k + 2))
        worst = max(worst, float(np.abs(calls[0] - y64).max()))
        levels, n, size = _byte_distance(calls8[0], _q(y64))
        assert levels <= 1, (name, h, w, levels)
        off, total = off + n, total + size
    print("\njob caps inference %s: %.3f of the float bar, %d of %d bytes a level off (%.3f of the share allowed)"
          % (name, worst / FLOAT_BAR, off, total, off / (U8_SHARE * total)))
    assert worst <= FLOAT_BAR and off <= U8_SHARE * total


class _NoVal:
    def get_num_images(self):
        return 0


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_fp16_at_the_default_depth_passes_the_quality_bar(hip_device, name):
    """tests/test_half_infer.py's bar at --num_blocks=16,16: weights trained by the fp32 step (here 80 steps on one
    batch of three smooth 12 x 24 images, 48 x 96 HR), fp16 against fp32 on a 7 x 9 and a 12 x 24 image."""
    import test_half_infer as HI
    from larvanet_amd.metrics import image_psnr, image_to_uint8
    t = _plugin(name, "default", training=True)
    g = torch.Generator().manual_seed(5)
    hr = HI._smooth_hr(g, 3, 48, 96)
    x, tr = HI._lr(hr).to(t.device).contiguous(), hr.to(t.device).contiguous()
    for _ in range(80):
        t.train_step_larva(None, _NoVal(), x, tr)
    sd = {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()}
    m32 = AC._load(_plugin(name, "default"), sd)
    m16 = AC._load(_plugin(name, "default", extra=("--precision=fp16",)), sd)
    g = torch.Generator().manual_seed(9)
    worst = 0.0
    for h, w in INFER_SHAPES:
        truth = HI._smooth_hr(g, 1, 4 * h, 4 * w)
        x = HI._lr(truth)[0].numpy()
        o32, o16 = m32.upscale([x], 4)[0], m16.upscale([x], 4)[0]
        tu8 = image_to_uint8(truth[0].numpy())
        p32 = float(image_psnr(output_image=image_to_uint8(o32), truth_image=tu8))
        p16 = float(image_psnr(output_image=image_to_uint8(o16), truth_image=tu8))
        d = np.abs(o16.astype(np.float64) - o32)
        base = m32.model.base(torch.from_numpy(x[None]).to(hip_device))[0].cpu().numpy()
        assert np.abs(o32 - base).mean() > 0.01, "the model must have learned something for the comparison to mean anything"
        ratio = max(abs(p16 - p32) / 0.02, d.max() / 0.25, d.mean() / 0.03)
        worst = max(worst, ratio)
        print("\njob caps fp16 %s %dx%d: psnr fp32 %.5f fp16 %.5f, max |d| %.4f, mean |d| %.5f: %.3f of the bar"
              % (name, h, w, p32, p16, d.max(), d.mean(), ratio))
        assert abs(p16 - p32) <= 0.02 and d.max() <= 0.25 and d.mean() <= 0.03, (p32, p16, d.max(), d.mean())
    assert not m16.fp16_overflowed()


# =====================================================================================================================
# C. more exits than a job launch holds: nine bodies
# =====================================================================================================================
NINE = ["--num_modules=9", "--num_blocks=1,1,1,1,1,1,1,1,1"]
EXIT_SHAPES = [(1, 7, 9), (2, 8, 12)]


def _nine(name, extra=(), precision="fp32"):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(NINE + ["--precision=" + precision] + list(extra))
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    m.strict_graph = True
    return m


@functools.lru_cache(maxsize=None)
def _nine_family(precision):
    """One nine-exit LarvaNet and its nine LarvaLeg --leg=k plugins over one random state_dict."""
    import test_all_exits as AE
    net = _nine("LarvaNet", (), precision)
    sd = AE._random_state(net, 4321)
    AE._load(net, sd)
    return net, [AE._load(_nine("LarvaLeg", ("--leg=%d" % k,), precision), sd) for k in range(1, 10)]


@gpu
@pytest.mark.parametrize("shape", EXIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_nine_exits_equal_their_larvaleg_plugins(hip_device, monkeypatch, precision, shape):
    """All-exit inference with nine exits: fp16 issues the legs as 8 + 1 jobs (kernels.F16_MAX_JOBS), fp32 as batched
    launches of 4 + 3 + 2; every exit, float and uint8, equals its LarvaLeg --leg=k plugin bit for bit."""
    import test_all_exits as AE
    from larvanet_amd import kernels as K
    net, legs = _nine_family(precision)
    n, h, w = shape
    img8 = AE._images(shape, 3)
    chw = [np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) + 0.25 for a in img8]
    seen = []
    for fn in ("f16_conv3x3_jobs", "f16_conv3x3_shuffle_base_jobs", "conv3x3_batch"):
        real = getattr(K, fn)
        monkeypatch.setattr(K, fn, lambda jobs, *a, _fn=fn, _real=real, **kw: (seen.append((_fn, len(jobs))), _real(jobs, *a, **kw))[1])
    got = net.upscale_exits(chw, 4)            # (the first call at a shape runs eagerly: the wrappers are seen)
    got8 = net.upscale_exits_u8(list(img8), 4)
    if precision == "fp16":
        assert K.F16_MAX_JOBS == 8
        assert seen == [("f16_conv3x3_jobs", 8), ("f16_conv3x3_shuffle_base_jobs", 8), ("f16_conv3x3_jobs", 1),
                        ("f16_conv3x3_shuffle_base_jobs", 1)] * 2, seen
    else:
        assert seen == [("conv3x3_batch", k) for k in (4, 4, 3, 3, 2, 2)] * 2, seen
    monkeypatch.undo()
    assert got.shape == (9, n, 3, 4 * h, 4 * w) and got8.shape == (9, n, 4 * h, 4 * w, 3)
    tag = "nine exits %s %s " % (precision, shape)
    for i, leg in enumerate(legs):
        X.assert_bits_equal(got[i], leg.upscale(chw, 4), tag + "upscale_exits[%d]" % i)
        X.assert_bits_equal(got8[i], leg.upscale_u8(list(img8), 4), tag + "upscale_exits_u8[%d]" % i)
    X.assert_bits_equal(got[-1], net.upscale(chw, 4), tag + "last exit against LarvaNet.upscale")
    assert all(not np.array_equal(got[i], got[i + 1]) for i in range(8))      # (the exits do differ)
    X.assert_bits_equal(net.upscale_exits(chw, 4), got, tag + "captured call against the eager one")
    X.assert_bits_equal(net.upscale_exits_u8(list(img8), 4), got8, tag + "captured uint8 call against the eager one")
    print("\njob caps %s: nine exits equal to their LarvaLeg plugins (exact)" % tag)


@gpu
def test_overflow_in_the_ninth_exit_alone_still_raises(hip_device):
    """The ninth leg is the lone job of the second fp16 job launch: an activation of its first conv past 65504 (its
    weights times 1e6; no other exit reads them) sets the flag and upscale_exits raises, float and uint8."""
    import test_all_exits as AE
    net = _nine("LarvaNet", (), "fp16")
    AE._load(net, AE._random_state(net, 4321))
    img8 = AE._images((1, 7, 9), 3)
    chw = [np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) for a in img8]
    clean = net.upscale_exits(chw, 4)
    with torch.no_grad():
        net.model.body_8.leg.recon_block[0].weight.mul_(1e6)
    net.model.invalidate_packed_weights()
    with pytest.raises(FloatingPointError, match="--precision fp16"):
        net.upscale_exits(chw, 4)
    with pytest.raises(FloatingPointError, match="--precision fp16"):
        net.upscale_exits_u8(list(img8), 4)
    # the first eight exits do not depend on that leg: the unchecked forward still returns them unchanged
    with torch.no_grad():
        out = net._forward_nograd(AE._dev(np.stack(chw), hip_device), exits=True).cpu().numpy()
    assert net.fp16_overflowed() is True
    X.assert_bits_equal(out[:8], clean[:8], "the eight exits of the first job launch")


def test_larvanet_v2_with_nine_bodies_is_refused_at_prepare():
    """The tail's merge conv would read nine tensors; conv3x3 and larva_f16_conv3x3 take eight.  prepare() says so, for
    training and for inference, before anything is built; eight bodies prepare; LarvaLegV2, whose inference route never
    reaches the tail, prepares for inference and is refused for training (V2's step includes the tail)."""
    def make(name, flags):
        m = importlib.import_module("larvanet_amd.models." + name).create_model()
        m.parse_args(flags)
        return m
    for training in (False, True):
        with pytest.raises(ValueError, match="^larvanet_amd: LarvaNetV2 merges the outputs of at most 8 bodies"):
            make("LarvaNetV2", NINE).prepare(is_training=training, scales=[4])
    with pytest.raises(ValueError, match="^larvanet_amd: LarvaNetV2 merges the outputs of at most 8 bodies"):
        make("LarvaNetV2", NINE + ["--precision=fp16"]).prepare(is_training=False, scales=[4])
    make("LarvaNetV2", ["--num_modules=8", "--num_blocks=1,1,1,1,1,1,1,1"]).prepare(is_training=False, scales=[4])
    make("LarvaLegV2", NINE + ["--leg=9"]).prepare(is_training=False, scales=[4])
    with pytest.raises(ValueError, match="^larvanet_amd: LarvaLegV2 merges the outputs of at most 8 bodies"):
        make("LarvaLegV2", NINE + ["--leg=9"]).prepare(is_training=True, scales=[4])
