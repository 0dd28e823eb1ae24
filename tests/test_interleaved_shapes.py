"""One call's state must stay out of the next call's result.  Several pieces of state outlive a call: the head's cached
zero-padded input (autograd.StepScope._padded), a plugin's four graph tables with the static buffers of every captured
forward, the strip / resize / alpha tables of kernels.py, the slots of pipeline._stream, the fp16 packs and overflow
flag, and the captured training step's buffers.  Every other test shows a model one shape at a time; here shapes that
share cached state are interleaved: widths with one row pitch (21..24 -> 24, 5..7 -> 8) under captured graphs, streams
over a mix of sizes, and training steps between captured inference calls of the training shape.

Every test makes the stale content itself: the wider shape goes first, and every pixel of every image is >= 64, so a
pad column that is not zero any more holds values of order 100.  Two references, for every output of parts 1 and 3:

  bit for bit   a second plugin with the same weights and use_hip_graph = False that sees each image once, as a batch
                of its own (captured equals eager is the project's rule, and a pixel does not depend on its batch slot);
  high precision   oracle/larva_torch.py on the CPU in float64 over the same weights.  Float outputs: 2e-3 absolute on
                the 0..255 scale (the bar of tests/test_model_parity.py).  uint8 outputs: at most one level, on at most
                0.1 % of the bytes of a case (roundings within 2e-3 of a tie); test_fp32_rounds_like_float64_... checks
                on the CPU that the oracle's own fp32 run stays inside that share on these very images.

test_an_extra_input_column_moves_the_right_edge (CPU) shows that a leaked column would move the output by more than 100
times the bar.  All models are the tiny two-body network (48 filters, x4); no image is larger than 12 x 24 LR pixels."""
import gc
import importlib
import types

import numpy as np
import pytest
import torch

from larvanet_amd import image_utils as U
from oracle import larva_torch as T
from test_model_parity import FakeValLoader

TINY = ["--num_modules=2", "--num_blocks=1,1"]
BLOCKS = [1, 1]
MODELS = ("LarvaNet", "LarvaNetV2")
SEED = 3
FLOAT_BAR = 2e-3          # tests/test_model_parity.py's header
U8_SHARE = 1e-3           # at most 0.1 % of a case's bytes may be one level off float64
H = 7
CLASSES = {"pitch24": (21, 22, 23, 24), "pitch8": (5, 6, 7)}
ORDERS = {"descending": {"pitch24": (24, 23, 22, 21), "pitch8": (7, 6, 5)},
          "ascending": {"pitch24": (21, 22, 23, 24), "pitch8": (5, 6, 7)},
          "mixed": {"pitch24": (23, 21, 23, 22, 21), "pitch8": (7, 5, 7, 6, 5)}}
FORMS = ("f32", "u8", "rgba", "yuv", "exits")
TABLE = {"f32": "_infer_graphs", "u8": "_infer_graphs_u8", "rgba": "_infer_graphs_u8", "yuv": "_infer_graphs_u8",
         "exits": "_infer_graphs_ex", "se_f32": "_infer_graphs_se", "se_u8": "_infer_graphs_se"}
WIDTH_AXIS = {"f32": 2, "u8": 1, "rgba": 1, "yuv": None, "exits": 2, "se_f32": 2, "se_u8": 1}   # of one image's result
STREAM_SIZES = ((7, 23), (7, 21), (12, 24), (5, 6), (7, 22), (7, 21), (5, 7), (12, 24), (7, 23), (5, 5))   # (H, W)
SIZE = (20, 30)

_TWINS, _WEIGHTS, _ORACLE = {}, {}, {}


# ---------------------------------------------------------------- models and weights
# A plugin holds its captured graphs in reference cycles, and a graph freed by the collector while another one is being
# captured aborts the process (tests/test_yuv.py, _collect).  So the collector may not run while a test of this file
# does: what earlier files dropped is collected once before the first test, every test runs with the automatic
# collector off (it makes and drops a handful of plugins), and what it dropped is collected when it ends, before a test
# of this file or another captures anything.  (A full collection in a long pytest process costs ~0.2 s: one per test.)
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


def _plugin(name, graph, extra=(), seed=SEED, precision="fp32"):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(TINY + ["--precision=" + precision] + list(extra))
    torch.manual_seed(seed)
    m.prepare(is_training=False, scales=[4])
    m.strict_graph = True
    m.use_hip_graph = graph
    return m


def _twin(name, extra=(), seed=SEED, precision="fp32"):
    """The eager plugin of these weights: one per module run, it keeps no graph and no padded buffer."""
    key = (name, tuple(extra), seed, precision)
    if key not in _TWINS:
        t = _TWINS[key] = _plugin(name, False, extra, seed, precision)
        if precision == "fp32":   # the oracle's weights are the plugin's: same seed, same draw order
            sd = _weights(name, seed, torch.float32)
            for k, v in t.model.state_dict().items():
                assert torch.equal(v.cpu(), sd[k]), k
    return _TWINS[key]


def _weights(name, seed, dtype):
    key = (name, seed, dtype)
    if key not in _WEIGHTS:
        sd = T.init_state_dict(BLOCKS, v2=name == "LarvaNetV2", seed=seed)
        _WEIGHTS[key] = {k: v.to(dtype) for k, v in sd.items()}
    return _WEIGHTS[key]


def _net(name, seed, dtype, x, exits=False):
    """The oracle's forward of ONE float32 (3, H, W) image in `dtype` -> numpy (3, 4H, 4W), or (M, 3, 4H, 4W) with
    exits.  Computed once per image and shared."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    key = (name, seed, dtype, exits, x.shape, x.tobytes())
    if key not in _ORACLE:
        sd = _weights(name, seed, dtype)
        xt = torch.from_numpy(x).to(dtype)[None]
        threads = torch.get_num_threads()
        torch.set_num_threads(1)   # (images this small: torch's fp32 CPU operators are 100x slower on many threads)
        try:
            with torch.no_grad():
                if exits:
                    y = torch.stack(T.forward_exits(sd, xt, BLOCKS)[0])[:, 0]
                else:
                    y = (T.forward_v2 if name == "LarvaNetV2" else T.forward)(sd, xt, BLOCKS)[0]
        finally:
            torch.set_num_threads(threads)
        _ORACLE[key] = y.numpy()
    return _ORACLE[key]


def _q(y):
    """float (..., 3, h, w) -> uint8 (..., h, w, 3): round half to even, clamp (metrics.image_to_uint8, transposed)."""
    return np.ascontiguousarray(np.moveaxis(np.clip(np.rint(y), 0, 255).astype(np.uint8), -3, -1))


# ---------------------------------------------------------------- images: every value >= 64
def _rgb(n, h, w, k):
    """The k-th batch shown at (n, h, w): uint8 (n, h, w, 3) noise on 64..255."""
    return np.random.default_rng([n, h, w, k, 50]).integers(64, 256, (n, h, w, 3), dtype=np.uint8)


def _chw(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, -3)).astype(np.float32)


def _rgba(n, h, w, k):
    """_rgb with an alpha channel: image 0 translucent (64..255, so its alpha plane is a batch slot of its own: N + 1
    slots), the others opaque."""
    a = np.concatenate([_rgb(n, h, w, k), np.full((n, h, w, 1), 255, np.uint8)], axis=3)
    a[0, :, :, 3] = np.random.default_rng([n, h, w, k, 51]).integers(64, 256, (h, w), dtype=np.uint8)
    a[0, 0, 0, 3] = 100
    return a


def _frames(n, h, w, k):
    """n I420 frames whose RGB image is >= 64 everywhere: Y on 100..200, chroma on 118..138 (limited range BT.601:
    R, G, B >= 1.164 * 84 - 1.6 * 10 - ... > 80)."""
    rng = np.random.default_rng([n, h, w, k, 52])
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [np.concatenate([rng.integers(100, 201, h * w, dtype=np.uint8),
                            rng.integers(118, 139, 2 * cw * ch, dtype=np.uint8)]) for _ in range(n)]


def _items(form, n, h, w, k):
    """The n inputs of the k-th call at (n, h, w), as `form`'s entry point takes them."""
    if form in ("f32", "se_f32"):
        return list(_chw(_rgb(n, h, w, k)))
    if form == "rgba":
        return list(_rgba(n, h, w, k))
    if form == "yuv":
        return _frames(n, h, w, k)
    return list(_rgb(n, h, w, k))


def _run(m, form, items, h, w, k):
    """The entry point of `form` on the whole batch -> one result per image."""
    if form in ("f32", "se_f32"):
        return list(m.upscale(items, 4))
    if form in ("u8", "se_u8"):
        if k % 2:   # (both entry points share the table and the key)
            return list(m.upscale_u8_tensor(torch.from_numpy(np.stack(items)).to(m.device)).cpu().numpy())
        return list(m.upscale_u8(items, 4))
    if form == "rgba":
        return list(m.upscale_rgba_u8(items, 4))
    if form == "yuv":
        return list(m.upscale_yuv420(items, 4, w, h))
    out = m.upscale_exits_u8(items, 4)
    return [out[:, i] for i in range(len(items))]


def _alone(form, twin, item, h, w):
    return _run(twin, form, [item], h, w, 0)[0]


def _ensemble(name, seed, dtype, x):
    """image_utils.self_ensemble with the oracle as f, summed in `dtype`."""
    acc = 0
    for t in range(8):
        acc = acc + U.dihedral_inv(_net(name, seed, dtype, U.dihedral(x, t, (1, 2))), t, (1, 2))
    return acc * np.asarray(0.125, acc.dtype)


def _expect(form, name, seed, dtype, item, h, w):
    """What the entry point of `form` returns for one image according to the oracle run in `dtype`."""
    if form == "f32":
        return _net(name, seed, dtype, item)
    if form == "u8":
        return _q(_net(name, seed, dtype, _chw(item)))
    if form == "exits":
        return _q(_net(name, seed, dtype, _chw(item), exits=True))
    if form == "rgba":
        slots, _ = U.alpha_slots([bool(item[..., 3].min() == 255)])
        planes = U.rgba_split_f32(item[None], slots)
        return U.rgba_merge_u8(np.stack([_q(_net(name, seed, dtype, p)) for p in planes]), slots, 1)[0]
    if form == "yuv":
        return U.rgb_u8_to_i420(_q(_net(name, seed, dtype, U.i420_to_rgb_f32(item, w, h))))
    e = _ensemble(name, seed, dtype, item if form == "se_f32" else _chw(item))
    return e if form == "se_f32" else _q(e)


# ---------------------------------------------------------------- the two comparisons
class _Bytes:
    """The uint8 bar over one case: no byte more than a level off, and at most U8_SHARE of all bytes off at all."""

    def __init__(self):
        self.off = self.total = 0

    def add(self, got, want, what):
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert int(d.max()) <= 1, "%s: %d levels from float64 (%d of %d bytes differ)" % (what, d.max(), (d > 0).sum(), d.size)
        self.off += int((d > 0).sum())
        self.total += int(d.size)

    def close(self, what):
        print("%s: %d of %d bytes one level off float64" % (what, self.off, self.total))
        assert self.off <= U8_SHARE * self.total, "%s: %d of %d bytes one level off float64" % (what, self.off, self.total)


def _where(form, d):
    """Which HR columns of one image's result differ."""
    ax = WIDTH_AXIS.get(form)
    if ax is None:
        return ""
    cols = np.nonzero(d.any(axis=tuple(i for i in range(d.ndim) if i != ax)))[0]
    return ", HR columns %d..%d of %d" % (cols.min(), cols.max(), d.shape[ax])


def _same_bits(form, got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        raise AssertionError("%s: differs from the eager twin at %d of %d values, by up to %.4g%s"
                             % (what, int((d > 0).sum()), d.size, d.max(), _where(form, d)))


def _near_float64(form, got, want, what, tally):
    if got.dtype == np.uint8:
        tally.add(got, want, what)
        return
    d = np.abs(got.astype(np.float64) - want)
    assert float(d.max()) <= FLOAT_BAR, "%s: %.4g from float64 (bar %g)%s" % (what, d.max(), FLOAT_BAR, _where(form, d > FLOAT_BAR))


# ---------------------------------------------------------------- the walk over interleaved shapes
def _schedule(order):
    """[(shape, visit)]: every shape of `order` three times running (the first sight of a shape is eager, the second is
    captured, every later one replays), then each other shape shown so far once more."""
    count, seen, out = {}, [], []

    def show(shape):
        out.append((shape, count.get(shape, 0)))
        count[shape] = count.get(shape, 0) + 1

    for shape in order:
        for _ in range(3):
            show(shape)
        for earlier in seen:
            if earlier != shape:
                show(earlier)
        if shape not in seen:
            seen.append(shape)
    return out


def _walk(m, form, name, order, tally, seed=SEED, extra=(), precision="fp32"):
    """Show `m` the (n, h, w) shapes of _schedule(order).  After each call: the table holds a live capture of exactly
    the shapes shown twice, and every image of the result equals the eager twin's and is near float64."""
    table = getattr(m, TABLE[form])
    twin = _twin(name, extra, seed, precision)
    shown = {}
    for shape, k in _schedule(order):
        n, h, w = shape
        items = _items(form, n, h, w, k)
        got = _run(m, form, items, h, w, k)
        shown[shape] = k + 1
        twice = sum(1 for c in shown.values() if c >= 2)
        assert len(table) == twice and all(v is not False for v in table.values()), (form, shape, k, len(table), twice)
        for i, item in enumerate(items):
            what = "%s %s N=%d %dx%d visit %d image %d" % (name, form, n, h, w, k, i)
            _same_bits(form, got[i], _alone(form, twin, item, h, w), what)
            if precision == "fp32":
                _near_float64(form, got[i], _expect(form, name, seed, torch.float64, item, h, w), what, tally)


def _widths(form, order, cls):
    ws = ORDERS[order][cls]
    return [w for w in ws if w % 2] if form == "yuv" else list(ws)   # (the video case: odd widths, odd height)


CORE = [(name, form, order, n) for name in MODELS for form in FORMS for order in ORDERS for n in (1, 3)
        if not (form == "exits" and name == "LarvaNetV2")]   # (the V2 tail has no per-body exits)


# ---------------------------------------------------------------- 1. widths that share a row pitch, under captured graphs
@pytest.mark.gpu
@pytest.mark.parametrize("name,form,order,n", CORE, ids=lambda v: str(v))
def test_widths_of_one_row_pitch_keep_their_own_pad_columns(hip_device, name, form, order, n):
    """W = 21..24 have pitch 24 and W = 5..7 pitch 8: under PaddedWidth the head's padded input of (N, H, pitch) is one
    cached buffer inside a capture, and columns [W, pitch) of it must be zero for every width that uses it."""
    tally = _Bytes()
    for cls in CLASSES:   # (a plugin per class: a table holds four shapes)
        m = _plugin(name, True)
        _walk(m, form, name, [(n, H, w) for w in _widths(form, order, cls)], tally)
        del m
    if form != "f32":
        tally.close("%s %s %s N=%d" % (name, form, order, n))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["f32", "u8"])
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("apart", ["height", "batch"])
def test_the_same_widths_at_another_height_or_batch_share_nothing(hip_device, name, form, apart):
    """Controls: the wide and the narrow width at two heights, or at two batch sizes, never had a buffer in common.  (The
    heights are this test's own, so that no other test's shapes meet these.)"""
    order = [(1, 9, 23), (1, 11, 21)] if apart == "height" else [(3, 10, 23), (1, 10, 21)]
    tally = _Bytes()
    _walk(_plugin(name, True), form, name, order, tally)
    if form != "f32":
        tally.close("%s %s apart in %s" % (name, form, apart))


SE_ORDERS = {"square-after-7x6": [(1, 7, 6), (1, 7, 7)],        # 8 N slots of 7 x 7 after 4 N of 7 x 6 and 4 N of 6 x 7
             "7x22-after-7x23": [(1, 7, 23), (1, 7, 22)],       # 4 N slots each way: also the transposed forward, 22 x 7
             "2x7x6-after-square": [(1, 7, 7), (2, 7, 6)]}      # 8 slots of 7 x 6 in the buffer of the square's 8 slots


@pytest.mark.gpu
@pytest.mark.parametrize("order", list(SE_ORDERS))
@pytest.mark.parametrize("form", ["se_f32", "se_u8"])
@pytest.mark.parametrize("name", MODELS)
def test_self_ensemble_slots_keep_their_own_pad_columns(hip_device, name, form, order):
    tally = _Bytes()
    m = _plugin(name, True, ["--self_ensemble"])
    _walk(m, form, name, SE_ORDERS[order], tally, extra=["--self_ensemble"])
    if form == "se_u8":
        tally.close("%s %s %s" % (name, form, order))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["f32", "u8"])
@pytest.mark.parametrize("name", MODELS)
def test_two_plugins_of_one_process_replay_side_by_side(hip_device, name, form):
    """Plugin A captures width 22 and plugin B, with other weights, width 21: the class-level cache is theirs in common.
    Replayed alternately, each equals its own eager twin."""
    a, b = _plugin(name, True, seed=SEED), _plugin(name, True, seed=SEED + 1)
    tally = _Bytes()
    turns = [(a, SEED, 22)] * 3 + [(b, SEED + 1, 21)] * 3 + [(a, SEED, 22), (b, SEED + 1, 21)] * 3
    for k, (m, seed, w) in enumerate(turns):
        items = _items(form, 1, H, w, 100 + k)
        got = _run(m, form, items, H, w, k)
        what = "%s %s plugin of seed %d, width %d, turn %d" % (name, form, seed, w, k)
        _same_bits(form, got[0], _alone(form, _twin(name, seed=seed), items[0], H, w), what)
        _near_float64(form, got[0], _expect(form, name, seed, torch.float64, items[0], H, w), what, tally)
    for m in (a, b):
        table = getattr(m, TABLE[form])
        assert len(table) == 1 and all(v is not False for v in table.values())
    if form == "u8":
        tally.close("%s two plugins" % name)


# ---------------------------------------------------------------- 2. sensitivity, on the CPU
PAIRS = [(wide, narrow) for ws in CLASSES.values() for wide in ws for narrow in ws if narrow < wide]


@pytest.mark.parametrize("name", MODELS)
def test_an_extra_input_column_moves_the_right_edge(name):
    """Part 1 can see a leak: the oracle on the narrow image with the wide image's column W appended, cropped back to the
    narrow output's 4 W columns, is more than 100 float bars (0.2 on the 0..255 scale) away from the plain narrow output
    somewhere in the last 8 HR columns.  The margin is derived, not measured: the extra column reaches the last real
    column through the head's three right-hand taps, a pixel >= 64 times nine head weights of order 0.03 each moves a
    feature by order 1, and the exit's gain to the image is of order 1.  Every (wide, narrow) pair of part 1, both batch
    sizes, the first image shown."""
    for wide, narrow in PAIRS:
        for n in (1, 3):
            a, b = _chw(_rgb(n, H, narrow, 0)[0]), _chw(_rgb(n, H, wide, 0)[0])
            leaked = np.concatenate([a, b[:, :, narrow:narrow + 1]], axis=2)
            plain = _net(name, SEED, torch.float64, a)
            moved = _net(name, SEED, torch.float64, leaked)[:, :, :4 * narrow]
            d = float(np.abs(moved - plain)[:, :, -8:].max())
            assert d > 100 * FLOAT_BAR, (name, wide, narrow, n, d)


def _case_images(form, orders):
    """Every (item, h, w) that _walk shows for `orders`."""
    return [(item, h, w) for order in orders for (n, h, w), k in _schedule(order) for item in _items(form, n, h, w, k)]


@pytest.mark.parametrize("name", MODELS)
def test_fp32_rounds_like_float64_on_these_images(name):
    """The uint8 bar allows U8_SHARE of a case's bytes to round the other way.  The oracle's own fp32 run against its
    float64 run stays inside it (and inside one level) on the images of every uint8 case of part 1, so a correct fp32
    forward can meet the bar."""
    worst = 0.0
    for form in FORMS[1:] + ("se_u8",):
        if form == "exits" and name == "LarvaNetV2":
            continue
        cases = ([[(n, H, w) for w in _widths(form, order, cls)] for cls in CLASSES] for order in ORDERS for n in (1, 3))
        if form == "se_u8":
            cases = [[o] for o in SE_ORDERS.values()]
        for orders in cases:
            tally = _Bytes()
            for item, h, w in _case_images(form, orders):
                tally.add(_expect(form, name, SEED, torch.float32, item, h, w),
                          _expect(form, name, SEED, torch.float64, item, h, w), form)
            assert tally.off <= U8_SHARE * tally.total, (name, form, tally.off, tally.total)
            worst = max(worst, tally.off / tally.total)
    print("%s: worst share of bytes that fp32 rounds the other way: %.5f (allowed %.5f)" % (name, worst, U8_SHARE))


# ---------------------------------------------------------------- 3. streams over a mix of sizes
def _stream_images():
    """The ten images of STREAM_SIZES.  Four are RGBA with real transparency (two batch slots): 5x6, 5x7, the second 12x24
    and 5x5; the 7-row images of widths 23, 21 and 22 are all RGB, so that they meet in one padded input."""
    return [(_rgba(1, h, w, 200 + i) if i in (3, 6, 7, 9) else _rgb(1, h, w, 200 + i))[0]
            for i, (h, w) in enumerate(STREAM_SIZES)]


def _stream_form(image):
    return "rgba" if image.shape[2] == 4 else "u8"


def _check_stream(name, got, images, tally, what):
    twin = _twin(name)
    assert len(got) == len(images)
    for i, (g, a) in enumerate(zip(got, images)):
        form, (h, w) = _stream_form(a), a.shape[:2]
        _same_bits(form, g, _alone(form, twin, a, h, w), "%s image %d (%dx%d)" % (what, i, h, w))
        _near_float64(form, g, _expect(form, name, SEED, torch.float64, a, h, w), "%s image %d" % (what, i), tally)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_image_stream_over_mixed_sizes(hip_device, name, depth):
    """Slots shrink, grow and are viewed at a smaller size after a larger one; 7x21 follows 7x23 and 7x22, RGB and RGBA
    alternate.  Run twice, so that the second pass replays what the first captured."""
    from larvanet_amd import pipeline
    m, images, tally = _plugin(name, True), _stream_images(), _Bytes()
    for run in range(2):
        got = list(pipeline.upscale_stream(m, iter(images), 4, depth=depth, keep_alpha=True))
        _check_stream(name, got, images, tally, "%s stream depth %d pass %d" % (name, depth, run))
    assert len(m._infer_graphs_u8) == 4 and all(v is not False for v in m._infer_graphs_u8.values())
    tally.close("%s stream depth %d" % (name, depth))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_image_stream_over_mixed_sizes_resized_to_one_size(hip_device, name):
    """output_size = (20, 30): the eager twin's call with the same argument bit for bit; image_utils.resize_u8 of the
    float64 image under the uint8 bar (the resize is exact integer arithmetic on the bytes)."""
    from larvanet_amd import pipeline
    m, twin, images, tally = _plugin(name, True), _twin(name), _stream_images(), _Bytes()
    for run in range(2):
        got = list(pipeline.upscale_stream(m, iter(images), 4, depth=2, keep_alpha=True, output_size=SIZE))
        for i, (g, a) in enumerate(zip(got, images)):
            form, (h, w) = _stream_form(a), a.shape[:2]
            what = "%s resized stream pass %d image %d (%dx%d)" % (name, run, i, h, w)
            call = twin.upscale_rgba_u8 if form == "rgba" else twin.upscale_u8
            _same_bits(form, g, call([a], 4, output_size=SIZE)[0], what)
            tally.add(g, _resized(form, name, torch.float64, a), what)
    tally.close("%s resized stream" % name)


def _resized(form, name, dtype, a):
    """upscale_u8 / upscale_rgba_u8 with output_size = SIZE by the oracle: colour and alpha resized before the merge."""
    h, w = a.shape[:2]
    if form == "u8":
        return U.resize_u8(_expect("u8", name, SEED, dtype, a, h, w), *SIZE)
    slots, _ = U.alpha_slots([False])
    planes = U.rgba_split_f32(a[None], slots)
    return U.rgba_merge_u8(np.stack([U.resize_u8(_q(_net(name, SEED, dtype, p)), *SIZE) for p in planes]), slots, 1)[0]


@pytest.mark.parametrize("name", MODELS)
def test_fp32_rounds_like_float64_on_the_stream_images(name):
    """The CPU check of the uint8 bar for part 3's images, resized ones included."""
    images = _stream_images()
    plain, sized, video = _Bytes(), _Bytes(), _Bytes()
    for a in images:
        form, (h, w) = _stream_form(a), a.shape[:2]
        plain.add(_expect(form, name, SEED, torch.float32, a, h, w), _expect(form, name, SEED, torch.float64, a, h, w), "plain")
        sized.add(_resized(form, name, torch.float32, a), _resized(form, name, torch.float64, a), "sized")
    for i, (h, w) in enumerate(STREAM_SIZES):
        f = _frames(1, h, w, 300 + i)[0]
        video.add(_expect("yuv", name, SEED, torch.float32, f, h, w), _expect("yuv", name, SEED, torch.float64, f, h, w), "video")
    for tally in (plain, sized, video):
        assert tally.off <= U8_SHARE * tally.total, (name, tally.off, tally.total)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_video_stream_over_mixed_sizes(hip_device, name, depth):
    from larvanet_amd import pipeline
    m, twin, tally = _plugin(name, True), _twin(name), _Bytes()
    triples = [(_frames(1, h, w, 300 + i)[0], w, h) for i, (h, w) in enumerate(STREAM_SIZES)]
    for run in range(2):
        got = list(pipeline.upscale_yuv_stream(m, iter(triples), 4, depth=depth))
        assert len(got) == len(triples)
        for i, (g, (f, w, h)) in enumerate(zip(got, triples)):
            what = "%s video stream depth %d pass %d frame %d (%dx%d)" % (name, depth, run, i, h, w)
            _same_bits("yuv", g, _alone("yuv", twin, f, h, w), what)
            tally.add(g, _expect("yuv", name, SEED, torch.float64, f, h, w), what)
    assert all(v is not False for v in m._infer_graphs_u8.values())
    tally.close("%s video stream depth %d" % (name, depth))


def _same_record(a, b):   # (tests/test_metrics_device.py's _same)
    return a["sse"] == b["sse"] and a["n"] == b["n"] and a["psnr"] == b["psnr"] and a["ssim"] == b["ssim"]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_evaluate_stream_over_mixed_sizes(hip_device, name, depth):
    """(lr, truth) and (None, truth) pairs alternate; the truth of a made input is exactly 4H x 4W, the others are a
    little larger than the output, as validation truths are."""
    from larvanet_amd import kernels as K
    from larvanet_amd import pipeline
    m, twin, tally = _plugin(name, True), _twin(name), _Bytes()
    pairs = []
    for i, (h, w) in enumerate(STREAM_SIZES):
        if i % 3 == 2:
            pairs.append((None, _rgb(1, 4 * h, 4 * w, 400 + i)[0]))
        else:
            pairs.append((_rgb(1, h, w, 400 + i)[0], _rgb(1, 4 * h + 1, 4 * w + 2, 400 + i)[0]))
    for run in range(2):
        got = list(pipeline.evaluate_stream(m, iter(pairs), 4, depth=depth, keep_images=True))
        assert len(got) == len(pairs)
        for i, ((record, image), (lr, truth)) in enumerate(zip(got, pairs)):
            what = "%s evaluate stream depth %d pass %d pair %d" % (name, depth, run, i)
            t = torch.from_numpy(truth[None]).to(hip_device)
            x = K.bicubic_down_u8(t[0], 4)[None] if lr is None else torch.from_numpy(lr[None]).to(hip_device)
            assert _same_record(record, twin.evaluate_u8_tensor(x, t)[0]), (what, record)
            lr = x[0].cpu().numpy()
            _same_bits("u8", image, _alone("u8", twin, lr, *lr.shape[:2]), what)
            tally.add(image, _expect("u8", name, SEED, torch.float64, lr, *lr.shape[:2]), what)
    tally.close("%s evaluate stream depth %d" % (name, depth))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_an_abandoned_stream_leaves_nothing_behind(hip_device, name):
    from larvanet_amd import pipeline
    m, tally = _plugin(name, True), _Bytes()
    images = _stream_images()[:6]
    gen = pipeline.upscale_stream(m, iter(images), 4, depth=3, keep_alpha=True)
    first = [next(gen), next(gen)]
    gen.close()
    _check_stream(name, first, images[:2], tally, "%s abandoned stream" % name)
    for run in range(2):
        got = list(pipeline.upscale_stream(m, iter(images), 4, depth=3, keep_alpha=True))
        _check_stream(name, got, images, tally, "%s stream after an abandoned one, pass %d" % (name, run))
    tally.close("%s abandoned stream" % name)


# ---------------------------------------------------------------- 4. training and inference interleaved
def _trainer(name, seed=5):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(TINY)
    torch.manual_seed(seed)
    m.prepare(is_training=True, scales=[4])
    m.strict_graph = True
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_captured_inference_between_captured_training_steps(hip_device, name, tmp_path):
    """Three captured training steps on (4, 3, 8, 8) with upscale() of a (4, 3, 8, 8) batch three times after each (eager,
    captured, replayed from then on): the captured step and the captured forward write the same block of the same
    (4, 16, 8, 8) padded input.  Losses and final weights equal a twin's that trained undisturbed, bit for bit, and every
    upscale equals an eager plugin's that was handed the weights of that moment."""
    g = torch.Generator().manual_seed(43)
    steps = [((torch.rand(4, 3, 8, 8, generator=g) * 255).to(hip_device),
              (torch.rand(4, 3, 32, 32, generator=g) * 255).to(hip_device)) for _ in range(3)]
    args = types.SimpleNamespace(train_path=str(tmp_path))
    busy, calm, eager = _trainer(name), _trainer(name), _plugin(name, False, seed=99)
    assert busy.use_hip_graph and calm.use_hip_graph
    losses = [[], []]
    for s, (x, t) in enumerate(steps):
        losses[0].append(busy.train_step_larva(args, FakeValLoader(7), x, t))
        losses[1].append(calm.train_step_larva(args, FakeValLoader(7), x, t))
        eager.restore(busy.save(str(tmp_path)))
        for k in range(3):
            batch = list(_chw(_rgb(4, 8, 8, 10 * s + k)))
            got = busy.upscale(batch, 4)
            for i, image in enumerate(batch):
                _same_bits("f32", got[i], eager.upscale([image], 4)[0], "%s after step %d, call %d, image %d" % (name, s + 1, k, i))
        assert busy._step is not None and busy.use_hip_graph and busy.hip_graph_fell_back is None
    assert len(busy._infer_graphs) == 1 and all(v is not False for v in busy._infer_graphs.values())
    assert losses[0] == losses[1], losses
    calm_sd = calm.model.state_dict()
    for k, v in busy.model.state_dict().items():
        assert torch.equal(v, calm_sd[k]), k


# ---------------------------------------------------------------- 5. fp16 as a regression control
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("form", ["f32", "u8"])
@pytest.mark.parametrize("name", MODELS)
def test_fp16_widths_of_one_row_pitch(hip_device, name, form, n):
    """The fp16 forward pads no input (channels-last activations, no 16-channel image): captured equals eager."""
    for cls in CLASSES:
        m = _plugin(name, True, precision="fp16")
        _walk(m, form, name, [(n, H, w) for w in ORDERS["descending"][cls]], None, precision="fp16")
        assert m.fp16_overflowed() is False
        del m
