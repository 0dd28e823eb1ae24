"""What each stream of pipeline.py launches per item, in order: the kernels wrappers around the forward are recorded, and
the last launch of an item must have been handed the slot's own buffer (out= / result=), which is what shows that no copy
was added between it and the host link.  The yielded bytes equal the non-stream entry point's.  Each stream runs at depth
2 over items of one shape, so the forward runs eagerly, is captured and is replayed."""
import gc

import numpy as np
import pytest
import torch

from larvanet_amd import image_utils as U

RECORDED = ("alpha_slot_table", "rgba_u8_split_f32", "rgb_u8_merge_rgba", "resize_u8", "i420_to_rgb_f32", "rgb_u8_to_i420",
            "bicubic_down_u8", "u8_metrics")
SIZE = (20, 30)


def _model():
    from larvanet_amd.models import LarvaNet as L
    gc.collect()   # (a dropped plugin's captured graphs must be gone before the next capture: see tests/test_yuv.py)
    m = L.create_model()
    m.parse_args(["--num_modules=2", "--num_blocks=1,1", "--precision=fp32"])
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    m.strict_graph = True
    return m


def _recording(monkeypatch, m):
    """-> the log [(name, keyword arguments)] that every recorded wrapper and m._infer_u8_images append to."""
    from larvanet_amd import kernels as K
    log = []

    def spy(name, inner):
        def call(*a, **k):
            log.append((name, k))
            return inner(*a, **k)
        return call

    for name in RECORDED:
        monkeypatch.setattr(K, name, spy(name, getattr(K, name)))
    monkeypatch.setattr(m, "_infer_u8_images", spy("_infer_u8_images", m._infer_u8_images))
    return log


def _taken(log):
    names, last = [name for name, _ in log], [k for _, k in log]
    del log[:]
    return names, last


def _smooth(seed, h, w, c=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = 40 + 150 * (xx + yy) / max(1, w + h - 2)
    return np.ascontiguousarray(np.stack([ramp + rng.integers(0, 12, (h, w))] * c, axis=-1).astype(np.uint8))


def _check(log, per_item, items, last_key):
    """The log is `items` times per_item, and each item's last launch was given a destination under last_key."""
    names, kwargs = _taken(log)
    assert names == per_item * items
    if last_key is not None:
        for i in range(items):
            assert kwargs[(i + 1) * len(per_item) - 1].get(last_key) is not None, (i, per_item[-1])


@pytest.mark.gpu
def test_rgb_stream_launches(hip_device, monkeypatch):
    from larvanet_amd import pipeline
    m = _model()
    log = _recording(monkeypatch, m)
    images = [_smooth(i, 9, 14) for i in range(3)]
    got = list(pipeline.upscale_stream(m, iter(images), 4, depth=2))
    _check(log, ["_infer_u8_images"], 3, None)
    sized = list(pipeline.upscale_stream(m, iter(images), 4, depth=2, output_size=SIZE))
    _check(log, ["_infer_u8_images", "resize_u8"], 3, "out")
    assert all(v is not False for v in m._infer_graphs_u8.values()) and len(m._infer_graphs_u8) == 1
    for a, g, s in zip(images, got, sized):
        assert np.array_equal(g, m.upscale_u8([a], 4)[0])
        assert s.shape == SIZE + (3,) and np.array_equal(s, m.upscale_u8([a], 4, output_size=SIZE)[0])


@pytest.mark.gpu
def test_rgba_stream_launches(hip_device, monkeypatch):
    from larvanet_amd import pipeline
    m = _model()
    log = _recording(monkeypatch, m)
    images = []
    for i in range(4):   # three with real transparency (eager, capture, replay), then an opaque one
        a = _smooth(i, 6, 8, 4)
        a[..., 3] = 255 if i == 3 else np.linspace(0, 255, 48).reshape(6, 8).astype(np.uint8)
        images.append(a)
    got = list(pipeline.upscale_stream(m, iter(images), 4, depth=2, keep_alpha=True))
    _check(log, ["alpha_slot_table", "rgba_u8_split_f32", "_infer_u8_images", "rgb_u8_merge_rgba"], 4, "out")
    sized = list(pipeline.upscale_stream(m, iter(images), 4, depth=2, keep_alpha=True, output_size=SIZE))
    _check(log, ["alpha_slot_table", "rgba_u8_split_f32", "_infer_u8_images", "resize_u8", "rgb_u8_merge_rgba"], 4, "out")
    assert all(v is not False for v in m._infer_graphs_u8.values()) and len(m._infer_graphs_u8) == 2
    for a, g, s in zip(images, got, sized):
        assert g.shape == (24, 32, 4) and np.array_equal(g, m.upscale_rgba_u8([a], 4)[0])
        assert s.shape == SIZE + (4,) and np.array_equal(s, m.upscale_rgba_u8([a], 4, output_size=SIZE)[0])
    assert np.all(got[3][..., 3] == 255) and int(np.ptp(got[0][..., 3])) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(8, 6), (9, 7)], ids=["even", "odd"])
def test_video_stream_launches(hip_device, monkeypatch, w, h):
    from larvanet_amd import pipeline
    m = _model()
    log = _recording(monkeypatch, m)
    rng = np.random.default_rng(w)
    frames = [rng.integers(16, 236, U.i420_frame_bytes(w, h), dtype=np.uint8) for _ in range(3)]
    got = list(pipeline.upscale_yuv_stream(m, iter(frames), 4, w, h, depth=2))
    _check(log, ["i420_to_rgb_f32", "_infer_u8_images", "rgb_u8_to_i420"], 3, "out")
    sized = list(pipeline.upscale_yuv_stream(m, ((f, w, h) for f in frames), 4, depth=2, output_size=SIZE))
    _check(log, ["i420_to_rgb_f32", "_infer_u8_images", "resize_u8", "rgb_u8_to_i420"], 3, "out")
    assert all(v is not False for v in m._infer_graphs_u8.values()) and len(m._infer_graphs_u8) == 1
    for f, g, s in zip(frames, got, sized):
        assert g.shape == (U.i420_frame_bytes(4 * w, 4 * h),) and np.array_equal(g, m.upscale_yuv420([f], 4, w, h)[0])
        assert s.shape == (U.i420_frame_bytes(SIZE[1], SIZE[0]),)
        assert np.array_equal(s, m.upscale_yuv420([f], 4, w, h, output_size=SIZE)[0])


@pytest.mark.gpu
def test_evaluate_stream_launches(hip_device, monkeypatch):
    from larvanet_amd import kernels as K
    from larvanet_amd import pipeline
    m = _model()
    log = _recording(monkeypatch, m)
    truths = [_smooth(10 + i, 36, 56) for i in range(3)]
    lrs = [_smooth(i, 9, 14) for i in range(3)]
    got = list(pipeline.evaluate_stream(m, zip(lrs, truths), 4, depth=2))
    _check(log, ["_infer_u8_images", "u8_metrics"], 3, "result")
    made = list(pipeline.evaluate_stream(m, [(None, t) for t in truths], 4, depth=2, keep_images=True))
    names, kwargs = _taken(log)
    assert names == ["bicubic_down_u8", "_infer_u8_images", "u8_metrics"] * 3
    assert all(kwargs[3 * i].get("out") is not None and kwargs[3 * i + 2].get("result") is not None for i in range(3))
    assert all(v is not False for v in m._infer_graphs_u8.values()) and len(m._infer_graphs_u8) == 1
    for lr, t, g, (r, image) in zip(lrs, truths, got, made):
        x, truth = torch.from_numpy(lr[None]).to(hip_device), torch.from_numpy(t[None]).to(hip_device)
        assert g == m.evaluate_u8_tensor(x, truth)[0]
        down = K.bicubic_down_u8(truth[0], 4)[None]
        assert r == m.evaluate_u8_tensor(down, truth)[0]
        assert np.array_equal(image, m.upscale_u8_tensor(down)[0].cpu().numpy())
