"""larvanet_amd.y4m (the YUV4MPEG2 reader and writer) and the larvanet_amd.upscale_video driver.  The Y4M and argument
tests run anywhere; the end-to-end runs start the module in a child process on the GPU."""
import gc
import importlib
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from larvanet_amd import upscale_video as V
from larvanet_amd import y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(n, w, h, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):   # smooth luma, chroma near the centre: a frame a network takes at any precision
        yy, xx = np.mgrid[0:h, 0:w]
        y = (40 + 150 * (xx + yy) / (w + h) + rng.integers(0, 12, (h, w))).astype(np.uint8)
        c = rng.integers(100, 156, 2 * ((w + 1) // 2) * ((h + 1) // 2)).astype(np.uint8)
        out.append(np.concatenate([y.reshape(-1), c]))
    return out


def _stream_bytes(header, frames):
    b = io.BytesIO()
    y4m.write_header(b, header)
    for f in frames:
        y4m.write_frame(b, f)
    return b.getvalue()


# ---------------------------------------------------------------- Y4M (host)
def test_header_round_trip_and_scaling():
    h = y4m.Header(64, 48, "30000:1001", "p", "1:1", "420jpeg", ["YSCSS=420JPEG", "COLORRANGE=LIMITED"])
    line = h.to_bytes()
    assert line == b"YUV4MPEG2 W64 H48 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=LIMITED\n"
    back = y4m.parse_header(line)
    assert back == h and back.to_bytes() == line and back.frame_bytes == 64 * 48 * 3 // 2
    assert (back.width, back.height, back.fps, back.interlace, back.aspect, back.chroma) == (64, 48, "30000:1001", "p", "1:1",
                                                                                           "420jpeg")
    assert back.comments == ("YSCSS=420JPEG", "COLORRANGE=LIMITED")
    up = h.scaled(3)
    assert up.to_bytes() == b"YUV4MPEG2 W192 H144 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=LIMITED\n"
    bare = y4m.parse_header(b"YUV4MPEG2 W5 H3\n")   # no C tag, odd sizes
    assert bare.chroma is None and bare.frame_bytes == 15 + 2 * 3 * 2 and bare.to_bytes() == b"YUV4MPEG2 W5 H3\n"
    assert bare.full_range is None and bare.siting_warning() is None


@pytest.mark.parametrize("chroma", ["420jpeg", "420mpeg2", "420paldv", "420"])
def test_accepted_colour_spaces_and_the_siting_warning(chroma):
    h = y4m.parse_header(("YUV4MPEG2 W8 H8 F25:1 C%s\n" % chroma).encode())
    assert h.chroma == chroma
    warning = h.siting_warning()
    if chroma in ("420mpeg2", "420paldv"):
        assert warning and "centred" in warning and "\n" not in warning
    else:
        assert warning is None


@pytest.mark.parametrize("tag", ["C444", "C422", "Cmono", "C420p10", "C420p12", "C420p16", "C444p10", "C422p12", "C444alpha",
                                 "It", "Ib", "Im"])
def test_refusals(tag):
    with pytest.raises(ValueError, match="not supported"):
        y4m.parse_header(("YUV4MPEG2 W8 H8 F25:1 %s\n" % tag).encode())
    with pytest.raises(ValueError, match="not supported"):
        y4m.read_header(io.BytesIO(("YUV4MPEG2 W8 H8 %s\nFRAME\n" % tag).encode()))


def test_bad_streams():
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        y4m.parse_header(b"RIFF W8 H8\n")
    with pytest.raises(ValueError, match="no W or no H"):
        y4m.parse_header(b"YUV4MPEG2 W8 F25:1\n")
    with pytest.raises(ValueError, match="empty"):
        y4m.read_header(io.BytesIO(b""))
    with pytest.raises(ValueError, match="ends inside the header"):
        y4m.read_header(io.BytesIO(b"YUV4MPEG2 W8 H8"))
    with pytest.raises(ValueError):
        y4m.Header(0, 8)


def test_multi_frame_streams_and_the_truncated_frame_error():
    h = y4m.Header(6, 5, "25:1", None, None, "420jpeg", ())
    frames = _frames(3, 6, 5)
    data = _stream_bytes(h, frames)
    s = io.BytesIO(data)
    back = y4m.read_header(s)
    got = list(y4m.read_frames(s, back))
    assert back == h and len(got) == 3 and all(g.dtype == np.uint8 and np.array_equal(g, f) for g, f in zip(got, frames))
    # FRAME lines may carry parameters
    s = io.BytesIO(data.replace(b"FRAME\n", b"FRAME Ip\n"))
    assert len(list(y4m.read_frames(s, y4m.read_header(s)))) == 3

    class Dribble(io.BytesIO):   # a pipe: short reads
        def read(self, n=-1):
            return super().read(min(n, 7) if n and n > 0 else n)

    s = Dribble(data)
    assert all(np.array_equal(g, f) for g, f in zip(y4m.read_frames(s, y4m.read_header(s)), frames))
    for cut in (1, 20):
        s = io.BytesIO(data[:-cut])
        hh = y4m.read_header(s)
        seen = []
        with pytest.raises(ValueError, match="frame 2 is truncated"):
            for f in y4m.read_frames(s, hh):
                seen.append(f)
        assert len(seen) == 2
    s = io.BytesIO(data[:len(h.to_bytes()) + 6 + h.frame_bytes] + b"JUNK!\n" + b"x" * h.frame_bytes)
    hh = y4m.read_header(s)
    with pytest.raises(ValueError, match="frame 1 does not start with FRAME"):
        list(y4m.read_frames(s, hh))
    raw = b"".join(f.tobytes() for f in frames)
    assert all(np.array_equal(g, f) for g, f in zip(y4m.read_raw_frames(io.BytesIO(raw), 6, 5), frames))
    with pytest.raises(ValueError, match="frame 2 is truncated"):
        list(y4m.read_raw_frames(io.BytesIO(raw[:-3]), 6, 5))


def test_xcolorrange_selects_the_range_unless_the_flag_is_given():
    parse = V.build_parser().parse_args
    for comment, said in (("XCOLORRANGE=FULL", True), ("XCOLORRANGE=LIMITED", False), ("", None)):
        data = ("YUV4MPEG2 W4 H4 F25:1 C420jpeg %s" % comment).strip().encode() + b"\n"
        assert y4m.parse_header(data).full_range is said
        for flag, want in ((None, bool(said)), ("full", True), ("limited", False)):
            args = parse(["--input", "-", "--output", "-"] + (["--range", flag] if flag else []))
            header, size, full, frames, _ = V.open_input(args, io.BytesIO(data))
            assert size == (4, 4) and full is want and header.full_range is said and list(frames) == []


# ---------------------------------------------------------------- the driver's checks that need no device
def test_cli_refuses_bad_arguments_and_unsupported_streams_before_any_device_work(tmp_path, monkeypatch):
    def no_model(name):
        raise AssertionError("the model was prepared before the input was checked")

    monkeypatch.setattr(V, "importlib", types.SimpleNamespace(import_module=no_model))
    src = tmp_path / "in.yuv"
    src.write_bytes(b"\0" * 24)
    for argv in (["--input", str(src), "--output", "-"],                                   # .yuv without a size
                 ["--input", str(src), "--output", "-", "--width", "4"],
                 ["--input", str(src), "--output", "-", "--width", "0", "--height", "4"],
                 ["--input", str(tmp_path / "in.y4m"), "--output", "-", "--width", "4", "--height", "4"],
                 ["--input", str(src), "--output", "-", "--width", "4", "--height", "4", "--depth", "0"],
                 ["--input", str(src), "--output", "-", "--width", "4", "--height", "4", "--scale", "5"]):
        with pytest.raises(ValueError):
            V.main(argv)
    with pytest.raises(SystemExit):
        V.main(["--input", str(src), "--output", "-", "--width", "4", "--height", "4", "--matrix", "bt2020"])
    for tag in ("C444", "C420p10", "It"):
        bad = tmp_path / ("bad_%s.y4m" % tag)
        bad.write_bytes(("YUV4MPEG2 W4 H4 F25:1 %s\nFRAME\n" % tag).encode() + b"\0" * 48)
        out = tmp_path / "never.y4m"
        with pytest.raises(ValueError, match="not supported"):
            V.main(["--input", str(bad), "--output", str(out)])
        assert not out.exists()
    args = V.build_parser().parse_args(["--input", "-", "--output", "-", "--width", "8", "--height", "6"])
    assert V.input_is_y4m(args) is False
    assert V.input_is_y4m(V.build_parser().parse_args(["--input", "-", "--output", "-"])) is True


# ---------------------------------------------------------------- end to end (GPU, a child process)
MODEL_FLAGS = ["--model=LarvaNet", "--num_modules=2", "--num_blocks=2,2", "--scale=4"]


def _expected(frames, w, h, matrix, full_range, ckpt):
    gc.collect()   # (no dropped model's captured graph may be freed while this one captures: tests/test_yuv.py, _collect)
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(MODEL_FLAGS[1:3])
    m.prepare(is_training=False, scales=[4])
    m.restore(ckpt)
    return [m.upscale_yuv420([f], 4, w, h, matrix, full_range)[0] for f in frames]


def _checkpoint(tmp_path):
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(MODEL_FLAGS[1:3])
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    return m.save(str(tmp_path))


def _run_module(argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "larvanet_amd.upscale_video"] + argv, cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.gpu
def test_upscale_video_y4m_end_to_end(hip_device, tmp_path):
    w, h = 64, 48
    frames = _frames(4, w, h, seed=3)
    header = y4m.Header(w, h, "24:1", "p", "1:1", "420mpeg2", ["COLORRANGE=FULL", "note"])
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(_stream_bytes(header, frames))
    ckpt = _checkpoint(tmp_path)
    r = _run_module(MODEL_FLAGS + ["--restore_path", ckpt, "--input", str(src), "--output", str(dst), "--matrix", "bt709"])
    log = r.stderr.decode(errors="replace")
    assert r.returncode == 0, log
    assert log.count("treated as centred") == 1 and "finished: 4 frames" in log and "frames per second" in log
    with open(dst, "rb") as s:
        back = y4m.read_header(s)
        got = list(y4m.read_frames(s, back))
    assert back == header.scaled(4) and (back.width, back.height) == (256, 192)
    assert (back.fps, back.aspect, back.chroma, back.comments) == ("24:1", "1:1", "420mpeg2", ("COLORRANGE=FULL", "note"))
    want = _expected(frames, w, h, "bt709", True, ckpt)   # (XCOLORRANGE=FULL selected full range)
    assert len(got) == 4 and all(np.array_equal(g, t) for g, t in zip(got, want))


@pytest.mark.gpu
def test_upscale_video_headerless_yuv_end_to_end(hip_device, tmp_path):
    w, h = 64, 48
    frames = _frames(4, w, h, seed=4)
    src, dst = tmp_path / "in.yuv", tmp_path / "out.yuv"
    src.write_bytes(b"".join(f.tobytes() for f in frames))
    ckpt = _checkpoint(tmp_path)
    r = _run_module(MODEL_FLAGS + ["--restore_path", ckpt, "--input", str(src), "--output", str(dst), "--width", str(w),
                                   "--height", str(h), "--depth", "3"])
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert "finished: 4 frames" in r.stderr.decode(errors="replace")
    with open(dst, "rb") as s:
        got = list(y4m.read_raw_frames(s, 4 * w, 4 * h))
    want = _expected(frames, w, h, "bt601", False, ckpt)
    assert len(got) == 4 and all(np.array_equal(g, t) for g, t in zip(got, want))
    # a truncated last frame is an error that names the frame
    src.write_bytes(b"".join(f.tobytes() for f in frames)[:-10])
    r = _run_module(MODEL_FLAGS + ["--restore_path", ckpt, "--input", str(src), "--output", str(dst), "--width", str(w),
                                   "--height", str(h)])
    assert r.returncode != 0 and "frame 3 is truncated" in r.stderr.decode(errors="replace")
