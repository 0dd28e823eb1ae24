"""larvanet_amd.upscale_images: a folder of PNGs in, a folder of upscaled PNGs out.  The host logic (flags, listing,
sharding, naming, an empty folder) runs anywhere; the end-to-end run is marked gpu."""
import importlib
import os

import numpy as np
import pytest
import torch


def _blocks_image(seed, h, w):
    """uint8 (h, w, 3): hard-edged 8 x 8 blocks, every block and colour drawn from {0, 64, 200, 255}."""
    rng = np.random.default_rng(seed)
    levels = np.array([0, 64, 200, 255], np.uint8)
    grid = levels[rng.integers(0, 4, ((h + 7) // 8, (w + 7) // 8, 3))]
    return np.ascontiguousarray(np.repeat(np.repeat(grid, 8, 0), 8, 1)[:h, :w])


def test_flags_match_the_reference_tool_and_model_flags_pass_through():
    from larvanet_amd import upscale_images as U
    args, rest = U.build_parser().parse_known_args([])
    assert (args.model, args.scale, args.cuda_device, args.restore_path, args.restore_target, args.restore_global_step,
            args.input_path, args.output_path, args.io_threads) == ("LarvaNet", 4, None, None, None, 0, "LR", "SR", None)
    args, rest = U.build_parser().parse_known_args(
        ["--model=LarvaNetV2", "--scale=2", "--cuda_device=3", "--restore_path=a.pth", "--restore_target=t",
         "--restore_global_step=7", "--input_path=in", "--output_path=out", "--io_threads=3", "--num_modules=4",
         "--precision=fp16"])
    assert (args.model, args.scale, args.cuda_device, args.restore_path, args.restore_target, args.restore_global_step,
            args.input_path, args.output_path, args.io_threads) == ("LarvaNetV2", 2, "3", "a.pth", "t", 7, "in", "out", 3)
    assert rest == ["--num_modules=4", "--precision=fp16"]
    assert not hasattr(args, "chop_forward")


def test_listing_is_sorted_and_case_insensitive(tmp_path):
    from larvanet_amd import upscale_images as U
    for f in ("b.png", "a.PNG", "c.Png", "d.jpg", "e.png.txt", "0010.png", "0002.png"):
        (tmp_path / f).write_bytes(b"")
    assert U.list_pngs(str(tmp_path)) == ["0002.png", "0010.png", "a.PNG", "b.png", "c.Png"]


def test_sharding_and_output_names():
    from larvanet_amd import upscale_images as U
    files = ["%02d.png" % i for i in range(7)]
    for world in (1, 2, 3, 8):
        parts = [U.shard(files, r, world) for r in range(world)]
        assert parts == [files[r::world] for r in range(world)]
        assert sorted(f for p in parts for f in p) == files
    assert U.output_name("a.PNG") == "a.png" and U.output_name("x.y.png") == "x.y.png"


def test_io_threads_default_and_cap_are_this_ranks_share_of_the_cores(monkeypatch):
    from larvanet_amd import dist, upscale_images as U
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    cap = dist.host_threads()
    assert U.io_threads(None) == cap and U.io_threads(10 ** 6) == cap and U.io_threads(0) == 1 and U.io_threads(1) == 1
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    assert U.io_threads(None) == 1 and U.io_threads(64) == 1


def test_an_empty_folder_exits_cleanly_without_a_device(tmp_path, capsys):
    from larvanet_amd import upscale_images as U
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "notes.txt").write_text("no images here")
    out = U.main(["--input_path", str(tmp_path / "in"), "--output_path", str(tmp_path / "out")])
    assert out == {} and os.listdir(str(tmp_path / "out")) == []
    assert "0 images" in capsys.readouterr().out


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_main_writes_upscale_u8_of_every_decoded_input(hip_device, tmp_path, precision):
    from PIL import Image
    from larvanet_amd import upscale_images as U
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rgb = {"b_02.png": _blocks_image(1, 40, 56), "a_01.png": _blocks_image(2, 33, 47), "c_03.PNG": _blocks_image(3, 40, 56),
           "e_05.png": _blocks_image(4, 33, 47)}
    for name, a in rgb.items():
        Image.fromarray(a).save(str(src / name), format="PNG")
    grey = _blocks_image(5, 40, 56)[:, :, 0]
    Image.fromarray(grey).save(str(src / "d_04.png"))
    rgb["d_04.png"] = np.ascontiguousarray(np.repeat(grey[:, :, None], 3, 2))
    (src / "readme.txt").write_text("not an image")
    flags = ["--num_modules=4", "--num_blocks=4,4,4,4", "--precision=" + precision]
    torch.manual_seed(0)
    durations = U.main(["--input_path", str(src), "--output_path", str(dst), "--io_threads=3"] + flags)
    assert list(durations) == sorted(rgb) and all(v > 0 for v in durations.values())
    assert sorted(os.listdir(str(dst))) == sorted(os.path.splitext(n)[0] + ".png" for n in rgb)
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(flags)
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    for name, a in rgb.items():
        got = np.asarray(Image.open(str(dst / (os.path.splitext(name)[0] + ".png"))))
        assert got.dtype == np.uint8 and np.array_equal(got, m.upscale_u8([a], 4)[0]), name
