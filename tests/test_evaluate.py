"""larvanet_amd.evaluate: a folder of truth images and a folder of inputs in, PSNR / SSIM lines out.  The host logic
(flags, pairing, sharding, an empty shard) runs anywhere; the end-to-end run is marked gpu."""
import importlib
import os

import numpy as np
import pytest
import torch

import metrics_ref


def _blocks_image(seed, h, w):
    """uint8 (h, w, 3): hard-edged 8 x 8 blocks, every block and colour drawn from {0, 64, 200, 255}."""
    rng = np.random.default_rng(seed)
    levels = np.array([0, 64, 200, 255], np.uint8)
    grid = levels[rng.integers(0, 4, ((h + 7) // 8, (w + 7) // 8, 3))]
    return np.ascontiguousarray(np.repeat(np.repeat(grid, 8, 0), 8, 1)[:h, :w])


def _truth_for(lr, scale, seed, extra=(0, 0)):
    h, w = lr.shape[0] * scale + extra[0], lr.shape[1] * scale + extra[1]
    big = np.pad(np.repeat(np.repeat(lr, scale, 0), scale, 1).astype(np.int16), ((0, extra[0]), (0, extra[1]), (0, 0)), mode="edge")
    return np.clip(big + np.random.default_rng(seed).integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def test_flags_chain_to_the_model():
    from larvanet_amd import evaluate as E
    args, rest = E.build_parser().parse_known_args([])
    assert (args.model, args.scale, args.cuda_device, args.restore_path, args.input_path, args.truth_path, args.output_path,
            args.channel, args.shave, args.no_ssim, args.log, args.io_threads, args.depth) == \
        ("LarvaNet", 4, None, None, "LR", "HR", None, "y", None, False, None, None, 2)
    args, rest = E.build_parser().parse_known_args(
        ["--model=LarvaNetV2", "--scale=2", "--cuda_device=3", "--restore_path=a.pth", "--input_path=in", "--truth_path=hr",
         "--output_path=out", "--channel=rgb", "--shave=0", "--no_ssim", "--log=l.txt", "--io_threads=3", "--depth=1",
         "--num_modules=4", "--precision=fp16"])
    assert (args.model, args.scale, args.cuda_device, args.restore_path, args.input_path, args.truth_path, args.output_path,
            args.channel, args.shave, args.no_ssim, args.log, args.io_threads, args.depth) == \
        ("LarvaNetV2", 2, "3", "a.pth", "in", "hr", "out", "rgb", 0, True, "l.txt", 3, 1)
    assert rest == ["--num_modules=4", "--precision=fp16"]
    with pytest.raises(SystemExit):
        E.build_parser().parse_known_args(["--channel=cmyk"])


def test_pairing_by_stem_with_the_scale_suffix_and_any_letter_case():
    from larvanet_amd import evaluate as E
    truths = ["0801.png", "0802.PNG", "baby.png", "bird.Png"]
    inputs = ["0801x4.png", "0802x4.png", "0802x2.png", "baby.PNG", "bird.png", "extra.png"]
    assert E.pair_files(truths, inputs, 4) == [("0801.png", "0801x4.png"), ("0802.PNG", "0802x4.png"), ("baby.png", "baby.PNG"),
                                               ("bird.Png", "bird.png")]
    assert E.pair_files(["0802.png"], inputs, 2) == [("0802.png", "0802x2.png")]
    assert E.pair_files(["a.png"], ["a.png", "ax4.png"], 4) == [("a.png", "a.png")]   # (the plain stem comes first)
    with pytest.raises(FileNotFoundError, match="0803.png"):
        E.pair_files(["0801.png", "0803.png"], inputs, 4)
    with pytest.raises(FileNotFoundError, match="0801.png"):
        E.pair_files(["0801.png"], inputs, 3)
    assert E.pair_files([], inputs, 4) == []


def test_sharding_and_result_lines():
    from larvanet_amd import evaluate as E
    pairs = [("%02d.png" % i, "%02dx4.png" % i) for i in range(7)]
    for world in (1, 2, 3, 8):
        parts = [E.shard(pairs, r, world) for r in range(world)]
        assert parts == [pairs[r::world] for r in range(world)] and sorted(p for part in parts for p in part) == pairs
    assert E.result_line(4, 2, 7, {"psnr": 31.23456, "ssim": 0.912345}) == "x4, 2/7, psnr=31.2346, ssim=0.9123"
    assert E.result_line(2, 1, 1, {"psnr": 30.0, "ssim": None}) == "x2, 1/1, psnr=30.0000"


def test_an_empty_shard_launches_nothing(tmp_path, capsys, monkeypatch):
    from larvanet_amd import evaluate as E, pipeline
    (tmp_path / "lr").mkdir()
    (tmp_path / "hr").mkdir()
    (tmp_path / "hr" / "notes.txt").write_text("no images here")

    def never(*a, **k):
        raise AssertionError("the device pipeline was entered for an empty shard")

    monkeypatch.setattr(pipeline, "evaluate_stream", never)
    log = tmp_path / "log.txt"
    out = E.main(["--input_path", str(tmp_path / "lr"), "--truth_path", str(tmp_path / "hr"), "--log", str(log)])
    printed = capsys.readouterr().out
    assert out == {} and "0 images" in printed and "prepare model" not in printed
    assert log.read_text() == "finished\n"


def test_a_truth_without_an_input_is_an_error_naming_the_file(tmp_path):
    from PIL import Image
    from larvanet_amd import evaluate as E
    (tmp_path / "lr").mkdir()
    (tmp_path / "hr").mkdir()
    Image.fromarray(_blocks_image(1, 16, 16)).save(str(tmp_path / "hr" / "lonely.png"))
    with pytest.raises(FileNotFoundError, match="lonely.png"):
        E.main(["--input_path", str(tmp_path / "lr"), "--truth_path", str(tmp_path / "hr")])


@pytest.mark.gpu
@pytest.mark.parametrize("precision,channel,shave", [("fp32", "y", None), ("fp16", "rgb", 0)])
def test_main_prints_the_host_oracles_values_and_writes_upscale_images_output(hip_device, tmp_path, precision, channel, shave):
    from PIL import Image
    from larvanet_amd import evaluate as E, upscale_images as U
    lr_dir, hr_dir, sr_dir, ref_dir = (tmp_path / n for n in ("lr", "hr", "sr", "ref"))
    lr_dir.mkdir()
    hr_dir.mkdir()
    lrs = {"b_02.png": _blocks_image(1, 40, 56), "a_01x4.png": _blocks_image(2, 33, 47), "c_03.png": _blocks_image(3, 40, 56)}
    truths = {}
    for i, (name, a) in enumerate(sorted(lrs.items())):
        Image.fromarray(a).save(str(lr_dir / name))
        truth_name = name.replace("x4", "")
        truths[truth_name] = _truth_for(a, 4, 10 + i, extra=(i, 2 * i))
        Image.fromarray(truths[truth_name]).save(str(hr_dir / truth_name))
    flags = ["--num_modules=4", "--num_blocks=2,2,2,2", "--precision=" + precision]
    log = tmp_path / "log.txt"
    argv = ["--input_path", str(lr_dir), "--truth_path", str(hr_dir), "--output_path", str(sr_dir), "--log", str(log),
            "--channel", channel, "--io_threads=3"] + ([] if shave is None else ["--shave", str(shave)])
    torch.manual_seed(0)
    results = E.main(argv + flags)
    assert list(results) == sorted(truths)
    torch.manual_seed(0)
    U.main(["--input_path", str(lr_dir), "--output_path", str(ref_dir), "--io_threads=3"] + flags)
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(flags)
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[4])
    lines = log.read_text().splitlines()
    eff = 4 if shave is None else shave
    psnrs, ssims = [], []
    for i, truth_name in enumerate(sorted(truths)):
        lr_name = truth_name if truth_name in lrs else truth_name.replace(".png", "x4.png")
        image = m.upscale_u8([lrs[lr_name]], 4)[0]
        got = np.asarray(Image.open(str(sr_dir / truth_name)))
        assert np.array_equal(got, image) and np.array_equal(got, np.asarray(Image.open(str(ref_dir / lr_name))))
        want = metrics_ref.evaluate(image, truths[truth_name], eff, channel)
        assert lines[i] == "x4, %d/3, psnr=%.4f, ssim=%.4f" % (i + 1, want["psnr"], want["ssim"]), (lines[i], want)
        assert results[truth_name]["sse"] == want["sse"]
        psnrs.append(want["psnr"])
        ssims.append(want["ssim"])
    assert lines[3] == "finished"
    assert lines[4] == "- average psnr=%.4f, ssim=%.4f" % (np.mean(psnrs), np.mean(ssims))
    assert lines[5].startswith("- duration: ") and len(lines) == 6
    # PSNR only, nothing written
    results = E.main(["--input_path", str(lr_dir), "--truth_path", str(hr_dir), "--no_ssim", "--channel", channel] + flags)
    assert all(r["ssim"] is None for r in results.values()) and sorted(os.listdir(str(tmp_path))) == ["hr", "log.txt", "lr", "ref", "sr"]
