"""The drivers that make their low-resolution images themselves (all on the GPU): the folder downscaler, evaluate
--lr_from_truth / evaluate_stream with a None input, device_patch_loader --lr_from_hr."""
import importlib
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAGS = ["--num_modules=1", "--num_blocks=1"]
SIZES = {"b_02.png": (48, 52), "a_01.png": (33, 47), "c_03.png": (64, 64)}


def _image(seed, h, w):
    """uint8 (h, w, 3): smooth colour field + noise (what a model can be scored on)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 90 * np.sin(xx / (5.0 + c)) * np.cos(yy / (7.0 - c)) for c in range(3)], axis=2)
    return np.clip(np.round(base + rng.normal(0, 10, (h, w, 3))), 0, 255).astype(np.uint8)


def _write_truths(folder):
    from PIL import Image
    folder.mkdir()
    truths = {name: _image(i, *hw) for i, (name, hw) in enumerate(sorted(SIZES.items()))}
    for name, a in truths.items():
        Image.fromarray(a).save(str(folder / name))
    return truths


@pytest.mark.parametrize("s,suffix", [(2, False), (3, True), (4, True)])
def test_downscale_images_writes_the_host_restatement(hip_device, tmp_path, s, suffix):
    from PIL import Image
    from larvanet_amd import downscale_images as D, image_utils as U
    truths = _write_truths(tmp_path / "hr")
    written = D.main(["--input_path", str(tmp_path / "hr"), "--output_path", str(tmp_path / "lr"), "--scale", str(s),
                      "--io_threads=2"] + (["--suffix"] if suffix else []))
    assert written == [D.output_name(n, s, suffix) for n in sorted(truths)]
    for name, a in truths.items():
        got = np.asarray(Image.open(str(tmp_path / "lr" / D.output_name(name, s, suffix))))
        assert np.array_equal(got, U.bicubic_downscale_u8(a, s)), name


@pytest.mark.parametrize("extra,names", [((), sorted(SIZES)), (("--self_ensemble",), ["c_03.png"]),
                                         (("--precision=fp16",), ["a_01.png"])])
def test_evaluate_lr_from_truth_equals_evaluate_over_the_written_folder(hip_device, tmp_path, extra, names):
    from PIL import Image
    from larvanet_amd import downscale_images as D, evaluate as E
    truths = _write_truths(tmp_path / "all")
    (tmp_path / "hr").mkdir()
    for name in names:
        Image.fromarray(truths[name]).save(str(tmp_path / "hr" / name))
    D.main(["--input_path", str(tmp_path / "hr"), "--output_path", str(tmp_path / "lr"), "--scale=4", "--suffix"])
    flags = FLAGS + list(extra)
    torch.manual_seed(0)
    want = E.main(["--input_path", str(tmp_path / "lr"), "--truth_path", str(tmp_path / "hr")] + flags)
    torch.manual_seed(0)
    got = E.main(["--truth_path", str(tmp_path / "hr"), "--lr_from_truth", "--input_path", str(tmp_path / "absent")] + flags)
    assert list(got) == names == list(want)
    for name in names:
        assert got[name]["sse"] == want[name]["sse"] and got[name]["n"] == want[name]["n"], name
        assert got[name]["ssim"] == want[name]["ssim"] and got[name]["psnr"] == want[name]["psnr"], name
        assert got[name]["n"] > 0 and got[name]["sse"] > 0
    # without the flag nothing changes: the missing folder's pairing error stays
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError, match=names[0]):
        E.main(["--input_path", str(tmp_path / "empty"), "--truth_path", str(tmp_path / "hr")] + flags)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_evaluate_stream_with_a_none_input_equals_the_pair_form(hip_device, s):
    from larvanet_amd import image_utils as U, pipeline
    m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
    m.parse_args(FLAGS)
    torch.manual_seed(0)
    m.prepare(is_training=False, scales=[s])
    truths = [_image(20 + i, h, w) for i, (h, w) in enumerate([(48, 52), (33, 47), (64, 64), (48, 52)])]
    pairs = [(U.bicubic_downscale_u8(t, s), t) for t in truths]
    want = list(pipeline.evaluate_stream(m, pairs, s, keep_images=True))
    mixed = [(None, t) if i != 2 else pairs[2] for i, t in enumerate(truths)]   # (both kinds in one stream)
    got = list(pipeline.evaluate_stream(m, mixed, s, keep_images=True))
    for (gr, gi), (wr, wi) in zip(got, want):
        assert gr == wr and np.array_equal(gi, wi)
    assert list(pipeline.evaluate_stream(m, [(None, t) for t in truths], s, depth=1)) == [w[0] for w in want]
    with pytest.raises(ValueError, match="smaller than one pixel"):
        list(pipeline.evaluate_stream(m, [(None, np.zeros((1, 40, 3), np.uint8))], s))


class _NoVal:
    def get_num_images(self):
        return 0


def test_the_resident_loader_makes_its_lr_tables_from_the_hr_tables(hip_device):
    from larvanet_amd import image_utils as U
    from larvanet_amd.dataloaders import device_patch_loader as D
    scales = [2, 3, 4]
    common = ["--device_source=synthetic_loader", "--synthetic_images=4", "--synthetic_lr_size=24", "--data_seed=3"]
    ld = D.create_loader()
    ld.parse_args(common + ["--lr_from_hr"])
    ld.prepare(scales)
    plain = D.create_loader()
    plain.parse_args(common)
    plain.prepare(scales)
    assert ld.shapes == plain.shapes and ld.get_num_images() == 4
    for s in scales:
        t, p = {k: v.cpu().numpy() for k, v in ld.tables[s].items()}, plain.tables[s]
        assert sorted(t) == sorted(p) and all(ld.tables[s][k].dtype == D.TABLE_DTYPES[k] for k in t)
        assert np.array_equal(t["hr"], p["hr"].cpu().numpy()) and np.array_equal(t["hr_off"], p["hr_off"].cpu().numpy())
        assert np.array_equal(t["lr_hw"], p["lr_hw"].cpu().numpy()) and np.array_equal(t["lr_off"], p["lr_off"].cpu().numpy())
        lrs, hrs = [], []
        for i in range(4):
            H, W = t["hr_hw"][2 * i:2 * i + 2]
            hr = t["hr"][t["hr_off"][i]:][:3 * H * W].reshape(3, H, W)
            want = U.bicubic_downscale_u8(np.ascontiguousarray(hr.transpose(1, 2, 0)), s).transpose(2, 0, 1)
            h, w = t["lr_hw"][2 * i:2 * i + 2]
            assert (h, w) == want.shape[1:]
            assert np.array_equal(t["lr"][t["lr_off"][i]:][:3 * h * w].reshape(3, h, w), want), (s, i)
            lrs.append(want)
            hrs.append(hr)
        assert t["lr"].size == sum(a.size for a in lrs)
        draws = D.draw_batch(np.random.RandomState(5), ld.shapes, 2, 16)
        x, y = ld.get_device_batch(2, s, 16, draws=draws)
        for b in range(2):
            wx, wy = D.apply_draw_numpy(draws[b], lrs[draws[b][0]], hrs[draws[b][0]], s, 16)
            assert np.array_equal(x[b].cpu().numpy(), wx) and np.array_equal(y[b].cpu().numpy(), wy)
        m = importlib.import_module("larvanet_amd.models.LarvaNet").create_model()
        m.parse_args(FLAGS)
        torch.manual_seed(0)
        m.prepare(is_training=True, scales=[s])
        loss = m.train_step_larva(types.SimpleNamespace(train_path="/tmp"), _NoVal(), x, y, None)
        assert np.isfinite(loss) and loss > 0
