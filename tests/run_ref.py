"""Helpers of tests/test_run_lifecycle.py: the tiny runs' flags, their data rebuilt on the host, and the float64 / fp32
oracle runs they are compared with (oracle/larva_torch.py, torch on the CPU).  No GPU is touched here.

The runs: two bodies of one block (V1 and V2 form), batch 4 of 12 x 12 LR patches cut from 3 synthetic images of LR size
20, validated on 2 synthetic uint8 images of LR size 16, 12 steps.  V1 under train_larva validates and saves every two
steps of volume (steps 1, 2, 4, ...); V2 under train_larvaV2 with --val_volume=0 validates and saves at every step
(twice at step 1: the first-step validation, then the volume one)."""
import sys
import types

import numpy as np
import torch

from larvanet_amd.dataloaders import device_patch_loader as DPL
from larvanet_amd.dataloaders import synthetic_loader as SL
from oracle import larva_torch as T

BLOCKS = [1, 1]
TINY = ["--num_modules=2", "--num_blocks=1,1"]
BATCH, PATCH = 4, 12
TRAIN_IMAGES, TRAIN_LR_SIZE = 3, 20
VAL_IMAGES, VAL_LR_SIZE = 2, 16
VOLUME_PER_STEP = PATCH * PATCH * BATCH * 3
STEPS = 12
DATA_SEED = 1
INIT_SEED = 3
VAL_LOADER = "lifecycle_val_loader"
PSNR_BAR = 0.02            # dB, DESIGN section 6 (F16, F17)
LOSS_BAR = 2e-3            # relative, the same trajectories
STEP_LOSS_BAR = 2e-5       # relative, one step (tests/test_model_parity.py)
MARGIN = 0.05              # dB: every plateau decision is at least this far from zero, 2.5 PSNR bars
FAR = 2e-5                 # an element of the final weights further than this from float64 counts into the share

# --lr / --threshold of the two driver runs compared with the oracle: chosen on the float64 oracle alone so that the lr
# drops at least twice, at least one validation leaves it alone, and no decision is closer than MARGIN to zero
# (test_the_oracle_runs_move_the_lr_with_margin holds them to that)
PLATEAU = {"LarvaNet": {"lr": 2e-3, "threshold": 0.1, "cooldown": 1},
           "LarvaNetV2": {"lr": 4e-3, "threshold": 0.12, "cooldown": 0}}   # (V2's flag set has no --cooldown)


# ---------------------------------------------------------------- the data
class _ValLoader(SL.SyntheticLoader):
    """synthetic_loader with the validation set's flags fixed: the driver hands a validation loader only what the
    training loader left of the command line, so two synthetic loaders cannot be given different sizes there."""

    def parse_args(self, args):
        _, remaining = super().parse_args(args)
        return super().parse_args(["--synthetic_images=%d" % VAL_IMAGES, "--synthetic_lr_size=%d" % VAL_LR_SIZE,
                                   "--synthetic_uint8"])[0], remaining


def register_val_loader(monkeypatch):
    """Make --val_dataloader=lifecycle_val_loader importable for the length of a test."""
    mod = types.ModuleType("larvanet_amd.dataloaders." + VAL_LOADER)
    mod.create_loader = _ValLoader
    monkeypatch.setitem(sys.modules, mod.__name__, mod)


def val_pairs(scale=4):
    return [SL.make_pair(i, VAL_LR_SIZE, VAL_LR_SIZE + 8 * (i % 3), scale, False) for i in range(VAL_IMAGES)]


def train_pairs(scale=4):
    return [SL.make_pair(i, TRAIN_LR_SIZE, TRAIN_LR_SIZE + 8 * (i % 3), scale, True) for i in range(TRAIN_IMAGES)]


def host_batches(steps, dtype, seed=DATA_SEED, scale=4):
    """The batches device_patch_loader --device_source=synthetic_loader --data_seed=seed cuts, rebuilt on the host from
    the same draws (draw_batch) by the host restatement of its kernel (apply_draw_numpy)."""
    pairs = train_pairs(scale)
    shapes = [tuple(p[0].shape[1:]) for p in pairs]
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        cut = [DPL.apply_draw_numpy(d, pairs[d[0]][0], pairs[d[0]][1], scale, PATCH)
               for d in DPL.draw_batch(rng, shapes, BATCH, PATCH)]
        out.append((torch.from_numpy(np.stack([c[0] for c in cut])).to(dtype),
                    torch.from_numpy(np.stack([c[1] for c in cut])).to(dtype)))
    return out


def driver_argv(model, train_path, loader="device", steps=STEPS, extra=()):
    v2 = model == "LarvaNetV2"
    p = PLATEAU[model]
    data = {"device": ["--dataloader=device_patch_loader", "--device_source=synthetic_loader",
                       "--data_seed=%d" % DATA_SEED],
            "host": ["--dataloader=synthetic_loader"]}[loader]
    return (["--model=" + model, "--val_dataloader=" + VAL_LOADER, "--train_path", str(train_path),
             "--max_steps=%d" % steps, "--batch_size=%d" % BATCH, "--input_patch_size=%d" % PATCH,
             "--synthetic_images=%d" % TRAIN_IMAGES, "--synthetic_lr_size=%d" % TRAIN_LR_SIZE,
             "--val_volume=%d" % (0 if v2 else 2 * VOLUME_PER_STEP), "--patience=0",
             "--lr=%g" % p["lr"], "--threshold=%g" % p["threshold"], "--save_train_state"]
            + ([] if v2 else ["--cooldown=1"]) + TINY + data + list(extra))


# ---------------------------------------------------------------- the oracle's runs, computed once
_RUNS = {}


def _single_thread(fn):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)   # (tensors this small: torch's CPU operators are much slower on many threads)
    try:
        return fn()
    finally:
        torch.set_num_threads(threads)


def init_weights(model, dtype, seed=INIT_SEED):
    sd = T.init_state_dict(BLOCKS, v2=model == "LarvaNetV2", seed=seed)
    return {k: v.to(dtype) for k, v in sd.items()}


def oracle_run(model, dtype, steps=STEPS):
    """oracle/larva_torch.train_trajectory of the driver run of `model` in `dtype` -> (record, final weights)."""
    key = (model, dtype, steps)
    if key not in _RUNS:
        v2 = model == "LarvaNetV2"
        p = PLATEAU[model]
        sd = init_weights(model, dtype)
        rec = _single_thread(lambda: T.train_trajectory(
            sd, host_batches(steps, dtype), steps, BLOCKS, val_pairs(), 0 if v2 else VOLUME_PER_STEP,
            0 if v2 else 2 * VOLUME_PER_STEP, lr=p["lr"], patience=0, cooldown=p["cooldown"],
            threshold=p["threshold"], min_lr=1e-7 if v2 else 1e-8, v2=v2))
        _RUNS[key] = (rec, sd)
    return _RUNS[key]


def plateau_decisions(psnrs, threshold):
    """PSNR - best - threshold of every validation after the first, with ReduceLROnPlateau's best (mode max, abs)."""
    best, out = psnrs[0], []
    for v in psnrs[1:]:
        out.append(v - best - threshold)
        if v > best + threshold:
            best = v
    return out


def lr_drops(lr0, lrs):
    before = [lr0] + list(lrs[:-1])
    return [i + 1 for i, (a, b) in enumerate(zip(before, lrs)) if b < a]   # the steps after which the lr is lower


def adamw_run(model, dtype, batches, lrs_used, reset_at=None):
    """Plain torch.optim.AdamW steps of the multi-exit loss, step s on batches[s % len(batches)] with learning rate
    lrs_used[s] -> (losses, final weights).  reset_at=k: the optimizer forgets its moments and step count after k steps
    (the mutant of a handover that drops them)."""
    v2 = model == "LarvaNetV2"

    def run():
        params = {k: v.clone().requires_grad_(True) for k, v in init_weights(model, dtype).items()}
        opt = torch.optim.AdamW(list(params.values()), lr=lrs_used[0])
        losses = []
        for s, lr in enumerate(lrs_used):
            if s == reset_at:
                opt = torch.optim.AdamW(list(params.values()), lr=lr)
            opt.param_groups[0]["lr"] = lr
            x, truth = batches[s % len(batches)]
            loss = T.multi_exit_loss(params, x.to(dtype), truth.to(dtype), BLOCKS, v2=v2)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.item()))
        return losses, {k: v.detach() for k, v in params.items()}
    return _single_thread(run)


def weight_distance(sd, ref):
    """(largest elementwise distance, share of elements further than FAR) of the weights `sd` from the float64 `ref`."""
    d = torch.cat([(sd[k].detach().cpu().double() - ref[k].double()).abs().reshape(-1) for k in ref])
    return float(d.max()), float((d > FAR).double().mean())


def fixed_batch(seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(BATCH, 3, PATCH, PATCH, generator=g) * 255, torch.rand(BATCH, 3, 4 * PATCH, 4 * PATCH, generator=g) * 255)]
