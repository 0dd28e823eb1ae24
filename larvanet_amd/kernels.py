"""Tensor-level wrappers over the C ABI (hip_lib): torch supplies device memory and the stream,
every byte of arithmetic happens in liblarva_hip.so.  Each wrapper validates what the kernel and
its grid assume (device, dtype, contiguity, shapes) before launching.
"""
import ctypes
import os
import struct

import torch

from . import hip_lib

_SUPPORTED_COUT = (32, 48, 64)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk_tensor(t, name, shape, dtype, last=None):
    """The checks every operand gets -> its device pointer.  float32 operands have any shape; `last` = the trailing
    dimension of the 4-D channels-last formats (fp16 activations [N][H][W][48], uint8 images [N][H][W][3])."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("larvanet_amd: %s must be a tensor on a HIP device (no CPU path exists)" % name)
    kind = str(dtype).replace("torch.", "")
    if last is None:
        if t.dtype != dtype:
            raise RuntimeError("larvanet_amd: %s must be %s, got %s" % (name, kind, t.dtype))
        if not t.is_contiguous():
            raise RuntimeError("larvanet_amd: %s must be contiguous" % name)
    else:
        if t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError("larvanet_amd: %s must be a contiguous %s tensor, got %s" % (name, kind, t.dtype))
        if t.dim() != 4 or int(t.shape[3]) != last:
            raise RuntimeError("larvanet_amd: %s must be [N][H][W][%d], got %s" % (name, last, tuple(t.shape)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError("larvanet_amd: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t.data_ptr()


def _chk(t, name, shape=None):
    return _chk_tensor(t, name, shape, torch.float32)


def _opt(t, name, shape):
    return None if t is None else _chk(t, name, shape)


def _out(out, shape, device, dtype=torch.float32, last=None, name="out"):
    """The caller's `out`, checked like any operand, or a new tensor of that shape."""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    _chk_tensor(out, name, shape, dtype, last)
    return out


def _src_list(srcs):
    return [srcs] if isinstance(srcs, torch.Tensor) else list(srcs)


def _try_launch(name, *args):
    """_launch, but hipErrorNotSupported (the entry point does not take these operands, e.g. unaligned ones; nothing was
    launched) -> False instead of raising."""
    code = getattr(hip_lib.load(), name)(*args, _stream())
    if code == 801:
        return False
    hip_lib.check(code, name)
    return True


def _launch(name, *args, stream=True):
    """Entry point `name` of the library on the current stream (stream=False: it takes none), its code checked.  The
    entry point is looked up on every call: tests put spies on the library object."""
    fn = getattr(hip_lib.load(), name)
    hip_lib.check(fn(*args, _stream()) if stream else fn(*args), name)


def packed_weight_floats(cout, cin):
    return int(hip_lib.load().larva_packed_weight_floats(cout, cin))


def pack_weights(w, cin_off=0, cin=None, cin_pad=None, want_bwd=True):
    """w: [cout][cin_total][3][3] -> (wpk_fwd, wpk_bwd) packed images for the conv kernel.

    Packs the input-channel slice [cin_off, cin_off+cin) (default: to the end).  cin_pad pads
    with zero channels up to that kernel channel count (head conv: 3 -> 16); padding is only
    meaningful when the slice ends at cin_total."""
    _chk(w, "w")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError("larvanet_amd: only [cout][cin][3][3] weights are supported")
    cout, cin_total = int(w.shape[0]), int(w.shape[1])
    cin = cin_total - cin_off if cin is None else cin
    if cin_off < 0 or cin < 1 or cin_off + cin > cin_total:
        raise RuntimeError("larvanet_amd: weight slice out of range")
    cin_k = cin if cin_pad is None else cin_pad
    if cin_k > cin and cin_off + cin != cin_total:
        raise RuntimeError("larvanet_amd: zero padding needs a slice that ends at cin_total")
    if cin_k % 8 or cout % 8 or cin_k < cin:
        raise RuntimeError("larvanet_amd: channel counts must be multiples of 8 (cout=%d cin=%d)" % (cout, cin_k))
    fwd = torch.empty(packed_weight_floats(cout, cin_k), device=w.device, dtype=torch.float32)
    bwd = torch.empty(packed_weight_floats(cin_k, cout), device=w.device, dtype=torch.float32) if want_bwd else None
    _launch("larva_pack_weights", w.data_ptr(), fwd.data_ptr(), bwd.data_ptr() if want_bwd else None,
            cout, cin_k, cin_total, cin_off)
    return fwd, bwd


def _pack_job_args(jobs):
    """Pack jobs (w, fwd_buf, bwd_buf or None, cout, cin_k, cin_off), checked -> the leading arguments of
    larva_pack_weights_batch / larva_step_prologue: weights, forward and backward images, cout, cin_k, cin_total,
    cin_off per job, and the job count."""
    ws, fs, bs, couts, cins, totals, offs = [], [], [], [], [], [], []
    for (w, fwd, bwd, cout, cin_k, cin_off) in jobs:
        _chk(w, "w")
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or int(w.shape[0]) != cout:
            raise RuntimeError("larvanet_amd: only [cout][cin][3][3] weights are supported")
        ws.append(w.data_ptr())
        fs.append(_chk(fwd, "wpk_fwd", (packed_weight_floats(cout, cin_k),)))
        bs.append(None if bwd is None else _chk(bwd, "wpk_bwd", (packed_weight_floats(cin_k, cout),)))
        couts.append(cout)
        cins.append(cin_k)
        totals.append(int(w.shape[1]))
        offs.append(cin_off)
    return (hip_lib.ptr_array(ws), hip_lib.ptr_array(fs), hip_lib.ptr_array(bs), hip_lib.int_array(couts),
            hip_lib.int_array(cins), hip_lib.int_array(totals), hip_lib.int_array(offs), len(jobs))


def pack_weights_batch(jobs):
    """jobs: list of (w, fwd_buf, bwd_buf or None, cout, cin_k, cin_off): packs every weight
    (slice) into its persistent kernel-layout buffers with one launch per 64 jobs."""
    for i in range(0, len(jobs), 64):
        _launch("larva_pack_weights_batch", *_pack_job_args(jobs[i:i + 64]))


_STRIP_TABLES = {}


def strip_tile_table(H, P, device, phase=0):
    """Device copy of the library's strip-tile table of one H x P image (cached per shape and
    device; built and uploaded outside any stream capture) -> (tensor, tiles per image) or None when
    the height cannot be cut into 5- and 4-row tiles."""
    key = (int(H), int(P), str(device), int(phase))
    hit = _STRIP_TABLES.get(key)
    if hit is None:
        cap = 4 * ((H + 3) // 4) * ((P + 15) // 16) + 16
        buf = (ctypes.c_uint * cap)()
        n = int(hip_lib.load().larva_strip_tile_table(int(H), int(P), int(phase), buf, cap))
        if n <= 0 or n > cap:
            hit = False
        else:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("larvanet_amd: strip-tile table for %dx%d requested during stream capture "
                                   "(run the step once outside the capture first)" % (H, P))
            import numpy as np
            # (entries use bit 31: the raw 32-bit patterns travel as int32); the host array is kept: the launch passes
            # it along, and small tables then travel inside the kernel arguments (larva_conv3x3_fwd_strips)
            hit = (torch.from_numpy(np.frombuffer(buf, dtype=np.int32, count=n).copy()).to(device), n, buf)
        _STRIP_TABLES[key] = hit
    return hit or None


def step_prologue(jobs, x, x16, base):
    """pack_weights_batch(jobs) (<= 64 jobs) + x16[:, :C] = x + base = bicubic4(x) in one launch."""
    if len(jobs) > 64:
        raise RuntimeError("larvanet_amd: at most 64 pack jobs per prologue launch")
    N, C, H, W = (int(v) for v in x.shape)
    _chk(x, "x")
    _chk(x16, "x16", (N, 16, H, W))
    _chk(base, "base", (N, C, 4 * H, 4 * W))
    _launch("larva_step_prologue", *_pack_job_args(jobs), x.data_ptr(), x16.data_ptr(), base.data_ptr(), N, C, H, W)


def conv3x3(srcs, wpk, cout, bias=None, relu=False, mask=None, res0=None, res1=None,
            shuffle=False, base=None, out=None, logical_w=None, images=None, strips=False, plain_stores=False,
            tile_rows=0):
    """Fused 3x3 conv over the channel concatenation of `srcs` (list of [N][c][H][P]).

    shuffle=False: returns [N][cout][H][P]; shuffle=True: returns PixelShuffle(4) layout
    [N][cout/16][4H][4W] (+ base).  logical_w: the image is W = logical_w <= P columns wide and
    the tensors' rows are padded to the pitch P (columns [W, P) hold zeros) -- lets widths that
    are not a multiple of 4 use the 16-byte staging path.
    images=(lo, hi): only images [lo, hi) of the batch are computed (every operand is the full-batch
    tensor; the other images of `out` are left untouched).  strips=True (or 2: the tile table
    starts with the other tile height): 5 x 16 / 4 x 16 tiles instead of 3 x 48 (same results bit for
    bit; see larva_conv3x3_fwd_strips) where the shape allows, else the regular tiles; plain_stores:
    the strip launch writes its output with plain instead of non-temporal stores.
    tile_rows: 0 = the library picks the tiling of a whole-tensor launch (3 x 48 tiles; 4 x 48 for large 32-channel
    launches; persistent workgroups where there are more tiles than workgroup slots), 3 / 4 = that tile height (tests,
    A/B timing; larva_conv3x3_fwd_tiled).
    Views: srcs, wpk, mask, res0, res1 and a shuffle=False out may start on any 4-byte boundary (off the 16-byte grid the
    register-staged kernel runs: same results; strips then fall back to the regular tiles, tile_rows=4 raises); with
    shuffle=True `out` and `base` must be 16-byte aligned (RuntimeError otherwise, nothing is written)."""
    srcs = _src_list(srcs)
    if not 1 <= len(srcs) <= 8:
        raise RuntimeError("larvanet_amd: 1..8 source tensors")
    if cout not in _SUPPORTED_COUT:
        raise RuntimeError("larvanet_amd: cout must be one of %s" % (_SUPPORTED_COUT,))
    N, cps, H, P = (int(v) for v in srcs[0].shape)
    W = P if logical_w is None else int(logical_w)
    if not 0 < W <= P:
        raise RuntimeError("larvanet_amd: logical width %d does not fit the row pitch %d" % (W, P))
    if cps % 8:
        raise RuntimeError("larvanet_amd: input channels per tensor must be a multiple of 8")
    ptrs = [_chk(s, "src[%d]" % i, (N, cps, H, P)) for i, s in enumerate(srcs)]
    cin = cps * len(srcs)
    _chk(wpk, "wpk", (packed_weight_floats(cout, cin),))
    full = (N, cout, H, P)
    hr = (N, cout // 16, 4 * H, 4 * W)
    out = _out(out, hr if shuffle else full, srcs[0].device)
    lo, hi = (0, N) if images is None else (int(images[0]), int(images[1]))
    if not 0 <= lo < hi <= N:
        raise RuntimeError("larvanet_amd: image range [%d, %d) outside the batch of %d" % (lo, hi, N))

    def at(ptr, per_image_floats):   # the same operand, starting at image `lo`
        return None if ptr is None else ptr + 4 * lo * per_image_floats

    lr_img, hr_img = H * P, 16 * H * W
    args = (hip_lib.ptr_array([at(p, cps * lr_img) for p in ptrs]), len(srcs), cps, wpk.data_ptr(),
            _opt(bias, "bias", (cout,)), at(_opt(res0, "res0", full), cout * lr_img),
            at(_opt(res1, "res1", full), cout * lr_img), at(_opt(mask, "mask", full), cout * lr_img),
            at(_opt(base, "base", hr), (cout // 16) * hr_img),
            at(out.data_ptr(), (cout // 16) * hr_img if shuffle else cout * lr_img),
            hi - lo, cout, H, W, P, 1 if relu else 0, 1 if shuffle else 0)
    if strips and cout in (48, 32, 64):
        tab = strip_tile_table(H, P, out.device, phase=1 if strips == 2 else 0)
        # (refused: unaligned operands -> the regular tiles below)
        if tab is not None and _try_launch("larva_conv3x3_fwd_strips", *args, tab[0].data_ptr(), tab[2], tab[1],
                                           1 if plain_stores else 0):
            return out
    if tile_rows:
        _launch("larva_conv3x3_fwd_tiled", *args, int(tile_rows))
    else:
        _launch("larva_conv3x3_fwd_pitched", *args)
    return out


def conv3x3_batch(jobs, cout, relu=False, shuffle=False, logical_w=None, outs=None):
    """2..4 INDEPENDENT convs of one shape and one fusion in one launch (their workgroups share
    the CUs two by two).  jobs: dicts with srcs (tensor or list), wpk and optionally bias, mask,
    res0, res1, base -- a fusion operand is given by every job or by none.  Returns the outputs
    (outs: the caller's tensors, one per job, e.g. slices of one buffer).
    Falls back to one launch per job where the 16-byte staging path does not apply."""
    if not 2 <= len(jobs) <= 4:
        raise RuntimeError("larvanet_amd: 2..4 conv jobs per batched launch")
    norm = [dict(j, srcs=_src_list(j["srcs"])) for j in jobs]
    n_src = len(norm[0]["srcs"])
    N, cps, H, P = (int(v) for v in norm[0]["srcs"][0].shape)
    W = P if logical_w is None else int(logical_w)
    if cout not in _SUPPORTED_COUT or cps % 8 or not 0 < W <= P or not 1 <= n_src <= 8:
        raise RuntimeError("larvanet_amd: unsupported batched conv shape")
    cin = cps * n_src
    full, hr = (N, cout, H, P), (N, cout // 16, 4 * H, 4 * W)
    names = ("bias", "res0", "res1", "mask", "base")
    used = {k: norm[0].get(k) is not None for k in names}
    given = None if outs is None else list(outs)
    if given is not None and len(given) != len(norm):
        raise RuntimeError("larvanet_amd: one output tensor per batched conv job")
    src_ptrs, cols, outs = [], {k: [] for k in names}, []
    for n_job, j in enumerate(norm):
        if len(j["srcs"]) != n_src or any((j.get(k) is not None) != used[k] for k in names):
            raise RuntimeError("larvanet_amd: batched conv jobs must share one shape and one fusion")
        src_ptrs += [_chk(t, "src", (N, cps, H, P)) for t in j["srcs"]]
        _chk(j["wpk"], "wpk", (packed_weight_floats(cout, cin),))
        for k, shape in (("bias", (cout,)), ("res0", full), ("res1", full), ("mask", full), ("base", hr)):
            if used[k]:
                cols[k].append(_chk(j[k], k, shape))
        outs.append(_out(None if given is None else given[n_job], hr if shuffle else full, j["srcs"][0].device))

    def arr(k):
        return hip_lib.ptr_array(cols[k]) if used[k] else None

    common = (len(norm), hip_lib.ptr_array(src_ptrs), n_src, cps, hip_lib.ptr_array([j["wpk"].data_ptr() for j in norm]),
              arr("bias"), arr("res0"), arr("res1"), arr("mask"), arr("base"),
              hip_lib.ptr_array([o.data_ptr() for o in outs]), N, cout, H, W, P, 1 if relu else 0, 1 if shuffle else 0)
    if not _try_launch("larva_conv3x3_fwd_batch", *common):   # unaligned shape: one launch per job
        return [conv3x3(j["srcs"], j["wpk"], cout, bias=j.get("bias"), relu=relu, mask=j.get("mask"),
                        res0=j.get("res0"), res1=j.get("res1"), shuffle=shuffle, base=j.get("base"), out=o,
                        logical_w=logical_w)
                for j, o in zip(norm, outs)]
    return outs


def head_conv3_direct(x, w, bias=None, pitch=None):
    """nn.Conv2d(3, cout, 3, 1, 1) on the raw image: x [N][3][H][W], w [cout][3][3][3] -> [N][cout][H][P]
    (P = pitch or W; columns [W, P) zero)."""
    N, C, H, W = (int(v) for v in x.shape)
    cout = int(w.shape[0])
    if C != 3 or tuple(w.shape[1:]) != (3, 3, 3) or cout % 16:
        raise RuntimeError("larvanet_amd: the direct head conv takes a 3-channel image and [cout][3][3][3] weights")
    _chk(x, "x")
    _chk(w, "w")
    P = W if pitch is None else int(pitch)
    out = torch.empty((N, cout, H, P), device=x.device, dtype=torch.float32)
    _launch("larva_head_conv3_direct", x.data_ptr(), w.data_ptr(), _opt(bias, "bias", (cout,)), out.data_ptr(), N, cout, H, W, P)
    return out


def conv3x3_exit_l1_batch(jobs, cout, truth, gvalue, gscale, want_image):
    """2..4 exits scored by L1 inside their pixel-shuffle conv launch.  jobs: dicts {srcs, wpk, bias,
    base}; truth [N][cout/16][4H][4W]; the gradient of every image element is sign(out - truth) *
    (gvalue * gscale) / numel; want_image[j]: also store exit j's image.  Returns (images (None where
    not wanted), partial-sum vectors, gradients [N][cout][H][W]) or None when the launch does not
    apply (unaligned operands, cout != 48): the caller then runs the conv and the L1 sweep separately."""
    if not 2 <= len(jobs) <= 4 or cout != 48:
        return None
    norm = [dict(j, srcs=_src_list(j["srcs"])) for j in jobs]
    n_src = len(norm[0]["srcs"])
    N, cps, H, P = (int(v) for v in norm[0]["srcs"][0].shape)
    hr = (N, cout // 16, 4 * H, 4 * P)
    _chk(truth, "truth", hr)
    numel = float(truth.numel())
    import numpy as np
    gval = float((np.float32(gvalue) * np.float32(gscale)) * (np.float32(1.0) / np.float32(numel)))
    npart = int(hip_lib.load().larva_exit_l1_partials(N, H, P))
    src_ptrs, outs, grads, parts = [], [], [], []
    for j, want in zip(norm, want_image):
        if len(j["srcs"]) != n_src:
            raise RuntimeError("larvanet_amd: batched exits must share one shape")
        src_ptrs += [_chk(t, "src", (N, cps, H, P)) for t in j["srcs"]]
        _chk(j["wpk"], "wpk", (packed_weight_floats(cout, cps * n_src),))
        _chk(j["bias"], "bias", (cout,))
        _chk(j["base"], "base", hr)
        outs.append(torch.empty(hr, device=truth.device, dtype=torch.float32) if want else None)
        grads.append(torch.empty((N, cout, H, P), device=truth.device, dtype=torch.float32))
        parts.append(torch.empty(npart, device=truth.device, dtype=torch.float32))
    done = _try_launch(
        "larva_conv3x3_exit_l1_batch",
        len(norm), hip_lib.ptr_array(src_ptrs), n_src, cps, hip_lib.ptr_array([j["wpk"].data_ptr() for j in norm]),
        hip_lib.ptr_array([j["bias"].data_ptr() for j in norm]), hip_lib.ptr_array([j["base"].data_ptr() for j in norm]),
        hip_lib.ptr_array([truth.data_ptr()] * len(norm)), hip_lib.ptr_array([None if o is None else o.data_ptr() for o in outs]),
        hip_lib.ptr_array([g.data_ptr() for g in grads]), hip_lib.ptr_array([p.data_ptr() for p in parts]),
        gval, N, cout, H, P, P)
    return (outs, parts, grads) if done else None


def wgrad_partial_floats(cout, cin, splits):
    return int(hip_lib.load().larva_wgrad_partial_floats(cout, cin, splits))


def max_wgrad_jobs():
    return 64


def wgrad_cu_share(cout, cin):
    """Workgroups of the (cout, cin) weight-gradient kernel that fit one CU together (1 or 2)."""
    return int(hip_lib.load().larva_wgrad_cu_share(int(cout), int(cin)))


def _dw_slice(j, cout, cin):
    """The dw [cout][cin_total][3][3] of a weight-gradient job and the channel slice it names, checked ->
    (cin_off, cin_valid, cin_total)."""
    dw = j["dw"]
    _chk(dw, "dw")
    if dw.dim() != 4 or int(dw.shape[0]) != cout or tuple(dw.shape[2:]) != (3, 3):
        raise RuntimeError("larvanet_amd: dw must be [cout][cin_total][3][3]")
    total = int(dw.shape[1])
    off = int(j.get("cin_off", 0))
    valid = int(j.get("cin_valid", cin))
    if off < 0 or valid < 1 or valid > cin or off + valid > total:
        raise RuntimeError("larvanet_amd: wgrad channel slice out of range")
    return off, valid, total


def conv3x3_wgrad(jobs, cout, cin, splits):
    """jobs: list (<= max_wgrad_jobs()) of dicts {dy, x, dw, db (or None), cin_off, cin_valid}; dw/db are
    overwritten.  All jobs share (N, cout, cin, H, W)."""
    if not 1 <= len(jobs) <= max_wgrad_jobs():
        raise RuntimeError("larvanet_amd: 1..%d wgrad jobs per call" % max_wgrad_jobs())
    N, _, H, W = (int(v) for v in jobs[0]["dy"].shape)
    dys, xs, parts, dws, dbs, offs, valids, totals, keep = [], [], [], [], [], [], [], [], []
    nfl = wgrad_partial_floats(cout, cin, splits)
    for j in jobs:
        dys.append(_chk(j["dy"], "dy", (N, cout, H, W)))
        xs.append(_chk(j["x"], "x", (N, cin, H, W)))
        off, valid, total = _dw_slice(j, cout, cin)
        part = _out(j.get("partial"), (nfl,), j["dw"].device, name="partial")
        keep.append(part)
        parts.append(part.data_ptr())
        dws.append(j["dw"].data_ptr())
        dbs.append(_opt(j.get("db"), "db", (cout,)))
        offs.append(off)
        valids.append(valid)
        totals.append(total)
    _launch("larva_conv3x3_wgrad",
            hip_lib.ptr_array(dys), hip_lib.ptr_array(xs), hip_lib.ptr_array(parts), hip_lib.ptr_array(dws),
            hip_lib.ptr_array(dbs), hip_lib.int_array(offs), hip_lib.int_array(valids), hip_lib.int_array(totals),
            len(jobs), splits, N, cout, cin, H, W)
    return keep


def conv3x3_wgrad_partial(jobs, cout, cin, splits):
    """Phase 1 only: jobs (<= 64 dicts {dy, x}) -> (partial tensors, splits actually used).
    Feed them to wgrad_reduce later (the partials must stay alive until then)."""
    if not 1 <= len(jobs) <= 64:
        raise RuntimeError("larvanet_amd: 1..64 wgrad jobs per call")
    N, _, H, W = (int(v) for v in jobs[0]["dy"].shape)
    splits = max(1, min(int(splits), N * ((H + 2) // 3) * ((W + 47) // 48)))  # the library's clamp
    nfl = wgrad_partial_floats(cout, cin, splits)
    dys = [_chk(j["dy"], "dy", (N, cout, H, W)) for j in jobs]
    xs = [_chk(j["x"], "x", (N, cin, H, W)) for j in jobs]
    parts = [torch.empty(nfl, device=jobs[0]["dy"].device, dtype=torch.float32) for _ in jobs]
    used = ctypes.c_int(0)
    _launch("larva_conv3x3_wgrad_partial",
            hip_lib.ptr_array(dys), hip_lib.ptr_array(xs), hip_lib.ptr_array([p.data_ptr() for p in parts]),
            len(jobs), splits, N, cout, cin, H, W, ctypes.byref(used))
    return parts, int(used.value)


def conv3x3_wgrad_partial_flat(jobs, cout, cin, nwg, head=None):
    """Phase 1 of ALL jobs (<= 64 dicts {dy, x}; 48 -> 48, 32 -> 32 or 64 -> 64 channels) as one grid of `nwg` workgroups ->
    (partial tensors, [partial images per job]) or None when the flat launch does not apply.  head: one more dict
    {dy [N][48][H][W], x [N][16][H][W]} -- the 3 -> 48 head on its padded input -- whose tiles the last workgroups of
    the same grid take; the result then ends with that job's partial tensor / image count."""
    lib = hip_lib.load()
    if not 1 <= len(jobs) <= 64 or (cout, cin) not in ((48, 48), (32, 32), (64, 64)) or (head is not None and cout != 48):
        return None
    N, _, H, W = (int(v) for v in jobs[0]["dy"].shape)
    if W % 4:
        return None
    tiles = N * ((H + 2) // 3) * ((W + 47) // 48)
    cap = int(lib.larva_wgrad_flat_max_splits(len(jobs), int(nwg), tiles))
    nfl = wgrad_partial_floats(cout, cin, cap)
    dys = [_chk(j["dy"], "dy", (N, cout, H, W)) for j in jobs]
    xs = [_chk(j["x"], "x", (N, cin, H, W)) for j in jobs]
    dev = jobs[0]["dy"].device
    parts = [torch.empty(nfl, device=dev, dtype=torch.float32) for _ in jobs]
    used = (ctypes.c_int * len(jobs))()
    if head is None:
        done = _try_launch(
            "larva_conv3x3_wgrad_partial_flat",
            hip_lib.ptr_array(dys), hip_lib.ptr_array(xs), hip_lib.ptr_array([p.data_ptr() for p in parts]),
            len(jobs), int(nwg), N, cout, cin, H, W, used)
    else:
        hcap = int(lib.larva_wgrad_flat_head_splits(len(jobs), int(nwg), tiles))
        hper = wgrad_partial_floats(48, 16, 1)
        hpart = torch.empty(hper * hcap, device=dev, dtype=torch.float32)
        hused = ctypes.c_int(0)
        done = _try_launch(
            "larva_conv3x3_wgrad_partial_flat_head",
            hip_lib.ptr_array(dys), hip_lib.ptr_array(xs), hip_lib.ptr_array([p.data_ptr() for p in parts]), len(jobs),
            _chk(head["dy"], "head dy", (N, 48, H, W)), _chk(head["x"], "head x", (N, 16, H, W)), hpart.data_ptr(),
            int(nwg), N, H, W, used, ctypes.byref(hused))
    if not done:
        return None
    splits = [int(v) for v in used]
    per = wgrad_partial_floats(cout, cin, 1)
    out = [p[:per * s] for p, s in zip(parts, splits)]
    if head is not None:
        out.append(hpart[:hper * int(hused.value)])
        splits.append(int(hused.value))
    return out, splits


def _loss_terms(terms, scales):
    ptrs, counts = [], []
    for t in terms:
        _chk(t, "term")
        if t.dim() > 1:
            raise RuntimeError("larvanet_amd: a loss term is a scalar or a vector of partial sums")
        ptrs.append(t.data_ptr())
        counts.append(max(1, int(t.numel())))
    sc = (ctypes.c_float * len(terms))(*[float(v) for v in scales])
    return hip_lib.ptr_array(ptrs), hip_lib.int_array(counts), sc


def wgrad_reduce(jobs, cout=None, cin=None, loss=None):
    """Phase 2: jobs (<= 64 dicts {partial, splits, dw, db (or None), cin_off, cin_valid[, cout, cin]})
    reduced in ONE launch; dw/db are overwritten.  cout/cin: the kernel shape of every job that does
    not carry its own.  loss = (terms, scales, divisor, out): the same launch also finishes
    loss_from_partials(terms, scales, divisor) into the 0-d tensor `out`."""
    if not 1 <= len(jobs) <= 64:
        raise RuntimeError("larvanet_amd: 1..64 reduce jobs per call")
    parts, dws, dbs, offs, valids, totals, splits, couts, cins = [], [], [], [], [], [], [], [], []
    for j in jobs:
        co, ci = int(j.get("cout", cout)), int(j.get("cin", cin))
        off, valid, total = _dw_slice(j, co, ci)
        sp = int(j["splits"])
        parts.append(_chk(j["partial"], "partial", (wgrad_partial_floats(co, ci, sp),)))
        dws.append(j["dw"].data_ptr())
        dbs.append(_opt(j.get("db"), "db", (co,)))
        offs.append(off)
        valids.append(valid)
        totals.append(total)
        splits.append(sp)
        couts.append(co)
        cins.append(ci)
    common = (hip_lib.ptr_array(parts), hip_lib.ptr_array(dws), hip_lib.ptr_array(dbs), hip_lib.int_array(offs),
              hip_lib.int_array(valids), hip_lib.int_array(totals), hip_lib.int_array(splits), hip_lib.int_array(couts),
              hip_lib.int_array(cins), len(jobs))
    if loss is None:
        _launch("larva_wgrad_reduce", *common)
    else:
        terms, scales, divisor, out = loss
        if not 1 <= len(terms) <= 8:
            raise RuntimeError("larvanet_amd: 1..8 loss terms")
        _chk(out, "loss", ())
        _launch("larva_wgrad_reduce_with_loss", *common, *_loss_terms(terms, scales), len(terms), float(divisor), out.data_ptr())


UPSAMPLE_MODES = {"bicubic": 0, "bilinear": 1}


def upsample4(x, mode="bicubic"):
    """F.interpolate(x, scale_factor=4, mode=mode, align_corners=False) (models/LarvaNet.py:283-285) for the two
    modes that call accepts for a 4-D input (nearest / area refuse align_corners, linear / trilinear the rank)."""
    if mode not in UPSAMPLE_MODES:
        raise RuntimeError("larvanet_amd: no x4 kernel for interpolate mode %r" % (mode,))
    N, C, H, W = (int(v) for v in x.shape)
    _chk(x, "x")
    out = torch.empty((N, C, 4 * H, 4 * W), device=x.device, dtype=torch.float32)
    _launch("larva_upsample4_fwd", x.data_ptr(), out.data_ptr(), N, C, H, W, UPSAMPLE_MODES[mode])
    return out


def upsample(x, scale, mode="bicubic"):
    """F.interpolate(x, scale_factor=scale, mode=mode, align_corners=False) for scale 2, 3 or 4 (4 = upsample4)."""
    if int(scale) == 4:
        return upsample4(x, mode)
    if mode not in UPSAMPLE_MODES or int(scale) not in (2, 3):
        raise RuntimeError("larvanet_amd: no kernel for interpolate mode %r at x%s" % (mode, scale))
    s = int(scale)
    N, C, H, W = (int(v) for v in x.shape)
    _chk(x, "x")
    out = torch.empty((N, C, s * H, s * W), device=x.device, dtype=torch.float32)
    _launch("larva_upsample_fwd", x.data_ptr(), out.data_ptr(), N, C, H, W, s, UPSAMPLE_MODES[mode])
    return out


def pixel_shuffle_base(y, base, scale, channels=3, logical_w=None):
    """x2 / x3 exit image: PixelShuffle(scale)(y[:, :channels * scale**2]) (+ base) for the plain conv output y
    [N][cpad][H][P] (logical_w: the image is W <= P columns wide) -> [N][channels][scale H][scale W]."""
    s = int(scale)
    N, cpad, H, P = (int(v) for v in y.shape)
    W = P if logical_w is None else int(logical_w)
    _chk(y, "y")
    hr = (N, channels, s * H, s * W)
    out = torch.empty(hr, device=y.device, dtype=torch.float32)
    _launch("larva_pixel_shuffle_base", y.data_ptr(), _opt(base, "base", hr), out.data_ptr(), N, channels, cpad, H, W, P, s)
    return out


def _lr_of(hr, scale, what="spatial dims must be"):
    """(N, C, H, W) of the image `scale` times smaller than hr [N][C][scale H][scale W]."""
    N, C, HH, WW = (int(v) for v in hr.shape)
    if HH % scale or WW % scale:
        raise RuntimeError("larvanet_amd: %s divisible by %d" % (what, scale))
    return N, C, HH // scale, WW // scale


def pixel_unshuffle(g, scale, cpad):
    """PixelShuffle(scale) backward: [N][C][sH][sW] -> [N][cpad][H][W], channels [C s^2, cpad) zero."""
    s = int(scale)
    _chk(g, "g")
    N, C, H, W = _lr_of(g, s)
    out = torch.empty((N, cpad, H, W), device=g.device, dtype=torch.float32)
    _launch("larva_pixel_unshuffle", g.data_ptr(), out.data_ptr(), N, C, cpad, H, W, s)
    return out


def l1_bwd_unshuffle(a, b, gout, scale, cpad, gscale=1.0):
    """Gradient of mean|a - b| * gscale w.r.t. a at scale 2 / 3, written as [N][cpad][H][W] (padding channels zero)."""
    s = int(scale)
    _chk(a, "a")
    _chk(b, "b", a.shape)
    _chk(gout, "gout", ())
    N, C, H, W = _lr_of(a, s)
    out = torch.empty((N, cpad, H, W), device=a.device, dtype=torch.float32)
    _launch("larva_l1_bwd_unshuffle", a.data_ptr(), b.data_ptr(), gout.data_ptr(), float(gscale), out.data_ptr(),
            N, C, cpad, H, W, s)
    return out


def shuffle_l1_partial_grad(y, base, truth, gvalue, gscale, scale, want_image=True):
    """One x2 / x3 training exit after its plain conv y [N][cpad][H][W]: -> (partials, 1 / numel, grad [N][cpad][H][W],
    image = PixelShuffle(scale)(y) + base or None), the L1 partial sums and the gradient sign(image - truth) * gvalue *
    gscale / numel from one pass."""
    s = int(scale)
    _chk(truth, "truth")
    N, C, H, W = _lr_of(truth, s)
    cpad = int(y.shape[1])
    _chk(y, "y", (N, cpad, H, W))
    _chk(base, "base", truth.shape)
    part = _l1_partials(y.device)
    grad = torch.empty((N, cpad, H, W), device=y.device, dtype=torch.float32)
    out = torch.empty(truth.shape, device=y.device, dtype=torch.float32) if want_image else None
    blocks = ctypes.c_int(0)
    _launch("larva_shuffle_l1_partial_grad", y.data_ptr(), base.data_ptr(), truth.data_ptr(), float(gvalue), float(gscale),
            part.data_ptr(), ctypes.byref(blocks), grad.data_ptr(), None if out is None else out.data_ptr(), N, C, cpad, H, W, s)
    return part[:int(blocks.value)], 1.0 / float(truth.numel()), grad, out


def bicubic4(x):
    N, C, H, W = (int(v) for v in x.shape)
    _chk(x, "x")
    out = torch.empty((N, C, 4 * H, 4 * W), device=x.device, dtype=torch.float32)
    _launch("larva_bicubic4_fwd", x.data_ptr(), out.data_ptr(), N, C, H, W)
    return out


_L1_WORKSPACES = {}


def _l1_partials(device):
    """A new buffer for the block partial sums of one L1 launch."""
    return torch.empty(int(hip_lib.load().larva_l1_workspace_floats()), device=device, dtype=torch.float32)


def _l1_workspace(device):
    """Block partial sums of l1_fwd, one buffer per (device, stream)."""
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    ws = _L1_WORKSPACES.get(key)
    if ws is None:
        ws = _L1_WORKSPACES[key] = _l1_partials(device)
    return ws


def l1_fwd(a, b):
    """mean |a - b| as a 0-d device tensor (one launch)."""
    _chk(a, "a")
    _chk(b, "b", a.shape)
    ws = _l1_workspace(a.device)
    loss = torch.empty((), device=a.device, dtype=torch.float32)
    _launch("larva_l1_fwd", a.data_ptr(), b.data_ptr(), a.numel(), ws.data_ptr(), loss.data_ptr())
    return loss


def l1_partial(a, b):
    """Block partial sums of sum|a - b| -> (partials [blocks], 1 / numel): an L1 term that
    loss_from_partials finishes together with the other exits' terms."""
    _chk(a, "a")
    _chk(b, "b", a.shape)
    part = _l1_partials(a.device)
    blocks = ctypes.c_int(0)
    _launch("larva_l1_partial", a.data_ptr(), b.data_ptr(), a.numel(), part.data_ptr(), ctypes.byref(blocks))
    return part[:int(blocks.value)], 1.0 / float(a.numel())


def l1_partial_grad(a, b, gvalue, gscale):
    """l1_partial + l1_bwd_unshuffle4 in one pass, for an upstream gradient known on the host:
    -> (partials, 1 / numel, grad [N][16C][H][W])."""
    _chk(a, "a")
    _chk(b, "b", a.shape)
    N, C, H, W = _lr_of(a, 4)
    part = _l1_partials(a.device)
    grad = torch.empty((N, 16 * C, H, W), device=a.device, dtype=torch.float32)
    blocks = ctypes.c_int(0)
    _launch("larva_l1_partial_grad", a.data_ptr(), b.data_ptr(), float(gvalue), float(gscale), part.data_ptr(),
            ctypes.byref(blocks), grad.data_ptr(), N, C, H, W)
    return part[:int(blocks.value)], 1.0 / float(a.numel()), grad


def l1_partial_grad_batch(outs, truth, gvalue, gscale):
    """l1_partial_grad for several exit images against one truth in one launch ->
    ([partials], 1 / numel, [grads])."""
    if not 1 <= len(outs) <= 8:
        raise RuntimeError("larvanet_amd: 1..8 images per batched L1 sweep")
    _chk(truth, "truth")
    N, C, H, W = _lr_of(truth, 4)
    ptrs = [_chk(o, "out", truth.shape) for o in outs]
    parts = [_l1_partials(truth.device) for _ in outs]
    grads = [torch.empty((N, 16 * C, H, W), device=truth.device, dtype=torch.float32) for _ in outs]
    blocks = ctypes.c_int(0)
    _launch("larva_l1_partial_grad_batch",
            hip_lib.ptr_array(ptrs), truth.data_ptr(), len(outs), float(gvalue), float(gscale),
            hip_lib.ptr_array([p.data_ptr() for p in parts]), ctypes.byref(blocks),
            hip_lib.ptr_array([g.data_ptr() for g in grads]), N, C, H, W)
    nb = int(blocks.value)
    return [p[:nb] for p in parts], 1.0 / float(truth.numel()), grads


class HostCell:
    """{float value, uint32 sequence} in coherent pinned host memory a kernel can store into (larva_host_cell_alloc):
    the host reads it without synchronising with a stream.  Every store of a kernel bumps the sequence number; the
    owner counts its launches (expect()) and take() returns a value only once the launch it waits for has stored."""

    def __init__(self):
        p = ctypes.c_void_p()
        _launch("larva_host_cell_alloc", ctypes.byref(p), stream=False)
        self.ptr = int(p.value)
        self._cell = ctypes.c_uint64.from_address(self.ptr)
        self.expected = 0
        # the sequence number in device memory as well: the storing launch reads it there instead of over PCIe
        self.dev_seq = torch.zeros(1, dtype=torch.int32, device="cuda") if torch.cuda.is_available() else None

    def expect(self):
        """Call once per launch (or graph replay) that stores into the cell, before it is issued."""
        self.expected = (self.expected + 1) & 0xFFFFFFFF

    def take(self):
        """The value of the launch announced last, or None while it has not stored yet."""
        raw = self._cell.value            # one aligned 8-byte load: value and sequence number belong together
        if (raw >> 32) != self.expected:
            return None
        return struct.unpack("<f", struct.pack("<I", raw & 0xFFFFFFFF))[0]

    @property
    def value(self):
        return struct.unpack("<f", struct.pack("<I", self._cell.value & 0xFFFFFFFF))[0]

    @property
    def sequence(self):
        return self._cell.value >> 32

    def __del__(self):
        ptr, self.ptr = getattr(self, "ptr", 0), 0
        if ptr:
            try:
                hip_lib.load().larva_host_cell_free(ptr)   # (synchronises with the device first)
            except Exception:   # interpreter shutdown
                pass


def loss_from_partials(terms, scales, divisor, host_cell=None):
    """( sum_i scales[i] * terms[i].sum() ) / divisor as a 0-d tensor, one launch, fixed order; host_cell
    (HostCell) receives the value too."""
    if not 1 <= len(terms) <= 8:
        raise RuntimeError("larvanet_amd: 1..8 loss terms")
    out = torch.empty((), device=terms[0].device, dtype=torch.float32)
    _launch("larva_loss_from_partials_to_host_seq",
            *_loss_terms(terms, scales), len(terms), float(divisor), out.data_ptr(),
            host_cell.ptr if host_cell is not None else None,
            host_cell.dev_seq.data_ptr() if host_cell is not None and host_cell.dev_seq is not None else None)
    return out


def l1_bwd_unshuffle4(a, b, gout, gscale=1.0):
    """Gradient of mean|a - b| * gscale w.r.t. a, written as [N][16C][H][W] (pixel-unshuffled)."""
    _chk(a, "a")
    _chk(b, "b", a.shape)
    _chk(gout, "gout", ())
    N, C, H, W = _lr_of(a, 4)
    out = torch.empty((N, 16 * C, H, W), device=a.device, dtype=torch.float32)
    _launch("larva_l1_bwd_unshuffle4", a.data_ptr(), b.data_ptr(), gout.data_ptr(), float(gscale), out.data_ptr(), N, C, H, W)
    return out


def sum_scalars(terms, divisor):
    ptrs = [_chk(t, "term", ()) for t in terms]
    out = torch.empty((), device=terms[0].device, dtype=torch.float32)
    _launch("larva_sum_scalars", hip_lib.ptr_array(ptrs), len(ptrs), float(divisor), out.data_ptr())
    return out


def l1_bwd(a, b, gout):
    _chk(a, "a")
    _chk(b, "b", a.shape)
    _chk(gout, "gout", ())
    ga = torch.empty_like(a)
    _launch("larva_l1_bwd", a.data_ptr(), b.data_ptr(), gout.data_ptr(), a.numel(), ga.data_ptr())
    return ga


def pixel_unshuffle4(g):
    _chk(g, "g")
    N, C, H, W = _lr_of(g, 4, "pixel_unshuffle4 needs spatial dims")
    out = torch.empty((N, 16 * C, H, W), device=g.device, dtype=torch.float32)
    _launch("larva_pixel_unshuffle4", g.data_ptr(), out.data_ptr(), N, C, H, W)
    return out


def adamw_step(p, g, m, v, step_lr, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    n = p.numel()
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, name, (n,))
    _chk(step_lr, "step_lr", (2,))
    _launch("larva_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step_lr.data_ptr(),
            beta1, beta2, eps, weight_decay, grad_scale, n)


def gather_patches(data, offsets, hw, draws, batch, patch, mult, out=None):
    """Augmented float patches [batch][3][patch][patch] from a uint8 dataset resident on the device
    (into `out` when given: e.g. the input buffer a captured training step reads)."""
    for t, name, dt in ((data, "data", torch.uint8), (offsets, "offsets", torch.int64), (hw, "hw", torch.int32),
                        (draws, "draws", torch.int32)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError("larvanet_amd: %s must be a contiguous %s tensor on the HIP device" % (name, dt))
    if tuple(draws.shape) != (batch, 5):
        raise RuntimeError("larvanet_amd: draws must be [batch][5]")
    out = _out(out, (batch, 3, patch, patch), data.device)
    _launch("larva_gather_patches", data.data_ptr(), offsets.data_ptr(), hw.data_ptr(), draws.data_ptr(),
            out.data_ptr(), batch, patch, mult)
    return out


def adamw_step_host(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0, copy=None):
    """One AdamW step over flat buffers, step count and learning rate given by the host.  copy = (src, dst):
    the launch also copies the 0-d tensor src into dst (the step's loss out of a captured graph's buffer)."""
    n = p.numel()
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, name, (n,))
    args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), int(step), float(lr), beta1, beta2, eps, weight_decay,
            grad_scale, n)
    if copy is None:
        _launch("larva_adamw_step_host", *args)
    else:
        src, dst = copy
        _chk(src, "copy source", ())
        _chk(dst, "copy destination", ())
        _launch("larva_adamw_step_host_copy", *args, src.data_ptr(), dst.data_ptr())


def psnr_u8(out_chw, truth_u8):
    """RGB PSNR of validate.py:17-27 computed on the device: out_chw float [C][H][W] (device),
    truth_u8 uint8 [C][TH][TW] (device), truth cropped top-left to the output size.  Returns a float
    (one 8-byte read-back instead of the whole HR image)."""
    import math
    _chk(out_chw, "out")
    if not truth_u8.is_cuda or truth_u8.dtype != torch.uint8 or not truth_u8.is_contiguous():
        raise RuntimeError("larvanet_amd: truth must be a contiguous uint8 tensor on the HIP device")
    C, H, W = (int(v) for v in out_chw.shape)
    TC, TH, TW = (int(v) for v in truth_u8.shape)
    if TC != C or TH < H or TW < W:
        raise RuntimeError("larvanet_amd: truth image smaller than the output")
    acc = torch.zeros(1, device=out_chw.device, dtype=torch.int64)
    _launch("larva_sqerr_u8", out_chw.data_ptr(), truth_u8.data_ptr(), C, H, W, TH, TW, acc.data_ptr())
    sq = int(acc.item())
    mse = sq / float(C * H * W)
    return float("inf") if mse == 0 else 10.0 * math.log10(255.0 ** 2 / mse)


# ------------------------------------------------------------------ fp16 inference (csrc/conv3x3_f16.hip)
F16_CHANNELS = 48
F16_MAX_SOURCES = 8


def _chk16(t, name, shape=None):
    """An fp16 channels-last activation [N][H][W][48] (torch.float16, contiguous, on the device)."""
    return _chk_tensor(t, name, shape, torch.float16, F16_CHANNELS)


def _chk_wpk16(wpk, n_src, what):
    """wpk is the fp16 A-operand image of a conv over n_src 48-channel inputs (f16_pack_weights)."""
    if wpk.dtype != torch.float16 or not wpk.is_cuda or wpk.numel() != f16_packed_weight_halves(F16_CHANNELS, F16_CHANNELS * n_src):
        raise RuntimeError("larvanet_amd: wpk is not the fp16 image of a %s conv" % what)


def _chk_flag(flag):
    if not isinstance(flag, torch.Tensor) or not flag.is_cuda or flag.dtype != torch.int32 or flag.numel() < 1:
        raise RuntimeError("larvanet_amd: the overflow flag must be an int32 device tensor")
    return flag.data_ptr()


def f16_packed_weight_halves(cout, cin):
    return int(hip_lib.load().larva_f16_packed_weight_halves(cout, cin))


def f16_pack_weights(w, out=None):
    """[48][48 m][3][3] fp32 weight -> its fp16 A-operand image (flat float16 tensor, include/larva_hip.h)."""
    _chk(w, "w")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError("larvanet_amd: only [cout][cin][3][3] weights are supported")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    n = f16_packed_weight_halves(cout, cin)
    if n < 0:
        raise RuntimeError("larvanet_amd: no fp16 conv for %d -> %d channels" % (cin, cout))
    if out is None:
        out = torch.empty(n, device=w.device, dtype=torch.float16)
    if out.dtype != torch.float16 or out.numel() != n or not out.is_contiguous():
        raise RuntimeError("larvanet_amd: fp16 weight image must be %d contiguous halves" % n)
    _launch("larva_f16_pack_weights", w.data_ptr(), out.data_ptr(), cout, cin)
    return out


def f16_head(x, w, bias, flag, out=None):
    """x fp32 [N][3][H][W] -> fp16 [N][H][W][48] = conv(x, w) + bias (fp32 operands, one rounding to fp16)."""
    N, C, H, W = (int(v) for v in x.shape)
    _chk(x, "x")
    _chk(w, "w", (F16_CHANNELS, 3, 3, 3))
    _chk(bias, "bias", (F16_CHANNELS,))
    if C != 3:
        raise RuntimeError("larvanet_amd: the fp16 head takes 3-channel images")
    out = _out(out, (N, H, W, F16_CHANNELS), x.device, torch.float16, F16_CHANNELS)
    _launch("larva_f16_head", x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), _chk_flag(flag), N, H, W)
    return out


def f16_conv3x3(srcs, wpk, bias, flag, relu=False, res0=None, res1=None, out=None):
    """48 -> 48 conv over the fp16 tensors `srcs` (consecutive 48-channel K chunks), + bias, then ReLU or + res0
    (+ res1), rounded once to fp16 -> [N][H][W][48]."""
    srcs = _src_list(srcs)
    if not 1 <= len(srcs) <= F16_MAX_SOURCES:
        raise RuntimeError("larvanet_amd: the fp16 conv takes 1 to %d inputs" % F16_MAX_SOURCES)
    shape = tuple(srcs[0].shape)
    ptrs = [_chk16(s, "srcs[%d]" % i, shape) for i, s in enumerate(srcs)]
    N, H, W = shape[:3]
    _chk_wpk16(wpk, len(srcs), "%d-input" % len(srcs))
    _chk(bias, "bias", (F16_CHANNELS,))
    if relu and res0 is not None:
        raise RuntimeError("larvanet_amd: the fp16 conv has no ReLU + residual epilogue")
    if res1 is not None and res0 is None:
        raise RuntimeError("larvanet_amd: res1 needs res0")
    r0 = None if res0 is None else _chk16(res0, "res0", shape)
    r1 = None if res1 is None else _chk16(res1, "res1", shape)
    out = _out(out, shape, srcs[0].device, torch.float16, F16_CHANNELS)
    _launch("larva_f16_conv3x3", hip_lib.ptr_array(ptrs), len(ptrs), wpk.data_ptr(), bias.data_ptr(), r0, r1,
            int(bool(relu)), out.data_ptr(), _chk_flag(flag), N, H, W)
    return out


def f16_conv3x3_shuffle_base(src, wpk, bias, base):
    """Leg end: fp32 [N][3][4H][4W] = PixelShuffle(4)(conv(src) + bias) + base, src fp16 [N][H][W][48]."""
    _chk16(src, "src")
    N, H, W = (int(v) for v in src.shape[:3])
    _chk_wpk16(wpk, 1, "48 -> 48")
    _chk(bias, "bias", (F16_CHANNELS,))
    hr = (N, 3, 4 * H, 4 * W)
    _chk(base, "base", hr)
    out = torch.empty(hr, device=src.device, dtype=torch.float32)
    _launch("larva_f16_conv3x3_shuffle_base", src.data_ptr(), wpk.data_ptr(), bias.data_ptr(), base.data_ptr(),
            out.data_ptr(), N, H, W)
    return out


def f16_conv3x3_shuffle_base_u8(src, wpk, bias, base, flag, out=None):
    """The leg end as a uint8 image: uint8 [N][4H][4W][3] = f32_chw_to_u8_hwc(f16_conv3x3_shuffle_base(...)), bit for
    bit, in one launch (the fp32 HR image is never stored).  A non-finite value sets `flag`."""
    _chk16(src, "src")
    N, H, W = (int(v) for v in src.shape[:3])
    _chk_wpk16(wpk, 1, "48 -> 48")
    _chk(bias, "bias", (F16_CHANNELS,))
    _chk(base, "base", (N, 3, 4 * H, 4 * W))
    out = _out(out, (N, 4 * H, 4 * W, 3), src.device, torch.uint8, 3)
    _launch("larva_f16_conv3x3_shuffle_base_u8", src.data_ptr(), wpk.data_ptr(), bias.data_ptr(), base.data_ptr(),
            out.data_ptr(), _chk_flag(flag), N, H, W)
    return out


F16_MAX_JOBS = 8


def _chk_f16_jobs(srcs, wpks, biases):
    """The per-job operands of a job launch -> ((N, H, W), the three pointer arrays)."""
    if not (1 <= len(srcs) <= F16_MAX_JOBS and len(wpks) == len(srcs) and len(biases) == len(srcs)):
        raise RuntimeError("larvanet_amd: an fp16 job launch takes 1 to %d jobs, each with a source, a weight image and "
                           "a bias" % F16_MAX_JOBS)
    shape = tuple(int(v) for v in srcs[0].shape)
    ps = [_chk16(s, "srcs[%d]" % j, shape) for j, s in enumerate(srcs)]
    for w in wpks:
        _chk_wpk16(w, 1, "48 -> 48")
    pb = [_chk(b, "biases[%d]" % j, (F16_CHANNELS,)) for j, b in enumerate(biases)]
    return shape[:3], (hip_lib.ptr_array(ps), hip_lib.ptr_array([w.data_ptr() for w in wpks]), hip_lib.ptr_array(pb))


def f16_conv3x3_jobs(srcs, wpks, biases, flag, relu=False, out=None):
    """len(srcs) (1..8) independent 48 -> 48 convs of one shape in ONE launch: job j = f16_conv3x3(srcs[j], wpks[j],
    biases[j], relu=relu), bit for bit -> fp16 [njobs][N][H][W][48] (one tensor; out[j] is job j's)."""
    (N, H, W), arrays = _chk_f16_jobs(srcs, wpks, biases)
    out = _out(out, (len(srcs), N, H, W, F16_CHANNELS), srcs[0].device, torch.float16)
    outs = hip_lib.ptr_array([out[j].data_ptr() for j in range(len(srcs))])
    _launch("larva_f16_conv3x3_jobs", len(srcs), *arrays, int(bool(relu)), outs, _chk_flag(flag), N, H, W)
    return out


def f16_conv3x3_shuffle_base_jobs(srcs, wpks, biases, base, flag=None, u8=False, out=None):
    """The leg end of every job against one shared base, in ONE launch: job j = f16_conv3x3_shuffle_base(srcs[j], wpks[j],
    biases[j], base) -> fp32 [njobs][N][3][4H][4W], or with u8 f16_conv3x3_shuffle_base_u8(...) -> uint8
    [njobs][N][4H][4W][3] (needs flag), bit for bit."""
    (N, H, W), arrays = _chk_f16_jobs(srcs, wpks, biases)
    _chk(base, "base", (N, 3, 4 * H, 4 * W))
    M = len(srcs)
    shape, dtype = ((M, N, 4 * H, 4 * W, 3), torch.uint8) if u8 else ((M, N, 3, 4 * H, 4 * W), torch.float32)
    out = _out(out, shape, srcs[0].device, dtype)
    outs = hip_lib.ptr_array([out[j].data_ptr() for j in range(M)])
    fl = _chk_flag(flag) if (u8 or flag is not None) else None
    _launch("larva_f16_conv3x3_shuffle_base_jobs", M, *arrays, base.data_ptr(), None if u8 else outs, outs if u8 else None,
            fl, N, H, W)
    return out


# ------------------------------------------------------------------ 8-bit images (csrc/larva_pointwise.hip)
def _chk_u8(t, name, shape=None):
    """A uint8 image batch [N][H][W][3] (torch.uint8, contiguous, on the device)."""
    return _chk_tensor(t, name, shape, torch.uint8, 3)


def u8_hwc_to_f32_chw(x, out=None):
    """uint8 [N][H][W][3] (decoded images) -> float32 [N][3][H][W], exact."""
    _chk_u8(x, "x")
    N, H, W = (int(v) for v in x.shape[:3])
    out = _out(out, (N, 3, H, W), x.device)
    _launch("larva_u8_hwc_to_f32_chw", x.data_ptr(), out.data_ptr(), N, H, W)
    return out


def f32_chw_to_u8_hwc(x, out=None):
    """float32 [N][3][H][W] -> uint8 [N][H][W][3] = clip(round half to even(x), 0, 255): metrics.image_to_uint8 on the
    device, transposed for an image writer."""
    _chk(x, "x")
    if x.dim() != 4 or int(x.shape[1]) != 3:
        raise RuntimeError("larvanet_amd: x must be [N][3][H][W], got %s" % (tuple(x.shape),))
    N, _, H, W = (int(v) for v in x.shape)
    out = _out(out, (N, H, W, 3), x.device, torch.uint8, 3)
    _launch("larva_f32_chw_to_u8_hwc", x.data_ptr(), out.data_ptr(), N, H, W)
    return out


# ------------------------------------------------------------------ geometric self-ensemble (csrc/larva_ensemble.hip)
def dihedral_inputs(x, out=None):
    """The eight dihedral images (image_utils.dihedral) of x, uint8 [N][H][W][3] or float32 [N][3][H][W], as batch slots,
    exact, in one launch -> (A float32 [4N][3][H][W], B float32 [4N][3][W][H]): image n under t is A[4 n + t] for t < 4
    and B[4 n + t - 4] for t >= 4.  out = (A, B) to fill the caller's buffers."""
    if isinstance(x, torch.Tensor) and x.dtype == torch.uint8:
        _chk_u8(x, "x")
        N, H, W = (int(v) for v in x.shape[:3])
        name = "larva_dihedral_inputs_u8"
    else:
        _chk(x, "x")
        if x.dim() != 4 or int(x.shape[1]) != 3:
            raise RuntimeError("larvanet_amd: x must be uint8 [N][H][W][3] or float32 [N][3][H][W], got %s" % (tuple(x.shape),))
        N, _, H, W = (int(v) for v in x.shape)
        name = "larva_dihedral_inputs_f32"
    if min(N, H, W) < 1:
        raise RuntimeError("larvanet_amd: x must not be empty, got %s" % (tuple(x.shape),))
    a, b = (None, None) if out is None else out
    a = _out(a, (4 * N, 3, H, W), x.device, name="A")
    b = _out(b, (4 * N, 3, W, H), x.device, name="B")
    _launch(name, x.data_ptr(), a.data_ptr(), b.data_ptr(), N, H, W)
    return a, b


def dihedral_mean(a, b, u8=False, out=None):
    """The self-ensemble's merge in one launch: a float32 [4N][3][H][W] and b float32 [4N][3][W][H] (the forward's outputs
    for dihedral_inputs' A and B) -> the fixed-order fp32 mean of the eight images mapped back (image_utils.dihedral_inv),
    float32 [N][3][H][W], or with u8 its uint8 [N][H][W][3] form (f32_chw_to_u8_hwc of the former, bit for bit)."""
    _chk(a, "A")
    if a.dim() != 4 or int(a.shape[1]) != 3 or int(a.shape[0]) % 4 or min(a.shape) < 1:
        raise RuntimeError("larvanet_amd: A must be [4N][3][H][W], got %s" % (tuple(a.shape),))
    n4, _, H, W = (int(v) for v in a.shape)
    _chk(b, "B", (n4, 3, W, H))
    if b.device != a.device:
        raise RuntimeError("larvanet_amd: A and B must be on one device")
    N = n4 // 4
    if u8:
        out = _out(out, (N, H, W, 3), a.device, torch.uint8, 3)
        f32, q8 = None, out.data_ptr()
    else:
        out = _out(out, (N, 3, H, W), a.device)
        f32, q8 = out.data_ptr(), None
    _launch("larva_dihedral_mean", a.data_ptr(), b.data_ptr(), f32, q8, N, H, W)
    return out


# ------------------------------------------------------------------ benchmark metrics (csrc/larva_metrics.hip)
METRIC_CHANNELS = {"rgb": 0, "y": 1}
METRIC_RESULT_WORDS = 8   # int64 words of a result record (include/larva_hip.h)
SSIM_WINDOW = 11


def _chk_u8_image(t, name):
    """One uint8 image [H][W][3] (torch.uint8, contiguous, on the device)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("larvanet_amd: %s must be a uint8 tensor, got %s" % (name, type(t).__name__))
    if t.dtype != torch.uint8:
        raise TypeError("larvanet_amd: %s must be a uint8 tensor, got %s" % (name, t.dtype))
    if t.dim() != 3 or int(t.shape[2]) != 3 or min(t.shape) < 1:
        raise ValueError("larvanet_amd: %s must be [H][W][3], got %s" % (name, tuple(t.shape)))
    if not t.is_cuda:
        raise RuntimeError("larvanet_amd: %s must be a tensor on a HIP device (no CPU path exists)" % name)
    if not t.is_contiguous():
        raise RuntimeError("larvanet_amd: %s must be contiguous" % name)
    return t.data_ptr()


def metric_window(out_shape, truth_shape, shave, ssim):
    """(y0, x0, h, w) of the evaluation window: the truth cropped top-left to the output, both shaved by `shave`.
    Raises ValueError for what no launch may see: a truth smaller than the output, a negative shave, an empty window,
    a window below 11 pixels when SSIM is wanted."""
    oh, ow = int(out_shape[0]), int(out_shape[1])
    th, tw = int(truth_shape[0]), int(truth_shape[1])
    shave = int(shave)
    if shave < 0:
        raise ValueError("larvanet_amd: metrics need shave >= 0, got %d" % shave)
    if th < oh or tw < ow:
        raise ValueError("larvanet_amd: the truth image (%d x %d) is smaller than the output (%d x %d)" % (th, tw, oh, ow))
    h, w = oh - 2 * shave, ow - 2 * shave
    if h < 1 or w < 1:
        raise ValueError("larvanet_amd: nothing is left of a %d x %d image after shaving %d pixels" % (oh, ow, shave))
    if ssim and (h < SSIM_WINDOW or w < SSIM_WINDOW):
        raise ValueError("larvanet_amd: SSIM needs a window of at least %d x %d pixels, got %d x %d"
                         % (SSIM_WINDOW, SSIM_WINDOW, h, w))
    return shave, shave, h, w


def u8_metrics(out_u8_hwc, truth_u8_hwc, shave, channel, ssim=True, result=None):
    """Squared error and SSIM of one uint8 [oh][ow][3] output against its uint8 [th][tw][3] truth (th >= oh, tw >= ow:
    cropped top-left), both without `shave` border pixels, on the colour planes (channel "rgb") or the BT.601 luma plane
    ("y").  Returns the device result record (int64 [8], include/larva_hip.h; `result` to write into a given one);
    metrics_from_record turns its host copy into numbers.  Nothing comes back to the host here."""
    if channel not in METRIC_CHANNELS:
        raise ValueError("larvanet_amd: channel must be 'y' or 'rgb', got %r" % (channel,))
    po = _chk_u8_image(out_u8_hwc, "out")
    pt = _chk_u8_image(truth_u8_hwc, "truth")
    if out_u8_hwc.device != truth_u8_hwc.device:
        raise RuntimeError("larvanet_amd: out and truth are on different devices")
    y0, x0, h, w = metric_window(out_u8_hwc.shape, truth_u8_hwc.shape, shave, ssim)
    mode = METRIC_CHANNELS[channel]
    nbytes = int(hip_lib.load().larva_u8_metrics_workspace_bytes(h, w, mode))
    if nbytes < 0:
        raise ValueError("larvanet_amd: no metric kernel for a %d x %d window" % (h, w))
    workspace = torch.empty(nbytes // 8, device=out_u8_hwc.device, dtype=torch.int64)
    if result is None:
        result = torch.empty(METRIC_RESULT_WORDS, device=out_u8_hwc.device, dtype=torch.int64)
    elif (not isinstance(result, torch.Tensor) or result.dtype != torch.int64 or result.numel() != METRIC_RESULT_WORDS
          or not result.is_contiguous() or result.device != out_u8_hwc.device):
        raise RuntimeError("larvanet_amd: result must be a contiguous int64 [%d] tensor on the images' device"
                           % METRIC_RESULT_WORDS)
    _launch("larva_u8_metrics", po, 3 * int(out_u8_hwc.shape[1]), pt, 3 * int(truth_u8_hwc.shape[1]), y0, x0, h, w,
            mode, int(bool(ssim)), workspace.data_ptr(), result.data_ptr())
    return result


def metrics_from_record(record):
    """Host copy of a result record (int64 [8], CPU tensor or numpy) -> {"psnr", "ssim", "sse", "n"}; ssim is None when
    the record was made without it."""
    import numpy as np
    from .metrics import psnr_from_sse
    r = np.ascontiguousarray(record.numpy() if isinstance(record, torch.Tensor) else record, dtype=np.int64)
    sse, count, n, planes = int(r.view(np.uint64)[0]), int(r[4]), int(r[5]), int(r[6])
    sums = r.view(np.float64)[1:1 + planes]
    ssim = None if count == 0 else float(sum(float(v) / count for v in sums) / planes)
    return {"psnr": psnr_from_sse(sse, n), "ssim": ssim, "sse": sse, "n": n}


# ------------------------------------------------------------------ bicubic decimation (csrc/larva_downscale.hip)
DOWN_TILE_ROWS = 8     # a workgroup's tile: 8 output rows x 96 output bytes (kDownRows / kDownBytes of the kernel)
DOWN_TILE_BYTES = 96


def bicubic_down_size(height, width, scale):
    """(h, w) of the decimated image; ValueError for a scale other than 2, 3, 4 or less than one output pixel."""
    from .image_utils import bicubic_down_size as size
    return size(height, width, scale)


def bicubic_down_u8(x_u8_hwc, scale, out=None):
    """uint8 [H][W][3] on the device -> uint8 [H // scale][W // scale][3]: the bicubic decimation of SR data preparation
    (image_utils.bicubic_downscale_u8, byte for byte), scale 2, 3 or 4, in one launch.  x may be a window into a larger
    image: pixels contiguous (strides (pitch, 3, 1) with pitch >= 3 W), any pitch and offset.  `out`: a contiguous uint8
    [h][w][3] tensor to fill."""
    x = x_u8_hwc
    if not isinstance(x, torch.Tensor):
        raise TypeError("larvanet_amd: x must be a uint8 tensor, got %s" % type(x).__name__)
    if x.dtype != torch.uint8:
        raise TypeError("larvanet_amd: x must be a uint8 tensor, got %s" % x.dtype)
    if x.dim() != 3 or int(x.shape[2]) != 3:
        raise ValueError("larvanet_amd: x must be [H][W][3], got %s" % (tuple(x.shape),))
    H, W = int(x.shape[0]), int(x.shape[1])
    h, w = bicubic_down_size(H, W, scale)
    if not x.is_cuda:
        raise RuntimeError("larvanet_amd: x must be a tensor on a HIP device (no CPU path exists)")
    pitch = 3 * W if H == 1 else int(x.stride(0))
    if int(x.stride(2)) != 1 or int(x.stride(1)) != 3 or pitch < 3 * W:
        raise RuntimeError("larvanet_amd: x must have contiguous pixels and rows that do not overlap (strides %s)"
                           % (tuple(x.stride()),))
    if out is None:
        out = torch.empty((h, w, 3), device=x.device, dtype=torch.uint8)
    else:
        _chk_u8_image(out, "out")
        if tuple(out.shape) != (h, w, 3) or out.device != x.device:
            raise RuntimeError("larvanet_amd: out must be [%d][%d][3] on the input's device, got %s"
                               % (h, w, tuple(out.shape)))
    _launch("larva_bicubic_down_u8", x.data_ptr(), H, W, pitch, int(scale), out.data_ptr())
    return out


def bicubic_down_table_layout(shapes, scale):
    """(H, W) per image -> (offsets int64 [n], hw int32 [2 n], bytes) of the table of their 3-channel decimated images
    laid end to end (either channel order)."""
    import numpy as np
    sizes = [bicubic_down_size(H, W, scale) for H, W in shapes]
    offsets = np.zeros(len(sizes), np.int64)
    offsets[1:] = np.cumsum([3 * h * w for h, w in sizes])[:-1]
    return offsets, np.asarray([d for hw in sizes for d in hw], np.int32), int(sum(3 * h * w for h, w in sizes))


def bicubic_down_u8_table(data, offsets, hw, scale, out, out_offsets, planar=False):
    """Every image of a uint8 table on the device decimated in ONE launch: image i at data[offsets[i]:] with (H, W) =
    hw[2 i], hw[2 i + 1] (gather_patches' arguments) -> out[out_offsets[i]:], each equal to bicubic_down_u8 of that image.
    planar=False: HWC images [H][W][3] -> [h][w][3]; planar=True: the sampler's CHW images [3][H][W] -> [3][h][w].  Bytes of
    `out` outside the images stay as they are.  The four small tables are read back once to check every image against
    both byte tables and to cut the flat grid (a dataset is prepared once); returns `out`."""
    import numpy as np
    for t, name, dt in ((data, "data", torch.uint8), (offsets, "offsets", torch.int64), (hw, "hw", torch.int32),
                        (out, "out", torch.uint8), (out_offsets, "out_offsets", torch.int64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError("larvanet_amd: %s must be a %s tensor" % (name, dt))
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("larvanet_amd: %s must be a contiguous 1-D tensor, got %s" % (name, tuple(t.shape)))
        if not t.is_cuda or t.device != data.device:
            raise RuntimeError("larvanet_amd: %s must be on the HIP device of the table (no CPU path exists)" % name)
    n = int(offsets.numel())
    if n < 1 or int(hw.numel()) != 2 * n or int(out_offsets.numel()) != n:
        raise ValueError("larvanet_amd: %d offsets need %d sizes and %d output offsets" % (n, 2 * n, n))
    src_off, dst_off, sizes = offsets.cpu().numpy(), out_offsets.cpu().numpy(), hw.cpu().numpy().reshape(n, 2)
    per_row = DOWN_TILE_BYTES if planar else DOWN_TILE_BYTES // 3
    prefix, spans = np.zeros(n + 1, np.int64), []
    for i, (H, W) in enumerate(sizes):
        h, w = bicubic_down_size(int(H), int(W), scale)
        if src_off[i] < 0 or src_off[i] + 3 * int(H) * int(W) > data.numel():
            raise ValueError("larvanet_amd: image %d lies outside the source table" % i)
        if dst_off[i] < 0 or dst_off[i] + 3 * h * w > out.numel():
            raise ValueError("larvanet_amd: image %d lies outside the destination table" % i)
        spans.append((int(dst_off[i]), int(dst_off[i]) + 3 * h * w))
        prefix[i + 1] = prefix[i] + (3 if planar else 1) * (-(-h // DOWN_TILE_ROWS)) * (-(-w // per_row))
    spans.sort()
    if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        raise ValueError("larvanet_amd: decimated images overlap in the destination table")
    if prefix[n] >= 2 ** 31:
        raise ValueError("larvanet_amd: too many tiles for one launch (%d)" % prefix[n])
    tiles = torch.from_numpy(prefix.astype(np.int32)).to(data.device)
    _launch("larva_bicubic_down_u8_table", data.data_ptr(), offsets.data_ptr(), hw.data_ptr(), n, int(scale),
            int(bool(planar)), out.data_ptr(), out_offsets.data_ptr(), tiles.data_ptr(), int(prefix[n]))
    return out


# ------------------------------------------------------------------ planar YUV 4:2:0 frames (csrc/larva_yuv.hip)
def _chk_frames(t, name, width, height):
    """A batch of I420 frames: uint8 [N][pitch] on the device, rows contiguous, pitch >= the frame's bytes -> (N, pitch)."""
    from .image_utils import i420_frame_bytes
    need = i420_frame_bytes(width, height)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("larvanet_amd: %s must be a tensor on a HIP device (no CPU path exists)" % name)
    if t.dtype != torch.uint8:
        raise RuntimeError("larvanet_amd: %s must be uint8, got %s" % (name, t.dtype))
    if t.dim() != 2 or int(t.shape[0]) < 1 or int(t.shape[1]) < need:
        raise RuntimeError("larvanet_amd: %s must be [N][>= %d bytes] (I420 frames of %d x %d), got %s"
                           % (name, need, width, height, tuple(t.shape)))
    if t.stride(1) != 1 or (int(t.shape[0]) > 1 and t.stride(0) < need):
        raise RuntimeError("larvanet_amd: the frames of %s must be contiguous and must not overlap" % name)
    return int(t.shape[0]), (int(t.stride(0)) if int(t.shape[0]) > 1 else int(t.shape[1]))


def _yuv_dims(width, height):
    width, height = int(width), int(height)
    if not (1 <= width <= 32768 and 1 <= height <= 32768):
        raise RuntimeError("larvanet_amd: a frame's width and height must be 1 .. 32768, got %d x %d" % (width, height))
    return width, height


def i420_to_rgb_f32(frames, width, height, matrix="bt601", full_range=False, out=None):
    """uint8 [N][pitch] I420 frames of width x height (pitch >= image_utils.i420_frame_bytes) -> float32 [N][3][H][W] RGB
    on [0, 255] in steps of 1 / 256: image_utils.i420_to_rgb_f32 per frame, bit for bit, in one launch."""
    from .image_utils import yuv_to_rgb_table
    W, H = _yuv_dims(width, height)
    table = hip_lib.int_array(yuv_to_rgb_table(matrix, full_range))
    N, pitch = _chk_frames(frames, "frames", W, H)
    out = _out(out, (N, 3, H, W), frames.device)
    if out.device != frames.device:
        raise RuntimeError("larvanet_amd: frames and out must be on one device")
    _launch("larva_i420_to_rgb_f32", frames.data_ptr(), pitch, out.data_ptr(), N, H, W, table)
    return out


def rgb_u8_to_i420(x, matrix="bt601", full_range=False, out=None):
    """uint8 [N][H][W][3] RGB -> uint8 [N][frame bytes] I420 frames: image_utils.rgb_u8_to_i420 per image, bit for bit, in
    one launch.  out: uint8 [N][pitch >= frame bytes] to fill (bytes of a row beyond the frame are left alone)."""
    from .image_utils import i420_frame_bytes, rgb_to_yuv_table
    table = hip_lib.int_array(rgb_to_yuv_table(matrix, full_range))
    _chk_u8(x, "x")
    N, H, W = (int(v) for v in x.shape[:3])
    if N < 1:
        raise RuntimeError("larvanet_amd: x must not be empty, got %s" % (tuple(x.shape),))
    _yuv_dims(W, H)
    if out is None:
        out = torch.empty((N, i420_frame_bytes(W, H)), device=x.device, dtype=torch.uint8)
    n_out, pitch = _chk_frames(out, "out", W, H)
    if n_out != N or out.device != x.device:
        raise RuntimeError("larvanet_amd: out must hold %d frames on x's device, got %s" % (N, tuple(out.shape)))
    _launch("larva_rgb_u8_to_i420", x.data_ptr(), out.data_ptr(), pitch, N, H, W, table)
    return out


# ------------------------------------------------------------------ bicubic resize to any size (csrc/larva_resize.hip)
RESIZE_TILE_ROWS = 16    # a workgroup's tile: 16 output rows x 32 output pixels (kResizeRows / kResizeCols of the kernel)
RESIZE_TILE_COLS = 32
_RESIZE_TABLES = {}      # (n_in, n_out, device) -> (bounds, coeffs, ksize) on the device; a few entries per video or folder
_RESIZE_TABLES_MAX = 64


def _resize_tables(n_in, n_out, device):
    """The device tables of one axis (image_utils.resize_coeffs), cached; (None, None, 0) for an axis that keeps its size."""
    if n_in == n_out:
        return None, None, 0
    key = (n_in, n_out, str(device))
    hit = _RESIZE_TABLES.get(key)
    if hit is None:
        from .image_utils import resize_coeffs
        bounds, coeffs = resize_coeffs(n_in, n_out)
        while len(_RESIZE_TABLES) >= _RESIZE_TABLES_MAX:
            _RESIZE_TABLES.pop(next(iter(_RESIZE_TABLES)))
        hit = (torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device), int(coeffs.shape[1]))
        _RESIZE_TABLES[key] = hit
    return hit


def resize_u8(x_u8_hwc, out_h, out_w, out=None):
    """uint8 [N][H][W][3] (or one image [H][W][3]) on the device -> uint8 [N][out_h][out_w][3] ([out_h][out_w][3]): Pillow's
    Image.resize((out_w, out_h), Image.BICUBIC) per image (image_utils.resize_u8, byte for byte), both passes in one launch.
    An axis shrinks by at most 4 (ValueError beyond); any upsampling.  `out`: a contiguous uint8 tensor of the result's
    shape to fill."""
    from .image_utils import check_resize
    x = x_u8_hwc
    if not isinstance(x, torch.Tensor):
        raise TypeError("larvanet_amd: x must be a uint8 tensor, got %s" % type(x).__name__)
    if x.dtype != torch.uint8:
        raise TypeError("larvanet_amd: x must be a uint8 tensor, got %s" % x.dtype)
    if x.dim() not in (3, 4) or int(x.shape[-1]) != 3 or min(x.shape) < 1:
        raise ValueError("larvanet_amd: x must be [N][H][W][3] or [H][W][3], got %s" % (tuple(x.shape),))
    H, W = int(x.shape[-3]), int(x.shape[-2])
    N = int(x.shape[0]) if x.dim() == 4 else 1
    h, w = check_resize(H, W, out_h, out_w)
    if not x.is_cuda:
        raise RuntimeError("larvanet_amd: x must be a tensor on a HIP device (no CPU path exists)")
    if not x.is_contiguous():
        raise RuntimeError("larvanet_amd: x must be contiguous (strides %s)" % (tuple(x.stride()),))
    shape = tuple(x.shape[:-3]) + (h, w, 3)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.uint8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape
          or out.device != x.device or not out.is_contiguous()):
        raise RuntimeError("larvanet_amd: out must be a contiguous uint8 %s tensor on the input's device" % (list(shape),))
    hb, hc, kx = _resize_tables(W, w, x.device)
    vb, vc, ky = _resize_tables(H, h, x.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    _launch("larva_resize_u8", x.data_ptr(), out.data_ptr(), N, H, W, h, w, ptr(hb), ptr(hc), kx, ptr(vb), ptr(vc), ky)
    return out


# ------------------------------------------------------------------ transparency: RGBA images (csrc/larva_rgba.hip)
_ALPHA_TABLES = {}       # (opacity flags, device) -> (int32 [N] device table, K); a handful of entries per folder
_ALPHA_TABLES_MAX = 64


def alpha_slot_table(opaque, device):
    """image_utils.alpha_slots(opaque) with the table on `device`, cached -> (int32 [N] device tensor, K)."""
    key = (tuple(bool(f) for f in opaque), str(device))
    hit = _ALPHA_TABLES.get(key)
    if hit is None:
        from .image_utils import alpha_slots
        table, k = alpha_slots(key[0])
        while len(_ALPHA_TABLES) >= _ALPHA_TABLES_MAX:
            _ALPHA_TABLES.pop(next(iter(_ALPHA_TABLES)))
        hit = (torch.from_numpy(table).to(device), k)
        _ALPHA_TABLES[key] = hit
    return hit


def _chk_alpha_slot(alpha_slot, n, k, device):
    _chk_tensor(alpha_slot, "alpha_slot", (n,), torch.int32)
    if alpha_slot.device != device:
        raise RuntimeError("larvanet_amd: alpha_slot must be on the images' device")
    k = int(k)
    if not 0 <= k <= n:
        raise RuntimeError("larvanet_amd: K (the alpha slots) must be 0 .. N = %d, got %d" % (n, k))
    return k


def rgba_u8_split_f32(x, alpha_slot, k, out=None):
    """uint8 [N][H][W][4] RGBA -> float32 [N + K][3][H][W], exact, in one launch (image_utils.rgba_split_f32): slot n = the
    colour planes of image n, slot alpha_slot[n] = its alpha three times.  alpha_slot: int32 [N] on the device
    (alpha_slot_table), K of its entries name the slots N .. N + K - 1, every other entry means opaque."""
    _chk_tensor(x, "x", None, torch.uint8, 4)
    N, H, W = (int(v) for v in x.shape[:3])
    if min(N, H, W) < 1:
        raise RuntimeError("larvanet_amd: x must not be empty, got %s" % (tuple(x.shape),))
    k = _chk_alpha_slot(alpha_slot, N, k, x.device)
    out = _out(out, (N + k, 3, H, W), x.device)
    if out.device != x.device:
        raise RuntimeError("larvanet_amd: x and out must be on one device")
    _launch("larva_rgba_u8_split_f32", x.data_ptr(), alpha_slot.data_ptr(), out.data_ptr(), N, k, H, W)
    return out


def rgb_u8_merge_rgba(rgb, alpha_slot, n, out=None):
    """uint8 [N + K][h][w][3] (the forward's result for rgba_u8_split_f32's slots) -> uint8 [N][h][w][4] in one launch
    (image_utils.rgba_merge_u8): colour from slot n, alpha = (r + g + b + 1) // 3 of slot alpha_slot[n], 255 for an image
    without a slot.  out: a contiguous uint8 [N][h][w][4] tensor to fill."""
    _chk_u8(rgb, "rgb")
    n = int(n)
    M, h, w = (int(v) for v in rgb.shape[:3])
    if n < 1 or min(h, w) < 1 or not n <= M <= 2 * n:
        raise RuntimeError("larvanet_amd: rgb must hold N + K slots (N = %d, 0 <= K <= N), got %s" % (n, tuple(rgb.shape)))
    k = _chk_alpha_slot(alpha_slot, n, M - n, rgb.device)
    out = _out(out, (n, h, w, 4), rgb.device, torch.uint8, 4)
    if out.device != rgb.device:
        raise RuntimeError("larvanet_amd: rgb and out must be on one device")
    _launch("larva_rgb_u8_merge_rgba", rgb.data_ptr(), alpha_slot.data_ptr(), out.data_ptr(), n, k, h, w)
    return out
