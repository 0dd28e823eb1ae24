"""Operands at a chosen address residue, inside a guarded buffer (test helper, not a test; imported by path like
exact_ref.py).

Many launchers pick a kernel variant, or refuse, from the low bits of the pointers they are given.  A fresh torch tensor
starts on a 256-byte boundary or better, so those predicates only ever see zeros.  placed() builds one flat uint8
allocation of guard + 16 + nbytes + guard bytes, all `fill`, reads its real data_ptr() (the allocator's alignment is
measured, not assumed) and returns a contiguous view of the wanted dtype and shape whose data_ptr() % 16 == offset, plus
a check() that copies the buffer back and asserts that every byte outside the view still holds `fill`: a store that
reaches outside an output, or any store to an input, is seen."""
import numpy as np
import torch

ALIGN = 16
FILL = 0xA5


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def placed(array_or_shape, dtype, device, offset, guard=64, fill=FILL, pitch=None):
    """-> (view, check).

    array_or_shape: a numpy array whose values the view starts with (cast to `dtype`), or a shape: the view then holds
    `fill` bytes like everything around it.  offset: the view's address modulo 16, a multiple of the item size.
    pitch (2-D frame batches [N][row bytes], uint8): rows are `pitch` >= row bytes apart; the view is [N][pitch], the
    array fills the first row bytes of each row, the rest of a row holds `fill` and is watched by check() like the guards.
    check(untouched=False): asserts the guards (and row tails) hold `fill`; untouched=True: the view's own bytes too."""
    item = _itemsize(dtype)
    offset = int(offset)
    if not 0 <= offset < ALIGN or offset % item:
        raise ValueError("placement: offset %d is not a multiple of the item size %d below %d" % (offset, item, ALIGN))
    arr = None
    if isinstance(array_or_shape, np.ndarray):
        arr = np.ascontiguousarray(array_or_shape)
        shape = tuple(arr.shape)
    else:
        shape = tuple(int(v) for v in array_or_shape)
    row = None
    if pitch is not None:
        if len(shape) != 2 or item != 1 or int(pitch) < shape[1]:
            raise ValueError("placement: a pitch needs a uint8 [N][row bytes] batch and pitch >= row bytes")
        row, shape = shape[1], (shape[0], int(pitch))
    count = int(np.prod(shape, dtype=np.int64))
    nbytes = count * item
    buf = torch.full((guard + ALIGN + nbytes + guard,), fill, dtype=torch.uint8, device=device)
    start = guard + (offset - (buf.data_ptr() + guard)) % ALIGN
    view = buf[start:start + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % ALIGN == offset and view.is_contiguous() and view.data_ptr() == buf.data_ptr() + start
    if arr is not None:
        src = torch.from_numpy(arr).to(dtype)
        if row is None:
            view.copy_(src)
        else:
            view[:, :row].copy_(src)
    watched = np.ones(buf.numel(), bool)              # bytes that must keep `fill`
    inside = np.zeros(shape, bool) if row is not None else None
    if row is not None:
        inside[:, :row] = True
        watched[start:start + nbytes] = ~inside.ravel()
    else:
        watched[start:start + nbytes] = False

    def check(untouched=False):
        got = buf.cpu().numpy()
        bad = np.flatnonzero((got != fill) & (True if untouched else watched))
        if bad.size:
            raise AssertionError("placement: %d byte(s) outside the operand were written (view of %d bytes at residue %d): "
                                 "first at offset %d, last at offset %d relative to the view's first byte"
                                 % (bad.size, nbytes, offset, int(bad[0]) - start, int(bad[-1]) - start))

    return view, check


def same_everywhere(results, what):
    """results: {placement: numpy array} -> asserts all of them hold identical bytes."""
    keys = list(results)
    first = results[keys[0]]
    for k in keys[1:]:
        a = results[k]
        assert a.shape == first.shape and a.dtype == first.dtype and np.array_equal(
            a.view(np.uint8).reshape(-1), first.view(np.uint8).reshape(-1)), \
            "%s: placement %r and placement %r give different bytes" % (what, keys[0], k)
