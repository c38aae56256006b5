"""Poisoned guards around strided operands (pure torch / numpy: importable without a GPU).

``guarded(view_shape, strides, fill)`` allocates ONE flat float32 tensor holding a front guard, the operand's whole
strided extent and a back guard, and describes the operand as a strided view into it:

* an input operand (``fill`` a float, NaN by default in the callers): guards and gap words - the words of the extent
  the view does not address - hold ``fill``, the body holds ``values``. A kernel that reads outside its operand and
  masks the product with a zero weight turns the NaN into a NaN result; ``3e38`` (beyond fp16) instead makes an f16x3
  kernel raise its overflow flag or produce ``inf * 0``.
* an output operand (``fill=SENTINEL``, an int32 bit pattern): guards and gaps hold the sentinel, the body holds NaN
  (or ``values``: the base of an accumulating / in-place launch). After the launch ``check()`` asserts on the int32
  view that every guard and gap word still holds the sentinel - an overshooting store, into the neighbouring tensor in
  the forward, is reported with its offset - and returns the body as a dense tensor, where an element the kernel never
  wrote is still NaN and fails any comparison.

Each guard is at least GUARD_ROWS rows of the operand's row stride, rounded up to a multiple of 128 floats, so a whole
overshooting tile still lands inside the allocation (never a fault) and the body keeps the 512-byte alignment torch
gives the allocation.
"""
import numpy as np
import torch

SENTINEL = 0x5EA7C0DE  # as fp32: 6.04e18, finite, and no value a kernel computes from the tests' inputs
GUARD_ROWS = 256
POISON = 3.0e38        # finite in fp32 and bf16, infinite in fp16


def _bits(fill):
    """The int32 bit pattern of ``fill`` (an int is taken as the pattern itself)."""
    if isinstance(fill, (int, np.integer)):
        return np.array([fill], np.uint32).view(np.int32)[0]
    return np.array([fill], np.float32).view(np.int32)[0]


def _strided(a, shape, strides):
    """numpy view of the flat array ``a`` with element strides."""
    return np.lib.stride_tricks.as_strided(a, shape, tuple(s * a.itemsize for s in strides))


class Guarded:
    def __init__(self, shape, strides, fill, values=None, device="cpu"):
        shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        assert len(shape) == len(strides) and all(s >= 1 for s in shape) and all(s >= 0 for s in strides)
        self.shape, self.strides = shape, strides
        self.extent = sum((n - 1) * s for n, s in zip(shape, strides)) + 1
        rows = [s for s in strides[:-1] if s > 0]
        self.row_stride = min(rows) if rows else shape[-1]
        self.guard = -(-GUARD_ROWS * self.row_stride // 128) * 128
        self.offset = self.guard
        self.total = self.guard + -(-self.extent // 128) * 128 + self.guard
        words = np.full(self.total, _bits(fill), np.int32)
        mask = np.zeros(self.total, bool)
        _strided(mask[self.offset:], shape, strides)[...] = True
        # the body: dims the view repeats (stride 0) hold one copy
        own = tuple(1 if s == 0 else n for n, s in zip(shape, strides))
        if values is None:
            body = np.full(own, np.nan, np.float32)
        else:
            body = np.ascontiguousarray(torch.as_tensor(values).detach().cpu().numpy(), np.float32)
            assert body.shape == own, f"values {body.shape} for a view holding {own}"
        _strided(words[self.offset:].view(np.float32), own, strides)[...] = body
        assert int(mask.sum()) == int(np.prod(own)), "the view overlaps itself"
        self.t = torch.from_numpy(words.view(np.float32)).to(device)
        self.mask = torch.from_numpy(mask).to(device)
        self.expect = self.t.view(torch.int32).clone()  # what every word outside the body must still hold
        self.guard_words = int(self.total - mask.sum())

    # --- the operand as the kernel sees it
    def ptr(self):
        return self.t.data_ptr() + 4 * self.offset

    def view(self):
        return torch.as_strided(self.t, self.shape, self.strides, self.offset)

    def refill(self, fill):
        """Every guard and gap word := fill (the body stays)."""
        ti = self.t.view(torch.int32)
        ti[~self.mask] = int(_bits(fill))
        self.expect = ti.clone()
        return self

    def window(self, shape, strides, start=0):
        """Another operand inside this allocation, its first element ``start`` floats after this one's: the same
        memory under a second declaration (a row the first launch skips, a narrower view, ...). Everything outside
        the new view must keep what it holds now, this operand's finished body included."""
        w = object.__new__(Guarded)
        w.shape, w.strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        w.row_stride, w.guard, w.total = self.row_stride, self.guard, self.total
        w.offset = self.offset + int(start)
        w.extent = sum((n - 1) * s for n, s in zip(w.shape, w.strides)) + 1
        assert start >= 0 and w.offset + w.extent <= self.total - self.guard, "the window leaves the operand's extent"
        mask = np.zeros(self.total, bool)
        _strided(mask[w.offset:], w.shape, w.strides)[...] = True
        w.t, w.mask = self.t, torch.from_numpy(mask).to(self.t.device)
        w.expect = self.t.view(torch.int32).clone()
        w.guard_words = int(self.total - mask.sum())
        return w

    # --- after the launch
    def dirty(self):
        """Offsets (floats, relative to the operand's first element) of words outside the body that changed."""
        bad = (self.t.view(torch.int32) != self.expect) & ~self.mask
        return (torch.nonzero(bad).flatten() - self.offset).cpu().tolist()

    def check(self):
        """Every guard and gap word still holds the fill; returns the body as a dense tensor (a clone)."""
        bad = self.dirty()
        assert not bad, (f"{len(bad)} guard / gap word(s) of the {self.shape} x {self.strides} operand overwritten, "
                         f"first at offsets {bad[:8]} from its start (row stride {self.row_stride})")
        return self.view().clone().contiguous()


def guarded(view_shape, strides, fill, values=None, device="cpu"):
    return Guarded(view_shape, strides, fill, values, device)


def dense_strides(shape):
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= n
    return tuple(reversed(st))
