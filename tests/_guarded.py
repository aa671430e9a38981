"""Guarded, poisoned buffers for the row-edge tests (plain torch, any device).

A kernel that walks a [rows, width] problem in fixed row blocks can go wrong at its last, ragged block in two ways that a
comparison of values does not see: it can leave elements of an output unwritten (the test then reads whatever the caching
allocator left there, often the right numbers of an earlier launch), and it can store past the end (into whatever the
allocator placed next).  `guarded` makes both visible:

    front guard | payload | back guard          one flat allocation; `.t` is the payload viewed in `shape`

  * the guards hold a fixed bit pattern (for fp32 a quiet NaN with a payload) and are compared bit for bit after the
    launch: each is at least 64 rows of `row_width` elements (the widest workgroup of the library covers 16 * 4 = 64 rows)
    and at least 1,024 elements, rounded so that the payload starts on a 16-byte boundary (the kernels use 16-byte accesses);
  * the payload starts as
      "poison"  the NaN attn_launch.allocator fills with: for outputs the header calls fully written -- none may be left;
      "zero"    for outputs the header has the caller zero-initialise and the kernel accumulate into;
      "scratch" for workspaces (contents irrelevant): guards only;
      a tensor  for inputs: the back guard then is what a read past the last row finds -- NaN for fp32, an id outside
                every table for int64 -- and `check` also holds the payload to its initial bits (inputs are never written).
"""
from __future__ import annotations

from typing import Optional

import torch

# payload poison: the bits of float("nan"), i.e. of torch.full(..., float("nan")) in attn_launch.allocator
_POISON = {torch.float32: 0x7FC00000, torch.uint8: 0xA5, torch.int64: -0x0123456789ABCDF0}
# guard pattern: not the poison, unlikely as data.  fp32: a quiet NaN with payload 0x25A5A5; uint8: neither 0 nor 1 (the
# only bytes the library writes); int64: 0x5A5A5A5A5A5A5A5A, an id far outside every table.
_GUARD = {torch.float32: 0x7FE5A5A5, torch.uint8: 0x5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
_BITS = {torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64}
MIN_GUARD_ROWS = 64
MIN_GUARD_ELEMS = 1024
ALIGN = 16


def guard_elems(row_width: int, dtype: torch.dtype) -> int:
    """Elements of one guard: >= 64 rows, >= 1024 elements, a whole number of 16-byte units."""
    unit = ALIGN // torch.empty(0, dtype=dtype).element_size()
    n = max(MIN_GUARD_ROWS * int(row_width), MIN_GUARD_ELEMS)
    return (n + unit - 1) // unit * unit


class Guarded:
    """One guarded buffer; `.t` is the tensor to hand to the kernel."""

    def __init__(self, shape, dtype, device, row_width, fill):
        if dtype not in _BITS:
            raise TypeError(f"guarded: no guard pattern for {dtype}")
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        self.dtype, self.numel, self.guard = dtype, n, guard_elems(row_width, dtype)
        esz = torch.empty(0, dtype=dtype).element_size()
        unit = ALIGN // esz
        # `unit` elements of slack: the payload is moved to a 16-byte boundary whatever the allocator's base address is
        self.flat = torch.empty(self.guard + n + self.guard + unit, dtype=dtype, device=device)
        self.bits = self.flat.view(_BITS[dtype])
        self.bits.fill_(_GUARD[dtype])
        self.start = self.guard + (-(self.flat.data_ptr() // esz + self.guard)) % unit
        self.t = self.flat[self.start:self.start + n].view(shape)
        assert self.t.data_ptr() % ALIGN == 0
        if isinstance(fill, torch.Tensor):
            assert fill.dtype == dtype and tuple(fill.shape) == shape, (fill.dtype, tuple(fill.shape), dtype, shape)
            self.fill = "input"
            self.t.copy_(fill)
            self.initial = self.t.clone().view(_BITS[dtype]).reshape(-1)
        elif fill == "poison":
            self.fill = fill
            self.bits[self.start:self.start + n] = _POISON[dtype]
        elif fill in ("zero", "scratch"):
            self.fill = fill
            self.t.zero_()
        else:
            raise ValueError(f"guarded: fill must be 'poison', 'zero', 'scratch' or a tensor, not {fill!r}")

    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.t.data_ptr())

    def _first(self, bad: torch.Tensor) -> int:
        return int(torch.nonzero(bad.reshape(-1))[0, 0])

    def check(self, name: str, unwritten: Optional[torch.Tensor] = None) -> None:
        """Both guards bit-identical to their pattern (first offending offset reported relative to the payload: negative
        = in front of it, >= numel = behind it); "poison": no element left as poison or any other NaN, except where
        `unwritten` (bool, shape of the payload) is set; inputs: every bit as it was."""
        pat = _GUARD[self.dtype]
        front, back = self.bits[:self.start], self.bits[self.start + self.numel:]
        bad = front != pat
        if bool(bad.any()):
            # the store closest to the payload is the informative one
            off = int(torch.nonzero(bad)[-1, 0]) - self.start
            raise AssertionError(f"{name}: front guard overwritten at payload offset {off} ({int(bad.sum())} elements touched)")
        bad = back != pat
        if bool(bad.any()):
            off = self.numel + self._first(bad)
            raise AssertionError(f"{name}: back guard overwritten at payload offset {off} ({int(bad.sum())} elements touched)")
        payload = self.bits[self.start:self.start + self.numel]
        if unwritten is not None:
            assert self.fill == "poison", f"{name}: unwritten= only applies to poisoned outputs"
            assert unwritten.dtype == torch.bool and tuple(unwritten.shape) == tuple(self.t.shape), name
            unwritten = unwritten.reshape(-1).to(payload.device)
            # the single exemption there is; it is for a few elements, never for a tensor
            assert self.numel > 0 and int(unwritten.sum()) < self.numel, f"{name}: unwritten= may not cover the whole tensor"
        if self.fill == "poison":
            left = payload == _POISON[self.dtype]
            if self.dtype == torch.float32:
                left = left | torch.isnan(self.t.reshape(-1))
            if unwritten is not None:
                left = left & ~unwritten
            if bool(left.any()):
                off = self._first(left)
                what = "poison left (element never written)" if int(payload[off]) == _POISON[self.dtype] else \
                    "NaN (a read past the end of an input, or a wrong value)"
                raise AssertionError(f"{name}: {what} at payload offset {off} = index "
                                     f"{_unravel(off, self.t.shape)} ({int(left.sum())} of {self.numel} elements)")
        elif self.fill == "input":
            bad = payload != self.initial
            if bool(bad.any()):
                raise AssertionError(f"{name}: input overwritten at payload offset {self._first(bad)}")
        elif self.fill == "zero" and self.dtype == torch.float32:  # accumulated into; a NaN there came from a read past an input's end
            bad = torch.isnan(self.t.reshape(-1))
            if bool(bad.any()):
                off = self._first(bad)
                raise AssertionError(f"{name}: NaN at payload offset {off} = index {_unravel(off, self.t.shape)}")


def _unravel(off: int, shape) -> tuple:
    idx = []
    for s in reversed(tuple(shape)):
        idx.append(off % s)
        off //= s
    return tuple(reversed(idx))


def guarded(shape, dtype, device, row_width, fill) -> Guarded:
    """A buffer of `shape` between two guards of >= 64 rows of `row_width` elements; see the module docstring."""
    return Guarded(shape, dtype, device, row_width, fill)


def check_all(bufs: dict, unwritten: Optional[dict] = None) -> None:
    """check() of every buffer of a launch, by name."""
    for name, g in bufs.items():
        if g is not None:
            g.check(name, None if unwritten is None else unwritten.get(name))
