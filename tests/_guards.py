"""Red zones for kernel tests (a plain helper module, no pytest hooks).

Every operand of a kernel under test sits between two guard bands poisoned with a sentinel: NaN around inputs (a value read past either end
that reaches an accumulator makes the result NaN or different), a finite sentinel around outputs and scratch (a store outside the tensor
changes it).  The bands live inside the same allocation as the tensor, so an overrun of up to GUARD elements is caught by a comparison and
never leaves allocated memory.  Works on CPU and device tensors alike (tests/test_guards_cpu.py checks the helpers themselves)."""
import torch

GUARD = 4096        # elements on either side (16 KiB of floats: more than any tile's halo)


def _guarded(t: torch.Tensor, fill: float):
    """(buffer, view): a copy of `t` between two GUARD-wide bands of `fill`; the view has t's shape and aliases the buffer"""
    flat = t.contiguous().flatten()
    buf = torch.full((GUARD + flat.numel() + GUARD,), fill, device=t.device, dtype=t.dtype)
    buf[GUARD:GUARD + flat.numel()] = flat
    return buf, buf[GUARD:GUARD + flat.numel()].view(t.shape)


def _guards_intact(buf: torch.Tensor, fill: float) -> bool:
    lo, hi = buf[:GUARD], buf[-GUARD:]
    if fill != fill:
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == fill).all() and (hi == fill).all())


def scratch_sentinel(dtype) -> float:
    """the value of the bands around a `scratch` view: -7.0 for floating-point workspaces, the byte 0x5A for integer (byte) ones"""
    return -7.0 if dtype.is_floating_point else 0x5A


def scratch(nelem: int, dtype=torch.float32, fill: float = 0.0, device="cuda"):
    """(buffer, view) for a caller-allocated workspace: the view has EXACTLY `nelem` elements of `dtype` (the figure a size function returned,
    nothing added), starts on a 16-byte boundary and is filled with `fill` (NaN or 0: what a previous user of the memory may have left);
    GUARD elements of `scratch_sentinel(dtype)` lie directly before and directly after it: `_guards_intact(buffer, scratch_sentinel(dtype))`
    checks them.  For a byte workspace pass dtype=torch.uint8 and fill 0xFF (four such bytes are a NaN) or 0."""
    nelem = int(nelem)
    assert nelem >= 0
    buf = torch.full((GUARD + nelem + GUARD,), scratch_sentinel(dtype), device=device, dtype=dtype)
    # a fresh allocation starts on (at least) a 16-byte boundary and GUARD * itemsize is a multiple of 16, so the view does as well
    view = buf[GUARD:GUARD + nelem]
    assert nelem == 0 or view.data_ptr() % 16 == 0, "allocator returned a buffer that is not 16-byte aligned"
    view.fill_(fill)
    return buf, view
