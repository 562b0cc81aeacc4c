"""Byte layouts of typed sections in one flat buffer, and the one argument check in front of every raw
device pointer.  Pure host code: torch is imported lazily, torch.cuda is never touched, CPU tensors work."""
import math

import numpy as np

_NP_DTYPES = None


def np_dtype(dtype) -> np.dtype:
    """the numpy dtype of a torch dtype (the one table: the dtypes that cross to the host as numpy views)"""
    global _NP_DTYPES
    if _NP_DTYPES is None:
        import torch
        _NP_DTYPES = {getattr(torch, k): np.dtype(k) for k in ("float32", "float64", "uint8", "int32", "int16", "uint16")}
    return _NP_DTYPES[dtype]


class Layout:
    """Sections ``(name, shape, torch dtype)`` laid out in the listed order in one uint8 buffer, each starting on an
    ``align``-byte boundary.  ``sections[name] = (offset, nbytes, shape, dtype)``; ``nbytes`` is the aligned total."""

    def __init__(self, sections, align: int = 256):
        self.align, self.sections, self.nbytes = align, {}, 0
        for name, shape, dtype in sections:
            n = math.prod(shape) * dtype.itemsize
            self.sections[name] = (self.nbytes, n, tuple(shape), dtype)
            self.nbytes += -(-n // align) * align

    def end(self, name) -> int:
        """the aligned end offset of section ``name``: the size of the prefix of the buffer that ends with it"""
        off, n = self.sections[name][:2]
        return off + -(-n // self.align) * self.align

    def torch_views(self, flat) -> dict:
        """typed views ``[..., *shape]`` of a uint8 tensor ``[..., nbytes]``, by name"""
        return {k: flat[..., off:off + n].view(dtype).unflatten(-1, shape) for k, (off, n, shape, dtype) in self.sections.items()}

    def numpy_views(self, host) -> dict:
        """typed views of a host uint8 array ``[nbytes]``, by name"""
        return {k: host[off:off + n].view(np_dtype(dtype)).reshape(shape) for k, (off, n, shape, dtype) in self.sections.items()}


class AtLeast(int):
    """``check_tensor(lead=AtLeast(n))``: the first dimension may exceed n (a plain int is exact)"""


def check_tensor(what, name, x, dtype, shape, *, device, lead=None, align=None) -> None:
    """``x`` is a contiguous ``dtype`` (one, or a tuple of allowed ones) tensor on ``device`` that starts on an ``align``-byte
    boundary (default: its element size).  Its shape is ``shape``; with ``lead``, ``shape`` is the trailing shape and the first
    dimension is exactly ``lead`` (an int) or at least ``lead`` (``AtLeast``).  ValueError otherwise: the callers hand
    ``x.data_ptr()`` to a kernel, so this is the only thing between a wrong argument and a GPU fault."""
    full = tuple(shape) if lead is None else (lead,) + tuple(shape)
    want = tuple(f">={int(n)}" if isinstance(n, AtLeast) else n for n in full)
    if x is None:
        raise ValueError(f"{what}: `{name}` is required ({dtype} {want} on {device})")
    if x.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)) or x.device != device or not x.is_contiguous():
        raise ValueError(f"{what}: `{name}` must be a contiguous {dtype} tensor on {device}")
    if x.dim() != len(full) or not all(a >= n if isinstance(n, AtLeast) else a == n for a, n in zip(x.shape, full)):
        raise ValueError(f"{what}: `{name}` has shape {tuple(x.shape)}, expected {want}")
    align = align or x.element_size()
    if x.data_ptr() % align:
        raise ValueError(f"{what}: `{name}` must start on a {align}-byte boundary (a view at an odd offset?)")
