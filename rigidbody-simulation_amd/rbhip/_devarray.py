"""Arguments of the device-resident boundaries (BatchWorld.*_device,
World.*_device): any object with __cuda_array_interface__ — C-contiguous, of
exactly the expected shape, float64 or float32, one element type per call.
Everything else is refused here, naming the argument, before the library is
reached."""
from __future__ import annotations

import ctypes as C

from . import _lib

_IO_CODES = {"<f8": _lib.RB_F64, "<f4": _lib.RB_F32}
_IO_NAMES = {"f64": "<f8", "f32": "<f4", "float64": "<f8", "float32": "<f4",
             "torch.float64": "<f8", "torch.float32": "<f4"}


def _device_array(name, a, shape, typestrs, out=False):
    """The device pointer and typestr of argument `name`, an object with
    __cuda_array_interface__: C-contiguous (strides None), of exactly `shape`,
    its typestr one of `typestrs`, writable if `out`.  ValueError / TypeError
    naming the argument otherwise (a numpy array or a CPU tensor included)."""
    try:
        cai = a.__cuda_array_interface__
    except Exception as exc:        # (torch raises TypeError from the attribute of a CPU tensor)
        raise TypeError(f"{name}: expected device memory (an object with __cuda_array_interface__, such as a "
                        f"torch tensor on the batch's GPU), got {type(a).__name__}") from exc
    if tuple(cai["shape"]) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(cai['shape'])}, expected {tuple(shape)}")
    if cai["typestr"] not in typestrs:
        raise TypeError(f"{name}: typestr {cai['typestr']!r}, expected one of {', '.join(typestrs)}")
    if cai.get("strides") is not None:
        raise ValueError(f"{name}: not C-contiguous (strides {cai['strides']})")
    ptr, readonly = cai["data"]
    if out and readonly:
        raise ValueError(f"{name}: read-only memory given for an output")
    return (C.c_void_p(ptr) if ptr else None), cai["typestr"]


def _io_typestr(name, dtype):
    ts = _IO_NAMES.get(str(dtype))
    if ts is None:
        raise ValueError(f"{name}: {dtype!r} is not 'f64' or 'f32'")
    return ts


def _pair_typestr(own, names, arrays, dtype):
    """The one typestr of the given arrays (and dtype, if given); that of `own`
    (the batch's or world's dtype) if none."""
    ts = None if dtype is None else _io_typestr("dtype", dtype)
    for name, a in zip(names, arrays):
        if a is None:
            continue
        try:
            t = a.__cuda_array_interface__["typestr"]
        except Exception:       # (not device memory: _device_array says so, naming the argument)
            t = None
        if t in _IO_CODES and ts is not None and t != ts:
            raise TypeError(f"{name}: typestr {t!r}, expected {ts!r} (one element type per call)")
        if t in _IO_CODES and ts is None:
            ts = t
    return ts or _IO_NAMES[own]


def _new_tensor(shape, typestr, device):
    import torch        # lazily: the package does not need torch until an output is omitted
    dt = {"<f8": torch.float64, "<f4": torch.float32, "<i4": torch.int32, "<i8": torch.int64}[typestr]
    return torch.empty(shape, dtype=dt, device=f"cuda:{device}")
