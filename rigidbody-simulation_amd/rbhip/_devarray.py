"""Arguments of the device-resident boundaries (BatchWorld.*_device,
World.*_device): any object with __cuda_array_interface__ — C-contiguous, of
exactly the expected shape, float64 or float32, one element type per call.
Everything else is refused here, naming the argument, before the library is
reached."""
from __future__ import annotations

import ctypes as C

import numpy as np

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


# The arrays of a contact query: (name, record, tail, real).  A record has R
# slots per body; tail: its trailing dimensions; real: of the call's real type,
# else int32.  The table's order is the C entry points' argument order: the
# callers pass `*ptrs.values()`, so a new field goes where the C-ABI has it.
_CONTACT_FIELDS = (("counts", False, (), False), ("partner", True, (), False), ("kind", True, (), False),
                   ("dist", True, (), True), ("pos", True, (3,), True), ("frame", True, (3,), True))
# the arrays of an impulse query (rb_batch_impulses, rb_query_impulses)
_IMPULSE_FIELDS = _CONTACT_FIELDS[:4] + (("jn", True, (), True), ("jt", True, (3,), True),
                                         ("vel", False, (6,), True), ("net", False, (6,), True))


def _field_shape(field, lead, R):
    """A query array's shape: `lead`, R slots per body if a record, its own tail."""
    _, record, tail, _ = field
    return tuple(lead) + ((R,) if record else ()) + tuple(tail)


def _host_arrays(fields, lead, R, skip=()):
    """A host-form query's dense arrays by field name: zeros, float64 or int32; None
    for a record with R <= 0 (a negative R is the library's to refuse) and for `skip`."""
    return {f[0]: None if f[0] in skip or (f[1] and R <= 0) else
            np.zeros(_field_shape(f, lead, R), np.float64 if f[3] else np.int32) for f in fields}


def _resolve_out(fields, lead, required, required_msg, out, max_records, dtype, own, device, default_R,
                 skip=(), exclusive=False):
    """The arrays of a device-form query: (R, typestr, given, ptrs), `given` the
    arrays by field name and `ptrs` their device pointers or None.  fields:
    (name, record, tail, real) in the entry point's order, "counts" first, each
    of _field_shape(field, lead, R), int32 or (real) of the call's one real
    type.  out None: new torch tensors, the records only with R = default_R()
    > 0, those of `skip` never.  Else an object or mapping with the fields'
    names: R is its partner's last dimension (none: 0), and max_records, if
    given, must agree.  The fields of `required` must all be there with R > 0
    (exclusive: and none with R == 0), else ValueError(required_msg).  own,
    device: the owner's dtype and device."""
    names = [f[0] for f in fields]
    if out is not None:
        given = {k: (out.get(k) if hasattr(out, "get") else getattr(out, k, None)) for k in names}
        if given["counts"] is None:
            raise ValueError("out: counts is required")
        if given["partner"] is None:
            R = 0
        else:
            try:
                R = int(given["partner"].__cuda_array_interface__["shape"][-1])
            except Exception as exc:
                raise TypeError("partner: expected device memory (an object with __cuda_array_interface__), "
                                f"got {type(given['partner']).__name__}") from exc
        if max_records is not None and int(max_records) != R:
            raise ValueError(f"partner: {R} slots per body, max_records is {int(max_records)}")
    else:
        given = dict.fromkeys(names)
        R = default_R()
    if R < 0:
        raise ValueError("max_records < 0")
    reals = [f[0] for f in fields if f[3]]
    ts = _pair_typestr(own, reals, [given[k] for k in reals], dtype)
    typestr = {f[0]: ts if f[3] else "<i4" for f in fields}
    if out is None:
        for f in fields:
            if f[0] not in skip and (R > 0 or not f[1]):
                given[f[0]] = _new_tensor(_field_shape(f, lead, R), typestr[f[0]], device)
    ptrs = {f[0]: None if given[f[0]] is None else
            _device_array(f[0], given[f[0]], _field_shape(f, lead, R), (typestr[f[0]],), out=True)[0] for f in fields}
    have = [ptrs[k] is not None for k in required]
    if (R > 0 and not all(have)) or (exclusive and R == 0 and any(have)):
        raise ValueError(required_msg)
    return R, ts, given, ptrs


def _new_tensor(shape, typestr, device):
    import torch        # lazily: the package does not need torch until an output is omitted
    dt = {"<f8": torch.float64, "<f4": torch.float32, "<i4": torch.int32, "<i8": torch.int64}[typestr]
    return torch.empty(shape, dtype=dt, device=f"cuda:{device}")
