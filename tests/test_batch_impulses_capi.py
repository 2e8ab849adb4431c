"""The impulse query of a batch (rb_batch_impulses, rb_batch_impulses_dev;
BatchWorld.impulses / impulses_device; kernels in rb_batch_impulses.hip): the
entry points are exported, bound and declared as the header declares them, a
null handle is refused before any device call, the Python argument checks
refuse what is not the device array they expect without reaching the library,
and the new kernels are built in sixteen instances (both real types, spheres
and boxes, the one-wave mapping and three wide blocks) without scratch, the
box ones at one wave per SIMD, the sphere ones at more (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

FUNCS = ["rb_batch_impulses", "rb_batch_impulses_dev"]
EINVAL = -22
# the names the resource pins of the other kernels parse `make resource-usage` by
PINNED_NAMES = ("batch_step_kernel", "batch_balls_kernel", "batch_mixed_kernel", "box_kernel", "batch_wide_kernel",
                "wide_contacts_kernel", "batch_contacts_kernel", "batch_contacts_boxes_kernel", "ragged_step_kernel",
                "ragged_wide_kernel", "ragged_contacts_kernel", "ragged_wide_contacts_kernel")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_entry_points_are_exported_bound_and_declared(lib):
    from rbhip import _lib
    import rbhip
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in FUNCS if f not in exported]
    assert not [f for f in FUNCS if f not in _lib.SIGNATURES]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    assert callable(rbhip.BatchWorld.impulses) and callable(rbhip.BatchWorld.impulses_device)
    assert [f for f in rbhip.BatchImpulses.__dataclass_fields__] == ["counts", "partner", "kind", "dist", "jn", "jt", "vel",
                                                                     "net", "truncated"]
    header = open(os.path.join(ROOT, "include", "rbhip.h")).read()
    host = re.search(r"\bint\s+rb_batch_impulses\s*\(rb_batch \*b, const int64_t \*env_ids, int64_t n, int32_t max_records,"
                     r"\s*double dt, double restitution, double friction, double contact_threshold,"
                     r"\s*int32_t \*counts, int32_t \*partner, int32_t \*kind, double \*dist,"
                     r"\s*double \*jn, double \*jt, double \*vel, double \*net, int64_t \*n_truncated\);", header)
    dev = re.search(r"\bint\s+rb_batch_impulses_dev\s*\(rb_batch \*b, int32_t max_records,"
                    r"\s*double dt, double restitution, double friction, double contact_threshold,"
                    r"\s*int32_t \*counts, int32_t \*partner, int32_t \*kind, void \*dist,"
                    r"\s*void \*jn, void \*jt, void \*vel, void \*net, int32_t io_dtype\);", header)
    assert host and dev
    # the ctypes signatures carry the header's argument kinds, in its order
    kinds = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, m in (("rb_batch_impulses", host), ("rb_batch_impulses_dev", dev)):
        args = [a.strip() for a in m.group(0)[m.group(0).index("(") + 1:m.group(0).rindex(")")].split(",")]
        want = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in args]
        res, got = _lib.SIGNATURES[name]
        got = [C.c_void_p if (g is not C.c_void_p and hasattr(g, "contents")) else g for g in got]
        assert res is C.c_int and got == want, name
    for word in ("collision.py:7-48", ":72-88", "physics_utils.py:25-49", "RB_NORMAL_ORIENTED", "sensor only",
                 "Not covered: the same query for an rb_world"):
        assert word in header, word


def test_null_handle_is_einval_before_any_device_call(lib):
    a = np.zeros(64, np.int32)
    d = np.zeros(64)
    p, q = a.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
    nt = C.c_int64(7)
    # (every other argument is one the call would also refuse, or accept: the handle is checked first)
    for args in ((None, None, 1, 4, 0.01, 0.5, 0.5, 0.0, p, p, p, q, q, q, q, q, C.byref(nt)),
                 (None, None, -1, -1, float("nan"), -1.0, -1.0, -1.0, None, None, None, None, None, None, None, None, None)):
        assert lib.rb_batch_impulses(*args) == EINVAL
        assert b"null batch" in lib.rb_last_error()
    for args in ((None, 4, 0.01, 0.5, 0.5, 0.0, p, p, p, q, q, q, q, q, 0),
                 (None, -1, 0.0, 0.0, 0.0, 0.0, None, None, None, None, None, None, None, None, 5)):
        assert lib.rb_batch_impulses_dev(*args) == EINVAL
        assert b"null batch" in lib.rb_last_error()
    assert nt.value == 7 and not a.any() and not d.any()


class _Fake:
    """An object with a __cuda_array_interface__ and nothing behind it."""

    def __init__(self, shape, typestr="<f8", strides=None, readonly=False):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x10000, readonly),
                                             strides=strides, version=3)


E, M, R = 5, 4, 6


@pytest.fixture()
def stand_in():
    """A BatchWorld that was never constructed: no handle and no library (an
    access to either is an AttributeError, which no check below expects)."""
    import rbhip
    from rbhip import scenes
    b = object.__new__(rbhip.BatchWorld)
    b.scene, b.dtype, b.device = scenes.multi_sphere4(), "f64", 0
    b.n_envs, b.n_bodies = E, M
    return b


SHAPES = {"counts": (E, M), "partner": (E, M, R), "kind": (E, M, R), "dist": (E, M, R), "jn": (E, M, R),
          "jt": (E, M, R, 3), "vel": (E, M, 6), "net": (E, M, 6)}
INTS = ("counts", "partner", "kind")


def _out(**repl):
    out = {k: _Fake(s, "<i4" if k in INTS else "<f8") for k, s in SHAPES.items()}
    out.update(repl)
    return out


def test_python_checks_refuse_host_arrays_wrong_shapes_and_types(stand_in):
    b = stand_in
    for name, shape in SHAPES.items():
        host = np.zeros(shape, np.int32 if name in INTS else np.float64)
        with pytest.raises(TypeError, match=name):
            b.impulses_device(out=_out(**{name: host}))
        ts = "<i4" if name in INTS else "<f8"
        if name != "partner":                                # (partner's last axis is the slot count)
            with pytest.raises(ValueError, match=name):
                b.impulses_device(out=_out(**{name: _Fake(shape[:-1] + (shape[-1] + 1,), ts)}))
        with pytest.raises(TypeError, match=name):
            b.impulses_device(out=_out(**{name: _Fake(shape, "<f2")}))
        with pytest.raises(ValueError, match=name):
            b.impulses_device(out=_out(**{name: _Fake(shape, ts, readonly=True)}))
    with pytest.raises(ValueError, match="partner"):
        b.impulses_device(max_records=R + 1, out=_out())
    with pytest.raises(TypeError, match="one element type per call"):
        b.impulses_device(out=_out(net=_Fake(SHAPES["net"], "<f4")))
    with pytest.raises(ValueError, match="dtype"):
        b.impulses_device(out=_out(), dtype="f16")
    with pytest.raises(ValueError, match="counts"):
        b.impulses_device(out=_out(counts=None))
    with pytest.raises(ValueError, match="all five"):
        b.impulses_device(out=_out(jn=None))
    with pytest.raises(ValueError, match="max_records"):
        b.impulses_device(max_records=-1)


def test_impulse_kernels_are_listed_without_scratch():
    """batch_impulses_kernel<T, BOXES> and batch_impulses_wide_kernel<T, BOXES,
    BLOCK> for T = double / float, BOXES = 0 / 1, BLOCK = 128 / 192 / 256:
    sixteen instances, none with scratch; the box ones at one wave per SIMD by
    design (the box narrowphase), the sphere ones at two or more: they do not
    pay for it; none under a name another kernel's resource pins parse by."""
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for m in re.finditer(r"Function Name: (\S*?\d+batch_impulses(_wide)?_kernelI([df])Lb([01])E(?:Li(\d+)E)?E\S*)\s+(?:.*\n)*?"
                         r".*ScratchSize \[bytes/lane\]: (\d+)(?:.*\n)*?.*Occupancy \[waves/SIMD\]: (\d+)(?:.*\n)*?"
                         r".*LDS Size \[bytes/block\]: (\d+)", out):
        key = (m.group(3), int(m.group(4)), int(m.group(5) or 64))
        assert key not in got and bool(m.group(2)) == (key[2] != 64)
        got[key] = (m.group(1), int(m.group(6)), int(m.group(7)), int(m.group(8)))
    assert sorted(got) == sorted((t, bx, blk) for t in "df" for bx in (0, 1) for blk in (64, 128, 192, 256)), sorted(got)
    for (t, boxes, block), (name, scratch, waves, lds) in got.items():
        assert scratch == 0, name
        assert not [p for p in PINNED_NAMES if re.search(rf"\d+{p}I", name)], name
        real = 8 if t == "d" else 4
        if boxes:
            assert waves == 1, name
            # snapshot, quaternion, extents, kind, and the polygon column of 48 reals per lane
            assert lds == block * (4 * real + 4 * real + 3 * real + 4 + 48 * real), name
        else:
            assert waves >= 2, name
            assert lds == block * 4 * real, name                 # the snapshots alone
