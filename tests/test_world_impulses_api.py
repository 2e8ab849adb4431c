"""The impulse query of a world (rb_query_impulses, rb_query_impulses_dev;
World.query_impulses, query_impulses_device, WorldImpulses): the entry points
are exported with the header's argument lists, the binding's argtypes match
them, a null handle is refused before any device call, WorldImpulses carries
the shapes of one row of BatchImpulses and `truncated` on hand-made arrays, and
the new kernels compile without scratch (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_world_contacts_api import CTYPES, _header_params

FUNCS = ["rb_query_impulses", "rb_query_impulses_dev"]
KERNELS = {"world_impulses_kernel", "world_impulses_boxes_kernel"}
EINVAL = -22
FIELDS = ("counts", "partner", "kind", "dist", "jn", "jt", "vel", "net")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_entry_points_are_exported_with_the_headers_argument_lists(lib):
    from rbhip import _lib
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in FUNCS if f not in exported]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    head = ["rb_world *", "int64_t", "int64_t", "int32_t", "double", "double", "double", "double",
            "int32_t *", "int32_t *", "int32_t *"]
    want = {"rb_query_impulses": head + ["double *"] * 5 + ["int64_t *"],
            "rb_query_impulses_dev": head + ["void *"] * 5 + ["int32_t"]}
    ctypes_of = dict(CTYPES, double=C.c_double)
    for f in FUNCS:
        params = _header_params(f)
        assert params == want[f], (f, params)
        res, args = _lib.SIGNATURES[f]
        assert res is C.c_int and args == [ctypes_of[t] for t in params], f
        assert getattr(lib, f).argtypes == args
    # the batch's query for one environment: the same arrays in the same order after the step parameters
    assert _header_params("rb_query_impulses")[4:] == _header_params("rb_batch_impulses")[4:]
    assert _header_params("rb_query_impulses_dev")[4:] == _header_params("rb_batch_impulses_dev")[2:]


def test_null_world_and_python_surface(lib):
    import rbhip
    a = np.zeros(64, np.int32)
    p = a.ctypes.data_as(C.c_void_p)
    none5 = (None,) * 5
    assert lib.rb_query_impulses(None, 0, 1, 0, 0.01, 0.5, 0.5, 0.0, p, *none5, None, None, None) == EINVAL
    assert b"null world" in lib.rb_last_error()
    assert lib.rb_query_impulses_dev(None, 0, 1, 0, 0.01, 0.5, 0.5, 0.0, p, *none5, None, None, 0) == EINVAL
    assert b"null world" in lib.rb_last_error()
    for m in ("query_impulses", "query_impulses_device"):
        assert callable(getattr(rbhip.World, m)), m
    assert rbhip.WorldImpulses is rbhip.world.WorldImpulses
    # the fields of BatchImpulses, in its order
    wi = rbhip.WorldImpulses(*range(9))
    bi = rbhip.BatchImpulses(*range(9))
    for f in FIELDS + ("truncated",):
        assert getattr(wi, f) == getattr(bi, f), f
    assert wi.first == 0 and rbhip.WorldImpulses(*range(9), first=7).first == 7


def test_world_impulses_shapes_and_truncated_on_hand_made_arrays():
    import rbhip
    from rbhip import _devarray
    counts = [0, 2, 5, -2, 3, 1, -2, 4]                    # 5 and 4 exceed R = 3; two bodies have no list
    n, R = len(counts), 3
    a = _devarray._host_arrays(_devarray._IMPULSE_FIELDS, (1, n), R)
    assert tuple(a) == FIELDS
    a["counts"][0] = counts
    imp = rbhip.WorldImpulses(*a.values(), int((a["counts"] > R).sum()), first=11)
    assert imp.max_records == R and imp.truncated == 2 and imp.first == 11
    assert imp.counts.shape == (1, n) and imp.counts.dtype == np.int32
    for f in ("partner", "kind", "dist", "jn"):
        assert getattr(imp, f).shape == (1, n, R), f
    assert imp.partner.dtype == imp.kind.dtype == np.int32 and imp.jn.dtype == imp.dist.dtype == np.float64
    assert imp.jt.shape == (1, n, R, 3) and imp.vel.shape == imp.net.shape == (1, n, 6)
    # the sensor-only call: no record arrays, the body's rows stay
    s = _devarray._host_arrays(_devarray._IMPULSE_FIELDS, (1, n), 0)
    only = rbhip.WorldImpulses(*s.values(), 0)
    assert only.max_records == 0 and only.partner is None and only.jn is None and only.jt is None
    assert only.counts.shape == (1, n) and only.vel.shape == only.net.shape == (1, n, 6)


def test_new_kernels_are_listed_without_scratch():
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for m in re.finditer(r"Function Name: (\S*?\d+(world_impulses\w*?_kernel)I\S*)\s+(?:.*\n)*?.*ScratchSize \[bytes/lane\]: (\d+)", out):
        got.setdefault(m.group(2), []).append((m.group(1), int(m.group(3))))
    assert set(got) == KERNELS, sorted(got)
    for kern, inst in got.items():
        assert len(inst) == 2, (kern, inst)                # fp64 and fp32
        assert not [n for n, scratch in inst if scratch], kern
