"""rb_batch_create_mixed (a batch whose template mixes spheres and boxes): the
entry point is exported and bound, refuses bad arguments before it touches a
device, and its kernel (batch_mixed_kernel, rb_batch_boxes.hip) is built in 8
instances without scratch next to a box_kernel that compiles to what it
compiled to before (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_create_mixed_is_exported_and_bound(lib):
    from rbhip import _lib
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "rb_batch_create_mixed" in exported
    assert "rb_batch_create_mixed" in _lib.SIGNATURES
    assert _lib.SIGNATURES["rb_batch_create_mixed"] == _lib.SIGNATURES["rb_batch_create"]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    header = open(os.path.join(PKG, "..", "include", "rbhip.h")).read()
    assert re.search(r"\bint\s+rb_batch_create_mixed\s*\(rb_batch \*\*out, const rb_scene_desc \*scene, int64_t n_envs\);",
                     header)
    assert "box-involved pairs (a box is accepted" not in header        # struck from "Not covered"


def _desc(n, kinds=None):
    """A scene description of n bodies (unit spheres unless kinds says otherwise) and what keeps its arrays alive."""
    from rbhip import _lib
    kind = np.zeros(n, np.int32) if kinds is None else np.asarray(kinds, np.int32)
    mass, inertia, size = np.ones(n), np.ones((n, 3)), np.ones((n, 3))
    planes = np.array([[0.0, 0, 1, 0, 0, 0]])
    d = _lib.SceneDesc()
    d.n_bodies, d.n_planes = n, 1
    d.dtype, d.normal_convention = _lib.RB_F64, _lib.RB_NORMAL_ORIENTED
    d.device, d.rank, d.world_size = 0, 0, 1
    d.kind, d.mass, d.inertia, d.size = _lib.ptr(kind), _lib.ptr(mass), _lib.ptr(inertia), _lib.ptr(size)
    d.planes = _lib.ptr(planes)
    d.gravity[2] = -9.8
    return d, (kind, mass, inertia, size, planes)


def test_create_mixed_refuses_bad_arguments_before_any_device_call(lib):
    """The validation of rb_batch_create: NULL out or scene, n_envs < 1, 65
    bodies, a bad kind are RB_EINVAL, and out is left NULL."""
    d, keep = _desc(3, [1, 1, 0])
    h = C.c_void_p(1)
    assert lib.rb_batch_create_mixed(None, C.byref(d), 4) == EINVAL
    assert lib.rb_batch_create_mixed(C.byref(h), None, 4) == EINVAL
    for n_envs in (0, -3):
        h = C.c_void_p(1)
        assert lib.rb_batch_create_mixed(C.byref(h), C.byref(d), n_envs) == EINVAL
        assert b"n_envs" in lib.rb_last_error() and not h.value
    d65, keep65 = _desc(65, [1] * 65)
    h = C.c_void_p(1)
    assert lib.rb_batch_create_mixed(C.byref(h), C.byref(d65), 1) == EINVAL
    assert b"n_bodies" in lib.rb_last_error() and not h.value
    dk, keepk = _desc(3, [1, 2, 0])
    h = C.c_void_p(1)
    assert lib.rb_batch_create_mixed(C.byref(h), C.byref(dk), 1) == EINVAL
    assert b"bad kind" in lib.rb_last_error() and not h.value
    # rb_batch_create still refuses the template, and now says where it is taken
    h = C.c_void_p(1)
    assert lib.rb_batch_create(C.byref(h), C.byref(d), 4) == -95
    assert b"rb_batch_create_mixed" in lib.rb_last_error() and not h.value


# VGPRs, LDS bytes per block and scratch bytes per lane of box_kernel<T, MAXP> as
# `make -C csrc resource-usage` reported them on the parent of the commit that
# added batch_mixed_kernel (profiles/batch/mixed_resources.txt, first listing):
# body_update, which holds the box-involved pair block, is unchanged.
PARENT_BOX_KERNEL = {
    ("d", 16): (256, 28672, 0),
    ("d", 32): (256, 32768, 0),
    ("f", 16): (249, 16384, 0),
    ("f", 32): (249, 20480, 0),
}


def _resources(pattern):
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for m in re.finditer(r"Function Name: _ZN2rb\d+" + pattern + r"\S*\s+(?:.*\n)*?.*VGPRs: (\d+)(?:.*\n)*?"
                         r".*ScratchSize \[bytes/lane\]: (\d+)(?:.*\n)*?.*LDS Size \[bytes/block\]: (\d+)", out):
        *key, vgpr, scratch, lds = m.groups()
        got[tuple(key)] = (int(vgpr), int(lds), int(scratch))
    return got


def test_mixed_kernel_instances_and_box_kernel_pin():
    """batch_mixed_kernel<T, REC, ENVS>: 2 x 2 x 2 instances, none with
    scratch, the static LDS the same with and without ENVS (the planes are
    dynamic LDS); box_kernel: the parent's numbers."""
    mixed = _resources(r"batch_mixed_kernelI([df])Lb([01])ELb([01])EE")
    assert sorted(mixed) == sorted((t, r, e) for t in "df" for r in "01" for e in "01"), sorted(mixed)
    assert not [k for k, v in mixed.items() if v[2] != 0], mixed
    for t in "df":
        assert len({mixed[(t, r, e)][1] for r in "01" for e in "01"}) == 1
    box = {(t, int(n)): v for (t, n), v in _resources(r"box_kernelI([df])Li(\d+)EE").items()}
    assert box == PARENT_BOX_KERNEL, box
