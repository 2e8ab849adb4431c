"""rb_batch_create_wide (environments of up to 256 bodies, one per workgroup
of 2 to 4 waves): the entry point is exported, prototyped and bound, refuses
bad arguments before it touches a device, leaves the 64-body bound of
rb_batch_create / rb_batch_create_mixed alone, and its kernels
(batch_wide_kernel, wide_contacts_kernel: rb_batch_wide.hip) are built in every
instance without scratch and with LDS that scales with the block (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG

EINVAL = -22
LDS_LIMIT = 163840          # bytes a workgroup may declare on gfx950


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_create_wide_is_exported_prototyped_and_bound(lib):
    from rbhip import _lib
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "rb_batch_create_wide" in exported
    assert "rb_batch_create_wide" in _lib.SIGNATURES
    assert _lib.SIGNATURES["rb_batch_create_wide"] == _lib.SIGNATURES["rb_batch_create"]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    header = open(os.path.join(PKG, "..", "include", "rbhip.h")).read()
    assert re.search(r"\bint\s+rb_batch_create_wide\s*\(rb_batch \*\*out, const rb_scene_desc \*scene, int64_t n_envs\);",
                     header)
    assert re.search(r"^#define RB_BATCH_MAX_BODIES 256$", header, re.M)
    assert "more than 64 bodies per" not in header and "more than 256 bodies per" in header     # "Not covered"


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


def test_create_wide_refuses_bad_arguments_before_any_device_call(lib):
    """The validation of rb_batch_create with the bound at 256: NULL out or
    scene, n_envs < 1, 0 or 257 bodies, the n_envs * n_bodies range and a bad
    kind are RB_EINVAL, and out is left NULL."""
    d, keep = _desc(70, [1] * 64 + [0] * 6)
    h = C.c_void_p(1)
    assert lib.rb_batch_create_wide(None, C.byref(d), 4) == EINVAL
    assert lib.rb_batch_create_wide(C.byref(h), None, 4) == EINVAL
    for n_envs in (0, -3):
        h = C.c_void_p(1)
        assert lib.rb_batch_create_wide(C.byref(h), C.byref(d), n_envs) == EINVAL
        assert b"n_envs" in lib.rb_last_error() and not h.value
    for n in (0, 257):
        dn, keepn = _desc(n)
        h = C.c_void_p(1)
        assert lib.rb_batch_create_wide(C.byref(h), C.byref(dn), 1) == EINVAL
        assert b"n_bodies" in lib.rb_last_error() and b"256" in lib.rb_last_error() and not h.value
    h = C.c_void_p(1)
    assert lib.rb_batch_create_wide(C.byref(h), C.byref(d), (2 ** 31 - 1) // 2 // 70 + 1) == EINVAL
    assert b"out of range" in lib.rb_last_error() and not h.value
    dk, keepk = _desc(70, [1, 2] + [0] * 68)
    h = C.c_void_p(1)
    assert lib.rb_batch_create_wide(C.byref(h), C.byref(dk), 1) == EINVAL
    assert b"bad kind" in lib.rb_last_error() and not h.value


@pytest.mark.parametrize("entry", ["rb_batch_create", "rb_batch_create_mixed"])
def test_the_one_wave_entries_still_refuse_65_bodies(lib, entry):
    d65, keep65 = _desc(65)
    h = C.c_void_p(1)
    assert getattr(lib, entry)(C.byref(h), C.byref(d65), 1) == EINVAL
    assert b"n_bodies" in lib.rb_last_error() and b"64" in lib.rb_last_error() and not h.value


def _listing():
    return subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                          capture_output=True, text=True, check=True).stdout


def _resources(out, pattern):
    got = {}
    for m in re.finditer(r"Function Name: _ZN2rb\S*?\d+" + pattern + r"\S*\s+(?:.*\n)*?"
                         r".*ScratchSize \[bytes/lane\]: (\d+)(?:.*\n)*?.*Occupancy \[waves/SIMD\]: (\d+)(?:.*\n)*?"
                         r".*LDS Size \[bytes/block\]: (\d+)", out):
        *key, scratch, waves, lds = m.groups()
        assert tuple(key) not in got, key
        got[tuple(key)] = (int(scratch), int(waves), int(lds))
    return got


def test_wide_kernel_instances():
    """batch_wide_kernel<T, BOXES, REC, ENVS, BLOCK>: 2 x 2 x 2 x 2 x 3
    instances and wide_contacts_kernel<T, BOXES, BLOCK>: 2 x 2 x 3; none with
    scratch, none above the LDS a workgroup may declare, the LDS growing with
    the block (a 70-body environment does not pay for 256 lanes), the sphere
    instances without the box instances' LDS, the box instances at one wave
    per SIMD as batch_mixed_kernel is."""
    out = _listing()
    step = _resources(out, r"batch_wide_kernelI([df])Lb([01])ELb([01])ELb([01])ELi(\d+)EE")
    assert sorted(step) == sorted((t, bx, r, e, n) for t in "df" for bx in "01" for r in "01" for e in "01"
                                  for n in ("128", "192", "256")), sorted(step)
    query = _resources(out, r"wide_contacts_kernelI([df])Lb([01])ELi(\d+)EE")
    assert sorted(query) == sorted((t, bx, n) for t in "df" for bx in "01" for n in ("128", "192", "256")), sorted(query)
    for name, got in (("step", step), ("query", query)):
        assert not [k for k, v in got.items() if v[0] != 0], (name, got)
        assert not [k for k, v in got.items() if v[2] > LDS_LIMIT], (name, got)
        assert not [k for k, v in got.items() if k[1] == "1" and v[1] != 1], (name, got)
    for t in "df":
        for r in "01":
            for e in "01":
                lds = [step[(t, "1", r, e, n)][2] for n in ("128", "192", "256")]
                assert lds[0] < lds[1] < lds[2], (t, r, e, lds)
                # polygon 48, snapshots 2 x 4, orientations 2 x 4, extents 3 reals and a kind per lane, the flag words
                real = 8 if t == "d" else 4
                assert lds[2] <= (48 + 8 + 8 + 3) * real * 256 + 4 * 256 + 64, (t, r, e, lds)
                # spheres only: the snapshots and the flag words
                assert step[(t, "0", r, e, "256")][2] <= 8 * real * 256 + 64
        assert query[(t, "1", "128")][2] < query[(t, "1", "256")][2]
    # the budget DESIGN 4.3 states for the largest instance
    assert step[("d", "1", "0", "0", "256")][2] == 138248
