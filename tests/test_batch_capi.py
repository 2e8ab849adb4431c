"""Batched worlds (rb_batch_*): the entry points are exported and their
argument validation runs before any device call (no GPU here)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG

BATCH_FUNCS = ["rb_batch_create", "rb_batch_destroy", "rb_batch_set_params", "rb_batch_set_bodies",
               "rb_batch_set_state", "rb_batch_get_state", "rb_batch_step", "rb_batch_status"]
EINVAL, EUNSUPPORTED = -22, -95


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


class Desc:
    """A scene descriptor of n bodies (kinds given) that keeps its arrays alive."""

    def __init__(self, kinds, **kw):
        from rbhip import _lib
        n = len(kinds)
        self.kind = np.asarray(kinds, np.int32)
        self.mass = np.ones(n)
        self.inertia = np.ones((n, 3))
        self.size = np.full((n, 3), 0.1)
        self.planes = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 0.0]])
        d = _lib.SceneDesc()
        d.n_bodies, d.n_planes, d.world_size = n, 1, 1
        d.kind, d.mass, d.inertia = _lib.ptr(self.kind), _lib.ptr(self.mass), _lib.ptr(self.inertia)
        d.size, d.planes = _lib.ptr(self.size), _lib.ptr(self.planes)
        d.gravity[2] = -9.8
        for k, v in kw.items():
            setattr(d, k, v)
        self.d = d


def test_batch_entry_points_are_exported_and_bound(lib):
    from rbhip import _lib
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in BATCH_FUNCS if f not in exported]
    assert not [f for f in BATCH_FUNCS if f not in _lib.SIGNATURES]
    assert b"0.4" in lib.rb_version()
    import rbhip
    assert rbhip.BatchWorld is not None


def _create(lib, desc, n_envs):
    h = C.c_void_p()
    rc = lib.rb_batch_create(C.byref(h), C.byref(desc.d) if desc is not None else None, n_envs)
    assert rc != 0 and not h.value
    return rc, lib.rb_last_error()


def test_batch_create_rejects_bad_arguments_without_device(lib):
    ok = Desc([0, 0, 0, 0])
    assert lib.rb_batch_create(None, C.byref(ok.d), 4) == EINVAL
    assert _create(lib, None, 4)[0] == EINVAL
    assert _create(lib, ok, 0)[0] == EINVAL
    assert _create(lib, ok, -3)[0] == EINVAL
    assert _create(lib, Desc([]), 4)[0] == EINVAL                      # n_bodies 0
    assert _create(lib, Desc([0] * 65), 4)[0] == EINVAL                # n_bodies 65
    assert _create(lib, Desc([0, 0], world_size=2), 4)[0] == EINVAL
    assert _create(lib, Desc([0, 0], world_size=2, rank=1), 4)[0] == EINVAL
    assert _create(lib, Desc([0, 0], kind=None), 4)[0] == EINVAL       # a null scene array
    assert _create(lib, Desc([0, 0], mass=None), 4)[0] == EINVAL
    assert _create(lib, Desc([0, 7]), 4)[0] == EINVAL                  # bad kind
    assert _create(lib, Desc([0, 0], dtype=5), 4)[0] == EINVAL


def test_batch_box_with_other_bodies_is_unsupported(lib):
    for kinds in ([1, 0], [0, 1], [1, 1], [0, 0, 1, 0]):
        rc, msg = _create(lib, Desc(kinds), 4)
        assert rc == EUNSUPPORTED and b"unsupported" in msg.lower(), (kinds, rc, msg)


def test_batch_null_handle_is_einval(lib):
    a = np.zeros(16)
    p = a.ctypes.data_as(C.c_void_p)
    nf = C.c_int64()
    assert lib.rb_batch_set_params(None, p, p) == EINVAL
    assert lib.rb_batch_set_bodies(None, p, p, p) == EINVAL
    assert lib.rb_batch_set_state(None, None, 1, p, p) == EINVAL
    assert lib.rb_batch_get_state(None, None, 1, p, p) == EINVAL
    assert lib.rb_batch_step(None, 1, 0.01, 0.5, 0.5, 0.0, C.byref(nf)) == EINVAL
    assert lib.rb_batch_status(None, p, p) == EINVAL
    lib.rb_batch_destroy(None)                                         # a no-op
