"""The device-resident boundary of a batch (rb_batch_set_stream, _step_async,
_sync, _set_state_dev, _get_state_dev, _set_xfrc_dev, _status_dev,
_run_sampled_dev; BatchWorld.*_device): the entry points are exported, bound
and declared, a null handle is refused before any device call, the Python
argument checks refuse everything that is not the device array they expect
without ever reaching the library, and the new kernels compile without
scratch (no GPU here)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

DEV_FUNCS = ["rb_batch_set_stream", "rb_batch_step_async", "rb_batch_sync", "rb_batch_set_state_dev",
             "rb_batch_get_state_dev", "rb_batch_set_xfrc_dev", "rb_batch_status_dev", "rb_batch_run_sampled_dev"]
DEV_METHODS = ["use_stream", "step_async", "sync", "set_state_device", "get_state_device", "set_xfrc_device",
               "status_device", "run_sampled_device"]
DEV_KERNELS = {"dev_state_in_kernel", "dev_state_out_kernel", "dev_xfrc_check_kernel", "dev_xfrc_in_kernel",
               "dev_samples_out_kernel"}
# the names the resource pins of the step kernels parse `make resource-usage` by
PINNED_NAMES = ("batch_step_kernel", "batch_balls_kernel", "batch_mixed_kernel", "box_kernel")
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_dev_entry_points_are_exported_bound_and_declared(lib):
    from rbhip import _lib
    import rbhip
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in DEV_FUNCS if f not in exported]
    assert not [f for f in DEV_FUNCS if f not in _lib.SIGNATURES]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    for m in DEV_METHODS:
        assert callable(getattr(rbhip.BatchWorld, m)), m
    header = open(os.path.join(PKG, "..", "include", "rbhip.h")).read()
    for f in DEV_FUNCS:
        assert re.search(rf"\bint\s+{f}\s*\(rb_batch \*b[,)]", header), f
    # the batch's "not covered" sentence no longer lists what this boundary covers
    assert "caller streams and" not in header


def test_dev_entry_points_null_handle_is_einval(lib):
    a = np.zeros(64)
    p = a.ctypes.data_as(C.c_void_p)
    nf = C.c_int64()
    calls = {
        "rb_batch_set_stream": (None, None),
        "rb_batch_step_async": (None, 1, 0.01, 0.5, 0.5, 0.0),
        "rb_batch_sync": (None, C.byref(nf)),
        "rb_batch_set_state_dev": (None, None, p, p, 0),
        "rb_batch_get_state_dev": (None, p, p, 0),
        "rb_batch_set_xfrc_dev": (None, p, 0),
        "rb_batch_status_dev": (None, p, p),
        "rb_batch_run_sampled_dev": (None, 10, 1, 0.01, 0.5, 0.5, 0.0, p, p, 0),
    }
    assert sorted(calls) == sorted(DEV_FUNCS)
    for f, args in calls.items():
        assert getattr(lib, f)(*args) == EINVAL, f
        assert b"null batch" in lib.rb_last_error(), f


class _Fake:
    """An object with a __cuda_array_interface__ and nothing behind it."""

    def __init__(self, shape, typestr="<f8", strides=None, readonly=False):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x10000, readonly),
                                             strides=strides, version=3)


@pytest.fixture()
def stand_in():
    """A BatchWorld that was never constructed: no handle and no library (an
    access to either is an AttributeError, which no check below expects)."""
    import rbhip
    from rbhip import scenes
    b = object.__new__(rbhip.BatchWorld)
    b.scene, b.dtype, b.device = scenes.multi_sphere4(), "f64", 0
    b.n_envs, b.n_bodies = 5, 4
    return b


E, M = 5, 4
Q, V, X = (E, M, 7), (E, M, 6), (E, M, 6)


def _calls(b):
    """(argument name, shape, output?, call taking the argument's value)."""
    return [
        ("qpos", Q, False, lambda a: b.set_state_device(a, _Fake(V))),
        ("qvel", V, False, lambda a: b.set_state_device(_Fake(Q), a)),
        ("out_qpos", Q, True, lambda a: b.get_state_device(a, _Fake(V))),
        ("out_qvel", V, True, lambda a: b.get_state_device(_Fake(Q), a)),
        ("xfrc", X, False, lambda a: b.set_xfrc_device(a)),
        ("out_qpos", (3,) + Q, True, lambda a: b.run_sampled_device(30, 10, out_qpos=a, out_qvel=_Fake((3,) + V))),
        ("out_qvel", (3,) + V, True, lambda a: b.run_sampled_device(30, 10, out_qpos=_Fake((3,) + Q), out_qvel=a)),
    ]


def test_python_checks_refuse_host_arrays(stand_in):
    for name, shape, _, call in _calls(stand_in):
        with pytest.raises(TypeError, match=name):
            call(np.zeros(shape))
    with pytest.raises(TypeError, match="mask"):
        stand_in.set_state_device(_Fake(Q), _Fake(V), mask=np.zeros(E, bool))
    with pytest.raises(TypeError, match="out_code"):
        stand_in.status_device(np.zeros(E, np.int32), _Fake((E,), "<i8"))
    with pytest.raises(TypeError, match="out_steps"):
        stand_in.status_device(_Fake((E,), "<i4"), np.zeros(E, np.int64))


def test_python_checks_refuse_wrong_shape_typestr_strides(stand_in):
    for name, shape, out, call in _calls(stand_in):
        itemsize = 8
        strides = tuple(int(np.prod(shape[k + 1:])) * itemsize for k in range(len(shape)))
        with pytest.raises(ValueError, match=name):
            call(_Fake(shape[:-1] + (shape[-1] + 1,)))
        with pytest.raises(ValueError, match=name):
            call(_Fake((shape[0] * shape[1],) + shape[2:]))
        with pytest.raises(TypeError, match=name):
            call(_Fake(shape, "<f2"))
        if name != "xfrc":                                 # (the other array of the call is <f8)
            with pytest.raises(TypeError, match="one element type per call"):
                call(_Fake(shape, "<f4"))
        with pytest.raises(ValueError, match=name):
            call(_Fake(shape, strides=strides))
        if out:
            with pytest.raises(ValueError, match=name):
                call(_Fake(shape, readonly=True))
    ok_q, ok_v = _Fake(Q), _Fake(V)
    for mask in (_Fake((E + 1,), "|b1"), _Fake((E, 1), "|u1")):
        with pytest.raises(ValueError, match="mask"):
            stand_in.set_state_device(ok_q, ok_v, mask=mask)
    with pytest.raises(TypeError, match="mask"):
        stand_in.set_state_device(ok_q, ok_v, mask=_Fake((E,), "<i4"))
    with pytest.raises(ValueError, match="mask"):
        stand_in.set_state_device(ok_q, ok_v, mask=_Fake((E,), "|b1", strides=(2,)))
    with pytest.raises(TypeError, match="out_code"):
        stand_in.status_device(_Fake((E,), "<i8"), _Fake((E,), "<i8"))
    with pytest.raises(ValueError, match="out_steps"):
        stand_in.status_device(_Fake((E,), "<i4"), _Fake((E,), "<i8", readonly=True))
    with pytest.raises(ValueError, match="dtype"):
        stand_in.get_state_device(ok_q, ok_v, dtype="f16")
    with pytest.raises(ValueError, match="out_qvel"):
        stand_in.run_sampled_device(30, 10, velocities=False, out_qpos=_Fake((3,) + Q), out_qvel=_Fake((3,) + V))


def test_package_imports_without_torch():
    """The package must not import torch at import time (only an omitted
    output allocates with it)."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import rbhip, rbhip.batch\n"
            "assert callable(rbhip.BatchWorld.get_state_device)\n")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)


def test_new_kernels_are_listed_without_scratch():
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for m in re.finditer(r"Function Name: (\S*?(dev_\w+?_kernel)\S*)\s+(?:.*\n)*?.*ScratchSize \[bytes/lane\]: (\d+)", out):
        got.setdefault(m.group(2), []).append((m.group(1), int(m.group(3))))
    assert set(got) == DEV_KERNELS, sorted(got)
    for kern, inst in got.items():
        assert not [n for n, scratch in inst if scratch], kern
        assert not [n for n, _ in inst if any(p in n for p in PINNED_NAMES)], kern
