"""The device-resident boundary of a world (rb_get_state_dev, rb_set_state_dev,
rb_set_xfrc_dev; World.get_state_device, set_state_device, set_xfrc_device,
run_sampled_device): the entry points are exported, bound and declared, a null
handle is refused before any device call, the Python argument checks refuse
everything that is not the device array they expect without ever reaching the
library, and the new kernels compile without scratch (no GPU here)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

DEV_FUNCS = ["rb_get_state_dev", "rb_set_state_dev", "rb_set_xfrc_dev"]
DEV_METHODS = ["get_state_device", "set_state_device", "set_xfrc_device", "run_sampled_device"]
DEV_KERNELS = {"wdev_state_in_kernel", "wdev_state_out_kernel", "wdev_xfrc_in_kernel"}
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_world_dev_entry_points_are_exported_bound_and_declared(lib):
    from rbhip import _lib
    import rbhip
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in DEV_FUNCS if f not in exported]
    assert not [f for f in DEV_FUNCS if f not in _lib.SIGNATURES]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    for m in DEV_METHODS:
        assert callable(getattr(rbhip.World, m)), m
    header = open(os.path.join(PKG, "..", "include", "rbhip.h")).read()
    for f in DEV_FUNCS:
        assert re.search(rf"\bint\s+{f}\s*\(rb_world \*w,", header), f
    # the header says that the reader waits for a tile-form run's check
    doc = header[header.index("the device-resident boundary (world_size 1)"):header.index("int rb_get_state_dev")]
    assert "tile form" in doc and "waits" in doc


def test_world_dev_entry_points_null_handle_is_einval(lib):
    a = np.zeros(64)
    p = a.ctypes.data_as(C.c_void_p)
    calls = {
        "rb_get_state_dev": (None, p, p, 0),
        "rb_set_state_dev": (None, p, p, 0, 1),
        "rb_set_xfrc_dev": (None, p, 0),
    }
    assert sorted(calls) == sorted(DEV_FUNCS)
    for f, args in calls.items():
        assert getattr(lib, f)(*args) == EINVAL, f
        assert b"null world" in lib.rb_last_error(), f


def test_helpers_are_shared_not_copied():
    """One copy of the argument rules: both classes import them."""
    from rbhip import _devarray, batch, world
    for name in ("_device_array", "_pair_typestr", "_new_tensor"):
        assert getattr(batch, name) is getattr(_devarray, name), name
        assert getattr(world, name) is getattr(_devarray, name), name


class _Fake:
    """An object with a __cuda_array_interface__ and nothing behind it."""

    def __init__(self, shape, typestr="<f8", strides=None, readonly=False):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x10000, readonly),
                                             strides=strides, version=3)


@pytest.fixture()
def stand_in():
    """A World that was never constructed: no handle and no library (an access
    to either is an AttributeError, which no check below expects)."""
    import rbhip
    from rbhip import scenes
    w = object.__new__(rbhip.World)
    w.scene, w.dtype, w.device = scenes.multi_sphere4(), "f64", 0
    return w


N = 4
Q, V, X = (N, 7), (N, 6), (N, 6)


def _calls(w):
    """(argument name, shape, output?, call taking the argument's value)."""
    return [
        ("qpos", Q, False, lambda a: w.set_state_device(a, _Fake(V))),
        ("qvel", V, False, lambda a: w.set_state_device(_Fake(Q), a, refit=False)),
        ("out_qpos", Q, True, lambda a: w.get_state_device(a, _Fake(V))),
        ("out_qvel", V, True, lambda a: w.get_state_device(_Fake(Q), a)),
        ("xfrc", X, False, lambda a: w.set_xfrc_device(a)),
        ("out_qpos", (3,) + Q, True, lambda a: w.run_sampled_device(30, 10, out_qpos=a, out_qvel=_Fake((3,) + V))),
        ("out_qvel", (3,) + V, True, lambda a: w.run_sampled_device(30, 10, out_qpos=_Fake((3,) + Q), out_qvel=a)),
    ]


def test_python_checks_refuse_host_arrays(stand_in):
    for name, shape, _, call in _calls(stand_in):
        with pytest.raises(TypeError, match=name):
            call(np.zeros(shape))


def test_python_checks_refuse_wrong_shape_typestr_strides(stand_in):
    for name, shape, out, call in _calls(stand_in):
        itemsize = 8
        strides = tuple(int(np.prod(shape[k + 1:])) * itemsize for k in range(len(shape)))
        with pytest.raises(ValueError, match=name):
            call(_Fake(shape[:-1] + (shape[-1] + 1,)))
        with pytest.raises(ValueError, match=name):
            call(_Fake((shape[0] * shape[1],) + shape[2:] if len(shape) > 2 else (shape[0] * shape[1],)))
        with pytest.raises(TypeError, match=name):
            call(_Fake(shape, "<f2"))
        if name != "xfrc":                                 # (the other array of the call is <f8)
            with pytest.raises(TypeError, match="one element type per call"):
                call(_Fake(shape, "<f4"))
        with pytest.raises(ValueError, match=name):        # a strided view
            call(_Fake(shape, strides=strides))
        if out:
            with pytest.raises(ValueError, match=name):
                call(_Fake(shape, readonly=True))
    ok_q, ok_v = _Fake(Q), _Fake(V)
    with pytest.raises(ValueError, match="dtype"):
        stand_in.get_state_device(ok_q, ok_v, dtype="f16")
    with pytest.raises(TypeError, match="one element type per call"):
        stand_in.get_state_device(ok_q, ok_v, dtype="f32")
    with pytest.raises(ValueError, match="out_qvel"):
        stand_in.run_sampled_device(30, 10, velocities=False, out_qpos=_Fake((3,) + Q), out_qvel=_Fake((3,) + V))
    with pytest.raises(ValueError, match="every"):
        stand_in.run_sampled_device(30, 0)


def test_package_imports_without_torch():
    """The package must not import torch at import time (only an omitted
    output allocates with it)."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import rbhip, rbhip.world\n"
            "assert callable(rbhip.World.get_state_device)\n")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)


def test_new_kernels_are_listed_without_scratch():
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for m in re.finditer(r"Function Name: (\S*?\d+(wdev_\w+?_kernel)I\S*)\s+(?:.*\n)*?.*ScratchSize \[bytes/lane\]: (\d+)", out):
        got.setdefault(m.group(2), []).append((m.group(1), int(m.group(3))))
    assert set(got) == DEV_KERNELS, sorted(got)
    for kern, inst in got.items():
        # world and io element types, aligned and element-wise: 2 x 2 x 2
        assert len(inst) == 8, (kern, inst)
        assert not [n for n, scratch in inst if scratch], kern
