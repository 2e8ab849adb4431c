"""The contact query of a batch (rb_batch_contacts, rb_batch_contacts_dev;
BatchWorld.contacts / contacts_device; kernels in rb_batch_contacts.hip): the
entry points are exported, bound and declared, a null handle is refused before
any device call, the Python argument checks refuse what is not the device
array they expect without reaching the library, BatchContacts.lists() gives
the CSR shape, and the new kernel is built in four instances (both real types,
the plain and the mixed template class) without scratch, the mixed ones at one
wave per SIMD (no GPU here)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

FUNCS = ["rb_batch_contacts", "rb_batch_contacts_dev"]
EINVAL = -22
# the names the resource pins of the step kernels parse `make resource-usage` by
PINNED_NAMES = ("batch_step_kernel", "batch_balls_kernel", "batch_mixed_kernel", "box_kernel")


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
    assert callable(rbhip.BatchWorld.contacts) and callable(rbhip.BatchWorld.contacts_device)
    assert callable(rbhip.BatchContacts.lists)
    header = open(os.path.join(ROOT, "include", "rbhip.h")).read()
    assert re.search(r"\bint\s+rb_batch_contacts\s*\(rb_batch \*b, const int64_t \*env_ids, int64_t n, int32_t max_records,"
                     r"\s*int32_t \*counts, int32_t \*partner, int32_t \*kind,"
                     r"\s*double \*dist, double \*pos, double \*frame, int64_t \*n_truncated\);", header)
    assert re.search(r"\bint\s+rb_batch_contacts_dev\s*\(rb_batch \*b, int32_t max_records, int32_t \*counts, int32_t \*partner,"
                     r"\s*int32_t \*kind, void \*dist, void \*pos, void \*frame, int32_t io_dtype\);", header)
    # the batch's "not covered" sentence no longer says a batch has no contact list
    assert "(use rb_world): contact recording" not in header
    for word in ("geom1", "kind -1", "count -1", "n_truncated"):
        assert word in header, word


def test_null_handle_is_einval_before_any_device_call(lib):
    a = np.zeros(64, np.int32)
    d = np.zeros(64)
    p, q = a.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
    nt = C.c_int64(7)
    # (every other argument is one the call would also refuse, or accept: the handle is checked first)
    for args in ((None, None, 1, 4, p, p, p, q, q, q, C.byref(nt)),
                 (None, None, -1, -1, None, None, None, None, None, None, None)):
        assert lib.rb_batch_contacts(*args) == EINVAL
        assert b"null batch" in lib.rb_last_error()
    for args in ((None, 4, p, p, p, q, q, q, 0), (None, -1, None, None, None, None, None, None, 5)):
        assert lib.rb_batch_contacts_dev(*args) == EINVAL
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


SHAPES = {"counts": (E, M), "partner": (E, M, R), "kind": (E, M, R), "dist": (E, M, R), "pos": (E, M, R, 3),
          "frame": (E, M, R, 3)}
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
            b.contacts_device(out=_out(**{name: host}))
        ts = "<i4" if name in INTS else "<f8"
        if name != "partner":                                # (partner's last axis is the slot count)
            with pytest.raises(ValueError, match=name):
                b.contacts_device(out=_out(**{name: _Fake(shape[:-1] + (shape[-1] + 1,), ts)}))
        with pytest.raises(TypeError, match=name):
            b.contacts_device(out=_out(**{name: _Fake(shape, "<f2")}))
        strides = tuple(int(np.prod(shape[k + 1:])) * 8 for k in range(len(shape)))
        with pytest.raises(ValueError, match=name):
            b.contacts_device(out=_out(**{name: _Fake(shape, ts, strides=strides)}))
        with pytest.raises(ValueError, match=name):
            b.contacts_device(out=_out(**{name: _Fake(shape, ts, readonly=True)}))
    with pytest.raises(ValueError, match="partner"):
        b.contacts_device(max_records=R + 1, out=_out())
    with pytest.raises(TypeError, match="one element type per call"):
        b.contacts_device(out=_out(pos=_Fake(SHAPES["pos"], "<f4")))
    with pytest.raises(ValueError, match="dtype"):
        b.contacts_device(out=_out(), dtype="f16")
    with pytest.raises(ValueError, match="counts"):
        b.contacts_device(out=_out(counts=None))
    with pytest.raises(ValueError, match="all three"):
        b.contacts_device(out=_out(kind=None))
    with pytest.raises(ValueError, match="max_records"):
        b.contacts_device(max_records=-1)


def test_default_max_records_is_the_scenes_bound_capped_at_16(stand_in):
    from rbhip import scenes
    b = stand_in
    assert b._max_records(None) == 4 * 1 + 3                     # four balls, one plane
    assert b._max_records(3) == 3 and b._max_records(0) == 0
    b.scene, b.n_bodies = scenes.box_pile(1, 1, 3), 4
    assert b._max_records(None) == 16                            # 4 + 4 * 3
    b.scene, b.n_bodies = scenes.single_cube(), 1
    assert b._max_records(None) == 4
    b.scene, b.n_bodies = scenes.mixed_spheres(8, 6), 48
    assert b._max_records(None) == 16                            # 12 + 47, capped


def test_lists_gives_the_csr_shape():
    import rbhip
    counts = np.array([[2, 0, 5], [-1, -1, -1]], np.int32)       # R = 3: body 2 truncated; a failed environment
    partner = np.arange(18, dtype=np.int32).reshape(2, 3, 3)
    kind = partner + 100
    dist = partner * 0.5
    pos = np.arange(54.0).reshape(2, 3, 3, 3)
    c = rbhip.BatchContacts(3, counts, partner, kind, dist, pos, None, 1)
    cnt, par, kin, dis, p, f = c.lists(0)
    assert cnt.tolist() == [2, 0, 5] and par.tolist() == [0, 1, 6, 7, 8] and kin.tolist() == [100, 101, 106, 107, 108]
    assert dis.tolist() == [0.0, 0.5, 3.0, 3.5, 4.0] and f is None
    assert p.shape == (5, 3) and p[2].tolist() == [18.0, 19.0, 20.0]
    cnt, par, kin, dis, p, f = c.lists(1)
    assert cnt.tolist() == [-1, -1, -1] and par.size == 0 and p.shape == (0, 3)
    with pytest.raises(ValueError, match="counts-only"):
        rbhip.BatchContacts(0, counts, None, None, None, None, None, 0).lists(0)


def test_package_imports_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import rbhip, rbhip.batch\n"
            "assert callable(rbhip.BatchWorld.contacts_device) and callable(rbhip.BatchContacts.lists)\n")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)


def test_contact_kernels_are_listed_without_scratch():
    """batch_contacts_kernel<T> (sphere-only and one-box templates) and
    batch_contacts_boxes_kernel<T> (mixed templates), T = double and float:
    four instances, none with scratch, the mixed ones at one wave per SIMD by
    design (the box narrowphase, as batch_mixed_kernel), none under a name the
    step kernels' resource pins parse by."""
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for m in re.finditer(r"Function Name: (\S*?\d+(batch_contacts(?:_boxes)?_kernel)I([df])E\S*)\s+(?:.*\n)*?"
                         r".*ScratchSize \[bytes/lane\]: (\d+)(?:.*\n)*?.*Occupancy \[waves/SIMD\]: (\d+)", out):
        assert (m.group(2), m.group(3)) not in got
        got[(m.group(2), m.group(3))] = (m.group(1), int(m.group(4)), int(m.group(5)))
    assert sorted(got) == [("batch_contacts_boxes_kernel", "d"), ("batch_contacts_boxes_kernel", "f"),
                           ("batch_contacts_kernel", "d"), ("batch_contacts_kernel", "f")], sorted(got)
    for (kern, t), (name, scratch, waves) in got.items():
        assert scratch == 0, name
        assert not [p for p in PINNED_NAMES if re.search(rf"\d+{p}", name)], name
        assert not re.search(r"dev_[a-z_]+_kernel", name), name
        if kern == "batch_contacts_boxes_kernel":
            assert waves == 1, name
