"""Contact-impulse curves of a sampled run (rb_batch_run_sampled_impulses,
rb_batch_run_sampled_impulses_dev; BatchWorld.run_sampled_impulses /
run_sampled_impulses_device; kernels in rb_batch_sensed.hip): the entry points
are exported, bound and declared as the header declares them, a null handle is
refused before any device call, the Python argument checks refuse what is not
the device array they expect without reaching the library, the new kernels are
built in sixteen instances without scratch under names of their own, and the
impulse query's kernels keep the resources they had before (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

FUNCS = ["rb_batch_run_sampled_impulses", "rb_batch_run_sampled_impulses_dev"]
EINVAL = -22
# the names the resource pins of the other kernels parse `make resource-usage` by
PINNED_NAMES = ("batch_step_kernel", "batch_balls_kernel", "batch_mixed_kernel", "box_kernel", "batch_wide_kernel",
                "wide_contacts_kernel", "batch_contacts_kernel", "batch_contacts_boxes_kernel", "ragged_step_kernel",
                "ragged_wide_kernel", "ragged_contacts_kernel", "ragged_wide_contacts_kernel", "batch_impulses_kernel",
                "batch_impulses_wide_kernel")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


@pytest.fixture(scope="module")
def resources():
    return subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                          capture_output=True, text=True, check=True).stdout


def test_entry_points_are_exported_bound_and_declared(lib):
    from rbhip import _lib
    import rbhip
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in FUNCS if f not in exported]
    assert not [f for f in FUNCS if f not in _lib.SIGNATURES]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    assert callable(rbhip.BatchWorld.run_sampled_impulses) and callable(rbhip.BatchWorld.run_sampled_impulses_device)
    header = open(os.path.join(ROOT, "include", "rbhip.h")).read()
    host = re.search(r"\bint\s+rb_batch_run_sampled_impulses\s*\(rb_batch \*b, int64_t nsteps, int64_t every, double dt,"
                     r"\s*double restitution,\s*double friction, double contact_threshold,"
                     r"\s*double \*qpos, double \*qvel, double \*net, int64_t \*n_failed\);", header)
    dev = re.search(r"\bint\s+rb_batch_run_sampled_impulses_dev\s*\(rb_batch \*b, int64_t nsteps, int64_t every, double dt,"
                    r"\s*double restitution,\s*double friction, double contact_threshold,"
                    r"\s*void \*qpos, void \*qvel, void \*net, int32_t io_dtype\);", header)
    assert host and dev
    # the ctypes signatures carry the header's argument kinds, in its order
    kinds = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, m in ((FUNCS[0], host), (FUNCS[1], dev)):
        args = [a.strip() for a in m.group(0)[m.group(0).index("(") + 1:m.group(0).rindex(")")].split(",")]
        want = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in args]
        res, got = _lib.SIGNATURES[name]
        got = [C.c_void_p if (g is not C.c_void_p and hasattr(g, "contents")) else g for g in got]
        assert res is C.c_int and got == want, name
    for word in ("collision.py:7-48", ":72-88", "physics_utils.py:25-49", "Not covered: the same query for an rb_world",
                 "Not covered (use rb_world)", "more than 256 bodies per", "per-contact records (jn, jt) inside"):
        assert word in header, word
    assert "impulses recorded inside\n * rb_batch_run_sampled;" not in header


def test_null_handle_is_einval_before_any_device_call(lib):
    d = np.zeros(64)
    q = d.ctypes.data_as(C.c_void_p)
    nf = C.c_int64(7)
    for args in ((None, 12, 3, 0.01, 0.5, 0.5, 0.0, q, q, q, C.byref(nf)),
                 (None, -1, 0, float("nan"), -1.0, -1.0, -1.0, None, None, None, None)):
        assert lib.rb_batch_run_sampled_impulses(*args) == EINVAL
        assert b"null batch" in lib.rb_last_error()
    for args in ((None, 12, 3, 0.01, 0.5, 0.5, 0.0, q, q, q, 0), (None, -1, 0, 0.0, 0.0, 0.0, 0.0, None, None, None, 5)):
        assert lib.rb_batch_run_sampled_impulses_dev(*args) == EINVAL
        assert b"null batch" in lib.rb_last_error()
    assert nf.value == 7 and not d.any()


class _Fake:
    """An object with a __cuda_array_interface__ and nothing behind it."""

    def __init__(self, shape, typestr="<f8", strides=None, readonly=False):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(0x10000, readonly),
                                             strides=strides, version=3)


E, M, S = 5, 4, 4


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


SHAPES = {"out_qpos": (S, E, M, 7), "out_qvel": (S, E, M, 6), "out_net": (S, E, M, 6)}


def _out(**repl):
    out = {k: _Fake(s) for k, s in SHAPES.items()}
    out.update(repl)
    return out


def test_python_checks_refuse_host_arrays_wrong_shapes_and_types(stand_in):
    b = stand_in
    run = lambda **kw: b.run_sampled_impulses_device(S * 3, 3, **kw)
    for name, shape in SHAPES.items():
        with pytest.raises(TypeError, match=name):
            run(**_out(**{name: np.zeros(shape)}))                                   # host memory
        with pytest.raises(ValueError, match=name):
            run(**_out(**{name: _Fake(shape[:-1] + (shape[-1] + 1,))}))              # a wrong shape
        with pytest.raises(ValueError, match=name):
            run(**_out(**{name: _Fake((S + 1,) + shape[1:])}))                       # a sample too many
        with pytest.raises(TypeError, match=name):
            run(**_out(**{name: _Fake(shape, "<f2")}))                               # a wrong dtype
        with pytest.raises(ValueError, match=name):
            run(**_out(**{name: _Fake(shape, strides=(8,) * 4)}))                    # a stride
        with pytest.raises(ValueError, match=name):
            run(**_out(**{name: _Fake(shape, readonly=True)}))                       # read-only
    # out_net alone, the other outputs switched off: still checked before anything else happens
    for bad, exc in ((_Fake(SHAPES["out_net"], readonly=True), ValueError), (_Fake((S, E, M, 5)), ValueError),
                     (_Fake(SHAPES["out_net"], "<i4"), TypeError), (np.zeros(SHAPES["out_net"]), TypeError)):
        with pytest.raises(exc, match="out_net"):
            run(positions=False, velocities=False, out_net=bad)
    with pytest.raises(TypeError, match="one element type per call"):
        run(**_out(out_net=_Fake(SHAPES["out_net"], "<f4")))
    with pytest.raises(ValueError, match="dtype"):
        run(dtype="f16", **_out())
    with pytest.raises(ValueError, match="out_qpos"):
        run(positions=False, **_out())
    with pytest.raises(ValueError, match="out_qvel"):
        run(velocities=False, **_out())


def _listed(out, pattern):
    """{groups: (name, VGPRs, scratch, waves per SIMD, LDS bytes)} of the kernels whose mangled name holds pattern"""
    got = {}
    for m in re.finditer(r"Function Name: (\S*?\d+" + pattern + r"\S*)\s+(?:.*\n)*?.*VGPRs: (\d+)(?:.*\n)*?"
                         r".*ScratchSize \[bytes/lane\]: (\d+)(?:.*\n)*?.*Occupancy \[waves/SIMD\]: (\d+)(?:.*\n)*?"
                         r".*LDS Size \[bytes/block\]: (\d+)", out):
        key = m.groups()[1:-4]
        assert key not in got, key
        got[key] = (m.group(1),) + tuple(int(x) for x in m.groups()[-4:])
    return got


INSTANCES = sorted((t, bx, blk) for t in "df" for bx in (0, 1) for blk in (64, 128, 192, 256))


def test_sensing_kernels_are_listed_without_scratch(resources):
    """sensed_run_kernel<T, BOXES> and sensed_run_wide_kernel<T, BOXES, BLOCK> for
    T = double / float, BOXES = 0 / 1, BLOCK = 128 / 192 / 256: sixteen
    instances, none with scratch; the box ones at one wave per SIMD (the box
    narrowphase, the polygon column in LDS), the sphere ones at two or more with
    no polygon, orientation, extent or kind LDS; none under a name another
    kernel's resource pins parse by.  The planes are dynamic LDS."""
    got = {}
    for (wide, t, bx, blk), v in _listed(resources, r"sensed_run(_wide)?_kernelI([df])Lb([01])E(?:Li(\d+)E)?E").items():
        key = (t, int(bx), int(blk or 64))
        assert bool(wide) == (key[2] != 64)
        got[key] = v
    assert sorted(got) == INSTANCES, sorted(got)
    for (t, boxes, block), (name, vgprs, scratch, waves, lds) in got.items():
        assert scratch == 0, name
        assert not [p for p in PINNED_NAMES if re.search(rf"\d+{p}I", name)], name
        assert not re.search(r"dev_[a-z_]+_kernel", name), name
        real = 8 if t == "d" else 4
        fail = 4 * (block if block == 64 else 2)                     # the failure flag: per environment, or ping-pong
        snaps = 2 * block * 4 * real                                 # position snapshots, ping-pong
        pad = lambda n: -(-n // 16) * 16                             # (the block's LDS is allocated in 16-byte units)
        if boxes:
            assert waves == 1, name
            # orientations (ping-pong), extents, kind, and the polygon column of 48 reals per lane
            assert lds == pad(snaps + fail + block * (2 * 4 * real + 3 * real + 4 + 48 * real)), name
        else:
            assert waves >= 2, name
            assert lds == pad(snaps + fail), name
    drain = _listed(resources, r"sensed_out_kernelI([df])([df])E")
    assert sorted(drain) == [("d", "d"), ("d", "f"), ("f", "d"), ("f", "f")]
    assert not [v[0] for v in drain.values() if v[2]]


# VGPRs, LDS bytes per block and scratch bytes per lane of batch_impulses_kernel<T, BOXES> (block 64) and
# batch_impulses_wide_kernel<T, BOXES, BLOCK>, read from `make resource-usage` of the commit before the
# sensing kernels were added: the impulse query's unit is untouched and compiles to what it did.
IMPULSES_PARENT = {
    ("d", 1, 64): (239, 30464, 0), ("d", 1, 128): (233, 60928, 0), ("d", 1, 192): (233, 91392, 0),
    ("d", 1, 256): (233, 121856, 0),
    ("d", 0, 64): (200, 2048, 0), ("d", 0, 128): (198, 4096, 0), ("d", 0, 192): (198, 6144, 0), ("d", 0, 256): (198, 8192, 0),
    ("f", 1, 64): (174, 15360, 0), ("f", 1, 128): (168, 30720, 0), ("f", 1, 192): (168, 46080, 0),
    ("f", 1, 256): (168, 61440, 0),
    ("f", 0, 64): (116, 1024, 0), ("f", 0, 128): (112, 2048, 0), ("f", 0, 192): (112, 3072, 0), ("f", 0, 256): (112, 4096, 0),
}


def test_impulse_query_kernels_keep_their_resources(resources):
    got = {}
    for (wide, t, bx, blk), (name, vgprs, scratch, waves, lds) in _listed(
            resources, r"batch_impulses(_wide)?_kernelI([df])Lb([01])E(?:Li(\d+)E)?E").items():
        got[t, int(bx), int(blk or 64)] = (vgprs, lds, scratch)
    assert got == IMPULSES_PARENT
