"""rb_batch_set_population (per-environment body counts and kinds): the entry
point is exported, prototyped and bound, refuses a null batch before it
touches a device, its kernels (rb_batch_ragged.hip) are built in every
instance without scratch, within the LDS a workgroup may declare, the box
instances at one wave per SIMD and the sphere instances without the box
instances' LDS, and BatchWorld.from_ragged_scenes pads and refuses as
documented (no GPU here)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG

EINVAL = -22
LDS_LIMIT = 163840          # bytes a workgroup may declare on gfx950
BLOCKS = ("128", "192", "256")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_set_population_is_exported_prototyped_and_bound(lib):
    import ctypes as C
    from rbhip import _lib
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "rb_batch_set_population" in exported
    assert _lib.SIGNATURES["rb_batch_set_population"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    header = open(os.path.join(PKG, "..", "include", "rbhip.h")).read()
    assert re.search(r"\bint\s+rb_batch_set_population\s*\(rb_batch \*b, const int32_t \*n_bodies, const int32_t \*kind\);",
                     header)
    # "Not covered": plane counts stay, kinds and body counts moved out
    covered = header[header.index("Not covered (use rb_world)"):header.index("A batch handle is not thread-safe")]
    assert "per-environment plane counts" in covered and "more than 256 bodies per" in covered
    assert "per-environment kinds" not in covered


def test_set_population_refuses_a_null_batch_before_any_device_call(lib):
    n = np.ones(4, np.int32)
    from rbhip import _lib
    assert lib.rb_batch_set_population(None, _lib.ptr(n), None) == EINVAL
    assert b"null batch" in lib.rb_last_error()
    assert lib.rb_batch_set_population(None, None, None) == EINVAL


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


def test_ragged_kernel_instances():
    """ragged_step_kernel<T, BOXES, REC> (2 x 2 x 2), ragged_wide_kernel<T,
    BOXES, REC, BLOCK> (2 x 2 x 2 x 3), ragged_contacts_kernel<T, BOXES> (2 x 2)
    and ragged_wide_contacts_kernel<T, BOXES, BLOCK> (2 x 2 x 3): 8 + 24 step
    and 4 + 12 query kernels; none with scratch, none above the LDS a
    workgroup may declare, the box instances at one wave per SIMD, the sphere
    instances with the snapshots and the flag words only, the wide LDS growing
    with the block."""
    out = _listing()
    step = _resources(out, r"ragged_step_kernelI([df])Lb([01])ELb([01])EE")
    assert sorted(step) == sorted((t, bx, r) for t in "df" for bx in "01" for r in "01"), sorted(step)
    wide = _resources(out, r"ragged_wide_kernelI([df])Lb([01])ELb([01])ELi(\d+)EE")
    assert sorted(wide) == sorted((t, bx, r, n) for t in "df" for bx in "01" for r in "01" for n in BLOCKS), sorted(wide)
    query = _resources(out, r"ragged_contacts_kernelI([df])Lb([01])EE")
    assert sorted(query) == sorted((t, bx) for t in "df" for bx in "01"), sorted(query)
    wquery = _resources(out, r"ragged_wide_contacts_kernelI([df])Lb([01])ELi(\d+)EE")
    assert sorted(wquery) == sorted((t, bx, n) for t in "df" for bx in "01" for n in BLOCKS), sorted(wquery)
    assert len(step) + len(wide) == 8 + 24 and len(query) + len(wquery) == 4 + 12
    for name, got in (("step", step), ("wide", wide), ("query", query), ("wide query", wquery)):
        assert not [k for k, v in got.items() if v[0] != 0], (name, got)
        assert not [k for k, v in got.items() if v[2] > LDS_LIMIT], (name, got)
        assert not [k for k, v in got.items() if k[1] == "1" and v[1] != 1], (name, got)
    for t in "df":
        real = 8 if t == "d" else 4
        for r in "01":
            # one wave, spheres only: the snapshots (2 x 4 reals per lane) and a flag word per lane
            assert step[(t, "0", r)][2] <= 8 * real * 64 + 4 * 64
            # one wave, boxes: polygon 48, snapshots 2 x 4, orientations 2 x 4, extents 3 reals, a kind and a flag per lane
            assert 48 * real * 64 < step[(t, "1", r)][2] <= (48 + 8 + 8 + 3) * real * 64 + 8 * 64
            lds = [wide[(t, "1", r, n)][2] for n in BLOCKS]
            assert lds[0] < lds[1] < lds[2], (t, r, lds)
            assert lds[2] <= (48 + 8 + 8 + 3) * real * 256 + 4 * 256 + 64, (t, r, lds)
            slds = [wide[(t, "0", r, n)][2] for n in BLOCKS]
            assert slds[0] < slds[1] < slds[2] <= 8 * real * 256 + 64, (t, r, slds)
        # the queries: one snapshot per lane without boxes
        assert query[(t, "0")][2] <= 4 * real * 64
        assert wquery[(t, "0", "256")][2] <= 4 * real * 256
        assert wquery[(t, "1", "128")][2] < wquery[(t, "1", "192")][2] < wquery[(t, "1", "256")][2]
    # the box instance's static LDS beside the planes block of a packed wave (64 x 8 planes x 6 reals):
    # what DESIGN 4.3 states for blocks per CU
    assert step[("d", "1", "0")][2] + 64 * 8 * 6 * 8 <= LDS_LIMIT // 2


# ---------------------------------------------------------------- from_ragged_scenes (no device: a stub constructor)
class _Recorded(Exception):
    pass


def _stub(monkeypatch):
    """BatchWorld with a constructor and setters that only record their arguments."""
    from rbhip import BatchWorld
    calls = {}

    def init(self, scene, n_envs, **kw):
        calls["init"] = (scene, n_envs, kw)
        self._h = None
        self.scene, self.n_envs, self.n_bodies = scene, n_envs, scene.n

    monkeypatch.setattr(BatchWorld, "__init__", init)
    for name in ("set_population", "set_planes", "set_gravity", "set_params", "set_bodies", "set_state"):
        monkeypatch.setattr(BatchWorld, name, (lambda nm: lambda self, *a, **kw: calls.__setitem__(nm, (a, kw)))(name))
    return BatchWorld, calls


def test_from_ragged_scenes_pads_shorter_scenes(monkeypatch):
    """single_sphere, single_cube and multi_sphere4 (made to agree in dt and
    threshold) in one batch: M = 4, the template is the first scene of four
    bodies, the population is every scene's count and kinds, the padding is
    mass and inertia 1, the template's size row, the identity pose at the
    origin and zero velocity."""
    from rbhip import scenes
    BatchWorld, calls = _stub(monkeypatch)
    scs = [sc.with_(dt=0.009, threshold=1e-4) for sc in (scenes.single_sphere(), scenes.single_cube(), scenes.multi_sphere4())]
    assert [sc.n for sc in scs] == [1, 1, 4] and list(scs[1].kind) == [1]
    b = BatchWorld.from_ragged_scenes(scs + [scs[2].with_(friction=0.25)], dtype="f32")
    t, E, kw = calls["init"]
    assert t is scs[2] and E == 4 and kw == {"dtype": "f32"} and b.n_bodies == 4
    (n, kinds), _ = calls["set_population"]
    assert n.tolist() == [1, 1, 4, 4]
    assert kinds.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    _, bodies = calls["set_bodies"]
    for e, sc in enumerate(scs):
        assert np.array_equal(bodies["mass"][e, :sc.n], sc.mass) and (bodies["mass"][e, sc.n:] == 1).all()
        assert np.array_equal(bodies["inertia"][e, :sc.n], sc.inertia) and (bodies["inertia"][e, sc.n:] == 1).all()
        assert np.array_equal(bodies["size"][e, :sc.n], sc.size)
        assert np.array_equal(bodies["size"][e, sc.n:], np.asarray(t.size)[sc.n:])
    (qpos, qvel), _ = calls["set_state"]
    assert qpos.shape == (4, 4, 7) and qvel.shape == (4, 4, 6)
    for e, sc in enumerate(scs):
        assert np.array_equal(qpos[e, :sc.n], sc.qpos0) and np.array_equal(qvel[e, :sc.n], sc.qvel0)
        assert (qpos[e, sc.n:] == [0, 0, 0, 1, 0, 0, 0]).all() and not qvel[e, sc.n:].any()
    # everything from_scenes takes per scene
    (planes,), _ = calls["set_planes"]
    (gravity,), _ = calls["set_gravity"]
    assert all(np.array_equal(planes[e], sc.planes) and np.array_equal(gravity[e], sc.gravity) for e, sc in enumerate(scs))
    _, params = calls["set_params"]
    assert params["friction"] == [sc.friction for sc in scs] + [0.25]
    assert params["restitution"] == [sc.restitution for sc in scs] + [scs[2].restitution]


def test_from_ragged_scenes_refuses_mismatched_scenes(monkeypatch):
    """Scenes that disagree in plane count, dt, threshold or normal
    convention: ValueError naming the first offender, before any batch is
    created; differing body counts and kinds reach the constructor."""
    from rbhip import BatchWorld, scenes

    def no_batch(self, *a, **kw):
        raise AssertionError("a batch was created")

    monkeypatch.setattr(BatchWorld, "__init__", no_batch)
    c = scenes.cube_incline
    two_planes = np.concatenate([c(0.2).planes, c(0.3).planes])
    for bad, what in ((c(0.2).with_(planes=two_planes), "plane count"),
                      (c(0.2).with_(dt=0.01), "dt"),
                      (c(0.2).with_(threshold=0.0), "threshold"),
                      (c(0.2).with_(normal_convention="raw"), "normal convention")):
        with pytest.raises(ValueError, match=f"scene 2 .*{what}"):
            BatchWorld.from_ragged_scenes([c(0.0), c(0.1), bad, bad])
    with pytest.raises(ValueError):
        BatchWorld.from_ragged_scenes([])
    pile = scenes.box_pile(1, 1, 3)
    with pytest.raises(AssertionError, match="a batch was created"):
        BatchWorld.from_ragged_scenes([pile, scenes.box_pile(1, 1, 1, sphere_every=0)])
    # from_scenes keeps its refusals
    with pytest.raises(ValueError, match="body count"):
        BatchWorld.from_scenes([pile, scenes.box_pile(1, 1, 1, sphere_every=0)])
