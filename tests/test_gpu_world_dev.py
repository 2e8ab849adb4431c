"""The device-resident boundary of a world on the GPU (World.get_state_device,
set_state_device, set_xfrc_device, run_sampled_device): torch tensors on the
device in and out, compared word for word, without a tolerance anywhere, with
the host path of the same world or of a twin world.  Every world sits on
torch's current stream."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -22, -95
NP = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _same(a, b):
    """Bit identity, as words of the arrays' own width (the sign of zeros and NaN payloads count)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype, (a.dtype, b.dtype)
    w = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    return a.shape == b.shape and np.array_equal(a.view(w), b.view(w))


def _host(t):
    return t.cpu().numpy()


def _dev(torch, a, offset=False):
    """The array on the device; offset: as a view that starts one element into its allocation."""
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()                # (torch wraps writable arrays only)
    if not offset:
        return torch.from_numpy(a).to("cuda:0")
    view = _empty(torch, a.shape, a.dtype, True)
    view.copy_(torch.from_numpy(a))
    return view


def _empty(torch, shape, np_dtype, offset=False):
    """An output tensor filled with a pattern no state holds; offset: as in _dev."""
    dt = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}[np.dtype(np_dtype)]
    n = int(np.prod(shape))
    flat = torch.full((n + 1,), -777.25, dtype=dt, device="cuda:0")
    view = (flat[1:] if offset else flat[:n]).view(shape)
    assert view.is_contiguous() and (view.data_ptr() % 16 != 0) == offset
    return view


def _scene(name):
    from rbhip import scenes
    return {"multi_sphere4": scenes.multi_sphere4, "single_cube": scenes.single_cube,
            "mixed_spheres": lambda: scenes.mixed_spheres(8, 6), "flat_spheres": lambda: scenes.flat_spheres(20, 15),
            "ball_collision": scenes.ball_collision, "balls_pile": lambda: scenes.balls_pile(4, 4)}[name]()


SCENES = ["multi_sphere4", "single_cube", "mixed_spheres", "flat_spheres"]


def _jittered(sc, seed=3):
    """The scene's start state moved: xy by +-0.02, orientations turned a little
    off theirs (none the identity), velocities by N(0, 0.3); every column
    carries its own values."""
    rng = np.random.default_rng(seed)
    q, v = sc.qpos0.copy(), sc.qvel0.copy()
    q[:, :2] += rng.uniform(-0.02, 0.02, (sc.n, 2))
    q[:, 3:] += rng.uniform(0.01, 0.06, (sc.n, 4))
    q[:, 3:] /= np.linalg.norm(q[:, 3:], axis=1, keepdims=True)
    v += rng.normal(0.0, 0.3, (sc.n, 6))
    return q, v


def _forces(n, k, seed):
    """k seeded applied-force arrays (n, 6): force N(0, 0.5), torque N(0, 0.05)."""
    rng = np.random.default_rng(seed)
    return [np.concatenate([rng.normal(0.0, 0.5, (n, 3)), rng.normal(0.0, 0.05, (n, 3))], axis=1) for _ in range(k)]


def _world(rb, torch, sc, **kw):
    """A world on torch's current stream (the documented way to share tensors with torch)."""
    w = rb.World(sc, **kw)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    return w


# ------------------------------------------------------------------ 1. round trip out
def _expect_out(w, world_dtype, io):
    q, v = w.get_state()
    return q.astype(NP[io]), v.astype(NP[io])     # (f64 io: the same words; f32 io on f64: the C cast)


@pytest.mark.parametrize("world_dtype,io", [("f64", "f64"), ("f64", "f32"), ("f32", "f64")])
@pytest.mark.parametrize("name", SCENES)
def test_get_state_device_equals_get_state(rb, torch, name, world_dtype, io):
    sc = _scene(name)
    with _world(rb, torch, sc, dtype=world_dtype) as w:
        w.step(7)
        q, v = _expect_out(w, world_dtype, io)
        gq, gv = w.get_state_device(dtype=io)                       # omitted outputs
        assert gq.shape == (sc.n, 7) and gv.shape == (sc.n, 6)
        assert _same(_host(gq), q) and _same(_host(gv), v)
        for offset in (False, True):
            oq, ov = _empty(torch, (sc.n, 7), NP[io], offset), _empty(torch, (sc.n, 6), NP[io], offset)
            rq, rv = w.get_state_device(oq, ov)
            assert rq is oq and rv is ov
            assert _same(_host(oq), q) and _same(_host(ov), v), f"offset {offset}"
            # only one of the two given: the other comes back new, both hold the state
            oq = _empty(torch, (sc.n, 7), NP[io], offset)
            rq, rv = w.get_state_device(out_qpos=oq)
            assert rq is oq and _same(_host(oq), q) and _same(_host(rv), v), f"qpos only, offset {offset}"
            ov = _empty(torch, (sc.n, 6), NP[io], offset)
            rq, rv = w.get_state_device(out_qvel=ov)
            assert rv is ov and _same(_host(ov), v) and _same(_host(rq), q), f"qvel only, offset {offset}"
        # the C entry with one null pointer writes the other array only
        oq = _empty(torch, (sc.n, 7), NP[io])
        code = 0 if io == "f64" else 1
        assert w._L.rb_get_state_dev(w._h, C.c_void_p(oq.data_ptr()), None, code) == 0
        assert _same(_host(oq), q)
        ov = _empty(torch, (sc.n, 6), NP[io], True)
        assert w._L.rb_get_state_dev(w._h, None, C.c_void_p(ov.data_ptr()), code) == 0
        assert _same(_host(ov), v)
        assert w._L.rb_get_state_dev(w._h, None, None, code) == EINVAL


# ------------------------------------------------------------------ 2. round trip in
@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("name", SCENES)
def test_set_state_device_equals_set_state(rb, torch, name, io):
    sc = _scene(name)
    q, v = _jittered(sc)
    qi, vi = q.astype(NP[io]), v.astype(NP[io])
    with rb.World(sc) as twin:
        twin.set_state(qi.astype(np.float64), vi.astype(np.float64))     # (f32 io: the widened values)
        tq0, tv0 = twin.get_state()
        twin.step(5)
        tq, tv = twin.get_state()
    for refit in (True, False):
        for offset in (False, True):
            with _world(rb, torch, sc) as w:
                w.step(2)                                               # (a state other than the start's)
                w.set_state_device(_dev(torch, qi, offset), _dev(torch, vi, offset), refit=refit)
                gq, gv = w.get_state()
                assert _same(gq, tq0) and _same(gv, tv0), f"state as set: refit {refit}, offset {offset}"
                w.step(5)
                gq, gv = w.get_state()
                assert _same(gq, tq) and _same(gv, tv), f"after 5 steps: refit {refit}, offset {offset}"


# ------------------------------------------------------------------ 3. boxes see the orientation
def test_set_state_device_reaches_the_box_narrowphase(rb, torch):
    from rbhip import scenes
    sc = scenes.incline_cubes(4, 4)
    q, v = _jittered(sc)
    with rb.World(sc) as twin, _world(rb, torch, sc) as w:
        for x in (twin, w):
            x.record_contacts(True)
            x.step(3)
        twin.set_state(q, v)
        w.set_state_device(_dev(torch, q), _dev(torch, v))
        twin.step(1)
        w.step(1)
        tc, tp, tk, td = twin.contacts()
        gc, gp, gk, gd = w.contacts()
        assert tc.sum() > 0
        assert np.array_equal(gc, tc) and np.array_equal(gp, tp) and np.array_equal(gk, tk) and _same(gd, td)
        assert all(_same(a, b) for a, b in zip(w.get_state(), twin.get_state()))


def test_set_state_device_reaches_box_partners(rb, torch):
    """The cubes of incline_cubes(4, 4) only touch the plane, and a plane
    contact reads the body's own orientation from the state rows.  A box pair
    reads the partner's from the orientation snapshot: a pile that has landed
    (80 steps) is set into worlds that hold other orientations, and the next
    step's box-box contacts must be the twin's."""
    from rbhip import scenes
    sc = scenes.box_pile(2, 2)
    with rb.World(sc, max_partners=32) as src:
        src.step(80)
        q, v = src.get_state()
    with rb.World(sc, max_partners=32) as twin, _world(rb, torch, sc, max_partners=32) as w:
        for x in (twin, w):
            x.record_contacts(True)
            x.step(3)
        twin.set_state(q, v)
        w.set_state_device(_dev(torch, q, True), _dev(torch, v, True))
        twin.step(1)
        w.step(1)
        tc, tp, tk, td = twin.contacts()
        gc, gp, gk, gd = w.contacts()
        assert (tk >= 32).any(), "no box-box contact in the twin's list"      # (RB_CK_BOX_BOX0)
        assert np.array_equal(gc, tc) and np.array_equal(gp, tp) and np.array_equal(gk, tk) and _same(gd, td)
        twin.step(3)
        w.step(3)
        assert all(_same(a, b) for a, b in zip(w.get_state(), twin.get_state()))


# ------------------------------------------------------------------ 4. the two-ball law
@pytest.mark.parametrize("name", ["ball_collision", "balls_pile"])
def test_two_ball_law_both_directions(rb, torch, name):
    sc = _scene(name)
    q, v = _jittered(sc)
    with rb.World(sc, law="balls") as twin, _world(rb, torch, sc, law="balls") as w:
        w.step(7)
        hq, hv = w.get_state()
        gq, gv = w.get_state_device()
        assert _same(_host(gq), hq) and _same(_host(gv), hv)
        twin.set_state(q, v)
        w.set_state_device(_dev(torch, q, True), _dev(torch, v, True))
        twin.step(5)
        w.step_async(5)
        gq, gv = w.get_state_device()
        tq, tv = twin.get_state()
        assert _same(_host(gq), tq) and _same(_host(gv), tv)


# ------------------------------------------------------------------ 5. forces
def test_set_xfrc_device_equals_set_xfrc(rb, torch):
    sc = _scene("mixed_spheres")
    (f,) = _forces(sc.n, 1, 11)
    for io, offset in (("f64", False), ("f64", True), ("f32", False), ("f32", True)):
        fi = f.astype(NP[io])
        with rb.World(sc) as twin, _world(rb, torch, sc) as w:
            twin.set_xfrc(fi.astype(np.float64))
            w.set_xfrc_device(_dev(torch, fi, offset))
            twin.step(6)
            w.step(6)
            assert all(_same(a, b) for a, b in zip(w.get_state(), twin.get_state())), (io, offset)


def test_force_sequence_none_device_device_none(rb, torch):
    """The first device set allocates the force rows and drops the graphs
    captured without forces; the stages use the same chunk length so that a
    stale graph would be replayed if it were kept."""
    sc = _scene("mixed_spheres")
    f1, f2 = _forces(sc.n, 2, 12)
    with rb.World(sc) as twin, _world(rb, torch, sc) as w:
        def stage(what):
            twin.step(4)
            w.step_async(4)
            gq, gv = w.get_state_device()
            tq, tv = twin.get_state()
            assert _same(_host(gq), tq) and _same(_host(gv), tv), what
        stage("no forces")
        twin.set_xfrc(f1)
        w.set_xfrc_device(_dev(torch, f1))
        stage("first device forces")
        twin.set_xfrc(f2)
        w.set_xfrc_device(_dev(torch, f2, True))
        stage("other device forces")
        twin.set_xfrc(None)
        w.set_xfrc(None)
        stage("forces cleared")


# ------------------------------------------------------------------ 6. closed loop
def test_closed_loop_without_synchronisation(rb, torch):
    sc = _scene("flat_spheres")
    q0, v0 = _jittered(sc)
    with rb.World(sc) as twin, _world(rb, torch, sc) as w:
        twin.set_state(q0, v0)
        w.set_state(q0, v0)
        q, v = torch.empty((sc.n, 7), dtype=torch.float64, device="cuda:0"), torch.empty((sc.n, 6), dtype=torch.float64, device="cuda:0")
        for _ in range(20):
            w.get_state_device(q, v)
            w.set_xfrc_device(-0.5 * v)
            w.step_async(1)
        for _ in range(20):
            _, hv = twin.get_state()
            twin.set_xfrc(-0.5 * hv)
            twin.step(1)
        gq, gv = w.get_state_device()
        tq, tv = twin.get_state()
        assert _same(_host(gq), tq) and _same(_host(gv), tv)


# ------------------------------------------------------------------ 7. tile form
def _tile_world(rb, torch, monkeypatch, sc, tile):
    monkeypatch.setenv("RBHIP_TILE", "1" if tile else "0")
    w = _world(rb, torch, sc)
    monkeypatch.delenv("RBHIP_TILE")
    return w


def test_tile_form_reads_and_writes_through_the_boundary(rb, torch, monkeypatch):
    from rbhip import scenes
    sc = scenes.flat_spheres(40, 40)
    q, v = _jittered(sc)
    with _tile_world(rb, torch, monkeypatch, sc, True) as wt, _tile_world(rb, torch, monkeypatch, sc, False) as wh:
        wt.step_async(8)
        wh.step(8)
        gq, gv = wt.get_state_device()                  # (waits for the tile run's check)
        hq, hv = wh.get_state()
        assert _same(_host(gq), hq) and _same(_host(gv), hv)
        st0 = wt.stats()
        assert st0["form"] == 5 and st0["tile_runs"] >= 1, st0
        wt.set_state_device(_dev(torch, q), _dev(torch, v))
        wh.set_state(q, v)
        wt.step(8)
        wh.step(8)
        assert all(_same(a, b) for a, b in zip(wt.get_state(), wh.get_state()))
        st = wt.stats()
        assert st["form"] == 5 and st["tile_runs"] > st0["tile_runs"], (st0, st)
        assert wh.stats()["form"] != 5


# ------------------------------------------------------------------ 8. the mirror trap
def test_set_state_after_set_state_device_uploads(rb, torch):
    sc = _scene("mixed_spheres")
    other = _jittered(sc)
    with _world(rb, torch, sc) as w:
        w.step(3)
        q, v = w.get_state()
        w.set_state_device(_dev(torch, other[0]), _dev(torch, other[1]))
        st0 = w.stats()
        w.set_state(q, v)                               # the bytes of the earlier get_state: must upload
        st = w.stats()
        gq, gv = w.get_state()
        assert _same(gq, q) and _same(gv, v)
        assert st["io_uploads"] == st0["io_uploads"] + 1 and st["io_skipped"] == st0["io_skipped"], (st0, st)


# ------------------------------------------------------------------ 9. layout
def test_refit_fits_the_layout_as_set_state_does(rb, torch):
    from rbhip import scenes
    sc = scenes.make("c3")
    q, v = sc.qpos0.copy(), sc.qvel0.copy()
    q[:, 0] += 200.0
    q[:, 1] += 200.0
    with rb.World(sc) as twin:
        twin.set_state(q, v)
        layout_twin = twin.stats()["grid_layout"]
        twin.step(5)
        tq, tv = twin.get_state()
    dq, dv = _dev(torch, q), _dev(torch, v)
    with _world(rb, torch, sc) as w:
        w.set_state_device(dq, dv, refit=True)
        assert w.stats()["grid_layout"] == layout_twin
    with _world(rb, torch, sc) as w:
        before = w.stats()["grid_layout"]
        w.set_state_device(dq, dv, refit=False)
        assert w.stats()["grid_layout"] == before
        w.step(5)
        gq, gv = w.get_state()
        assert _same(gq, tq) and _same(gv, tv)


# ------------------------------------------------------------------ 10. sampling
@pytest.mark.parametrize("prealloc", [True, False])
def test_run_sampled_device(rb, torch, prealloc):
    sc = _scene("multi_sphere4")
    with rb.World(sc) as twin, _world(rb, torch, sc) as w:
        want = []
        for _ in range(4):
            twin.step(5)
            want.append(twin.get_state())
        twin.step(3)
        if prealloc:
            oq, ov = _empty(torch, (4, sc.n, 7), np.float64), _empty(torch, (4, sc.n, 6), np.float64)
            sq, sv = w.run_sampled_device(23, 5, out_qpos=oq, out_qvel=ov)
            assert sq is oq and sv is ov
        else:
            sq, sv = w.run_sampled_device(23, 5)
            assert tuple(sq.shape) == (4, sc.n, 7) and tuple(sv.shape) == (4, sc.n, 6)
        for s, (tq, tv) in enumerate(want):
            assert _same(_host(sq[s]), tq) and _same(_host(sv[s]), tv), f"sample {s}"
        assert all(_same(a, b) for a, b in zip(w.get_state(), twin.get_state()))
        pq, none = w.run_sampled_device(4, 2, velocities=False, dtype="f32")
        assert none is None and tuple(pq.shape) == (2, sc.n, 7) and pq.dtype == torch.float32
        twin.step(4)
        assert _same(_host(pq[1]), twin.get_state()[0].astype(np.float32))


# ------------------------------------------------------------------ 11. refusals
def test_refusals(rb, torch):
    from rbhip import scenes
    sc = scenes.flat_spheres(8, 8)
    dq = torch.zeros((sc.n, 7), dtype=torch.float64, device="cuda:0")
    dv = torch.zeros((sc.n, 6), dtype=torch.float64, device="cuda:0")
    pq, pv = C.c_void_p(dq.data_ptr()), C.c_void_p(dv.data_ptr())
    with rb.World(sc, rank=0, world_size=2) as w:
        L, h = w._L, w._h
        q0, v0 = w.get_state()
        assert L.rb_get_state_dev(h, pq, pv, 0) == EUNSUPPORTED and b"world_size" in L.rb_last_error()
        assert L.rb_set_state_dev(h, pq, pv, 0, 1) == EUNSUPPORTED
        assert L.rb_set_xfrc_dev(h, pv, 0) == EUNSUPPORTED
        with pytest.raises(rb.RbError, match="EUNSUPPORTED"):
            w.set_state_device(dq, dv)
        assert all(_same(a, b) for a, b in zip(w.get_state(), (q0, v0)))
        assert not _host(dq).any() and not _host(dv).any()
    with _world(rb, torch, sc) as w:
        L, h = w._L, w._h
        q0, v0 = w.get_state()
        assert L.rb_get_state_dev(h, pq, pv, 7) == EINVAL and b"io_dtype" in L.rb_last_error()
        assert L.rb_set_state_dev(h, pq, pv, 7, 0) == EINVAL
        assert L.rb_set_xfrc_dev(h, pv, 7) == EINVAL
        assert L.rb_set_state_dev(h, pq, None, 0, 0) == EINVAL
        assert L.rb_set_xfrc_dev(h, None, 0) == EINVAL
        with pytest.raises(ValueError, match="qpos"):
            w.set_state_device(torch.zeros((sc.n, 6), dtype=torch.float64, device="cuda:0"), dv)
        with pytest.raises(ValueError, match="xfrc"):
            w.set_xfrc_device(torch.zeros((sc.n + 1, 6), dtype=torch.float64, device="cuda:0"))
        with pytest.raises(ValueError, match="out_qvel"):
            w.get_state_device(dq, torch.zeros((sc.n, 12), dtype=torch.float64, device="cuda:0")[:, ::2])
        with pytest.raises(TypeError, match="xfrc"):
            w.set_xfrc_device(np.zeros((sc.n, 6)))
        assert all(_same(a, b) for a, b in zip(w.get_state(), (q0, v0)))
