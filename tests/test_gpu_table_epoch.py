"""Append epochs of the wide step forms: a broadphase table read
by up to RBHIP_TABLE_EPOCH consecutive steps, to which only the bodies that
changed cell are appended, then one rebuild step.

Bar: whatever the schedule, states are bit-identical (64-bit words) and
contact lists equal to the oracle's / to a world that rebuilds every step.
Every test forces the wide forms at small sizes (RBHIP_COOP_MAX_BODIES=0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _same(a, b):
    """Bit identity as 64-bit words (the sign of zeros counts)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _wide(monkeypatch, epoch, help_wave=True):
    monkeypatch.setenv("RBHIP_COOP_MAX_BODIES", "0")
    monkeypatch.setenv("RBHIP_TABLE_EPOCH", str(epoch))
    monkeypatch.setenv("RBHIP_WIDE_HELP", "1" if help_wave else "0")


_flat_ref = {}


def _flat_reference(oracle):
    """flat_spheres(32, 32) after 300 oracle steps (computed once)."""
    if not _flat_ref:
        from rbhip import scenes
        sc = scenes.flat_spheres(32, 32)
        q, v = oracle.step(oracle.OracleScene(sc), sc.qpos0, sc.qvel0, 300)
        q.setflags(write=False)
        v.setflags(write=False)
        _flat_ref.update(sc=sc, q=q, v=v)
    return _flat_ref["sc"], _flat_ref["q"], _flat_ref["v"]


@pytest.mark.parametrize("help_wave", [True, False], ids=["help", "plain"])
@pytest.mark.parametrize("epoch", [1, 2, 16])
def test_movers_and_stale_entries_bit_exact(rb, oracle, monkeypatch, epoch, help_wave):
    """1,024 falling and bouncing spheres, 300 steps: 40 bodies change cell
    per step on average, so appended tables hold movers and stale entries.
    One step(300) graph and 300 single launches, each bit-exact with the
    oracle; the counters show append steps exactly when the epoch is > 1."""
    _wide(monkeypatch, epoch, help_wave)
    sc, q_ref, v_ref = _flat_reference(oracle)
    for mode in ("graph", "single"):
        with rb.World(sc) as w:
            if mode == "graph":
                w.step(300)
            else:
                for _ in range(300):
                    w.step_async(1)
                w.sync()
            q, v = w.get_state()
            st = w.stats()
        assert st["hashed_form"] == (4 if help_wave else 2), st
        assert _same(q, q_ref) and _same(v, v_ref), f"{mode}: state differs from the oracle"
        assert st["table_epoch"] == epoch, st
        if epoch > 1:
            assert st["append_steps"] > 0 and st["rebuild_steps"] > 0, st
            assert st["append_steps"] + st["rebuild_steps"] >= 300, st
            # every epoch of n steps ends with one rebuild
            assert st["rebuild_steps"] >= 300 // epoch, st
        else:
            assert st["append_steps"] == 0 and st["rebuild_steps"] == 0, st


def test_duplicates_on_a_hit_bit_exact(rb, oracle, monkeypatch):
    """C2 (4,096 spheres in frequent contact), 200 recorded steps at epoch
    16: contact lists and state equal to the oracle's at every step.  A
    partner that changed cell since its table was built is listed in its old
    bucket and its new one, so a body can reach it twice; the test follows
    the schedule through the counters (a step that advanced append_steps
    kept its table) and requires steps with such a partner in contact."""
    from rbhip import scenes
    _wide(monkeypatch, 16)
    sc = scenes.make("c2")
    cs = 4.0 * float(sc.size[:, 0].max()) * 1.001

    def cells(q):
        return np.floor(q.reshape(-1, 7)[:, :3] / cs).astype(np.int64)

    osc = oracle.OracleScene(sc)
    q, v = sc.qpos0, sc.qvel0
    built = cells(q)                              # cells at the build of the table the step reads
    moved_hits = 0
    with rb.World(sc) as w:
        w.record_contacts(True)
        appended = 0
        for t in range(200):
            start = cells(q)
            q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, record=True)
            w.step(1)
            gc, gp, gk, gd = w.contacts()
            assert np.array_equal(gc, cnt), f"contact counts differ at step {t}"
            assert np.array_equal(gp, par) and np.array_equal(gk, kin), f"partners / kinds differ at step {t}"
            assert _same(gd, dis), f"contact distances differ at step {t}"
            moved = (start != built).any(1)
            moved_hits += int(moved[par[kin == 16]].sum())
            st = w.stats()
            if st["append_steps"] == appended:    # a rebuild step: the next table, from the new positions
                built = cells(q)
            appended = st["append_steps"]
        gq, gv = w.get_state()
    assert _same(gq, q) and _same(gv, v)
    assert st["append_steps"] > 50, st
    assert moved_hits > 0, "no contact with a partner that changed cell during its epoch"


def test_crowding_guard_falls_back_to_rebuilds(rb, oracle, monkeypatch):
    """The crowded-cell scene (hundreds of bodies in one cell, ids spilling
    past the buckets) at epoch 16: contacts and state bit-exact with the
    oracle, and the schedule falls back — rebuild steps dominate."""
    from rbhip import scenes
    _wide(monkeypatch, 16)
    sc = scenes.crowded_cells()
    osc = oracle.OracleScene(sc)
    q, v = sc.qpos0, sc.qvel0
    with rb.World(sc) as w:
        for t in (99, 99):
            q, v = oracle.step(osc, q, v, t)
            w.step(t)
            w.record_contacts(True)
            q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, record=True)
            w.step(1)
            gc, gp, gk, gd = w.contacts()
            w.record_contacts(False)
            assert np.array_equal(gc, cnt) and np.array_equal(gp, par) and np.array_equal(gk, kin)
            assert _same(gd, dis)
            gq, gv = w.get_state()
            assert _same(gq, q) and _same(gv, v)
        st = w.stats()
    assert cnt.sum() > 100                            # the pile is in contact
    assert st["table_epoch"] == 16 and st["append_steps"] + st["rebuild_steps"] == 200, st
    assert st["rebuild_steps"] > 3 * st["append_steps"], st


def test_reprime_in_mid_epoch_bit_exact(rb, monkeypatch):
    """rb_set_state to a shifted state in the middle of an epoch, then a
    guarded chunk rolled back (an injected bucket overflow: refit, re-prime,
    replay) that also starts in mid-epoch, then 40 more steps: bit-exact
    with a fresh world that rebuilds its table every step."""
    from rbhip import scenes
    sc = scenes.flat_spheres(32, 32)
    _wide(monkeypatch, 16)
    monkeypatch.setenv("RBHIP_DIAG_OVERFLOW", "1")
    with rb.World(sc) as w:
        w.step(7)                                 # (an odd count: the 2-step start-up epoch is half done)
        q7, v7 = w.get_state()
        q7 = q7.copy()
        q7.reshape(-1, 7)[:, 0] += 0.37           # most bodies land in another cell
        w.set_state(q7, v7)
        w.step(7)                                 # a fresh schedule, in mid-epoch again
        assert w.stats()["refits"] == 0
        w.step(80)                                # guarded: rolled back once, replayed
        st_mid = w.stats()
        w.step(40)
        q, v = w.get_state()
        st = w.stats()
    assert st_mid["refits"] == 1, st_mid
    assert st["append_steps"] > 50, st
    monkeypatch.delenv("RBHIP_DIAG_OVERFLOW")
    monkeypatch.setenv("RBHIP_TABLE_EPOCH", "1")
    with rb.World(sc) as ref:
        ref.set_state(q7, v7)
        ref.step(7 + 80 + 40)
        rq, rv = ref.get_state()
        assert ref.stats()["append_steps"] == 0
    assert _same(q, rq) and _same(v, rv)


def test_box_world_takes_no_append_steps(rb, monkeypatch):
    """A world with boxes is not eligible: no append steps, and the same
    state as with RBHIP_TABLE_EPOCH=1."""
    from rbhip import scenes
    sc = scenes.box_pile(6, 6, 3, seed=0)
    res = []
    for epoch in (16, 1):
        _wide(monkeypatch, epoch)
        with rb.World(sc, max_partners=32) as w:
            w.step(60)
            res.append(w.get_state())
            st = w.stats()
        assert st["append_steps"] == 0 and st["rebuild_steps"] == 0, st
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])


def test_sharded_world_takes_no_append_steps(rb, monkeypatch):
    """Two in-process shards (their ghosts need an insert per step) are not
    eligible: no append steps, and bit-identical to one world."""
    import torch
    from rbhip import scenes
    from rbhip.shard import wrap_gpos
    _wide(monkeypatch, 16)
    sc = scenes.flat_spheres(32, 25, seed=7)
    steps = 40
    with rb.World(sc) as ref:
        ref.step(steps)
        rq, rv = ref.get_state()
        assert ref.stats()["append_steps"] > 0
    worlds = [rb.World(sc, rank=r, world_size=2) for r in range(2)]
    for _ in range(steps):
        for w in worlds:
            w.shard_step()
        for w in worlds:
            w.sync()
        bufs = [wrap_gpos(w, torch) for w in worlds]     # the buffers alternate per step
        n = bufs[0][1]
        for r, (buf, _) in enumerate(bufs):
            for o, (obuf, _) in enumerate(bufs):
                if o != r:
                    buf[o * n:(o + 1) * n].copy_(obuf[o * n:(o + 1) * n])
        torch.cuda.synchronize()
        for w in worlds:
            w.shard_exchange_done()
    q = np.zeros((sc.n, 7))
    v = np.zeros((sc.n, 6))
    for w in worlds:
        w.get_state(q, v)
        st = w.stats()
        w.close()
        assert st["append_steps"] == 0 and st["rebuild_steps"] == 0, st
    assert _same(q, rq) and _same(v, rv)


def test_more_blocks_than_resident_bit_exact(rb, oracle, monkeypatch):
    """131,044 spheres landing on each other (grid spacing 0.19 < 2r) in the
    hashed wide form (RBHIP_TILE=0) at epoch 2: 2,048 workgroups, about twice
    what the device holds at once, so late workgroups read bucket heads after
    early ones have appended their movers to the same table — also at an
    epoch's first step, every other step here.  70 steps, then a recorded
    one: contacts and state bit-exact with the oracle (16 threads)."""
    from rbhip import scenes
    monkeypatch.setenv("RBHIP_TILE", "0")
    monkeypatch.setenv("RBHIP_TABLE_EPOCH", "2")
    sc = scenes.flat_spheres(362, 362, seed=5, spacing=0.19)
    osc = oracle.OracleScene(sc)
    oracle.set_threads(16)
    try:
        q, v = oracle.step(osc, sc.qpos0, sc.qvel0, 70)
        q1, v1, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, record=True)
    finally:
        oracle.set_threads(1)
    with rb.World(sc) as w:
        w.step(70)
        gq, gv = w.get_state()
        assert _same(gq, q) and _same(gv, v)
        w.record_contacts(True)
        w.step(1)
        gq, gv = w.get_state()
        gc, gp, gk, gd = w.contacts()
        st = w.stats()
    # (landed cells hold 7+ bodies, so the crowding guard cuts many epochs: any append step will do)
    assert st["form"] in (2, 4) and st["append_steps"] > 0, st
    assert np.array_equal(gc, cnt) and np.array_equal(gp, par) and np.array_equal(gk, kin)
    assert _same(gd, dis)
    assert _same(gq, q1) and _same(gv, v1)
    assert (kin == 16).sum() > 1000
