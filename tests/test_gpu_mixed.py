"""Heterogeneous scenes through every step form (scenes.mixed_spheres,
scenes.trough_bricks): per-body radius, mass and anisotropic inertia, three
planes (a V trough and a wall), gravity with x and y components, a non-zero
contact threshold, and non-cubic boxes lying on two planes at once.

With identical bodies an l / i mix-up of the constants' index, a swapped
inertia column or a wrong R I R^T cannot show, and with one plane neither can
the plane loops' contact order, their -1 - pl partners, the records' stride
4 n_planes + ... or the helper wave's record count.  Bar: bit-exact, no
tolerance anywhere — np.array_equal against the reference's goldens, 64-bit
words (_same) against the oracle."""
import numpy as np
import pytest

from conftest import golden_scene, load_golden

pytestmark = pytest.mark.gpu

MIXED_GOLDENS = ["traj_mixed48", "traj_mixed48_raw", "traj_bricks6"]

# hashed_form of rb_world_stats (rbhip._lib.FORM_NAMES); "split" is the
# one-lane form in two kernels
FORMS = {
    "coop": (1, {"RBHIP_HELP_MAX_BODIES": "0"}),
    "coop_help": (3, {"RBHIP_HELP_MAX_BODIES": "100000"}),
    "wide": (4, {"RBHIP_COOP_MAX_BODIES": "0"}),
    "wide_plain": (2, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_HELP": "0"}),
    "one": (0, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_MAX_BODIES": "0"}),
    "split": (0, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_MAX_BODIES": "0", "RBHIP_SPLIT": "1"}),
}


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


@pytest.fixture
def oracle16(oracle):
    oracle.set_threads(16)
    yield oracle
    oracle.set_threads(1)


def _same(a, b):
    """Bit identity as 64-bit words (the sign of zeros counts)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _setenv(monkeypatch, env):
    for k in ("RBHIP_COOP_MAX_BODIES", "RBHIP_WIDE_MAX_BODIES", "RBHIP_HELP_MAX_BODIES", "RBHIP_WIDE_HELP",
              "RBHIP_SPLIT", "RBHIP_TABLE_EPOCH", "RBHIP_TILE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _planes_per_body(cnt, par):
    """Distinct planes in each body's recorded list."""
    owner = np.repeat(np.arange(cnt.size), cnt)
    pl = par < 0
    if not pl.any():
        return np.zeros(cnt.size, np.int64)
    pairs = np.unique(np.stack([owner[pl], par[pl].astype(np.int64)], axis=1), axis=0)
    return np.bincount(pairs[:, 0], minlength=cnt.size)


def _assert_contacts(got, want, tag):
    gc, gp, gk, gd = got
    cnt, par, kin, dis = want
    assert np.array_equal(gc, cnt), f"{tag}: contact counts differ at bodies {np.flatnonzero(gc != cnt)[:8]}"
    assert np.array_equal(gp, par), f"{tag}: contact partners differ"
    assert np.array_equal(gk, kin), f"{tag}: contact kinds differ"
    assert _same(gd, dis), f"{tag}: contact distances differ"


def _assert_state(got, want, tag):
    (gq, gv), (q, v) = got, want
    bad = np.flatnonzero((gq.view(np.uint64) != np.ascontiguousarray(q).view(np.uint64)).any(1) |
                         (gv.view(np.uint64) != np.ascontiguousarray(v).view(np.uint64)).any(1))
    assert bad.size == 0, f"{tag}: state differs at {bad.size} bodies, first {bad[:8]}"


# ---------------------------------------------------------------- 4.1 goldens through a World
@pytest.mark.parametrize("name", MIXED_GOLDENS)
def test_mixed_goldens_contacts_and_state(rb, monkeypatch, name):
    """The reference's goldens through a World in its default form, one step
    per launch, every step's contact list and every snapshot."""
    _setenv(monkeypatch, {})
    g = load_golden(name)
    with rb.World(golden_scene(g)) as w:
        w.record_contacts(True)
        snaps = list(g["snap_step"])
        si = 1
        for t in range(snaps[-1]):
            w.step(1)
            cnt, par, kin, dis = w.contacts()
            a, b = g["c_off"][t], g["c_off"][t + 1]
            assert np.array_equal(cnt, g["c_counts"][t]), f"contact counts differ at step {t}"
            assert np.array_equal(par, g["c_partner"][a:b]), f"partners differ at step {t}"
            assert np.array_equal(kin, g["c_kind"][a:b]), f"kinds differ at step {t}"
            assert np.array_equal(dis, g["c_dist"][a:b]), f"dists differ at step {t}"
            if si < len(snaps) and t + 1 == snaps[si]:
                q, v = w.get_state()
                assert np.array_equal(q, g["qpos"][si]), f"qpos differs at step {t + 1}"
                assert np.array_equal(v, g["qvel"][si]), f"qvel differs at step {t + 1}"
                si += 1
        assert si == len(snaps)


@pytest.mark.parametrize("name", MIXED_GOLDENS)
def test_mixed_goldens_graph_replayed(rb, monkeypatch, name):
    """The same goldens in graph-replayed chunks from snapshot to snapshot
    (box worlds: the optimistic chunks, whose helper wave solves the box
    corners), each chunk's last contact list against the golden's."""
    _setenv(monkeypatch, {})
    g = load_golden(name)
    snaps = list(g["snap_step"])
    with rb.World(golden_scene(g)) as w:
        w.record_contacts(True)
        for si in range(1, len(snaps)):
            w.step(int(snaps[si] - snaps[si - 1]))
            t = int(snaps[si]) - 1
            cnt, par, kin, dis = w.contacts()
            a, b = g["c_off"][t], g["c_off"][t + 1]
            assert np.array_equal(cnt, g["c_counts"][t]), f"contact counts differ at step {t}"
            assert np.array_equal(par, g["c_partner"][a:b]) and np.array_equal(kin, g["c_kind"][a:b]), t
            assert np.array_equal(dis, g["c_dist"][a:b]), f"dists differ at step {t}"
            q, v = w.get_state()
            assert np.array_equal(q, g["qpos"][si]), f"qpos differs at step {t + 1}"
            assert np.array_equal(v, g["qvel"][si]), f"qvel differs at step {t + 1}"
        st = w.stats()
    assert st["box_rollbacks"] == 0, st


# ---------------------------------------------------------------- 4.2 every hashed form
_ragged = {}


def _ragged_reference(oracle, dtype="f64"):
    """mixed_spheres(37, 29, seed=3) — 1,073 bodies, a partial last wave —
    after 120 oracle steps, and the recorded step 121 (computed once per
    precision, never modified)."""
    if dtype not in _ragged:
        from rbhip import scenes
        sc = scenes.mixed_spheres(37, 29, seed=3)
        assert sc.n == 1073 and sc.n % 64 != 0
        osc = oracle.OracleScene(sc)
        q, v = oracle.step(osc, sc.qpos0, sc.qvel0, 120, dtype=dtype)
        q1, v1, con = oracle.step(osc, q, v, 1, dtype=dtype, record=True)
        for a in (q, v, q1, v1) + tuple(con):
            a.setflags(write=False)
        _ragged[dtype] = dict(sc=sc, q120=q, v120=v, q121=q1, v121=v1, con=con)
    return _ragged[dtype]


def test_ragged_reference_is_not_vacuous(oracle):
    """Step 121 of the 1,073-body scene: sphere-sphere contacts, all three
    planes, bodies on two planes at once, contacts skipped by the threshold."""
    r = _ragged_reference(oracle)
    cnt, par, kin, dis = r["con"]
    assert (kin == 16).sum() == 110 and cnt.max() <= 4
    assert set(np.unique(par[par < 0]).tolist()) == {-1, -2, -3}
    assert (_planes_per_body(cnt, par) >= 2).sum() >= 1
    assert ((dis < 0) & (dis > -r["sc"].threshold)).any()


def _run_ragged(rb, r, dtype="f64"):
    sc = r["sc"]
    with rb.World(sc, dtype=dtype) as w:
        w.step(120)
        s120 = w.get_state()
        w.record_contacts(True)
        w.step(1)
        s121 = w.get_state()
        con = w.contacts()
        st = w.stats()
    return s120, s121, con, st


@pytest.mark.parametrize("form", list(FORMS))
def test_mixed_scene_every_step_form_bit_exact(rb, oracle, monkeypatch, form):
    """120 graph-replayed steps, then one recorded step, through each step
    form the library can pick: contacts and state against the oracle."""
    code, env = FORMS[form]
    _setenv(monkeypatch, env)
    r = _ragged_reference(oracle)
    s120, s121, con, st = _run_ragged(rb, r)
    assert st["hashed_form"] == code and st["form"] == code, st
    _assert_state(s120, (r["q120"], r["v120"]), f"{form}: step 120")
    _assert_contacts(con, r["con"], f"{form}: step 121")
    _assert_state(s121, (r["q121"], r["v121"]), f"{form}: step 121")


@pytest.mark.parametrize("form", ["coop_help", "wide"])
def test_mixed_scene_f32_bit_exact(rb, oracle, monkeypatch, form):
    """The same in fp32 against the oracle's fp32 restatement."""
    code, env = FORMS[form]
    _setenv(monkeypatch, env)
    r = _ragged_reference(oracle, "f32")
    assert (r["con"][2] == 16).sum() > 50
    s120, s121, con, st = _run_ragged(rb, r, "f32")
    assert st["hashed_form"] == code, st
    _assert_state(s120, (r["q120"], r["v120"]), f"{form} f32: step 120")
    _assert_contacts(con, r["con"], f"{form} f32: step 121")
    _assert_state(s121, (r["q121"], r["v121"]), f"{form} f32: step 121")


def test_mixed_scene_wide_append_epochs_bit_exact(rb, oracle, monkeypatch):
    """The wide form with append epochs of up to 16 steps: bodies of
    different radii appended to a kept table."""
    _setenv(monkeypatch, dict(FORMS["wide"][1], RBHIP_TABLE_EPOCH="16"))
    r = _ragged_reference(oracle)
    s120, s121, con, st = _run_ragged(rb, r)
    assert st["hashed_form"] == 4 and st["table_epoch"] == 16 and st["append_steps"] > 0, st
    _assert_state(s120, (r["q120"], r["v120"]), "epoch 16: step 120")
    _assert_contacts(con, r["con"], "epoch 16: step 121")
    _assert_state(s121, (r["q121"], r["v121"]), "epoch 16: step 121")


# ---------------------------------------------------------------- 4.3 bricks
_bricks = {}


def _bricks_reference(oracle):
    """trough_bricks(64, seed=2): the recorded step 140 and steps 141-150."""
    if not _bricks:
        from rbhip import scenes
        sc = scenes.trough_bricks(64, seed=2)
        osc = oracle.OracleScene(sc)
        q, v = oracle.step(osc, sc.qpos0, sc.qvel0, 139)
        steps = []
        for t in range(140, 151):
            q, v, con = oracle.step(osc, q, v, 1, record=True)
            for a in (q, v) + tuple(con):
                a.setflags(write=False)
            steps.append((t, q, v, con))
        _bricks.update(sc=sc, steps=steps)
    return _bricks["sc"], _bricks["steps"]


@pytest.mark.parametrize("form", ["coop_help", "wide"])
def test_trough_bricks_bit_exact(rb, oracle, monkeypatch, form):
    """64 non-cubic bricks in the two-plane trough.  140 steps in one
    optimistic chunk (no brick pair in range: the sphere step kernels, whose
    helper wave solves a box's corners plane by plane) with the last step
    recorded, then steps 141-150 one launch each (the box kernel): contact
    lists and state against the oracle."""
    code, env = FORMS[form]
    _setenv(monkeypatch, env)
    sc, steps = _bricks_reference(oracle)
    seen, both, full = set(), 0, 0
    with rb.World(sc) as w:
        w.record_contacts(True)
        w.step(140)
        for t, q, v, con in steps:
            if t > 140:
                w.step(1)
            _assert_contacts(w.contacts(), con, f"{form}: step {t}")
            _assert_state(w.get_state(), (q, v), f"{form}: step {t}")
            seen |= set(con[2].tolist())
            both += int((_planes_per_body(con[0], con[1]) == 2).sum())
            full += int((np.bincount(np.repeat(np.arange(sc.n), con[0]) * 2 + (-1 - con[1]), minlength=1) == 4).sum())
        st = w.stats()
    assert st["hashed_form"] == code and st["box_opt_chunks"] >= 1 and st["box_rollbacks"] == 0, st
    # the window holds every corner kind, bricks on both planes, and faces lying flat (4 corners on a plane)
    assert seen == set(range(1, 9)) and both >= 100 and full > 0, (seen, both, full)


# ---------------------------------------------------------------- 4.4 the tile form's type table
@pytest.mark.parametrize("types", [3, 4])
def test_tile_form_type_table_bit_exact(rb, oracle16, monkeypatch, types):
    """4,096 mixed spheres of 3 and of 4 distinct (m, I) in tile slots (type
    bits above TILE_ID_BITS in the id word, the constants selected by value):
    60 steps, then 2 recorded steps, contacts and state against the oracle;
    every step committed in the tile form."""
    from rbhip import scenes
    sc = scenes.mixed_spheres(64, 64, seed=3, types=types)
    rows = np.unique(np.concatenate([sc.mass[:, None], sc.inertia], axis=1), axis=0)
    assert rows.shape[0] == types
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 60)
    _setenv(monkeypatch, {"RBHIP_TILE": "1"})
    ss, planes = 0, set()
    with rb.World(sc) as w:
        monkeypatch.delenv("RBHIP_TILE")
        w.step(60)
        _assert_state(w.get_state(), (q, v), "step 60")
        w.record_contacts(True)
        for t in (61, 62):
            q, v, con = oracle16.step(osc, q, v, 1, record=True)
            w.step(1)
            _assert_contacts(w.contacts(), con, f"step {t}")
            _assert_state(w.get_state(), (q, v), f"step {t}")
            ss += int((con[2] == 16).sum())
            planes |= set(con[1][con[1] < 0].tolist())
        st = w.stats()
    assert st["form"] == 5 and st["tile_rollbacks"] == 0 and st["tile_steps"] == 62, st
    assert ss > 200 and planes == {-1, -2, -3}, (ss, planes)


@pytest.mark.parametrize("types", [5, None])
def test_tile_form_declines_more_types_than_its_table(rb, oracle16, monkeypatch, types):
    """More than TILE_TYPES distinct (m, I): the world steps with the hashed
    forms even with RBHIP_TILE=1 — and bit-exact all the same."""
    from rbhip import scenes
    sc = scenes.mixed_spheres(64, 64, seed=3, types=types)
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 60)
    q1, v1, con = oracle16.step(osc, q, v, 1, record=True)
    _setenv(monkeypatch, {"RBHIP_TILE": "1"})
    with rb.World(sc) as w:
        monkeypatch.delenv("RBHIP_TILE")
        w.step(60)
        _assert_state(w.get_state(), (q, v), "step 60")
        w.record_contacts(True)
        w.step(1)
        _assert_contacts(w.contacts(), con, "step 61")
        _assert_state(w.get_state(), (q1, v1), "step 61")
        st = w.stats()
    assert st["form"] != 5 and st["tile_steps"] == 0, st
    assert (con[2] == 16).sum() > 100


# ---------------------------------------------------------------- 4.5 shards
def test_mixed_scene_three_shards_match_one_world(rb, oracle, monkeypatch):
    """P = 3 body-range shards of the 1,073-body scene (S = 358: the last
    shard is short; constants are read by global id, state by local index),
    positions exchanged by device copies: 120 steps bit-identical to one
    World and to the oracle, the last step's contact lists equal."""
    import torch
    from rbhip.shard import wrap_gpos, wrap_gquat
    _setenv(monkeypatch, {})
    r = _ragged_reference(oracle)
    sc, P, steps = r["sc"], 3, 120
    with rb.World(sc) as ref:
        ref.step(steps - 1)
        ref.record_contacts(True)
        ref.step(1)
        rq, rv = ref.get_state()
        rc, rp, rk, rd = ref.contacts()
    worlds = [rb.World(sc, rank=k, world_size=P) for k in range(P)]
    assert [w.n_owned for w in worlds] == [358, 358, 357]
    for s in range(steps):
        if s == steps - 1:
            for w in worlds:
                w.record_contacts(True)
        for w in worlds:
            w.shard_step()
        for w in worlds:
            w.sync()
        for wrap in (wrap_gpos, wrap_gquat):
            bufs = [wrap(w, torch) for w in worlds]      # the buffers alternate per step
            n = bufs[0][1]
            if bufs[0][0] is None:                       # sphere worlds: no orientations
                continue
            for k, (buf, _) in enumerate(bufs):
                for o, (obuf, _) in enumerate(bufs):
                    if o != k:
                        buf[o * n:(o + 1) * n].copy_(obuf[o * n:(o + 1) * n])
        torch.cuda.synchronize()
        for w in worlds:
            w.shard_exchange_done()
    q = np.zeros((sc.n, 7))
    v = np.zeros((sc.n, 6))
    cnt, par, kin, dis = [], [], [], []
    for w in worlds:
        w.get_state(q, v)
        c, pa, k, d = w.contacts()
        cnt.append(c); par.append(pa); kin.append(k); dis.append(d)
        w.close()
    _assert_state((q, v), (rq, rv), "shards vs one world")
    _assert_state((q, v), (r["q120"], r["v120"]), "shards vs oracle")
    _assert_contacts((np.concatenate(cnt), np.concatenate(par), np.concatenate(kin), np.concatenate(dis)),
                     (rc, rp, rk, rd), "shards vs one world, step 120")
    assert (rk == 16).sum() > 50 and {-1, -2} <= set(rp[rp < 0].tolist())


# ---------------------------------------------------------------- 4.6 applied forces
@pytest.mark.parametrize("form", ["coop_help", "wide", "wide_plain"])
def test_mixed_scene_applied_forces_and_torques(rb, oracle, monkeypatch, form):
    """rb_set_xfrc on the 1,073-body scene: inv(I_w) @ (torque dt) with
    anisotropic inertia and rotated bodies (collision.py:66-70), 39 steps and
    a recorded one against the oracle."""
    code, env = FORMS[form]
    _setenv(monkeypatch, env)
    sc = _ragged_reference(oracle)["sc"]
    rng = np.random.default_rng(0)
    xf = np.concatenate([rng.normal(0.0, 0.5, (sc.n, 3)), rng.normal(0.0, 2e-3, (sc.n, 3))], axis=1)
    osc = oracle.OracleScene(sc)
    q, v = oracle.step(osc, sc.qpos0, sc.qvel0, 39, xfrc=xf)
    q1, v1, con = oracle.step(osc, q, v, 1, xfrc=xf, record=True)
    qn, _ = oracle.step(osc, sc.qpos0, sc.qvel0, 40)
    assert not _same(q1, qn) and con[0].sum() > 50       # the forces act, and the bodies have landed
    with rb.World(sc) as w:
        w.set_xfrc(xf)
        w.step(39)
        _assert_state(w.get_state(), (q, v), f"{form}: step 39")
        w.record_contacts(True)
        w.step(1)
        _assert_contacts(w.contacts(), con, f"{form}: step 40")
        _assert_state(w.get_state(), (q1, v1), f"{form}: step 40")
        st = w.stats()
    assert st["hashed_form"] == code, st


# ---------------------------------------------------------------- 4.7 batched worlds
@pytest.mark.parametrize("name", ["traj_mixed48", "traj_mixed48_raw"])
def test_mixed_golden_as_batch_template(rb, oracle, name):
    """The 48-body golden as the template of a BatchWorld (M = 48, one
    environment per wave with 16 idle lanes), 5 environments with their own
    restitution and friction: environment 0 keeps the golden's and equals it
    at every snapshot, the others equal the oracle on their own scene."""
    g = load_golden(name)
    sc = golden_scene(g)
    E = 5
    e = np.array([sc.restitution, 0.2, 0.9, 0.45, 1.0])
    mu = np.array([sc.friction, 0.0, 0.7, 0.25, 0.1])
    snaps = list(g["snap_step"])
    with rb.BatchWorld(sc, E) as b:
        b.set_params(restitution=e, friction=mu)
        for si in range(1, len(snaps)):
            assert b.step(int(snaps[si] - snaps[si - 1])) == 0
            gq, gv = b.get_state(envs=[0])
            assert np.array_equal(gq[0], g["qpos"][si]) and np.array_equal(gv[0], g["qvel"][si]), \
                f"{name}: environment 0 differs at step {snaps[si]}"
        aq, av = b.get_state()
    for k in range(1, E):
        osc = oracle.OracleScene(sc.with_(restitution=float(e[k]), friction=float(mu[k])))
        q, v = oracle.step(osc, sc.qpos0, sc.qvel0, int(snaps[-1]))
        assert _same(aq[k], q) and _same(av[k], v), f"{name}: environment {k} differs from the oracle"
        assert not _same(aq[k], aq[0])


def test_bricks_golden_as_one_body_environments(rb):
    """traj_bricks6 as six one-body environments: the template is one box,
    each environment's half extents, mass and inertia set with set_bodies —
    every environment equals its brick's rows of the golden at every
    snapshot (the golden's bricks never come in range of one another)."""
    g = load_golden("traj_bricks6")
    sc = golden_scene(g)
    E = sc.n
    one = sc.with_(kind=sc.kind[:1], mass=sc.mass[:1], inertia=sc.inertia[:1], size=sc.size[:1],
                   qpos0=sc.qpos0[:1], qvel0=sc.qvel0[:1])
    snaps = list(g["snap_step"])
    with rb.BatchWorld(one, E) as b:
        b.set_bodies(mass=sc.mass.reshape(E, 1), inertia=sc.inertia.reshape(E, 1, 3), size=sc.size.reshape(E, 1, 3))
        b.set_state(sc.qpos0.reshape(E, 1, 7), sc.qvel0.reshape(E, 1, 6))
        for si in range(1, len(snaps)):
            assert b.step(int(snaps[si] - snaps[si - 1])) == 0
            gq, gv = b.get_state()
            bad = [k for k in range(E) if not (np.array_equal(gq[k, 0], g["qpos"][si, k]) and
                                               np.array_equal(gv[k, 0], g["qvel"][si, k]))]
            assert not bad, f"bricks {bad} differ from the golden at step {snaps[si]}"
