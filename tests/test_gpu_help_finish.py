"""The wide + helper form with the shared search, whose helper
wave finishes the body: the body wave searches its four buckets, leaves its
hit count and defer flag in LDS and is done at the workgroup's one barrier;
the helper wave merges the two hit lists and runs the solves, the integration,
the insert and the kernel's tail (bounds, halo push, block 0's control words)
from the state it already holds in registers.

Bar: contacts, contact order and state are what the oracle computes, as 64-bit
words.  Every test forces the form at small sizes (the harness of
test_gpu_help_search.py) and checks hashed_form == 4 and help_search == 1."""
import os
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_gpu_help_search import _check_form, _crowded_reference, _form, _half_counts, _same
from test_gpu_shard_mp import _free_port

pytestmark = pytest.mark.gpu

SPHERE_PAIR = 16                                   # contact kind of a sphere-sphere contact; below it: plane contacts
FORM_ENV = {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_HELP": "1", "RBHIP_HELP_SEARCH": "1"}


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _assert_step(w, ref, what):
    cnt, par, kin, dis = ref
    gc, gp, gk, gd = w.contacts()
    assert np.array_equal(gc, cnt), f"contact counts differ at {what}"
    assert np.array_equal(gp, par) and np.array_equal(gk, kin), f"partners / kinds differ at {what}"
    assert _same(gd, dis), f"contact distances differ at {what}"


def _ragged_scene(n):
    """37 bodies: one partial wave in the only workgroup.  65: a second
    workgroup with one active lane, whose 63 idle lanes in both waves must
    reach the barrier.  Spacing 0.19 < 2 r, so neighbours touch."""
    from rbhip import scenes
    sc = scenes.flat_spheres(*{37: (37, 1), 65: (13, 5)}[n], spacing=0.19)
    assert sc.n == n
    return sc


@pytest.mark.parametrize("n", [37, 65])
def test_ragged_workgroups(rb, oracle, monkeypatch, n):
    """60 single recorded steps, each step's lists against the oracle's, then
    60 steps as one graph: state identical after both."""
    _form(monkeypatch)
    sc = _ragged_scene(n)
    osc = oracle.OracleScene(sc)
    q, v = sc.qpos0, sc.qvel0
    pairs = 0
    with rb.World(sc) as w:
        w.record_contacts(True)
        for t in range(60):
            q, v, con = oracle.step(osc, q, v, 1, record=True)
            w.step(1)
            _assert_step(w, con, f"step {t}")
            pairs += int((con[2] == SPHERE_PAIR).sum())
        gq, gv = w.get_state()
        assert _same(gq, q) and _same(gv, v)
        w.record_contacts(False)
        q, v = oracle.step(osc, q, v, 60)
        w.step(60)
        gq, gv = w.get_state()
        st = w.stats()
    _check_form(st)
    assert pairs > 0
    assert _same(gq, q) and _same(gv, v)


def test_applied_forces_on_the_finishing_wave(rb, oracle, monkeypatch):
    """A non-zero force and torque on every body of the 65-body scene: the
    helper skips gravity and the planes before the barrier and applies the
    force, then solves the planes, in its update.  40 recorded steps against
    the oracle's run with the same forces."""
    _form(monkeypatch)
    sc = _ragged_scene(65)
    rng = np.random.default_rng(3)
    xf = np.concatenate([rng.normal(0.0, 0.5, (sc.n, 3)), rng.normal(0.0, 2e-3, (sc.n, 3))], axis=1)
    assert np.abs(xf).min() > 0
    osc = oracle.OracleScene(sc)
    q, v = sc.qpos0, sc.qvel0
    planes = pairs = 0
    with rb.World(sc) as w:
        w.set_xfrc(xf)
        w.record_contacts(True)
        for t in range(40):
            q, v, con = oracle.step(osc, q, v, 1, xfrc=xf, record=True)
            w.step(1)
            _assert_step(w, con, f"step {t}")
            planes += int((con[2] < SPHERE_PAIR).sum())
            pairs += int((con[2] == SPHERE_PAIR).sum())
        gq, gv = w.get_state()
        st = w.stats()
    _check_form(st)
    assert planes > 0 and pairs > 0
    assert _same(gq, q) and _same(gv, v)
    qn, _ = oracle.step(osc, sc.qpos0, sc.qvel0, 40)
    assert not _same(q, qn)                            # the forces act


def _plane_and_both_halves(sc, q_start, cnt, par, kin):
    """Bodies with, in one step's oracle lists, a plane contact and sphere
    partners in both halves of the split."""
    na, nb, _ = _half_counts(sc, q_start, cnt, par, kin)
    body = np.repeat(np.arange(sc.n), cnt)
    npl = np.bincount(body[kin < SPHERE_PAIR], minlength=sc.n)
    return (npl > 0) & (na > 0) & (nb > 0)


def test_record_count_carried_across_the_move(rb, oracle, monkeypatch):
    """The helper's plane contacts are recorded before the barrier, the sphere
    partners of both halves after it, in one list per body: the crowded scene
    of test_gpu_help_search (its reference, computed once), 200 single
    recorded steps.  From the oracle's lists alone, at least 20 body-steps
    have a plane contact and sphere partners in both halves."""
    ref = _crowded_reference(oracle)
    sc = ref["sc"]
    osc = oracle.OracleScene(sc)
    q, v = sc.qpos0, sc.qvel0
    carried = 0
    for cnt, par, kin, dis in ref["steps"]:
        carried += int(_plane_and_both_halves(sc, q, cnt, par, kin).sum())
        q, v = oracle.step(osc, q, v, 1)
    assert _same(q, ref["q"])
    print(f"body-steps with a plane contact and partners in both halves: {carried}")
    assert carried >= 20
    _form(monkeypatch)
    with rb.World(sc) as w:
        w.record_contacts(True)
        for t, con in enumerate(ref["steps"]):
            w.step(1)
            _assert_step(w, con, f"step {t}")
        gq, gv = w.get_state()
        st = w.stats()
    _check_form(st)
    assert _same(gq, ref["q"]) and _same(gv, ref["v"])


def test_max_partners_32_instance(rb, oracle, monkeypatch):
    """The same crowded scene in a world created with max_partners=32 (the
    kernel's other instance: the helper's list starts at row 31; it keeps the
    hand-over to the body wave): 120 graph-replayed steps, then one
    recorded step."""
    _form(monkeypatch)
    sc = _crowded_reference(oracle)["sc"]
    osc = oracle.OracleScene(sc, max_partners=32)
    q0, v0 = oracle.step(osc, sc.qpos0, sc.qvel0, 120)
    q1, v1, con = oracle.step(osc, q0, v0, 1, record=True)
    na, nb, _ = _half_counts(sc, q0, con[0], con[1], con[2])
    assert ((na > 0) & (nb > 0)).sum() > 0
    with rb.World(sc, max_partners=32) as w:
        w.step(120)
        w.record_contacts(True)
        w.step(1)
        _assert_step(w, con, "the recorded step")
        gq, gv = w.get_state()
        st = w.stats()
    _check_form(st)
    assert st["max_partners"] == 32, st
    assert _same(gq, q1) and _same(gv, v1)


# ---------------------------------------------------------------- the tail on the finishing wave
# No other shard or halo test steps this form with the shared search (their
# ranks hold at most 20,480 bodies: the cooperative form), so: two ranks on one
# GPU, 100 bodies each, peer-to-peer exchange with the halo push — the step's
# bound fold, the push and block 0's stores all run on the helper wave.
def _tail_scene():
    from rbhip import scenes
    return scenes.tiled(scenes.flat_spheres, 2, 10, 10, seed=2)


def _tail_worker(rank, P, port, out):
    for pth in (ROOT, PKG):
        sys.path.insert(0, pth)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.update(FORM_ENV)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=P)
    from rbhip.shard import ShardedWorld
    sw = ShardedWorld(_tail_scene(), device=0, transport="p2p", halo=True)
    assert sw.transport == "p2p" and sw.halo
    sw.step(50)
    sw.sync()
    q, v = sw.gather_state()
    st = sw.world.stats()
    print(f"rank {rank}: {st}", flush=True)
    np.save(f"{out}.form{rank}.npy", np.array([st["hashed_form"], st["help_search"]]))
    if rank == 0:
        np.save(out, np.concatenate([q, v], axis=1))
    dist.barrier()
    dist.destroy_process_group()


def test_tail_runs_on_the_finishing_wave(rb, monkeypatch, tmp_path):
    """200 bodies on two halo-exchanging ranks, 50 steps: the gathered state
    is bit-identical to one World of the whole scene, and both ranks stepped
    form 4 with the shared search."""
    import torch.multiprocessing as mp
    _form(monkeypatch)
    sc = _tail_scene()
    assert sc.n == 200
    with rb.World(sc) as w:
        w.step(50)
        q1, v1 = w.get_state()
        _check_form(w.stats())
    out = str(tmp_path / "state.npy")
    mp.start_processes(_tail_worker, args=(2, _free_port(), out), nprocs=2, start_method="spawn")
    for rank in range(2):
        assert np.load(f"{out}.form{rank}.npy").tolist() == [4, 1], f"rank {rank} stepped another form"
    got = np.load(out)
    assert _same(got[:, :7], q1) and _same(got[:, 7:], v1)
