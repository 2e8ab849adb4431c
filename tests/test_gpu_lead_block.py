"""The step kernels' lead block (DESIGN §3, §4 "Kernel arguments"): the two
table generations and the two epoch control words in one device allocation,
read with one scalar load by the wide kernels of worlds with append epochs and
through Table::gen by every other step kernel, and written by every prime (world creation, rb_set_state, roll-back and refit
of a guarded chunk, the tile form's retirement) and by block 0 of each step.

Bar: states and contact lists bit-identical (64-bit words) to the oracle's,
whatever the form, the epoch schedule or the sequence of primes.  The forms
are forced at 1,024 bodies (16 or 128 workgroups: block 0 is never alone)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 40


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _same(a, b):
    """Bit identity as 64-bit words (the sign of zeros counts)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _same_contacts(got, ref):
    (gc, gp, gk, gd), (cnt, par, kin, dis) = got, ref
    return np.array_equal(gc, cnt) and np.array_equal(gp, par) and np.array_equal(gk, kin) and _same(gd, dis)


def _forms(monkeypatch, form, epoch, help_search=True):
    """Force one step kernel form on a small world (rb_api_step.hip step_form)."""
    coop, wide, helpmax, wide_help = {
        "wide_help": (0, 1 << 30, 0, 1), "wide": (0, 1 << 30, 0, 0), "coop": (1 << 30, 1 << 30, 0, 0),
        "coop_help": (1 << 30, 1 << 30, 1 << 30, 0), "one": (0, 0, 0, 0)}[form]
    monkeypatch.setenv("RBHIP_COOP_MAX_BODIES", str(coop))
    monkeypatch.setenv("RBHIP_WIDE_MAX_BODIES", str(wide))
    monkeypatch.setenv("RBHIP_HELP_MAX_BODIES", str(helpmax))
    monkeypatch.setenv("RBHIP_WIDE_HELP", str(wide_help))
    monkeypatch.setenv("RBHIP_HELP_SEARCH", "1" if help_search else "0")
    monkeypatch.setenv("RBHIP_TABLE_EPOCH", str(epoch))
    monkeypatch.setenv("RBHIP_TILE", "0")
    return {"one": 0, "coop": 1, "wide": 2, "coop_help": 3, "wide_help": 4}[form]


_ref = {}


def _reference(oracle):
    """flat_spheres(32, 32): the oracle's states (and the contact list of the
    last step) after 3, 7, 40 and 64 steps from t = 0, and after 9, 9 + 16
    steps from the 3-step state.  Computed once, read-only."""
    if not _ref:
        from rbhip import scenes
        sc = scenes.flat_spheres(32, 32)
        osc = oracle.OracleScene(sc)

        def run(q, v, n):
            q, v = oracle.step(osc, q, v, n - 1) if n > 1 else (q, v)
            q, v, con = oracle.step(osc, q, v, 1, record=True)
            for a in (q, v) + tuple(con):
                a.setflags(write=False)
            return q, v, con

        _ref["sc"] = sc
        _ref[3] = run(sc.qpos0, sc.qvel0, 3)
        _ref[7] = run(_ref[3][0], _ref[3][1], 4)
        _ref[40] = run(_ref[7][0], _ref[7][1], 33)
        _ref[64] = run(_ref[40][0], _ref[40][1], 24)
        _ref["3+9"] = run(_ref[3][0], _ref[3][1], 9)
        _ref["3+9+16"] = run(_ref["3+9"][0], _ref["3+9"][1], 16)
    return _ref


def _check(w, ref, what):
    q, v = w.get_state()
    assert _same(q, ref[0]) and _same(v, ref[1]), f"{what}: state differs from the oracle"
    assert _same_contacts(w.contacts(), ref[2]), f"{what}: contact list differs from the oracle"


@pytest.mark.parametrize("form,epoch", [("wide_help", 2), ("wide_help", 8), ("wide", 8)])
def test_epoch_worlds_bit_exact(rb, oracle, monkeypatch, form, epoch):
    """Append and rebuild steps: the control word and the generation of each
    parity come from the lead block.  From t = 0 the start-up epochs of two
    steps put the append steps on even step counts and the rebuild steps on
    odd ones (unless a crowded epoch is cut short); the primes test below
    restarts the schedule on an odd step count, which swaps them.  One
    step(40) graph and 40 single launches."""
    code = _forms(monkeypatch, form, epoch)
    ref = _reference(oracle)
    for mode in ("graph", "single"):
        with rb.World(ref["sc"]) as w:
            w.record_contacts(True)
            if mode == "graph":
                w.step(STEPS)
            else:
                for _ in range(STEPS):
                    w.step_async(1)
                w.sync()
            st = w.stats()
            assert st["hashed_form"] == code and st["table_epoch"] == epoch, st
            if form == "wide_help":
                assert st["help_search"] == 1, st
            assert st["append_steps"] > 0 and st["rebuild_steps"] > 0, st
            assert st["append_steps"] + st["rebuild_steps"] >= STEPS, st
            _check(w, ref[40], f"{form} epoch {epoch} {mode}")


def test_wide_help_without_shared_search_bit_exact(rb, oracle, monkeypatch):
    """The helper-wave form with RBHIP_HELP_SEARCH=0 (the helper only helps):
    another instance of the same lead."""
    code = _forms(monkeypatch, "wide_help", 8, help_search=False)
    ref = _reference(oracle)
    with rb.World(ref["sc"]) as w:
        w.record_contacts(True)
        w.step(STEPS)
        st = w.stats()
        assert st["hashed_form"] == code and st["help_search"] == 0 and st["append_steps"] > 0, st
        _check(w, ref[40], "wide_help, no shared search")


@pytest.mark.parametrize("form", ["coop", "coop_help", "one"])
def test_no_epoch_forms_bit_exact(rb, oracle, monkeypatch, form):
    """Worlds without epochs (RBHIP_TABLE_EPOCH=1) in the cooperative,
    cooperative + helper and one-lane forms: 40 steps read the generation of
    each parity 20 times, written by block 0 of the step before."""
    code = _forms(monkeypatch, form, 1)
    ref = _reference(oracle)
    with rb.World(ref["sc"]) as w:
        w.record_contacts(True)
        for n in (7, STEPS - 7):                  # (two graphs; the second starts at an odd step)
            w.step(n)
        st = w.stats()
        assert st["hashed_form"] == code, st
        assert st["append_steps"] == 0 and st["rebuild_steps"] == 0, st
        _check(w, ref[40], form)


@pytest.mark.parametrize("form,epoch", [("wide_help", 8), ("coop_help", 1)])
def test_primes_leave_the_block_consistent(rb, oracle, monkeypatch, form, epoch):
    """rb_step(7), rb_set_state to a saved state (a prime at an odd step
    count), rb_step(9), then rb_step_async(8) twice and rb_sync: state and
    contact list equal to the oracle's after each segment, and the second
    asynchronous call replays the graph the first one captured."""
    _forms(monkeypatch, form, epoch)
    ref = _reference(oracle)
    with rb.World(ref["sc"]) as w:
        w.record_contacts(True)
        w.step(7)
        _check(w, ref[7], "rb_step(7)")
        w.set_state(ref[3][0], ref[3][1])
        w.step(9)
        _check(w, ref["3+9"], "rb_set_state, rb_step(9)")
        w.step_async(8)
        g1 = w.stats()["graphs"]
        w.step_async(8)
        g2 = w.stats()["graphs"]
        w.sync()
        assert g1 >= 1 and g2 == g1, (g1, g2)
        _check(w, ref["3+9+16"], "rb_step_async(8) x 2")


def test_guarded_chunk_rollback_rewrites_the_block(rb, oracle, monkeypatch):
    """rb_step(64) is a guarded chunk; with an injected bucket overflow it is
    rolled back, the layout refitted, the table re-primed (generation and
    control word rewritten) and the chunk replayed: bit-exact with the run
    without the injection, and with the oracle."""
    _forms(monkeypatch, "wide_help", 8)
    ref = _reference(oracle)
    res = []
    for inject in (1, 0):
        monkeypatch.setenv("RBHIP_DIAG_OVERFLOW", str(inject))
        with rb.World(ref["sc"]) as w:
            w.record_contacts(True)
            w.step(64)
            st = w.stats()
            assert st["refits"] == inject, st
            assert st["append_steps"] > 0, st
            _check(w, ref[64], f"guarded chunk, injection {inject}")
            res.append(w.get_state())
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])


def test_tile_retirement_reprimes_the_block(rb, oracle, monkeypatch):
    """The smallest scene tests/test_gpu_tiles.py retires the tile form on
    (scenes.crowded_cells, 401 bodies, auto mode with the body threshold
    lowered), stepped across the retirement: the hashed forms take over from
    the rolled-back state with a fresh prime.  Bit-exact with the oracle."""
    from rbhip import scenes
    sc = scenes.crowded_cells()
    monkeypatch.setenv("RBHIP_TILE_MIN_BODIES", "1")
    monkeypatch.delenv("RBHIP_TILE", raising=False)
    with rb.World(sc) as w:
        monkeypatch.delenv("RBHIP_TILE_MIN_BODIES")
        for _ in range(3):
            w.step_async(10)
        w.sync()
        w.step(10)
        gq, gv = w.get_state()
        st = w.stats()
    oracle.set_threads(16)
    try:
        q, v = oracle.step(oracle.OracleScene(sc), sc.qpos0, sc.qvel0, 40)
    finally:
        oracle.set_threads(1)
    assert st["tile_rollbacks"] == 1 and st["tile_on"] == 0 and st["form"] != 5, st
    assert _same(gq, q) and _same(gv, v)
