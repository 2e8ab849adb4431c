"""Random call sequences on the device: the op lists of tests/call_sequences.py
played on a World and on its oracle model; every value the calls hand back
must be equal (fp64 as 64-bit words, fp32 against the oracle's f32
restatement, integers equal; no tolerance anywhere).  One case per
(variant, seed); the coverage the seeds reach is asserted on the CPU
(tests/test_call_sequences_model.py)."""
import pytest

import call_sequences as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _play(monkeypatch, oracle, variant, seed, ops=None):
    cfg = cs.WORLD_VARIANTS.get(variant, {"env": {}})
    for k in cs.FORM_ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    ops = cs.generate(variant, seed) if ops is None else ops
    model = cs.make_model(variant, oracle)
    want = cs.run(ops, model)
    dev = cs.make_device(variant)
    try:
        for k in cfg["env"]:
            monkeypatch.delenv(k)
        got = cs.run(ops, dev)
        st = dev.w.stats() if variant in cs.WORLD_VARIANTS else None
    finally:
        dev.close()
    i = cs.first_difference(got, want)
    assert i is None, cs.describe_failure(variant, seed, ops, i, got, want)
    return st, model


@pytest.mark.parametrize("variant,seed", [(v, s) for v in cs.WORLD_VARIANTS for s in range(cs.WORLD_SEEDS)])
def test_world_sequence_matches_the_model(rb, oracle, monkeypatch, variant, seed):
    st, model = _play(monkeypatch, oracle, variant, seed)
    cfg = cs.WORLD_VARIANTS[variant]
    assert st["hashed_form"] == cfg["form"], st
    if "RBHIP_TABLE_EPOCH" in cfg["env"]:
        assert st["table_epoch"] == int(cfg["env"]["RBHIP_TABLE_EPOCH"]), st
    if "RBHIP_TILE" in cfg["env"]:
        assert model.tileable > 0 and st["tile_steps"] > 0, st
    else:
        assert st["tile_steps"] == 0, st


@pytest.mark.parametrize("variant,seed", [(v, s) for v in cs.BATCH_VARIANTS for s in range(cs.BATCH_SEEDS)])
def test_batch_sequence_matches_the_model(rb, oracle, monkeypatch, variant, seed):
    _play(monkeypatch, oracle, variant, seed)


def test_tile_form_reports_a_nonfinite_height(rb, oracle, monkeypatch):
    """Found by ('tile', 5): the tile form binned bodies by x and y and never
    looked at z, so a state with one NaN height stepped on without RB_EDOM (the
    hashed-cell forms test all three coordinates).  The shortest list that
    shows it, with the error reported by the step and by the sync after an
    asynchronous step, and nothing of it left afterwards."""
    ops = [cs.Op("step", (17, 0)),
           cs.Op("set_state_nan", (0, 5)), cs.Op("step", (17, 0)), cs.Op("set_state", ("pool", 1)),
           cs.Op("step", (17, 0)), cs.Op("set_state_nan", (2, 1072)), cs.Op("step_async", (3, 1)), cs.Op("sync", ()),
           cs.Op("set_state", ("pool", 0)), cs.Op("step", (2, 0)), cs.Op("sync", ()), cs.Op("get_state", ())]
    st, model = _play(monkeypatch, oracle, "tile", None, ops)
    # (after a roll-back the next run steps hashed: only the first run commits in the tile form)
    assert st["form"] == 5 and st["tile_steps"] == 17 and st["tile_rollbacks"] == 2, st
