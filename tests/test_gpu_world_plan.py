"""What rb_world_create decides (csrc/rb_worldplan.hpp world_plan) is what the
commit before the plan was factored out decided: for every case below, the
world's stats and rb_query's answers equal the rows recorded at that commit
(tests/golden/world_plan_parent.json).  The switches bring every form within
reach of small scenes; one case steps, so that a table growth's period bump is
pinned too.  tests/test_host_worldplan.py checks the pure function against the
same rows without a GPU."""
import json
import os

import pytest

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "world_plan_parent.json")
SWITCHES = ["RBHIP_COOP_MAX_BODIES", "RBHIP_WIDE_MAX_BODIES", "RBHIP_HELP_MAX_BODIES", "RBHIP_WIDE_HELP",
            "RBHIP_HELP_SEARCH", "RBHIP_TILE", "RBHIP_TILE_MIN_BODIES", "RBHIP_BOX_OPTIMISTIC", "RBHIP_DIAG_OVERFLOW",
            "RBHIP_TABLE_EPOCH", "RBHIP_CONTACT_STAGE_BYTES", "RBHIP_HASH_FACTOR", "RBHIP_HASH_MAX_BYTES",
            "RBHIP_HASH_GROUP", "RBHIP_HASH_PERIOD", "RBHIP_HEADS_PER_LINE", "RBHIP_SPLIT", "RBHIP_FIT_PERIOD"]
STATS = ["buckets", "max_partners", "grid_layout", "hashed_form", "form", "help_search", "table_epoch", "tile_on"]
STEP_STATS = ["refits", "table_grows"]
WIDE = {"RBHIP_COOP_MAX_BODIES": "0"}
ONE = {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_MAX_BODIES": "0"}


def case(id, scene, env=None, dtype="f64", steps=0, **world):
    return dict(id=id, scene=scene, env=dict(env or {}), dtype=dtype, steps=steps, world=world)


S1, S100, S5000 = ["flat_spheres", 1, 1], ["flat_spheres", 10, 10], ["flat_spheres", 100, 50]
CASES = [case(f"spheres{sc[1] * sc[2]}-{dt}", sc, dtype=dt) for sc in (S1, S100, S5000) for dt in ("f64", "f32")]
CASES += [case("wide", S5000, WIDE)]
CASES += [case(f"wide-{k[6:].lower()}={v}", S5000, {**WIDE, k: v}) for k, v in (
    ("RBHIP_HEADS_PER_LINE", "4"), ("RBHIP_HASH_FACTOR", "1"), ("RBHIP_HASH_MAX_BYTES", "4194304"),
    ("RBHIP_HASH_PERIOD", "3:2:1"), ("RBHIP_HASH_PERIOD", "15:15:15"))]
# (the same two with the creation-time split kept: rb_set_state would refit it)
CASES += [case(f"wide-hash_period={v}-kept", S5000, {**WIDE, "RBHIP_HASH_PERIOD": v, "RBHIP_FIT_PERIOD": "0"})
          for v in ("3:2:1", "15:15:15")]
CASES += [case(f"one-heads={r}", S5000, {**ONE, "RBHIP_HEADS_PER_LINE": r}) for r in ("1", "2", "4", "3")]
CASES += [case(f"coop-group={g}", S5000, {"RBHIP_HASH_GROUP": g}) for g in ("2:2:1", "2:2:1:l")]
CASES += [case(f"small-group={g}", S100, {"RBHIP_HASH_GROUP": g}) for g in ("4:4:4", "4:4:4:l")]
CASES += [case("boxes5000", ["incline_cubes", 100, 50]), case("boxes4000", ["incline_cubes", 80, 50])]
CASES += [case("partners32", S100, max_partners=32)]
CASES += [case("rank1of2", ["flat_spheres", 4001, 1], world_size=2, rank=1)]
CASES += [case(f"epoch={e}", S100, {"RBHIP_TABLE_EPOCH": e}) for e in ("0", "100")]
CASES += [case("overflow-diag-steps64", S5000, {**WIDE, "RBHIP_DIAG_OVERFLOW": "2"}, steps=64)]


def observe(c, setenv):
    """the row of case c: its keys, the scene's counts, and what the world answers"""
    import numpy as np
    import rbhip
    from rbhip import scenes

    for k, v in c["env"].items():
        setenv(k, v)
    sc = getattr(scenes, c["scene"][0])(*c["scene"][1:])
    counts = dict(n=sc.n, n_spheres=int(np.sum(sc.kind == 0)), n_planes=int(sc.planes.shape[0]))
    with rbhip.World(sc, device=0, dtype=c["dtype"], **c["world"]) as w:
        if c["steps"]:
            w.step(c["steps"])
        st = w.stats()
        values = {k: st[k] for k in STATS + (STEP_STATS if c["steps"] else [])}
        values.update(n_owned=w.n_owned, bytes_per_body_step=w.bytes_per_body_step)
    return dict(id=c["id"], env=c["env"], scene=c["scene"], dtype=c["dtype"], steps=c["steps"], world=c["world"],
                counts=counts, values=values)


def recorded():
    with open(FIXTURE) as f:
        return {r["id"]: r for r in json.load(f)}


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_world_plan_is_the_parents(c, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    row = recorded()[c["id"]]
    assert observe(c, monkeypatch.setenv) == row
