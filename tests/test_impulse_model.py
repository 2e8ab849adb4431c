"""The yardstick of the impulse query (tests/impulse_model.py) against the
oracle's step: the model's velocity after gravity and all contacts equals
oracle.step(..., 1)'s qvel in every word, step after step, in f64 and in f32,
on scenes that reach every branch of the model (applied, separating and
threshold-skipped contacts).  No GPU, and no part of the library: this test
validates the expected values the GPU tests compare against."""
import numpy as np
import pytest

import impulse_model as IM

SCENES = {
    "multi_sphere4": (lambda s: s.multi_sphere4(), 400, 16),
    "single_cube": (lambda s: s.single_cube(), 300, 16),
    "box_pile_1_1_3": (lambda s: s.box_pile(1, 1, 3, seed=1), 250, 32),
    "flat_spheres_3_3": (lambda s: s.flat_spheres(3, 3, spacing=0.19), 150, 16),
    "mixed_spheres_2_2": (lambda s: s.mixed_spheres(2, 2), 200, 32),
}
_seen = {}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(SCENES))
def test_model_velocity_equals_the_oracles_step(oracle, name, dtype):
    from rbhip import scenes
    make, nsteps, maxp = SCENES[name]
    sc = make(scenes)
    osc = oracle.OracleScene(sc, max_partners=maxp)
    cast = (lambda a: a) if dtype == "f64" else (lambda a: a.astype(np.float32).astype(np.float64))
    q, v = cast(np.asarray(sc.qpos0, np.float64)), cast(np.asarray(sc.qvel0, np.float64))
    applied = separating = skipped = records = 0
    bad = []
    for s in range(nsteps):
        m = IM.impulses(sc, q, v, dtype=dtype, max_partners=maxp)
        q, v = oracle.step(osc, q, v, 1, dtype=dtype)
        if not np.array_equal(IM.words(m.vel, dtype), IM.words(v, dtype)):
            bad.append(s)
        applied += m.applied
        separating += m.separating
        skipped += m.skipped
        records += int(m.counts.sum())
    print(f"{name} {dtype}: {records} records, {applied} applied, {separating} separating, {skipped} skipped, "
          f"{len(bad)} mismatching steps")
    assert not bad, bad[:10]
    assert applied > 0
    _seen[(name, dtype)] = (separating, skipped)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_branch_of_the_model_is_reached(dtype):
    """(after the cases above) separating and threshold-skipped contacts occur in at least one scene"""
    got = [v for (name, t), v in _seen.items() if t == dtype]
    assert len(got) == len(SCENES), "run the whole file: this test sums over the scenes above"
    assert sum(s for s, _ in got) > 0 and sum(k for _, k in got) > 0
