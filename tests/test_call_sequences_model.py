"""The call-sequence harness on the CPU: the generator, the oracle models and
the coverage the committed seeds reach (tests/call_sequences.py; the device
side is tests/test_gpu_call_sequences.py).

The coverage conditions are asserted, not measured: a variant that misses one
gets more seeds, never an exception."""
import collections

import pytest

import call_sequences as cs

WORLD_CASES = [(v, s) for v in cs.WORLD_VARIANTS for s in range(cs.WORLD_SEEDS)]


def test_generator_is_deterministic():
    """The same (variant, seed) always gives the same ops, whatever was generated before."""
    a = {(v, s): cs.generate(v, s) for v, s in WORLD_CASES[::5]}
    cs._generate_world.cache_clear()
    for (v, s), ops in reversed(list(a.items())):
        assert cs.generate(v, s) == ops, (v, s)
    assert repr(eval(repr([tuple(o) for o in ops]))) == repr([tuple(o) for o in ops])    # prints as a literal


@pytest.mark.parametrize("variant", list(cs.WORLD_VARIANTS))
def test_world_coverage_of_the_committed_seeds(variant):
    kinds = cs.world_kinds(variant)
    count, pairs = collections.Counter(), set()
    for seed in range(cs.WORLD_SEEDS):
        names = [op.name for op in cs.generate(variant, seed)]
        count.update(names)
        pairs |= set(zip(names, names[1:]))
        assert names[-1] == "get_state"
    assert min(count[k] for k in kinds) >= 3, count
    legal = {(a, b) for a in kinds for b in kinds if cs.world_pair_legal(variant, a, b)}
    assert not pairs - legal, sorted(pairs - legal)
    assert not legal - pairs, f"kind pairs never consecutive: {sorted(legal - pairs)}"
    # set_state in its four kinds, the guarded chunk path, both partial reads
    args = collections.Counter((op.name, op.args[0]) for s in range(cs.WORLD_SEEDS) for op in cs.generate(variant, s)
                               if op.args)
    for k in ("same", "moved", "stale", "pool"):
        assert args[("set_state", k)] >= 1, (k, args)
    assert sum(args[("step", k)] + args[("step_async", k)] for k in (64, 70)) >= 1
    assert all(args[("step", k)] + args[("step_async", k)] >= 1 for k in cs.STEP_COUNTS), args
    assert args[("get_part", "qpos")] and args[("get_part", "qvel")]


@pytest.mark.parametrize("variant", list(cs.WORLD_VARIANTS))
def test_world_model_is_cut_independent_and_sequences_touch(oracle, variant):
    """step(k) as k times step(1) hands back the same values (the oracle's cut
    independence, and the model's own bookkeeping); at least half of the
    stepped steps of every sequence see a pair contact and a plane contact;
    every sequence makes at least 10 observations beyond "ok"."""
    unchanged_skips = 0
    for seed in range(cs.WORLD_SEEDS):
        ops = cs.generate(variant, seed)
        whole = cs.run(ops, cs.make_model(variant, oracle))
        m = cs.make_model(variant, oracle, split=True)
        cut = cs.run(ops, m)
        i = cs.first_difference(whole, cut)
        assert i is None, cs.describe_failure(variant, seed, ops, i, whole, cut)
        assert sum(o != ("ok",) for o in whole) >= 10
        both = sum(1 for pair, plane in m.touch if pair and plane)
        assert len(m.touch) > 0 and 2 * both >= len(m.touch), (seed, both, len(m.touch))
        unchanged_skips += m.io[0]
        if variant == "tile":
            assert m.tileable > 0, seed
    assert unchanged_skips >= 1       # "an unchanged rb_set_state uploads nothing" is exercised


def _run_twin(ops, twin):
    """A twin's mistake may leave it a state the oracle refuses (a NaN kept): that is a difference too."""
    obs = []
    for op in ops:
        try:
            obs.append(twin.do(op))
        except RuntimeError:
            obs.append(("raised",))
            break
    return obs


@pytest.mark.parametrize("twin,variants", [("stale_skip", ["mixed_coop", "law_coop_help"]),
                                           ("xfrc_keep", ["mixed_split", "boxes_wide", "law_coop_help"]),
                                           ("param_reuse", ["mixed_one", "f32_flat_wide"])])
def test_a_wrong_world_twin_is_caught(oracle, twin, variants):
    """The harness can fail: a model with one deliberate bookkeeping mistake
    differs from the model on a committed seed of every variant tried."""
    for variant in variants:
        caught = []
        for seed in range(cs.WORLD_SEEDS):
            ops = cs.generate(variant, seed)
            i = cs.first_difference(cs.run(ops, cs.make_model(variant, oracle)),
                                    _run_twin(ops, cs.make_model(variant, oracle, twin=twin)))
            if i is not None:
                caught.append((seed, i))
        assert caught, f"{twin} on {variant}: no committed seed differs"


# ---------------------------------------------------------------- batches
def test_batch_generator_is_deterministic():
    a = {(v, s): cs.generate(v, s) for v in cs.BATCH_VARIANTS for s in (0, cs.BATCH_SEEDS - 1)}
    cs._generate_batch.cache_clear()
    for (v, s), ops in reversed(list(a.items())):
        assert cs.generate(v, s) == ops, (v, s)


@pytest.mark.parametrize("variant", list(cs.BATCH_VARIANTS))
def test_batch_coverage_of_the_committed_seeds(variant):
    kinds = cs.batch_kinds(variant)
    count, pairs, forms = collections.Counter(), set(), collections.Counter()
    for seed in range(cs.BATCH_SEEDS):
        ops = cs.generate(variant, seed)
        names = [op.name for op in ops]
        count.update(names)
        pairs |= set(zip(names, names[1:]))
        forms.update((op.name, op.args[0]) for op in ops if op.args)
        forms.update(("io", op.args[3]) for op in ops if op.name == "set_state" and len(op.args) > 3)
        forms.update(("every", op.args[2]) for op in ops if op.name == "run_sampled")
        assert names[-1] == "get_state" and ops[-1].args == ("all",)
    assert min(count[k] for k in kinds) >= 3, count
    legal = {(a, b) for a in kinds for b in kinds if cs.batch_pair_legal(variant, a, b)}
    assert not pairs - legal, sorted(pairs - legal)
    assert not legal - pairs, f"kind pairs never consecutive: {sorted(legal - pairs)}"
    want = [("set_params", w) for w in ("both", "e", "mu", "none")] + \
           [("set_state", f) for f in ("all", "subset", "dev", "dev_mask")] + [("io", "f64"), ("io", "f32")] + \
           [("get_state", f) for f in ("all", "subset", "dev")] + [("status", "host"), ("status", "dev")] + \
           [("run_sampled", "host"), ("run_sampled", "dev"), ("every", 1), ("every", 7)] + \
           [("set_gravity", True), ("set_gravity", None), ("set_xfrc", None), ("contacts", "host"), ("contacts", "dev")] + \
           [("step", k) for k in cs.BATCH_STEPS]
    if cs.BATCH_VARIANTS[variant].get("start") != "balls":
        want += [("set_planes", True), ("set_planes", None), ("set_xfrc", 0), ("set_xfrc", "zeros"), ("set_xfrc", "dev")]
    else:
        want += [("law", "balls"), ("law", "mujoco")]
    assert not [w for w in want if not forms[w]], [w for w in want if not forms[w]]


@pytest.mark.parametrize("variant", list(cs.BATCH_VARIANTS))
def test_batch_model_is_cut_independent_and_sequences_touch(oracle, variant):
    """As for worlds.  A pair contact is asked of templates with more than one
    body: the one-cube template has no pair to touch (a plane contact is asked
    of it in at least half of the steps)."""
    one_body = cs.BATCH_VARIANTS[variant]["template"] == "cube"
    for seed in range(cs.BATCH_SEEDS):
        ops = cs.generate(variant, seed)
        whole = cs.run(ops, cs.make_model(variant, oracle))
        m = cs.make_model(variant, oracle, split=True)
        cut = cs.run(ops, m)
        i = cs.first_difference(whole, cut)
        assert i is None, cs.describe_failure(variant, seed, ops, i, whole, cut)
        assert sum(o != ("ok",) for o in whole) >= 10
        both = sum(1 for pair, plane in m.touch if (pair or one_body) and plane)
        assert len(m.touch) > 0 and 2 * both >= len(m.touch), (seed, both, len(m.touch))


@pytest.mark.parametrize("twin,variants", [("reset_keeps_status", ["b_multi4", "b_balls16"]),
                                           ("planes_keep", ["b_cube", "b_pile_f32"])])
def test_a_wrong_batch_twin_is_caught(oracle, twin, variants):
    for variant in variants:
        caught = []
        for seed in range(cs.BATCH_SEEDS):
            ops = cs.generate(variant, seed)
            i = cs.first_difference(cs.run(ops, cs.make_model(variant, oracle)),
                                    _run_twin(ops, cs.make_model(variant, oracle, twin=twin)))
            if i is not None:
                caught.append((seed, i))
        assert caught, f"{twin} on {variant}: no committed seed differs"
