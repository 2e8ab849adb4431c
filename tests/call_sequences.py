"""Random call sequences: one op list, two targets.

A seeded generator draws legal sequences of World and of BatchWorld calls;
run() plays the same list on a target made of the library (DeviceWorld,
DeviceBatch) and on a model made of the CPU oracle (ModelWorld, ModelBatch,
written from include/rbhip.h), and every value the calls hand back must be
equal.  What is under test is the host state between two calls (primed
tables, the graph cache, state_version / mirror_version, the error word, the
record and timing switches, the stream; a batch's have_* flags, law,
per-environment status and staging), which decides what the library
enqueues; the arithmetic is the oracle's in both.  DESIGN.md §2.7.

No GPU import at module level: the model, the generator and their CPU tests
(tests/test_call_sequences_model.py) run without a device.

Replaying a failure by hand:

    from call_sequences import *
    obs_d, obs_m = replay("law_coop_help", 2, upto=17)      # needs a GPU
"""
from __future__ import annotations

import functools
import os
from collections import namedtuple

import numpy as np

EINVAL, EDOM, EUNSUPPORTED = -22, -33, -95

# An op is a name and literal arguments; arrays are referred to by pool index
# or by role ("same": the arrays the last get_state handed out), so a list of
# ops prints as a Python literal.
Op = namedtuple("Op", "name args")

# The switches of FORMS in tests/test_gpu_mixed.py: (hashed_form, environment).
FORMS = {
    "coop": (1, {"RBHIP_HELP_MAX_BODIES": "0"}),
    "coop_help": (3, {"RBHIP_HELP_MAX_BODIES": "100000"}),
    "wide": (4, {"RBHIP_COOP_MAX_BODIES": "0"}),
    "wide_plain": (2, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_HELP": "0"}),
    "one": (0, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_MAX_BODIES": "0"}),
    "split": (0, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_MAX_BODIES": "0", "RBHIP_SPLIT": "1"}),
}
FORM_ENV_KEYS = ("RBHIP_COOP_MAX_BODIES", "RBHIP_WIDE_MAX_BODIES", "RBHIP_HELP_MAX_BODIES", "RBHIP_WIDE_HELP",
                 "RBHIP_SPLIT", "RBHIP_TABLE_EPOCH", "RBHIP_TILE")


def _variant(scene, form, dtype="f64", **env):
    code, e = FORMS[form]
    return dict(scene=scene, form=code, dtype=dtype, env=dict(e, **env), law=scene == "flat",
                max_partners=32 if scene == "boxes" else 16)


WORLD_VARIANTS = {
    **{f"mixed_{f}": _variant("mixed", f) for f in FORMS},
    "law_coop_help": _variant("flat", "coop_help"),
    "law_wide_epoch16": _variant("flat", "wide", RBHIP_TABLE_EPOCH="16"),
    "tile": _variant("flat", "coop_help", RBHIP_TILE="1"),
    "boxes_coop": _variant("boxes", "coop"),
    "boxes_wide": _variant("boxes", "wide"),
    "f32_mixed_coop_help": _variant("mixed", "coop_help", dtype="f32"),
    "f32_flat_wide": _variant("flat", "wide", dtype="f32"),
}
WORLD_SEEDS = 7          # sequences per variant (the coverage conditions decide: test_call_sequences_model.py)
WORLD_OPS = 44           # ops per sequence before the closing stats + get_state

STEP_COUNTS = (1, 2, 3, 17, 64, 70)      # 64 and above: the guarded chunks; 2 and above can tile
STEP_WEIGHTS = (0.24, 0.2, 0.2, 0.2, 0.08, 0.08)
POISON_STEP_COUNTS = (1, 3, 17)
TOLS = (0.01, 0.02)

WORLD_KINDS = ("step", "step_async", "sync", "get_state", "get_part", "set_state", "set_state_nan", "set_xfrc",
               "record", "contacts", "law", "stream", "timing", "stats", "refused")


def world_kinds(variant):
    return tuple(k for k in WORLD_KINDS if k != "law" or WORLD_VARIANTS[variant]["law"])


def world_pair_legal(variant, a, b):
    """May an op of kind b directly follow one of kind a (in some state)?
    After a NaN state only a step may follow (it, or the sync after an
    asynchronous one, reports EDOM); contacts() names the most recent
    recorded step, which the record switch and a law switch leave open."""
    kinds = world_kinds(variant)
    if a not in kinds or b not in kinds:
        return False
    if a == "set_state_nan":
        return b in ("step", "step_async")
    if b == "contacts":
        return a not in ("record", "law")
    return True


# ---------------------------------------------------------------- scenes and pools
@functools.lru_cache(maxsize=None)
def world_fixture(scene):
    """(scene, pool of four oracle states taken once bodies touch, two force
    arrays).  The pool states come from the scene's own run under the
    oracle, so none overflows a partner list by the oracle's own check."""
    from oracle import oracle as O
    from rbhip import scenes
    if scene == "mixed":
        sc, at, mp = scenes.mixed_spheres(37, 29, seed=3), (120, 135, 150, 165), 16
    elif scene == "flat":
        sc, at, mp = scenes.flat_spheres(37, 29, seed=3, spacing=0.19), (120, 135, 150, 165), 16
    else:
        sc, at, mp = scenes.box_pile(6, 6, 3, seed=0), (60, 80, 100, 120), 32       # 108 cubes + 12 spheres
    osc = O.OracleScene(sc, max_partners=mp)
    pool, q, v, t = [], sc.qpos0, sc.qvel0, 0
    for s in at:
        q, v = O.step(osc, q, v, s - t)
        t = s
        q.setflags(write=False)
        v.setflags(write=False)
        pool.append((q, v))
    rng = np.random.default_rng(11)
    xf = [rng.normal(0.0, 0.5, (sc.n, 6)) * sc.mass[:, None], rng.normal(0.0, 0.2, (sc.n, 6)) * sc.mass[:, None]]
    for a in xf:
        a.setflags(write=False)
    return sc.with_(qpos0=pool[0][0], qvel0=pool[0][1]), pool, xf


def step_params(sc, p):
    """The scene's parameters, or an alternate that differs from them in one
    of (dt, e, mu, thr) alone: graph keys recur and alternate, and a key
    that forgot one component replays the wrong graph."""
    par = [sc.dt, sc.restitution, sc.friction, sc.threshold]
    if p:
        par[p - 1] = (sc.dt * 0.5, 0.5 * sc.restitution + 0.05, sc.friction + 0.25, sc.threshold + 2e-4)[p - 1]
    return tuple(par)


N_STEP_PARAMS = 5
STEP_PARAM_WEIGHTS = (0.36, 0.16, 0.16, 0.16, 0.16)


def resolve_state(ref, pool, handed):
    kind = ref[0]
    if kind == "pool":
        return pool[ref[1]]
    if kind == "nan":
        q = pool[ref[1]][0].copy()
        q[ref[2], 2] = np.nan
        return q, pool[ref[1]][1]
    q, v = handed
    if kind == "moved":
        q = q.copy()
        q[ref[1], 0] += ref[2]
    return q, v


def resolve_xfrc(ref, xf):
    return None if ref is None else np.zeros_like(xf[0]) if ref == "zeros" else xf[ref]


# ---------------------------------------------------------------- the model
class ModelWorld:
    """A World as include/rbhip.h describes it, on the CPU oracle.

    dry: no arithmetic (the generator's legality state).  split: every
    step(k) as k times step(1), each recorded, with per-step contact
    statistics in self.touch (pair contact, plane contact).  twin: a
    deliberately wrong model ("stale_skip", "xfrc_keep", "param_reuse")."""

    def __init__(self, variant, oracle=None, dry=False, split=False, twin=None):
        self.cfg = WORLD_VARIANTS[variant]
        self.O, self.dry, self.split, self.twin = oracle, dry, split, twin
        self.dtype = self.cfg["dtype"]
        if dry:
            self.sc = self.pool = self.xf = self.osc = None
        else:
            self.sc, self.pool, self.xf = world_fixture(self.cfg["scene"])
            self.osc = oracle.OracleScene(self.sc, max_partners=self.cfg["max_partners"])
        self.q = self.v = None
        self.xfrc = None
        self.law, self.tol = "mujoco", 0.01
        self.record, self.last_record = False, None
        self.mirror = None            # the bytes an unchanged rb_set_state may skip
        self.handed = None
        self.have_handed = self.stepped_since_handed = False
        self.io = [0, 0]
        self.timing, self.t_n = False, 0
        self.poison = 0               # 1: NaN state set; 2: stepped asynchronously; 3: reported
        self.stream = "own"
        self.first_params = {}
        self.touch = []
        self.tileable = 0             # steps the tile form may take (runs of >= 2 steps, rb_api_tiles.hip)
        self.xfrc_cleared = 0         # 1: forces cleared after being set; 2: and stepped since
        self._set_state(("pool", 0))  # (World.__init__ uploads the scene's state)

    # -- what may follow
    def legal_kinds(self):
        if self.poison == 1:
            return ["step", "step_async"]
        if self.poison == 2:
            return ["sync"]
        if self.poison == 3:
            return ["set_state"]
        out = ["step", "step_async", "sync", "get_state", "get_part", "set_state", "set_state_nan", "record", "stream",
               "timing", "stats", "refused", "set_xfrc"]
        if self.record and self.last_record is not None:
            out.append("contacts")
        if self.cfg["law"]:
            out.append("law")
        return out

    # -- helpers
    def _round(self, a):
        return a.astype(np.float32).astype(np.float64) if self.dtype == "f32" else np.array(a, np.float64)

    def _set_state(self, ref):
        if self.dry:
            same = ref[0] == "same"
            self.io[0 if same else 1] += 1
            return
        q, v = resolve_state(ref, self.pool, self.handed)
        if self.twin == "stale_skip" and self.handed is not None and \
                q.tobytes() == self.handed[0].tobytes() and v.tobytes() == self.handed[1].tobytes():
            self.io[0] += 1
            return
        if self.mirror is not None and q.tobytes() == self.mirror[0] and v.tobytes() == self.mirror[1]:
            self.io[0] += 1           # rb_set_state: the bytes handed out, handed back unchanged
            return
        self.io[1] += 1
        self.q, self.v = self._round(q), self._round(v)
        self.mirror = (q.tobytes(), v.tobytes())

    def _advance(self, k, p):
        dt, e, mu, thr = step_params(self.sc, p)
        chunks = [1] * k if self.split else ([k - 1, 1] if self.record and k > 1 else [k])
        for n in chunks:
            rec = self.split or (self.record and n == 1)
            if self.law == "balls":
                if self.split:
                    r = self.sc.size[:, 0]
                    ground = bool((self.q[:, 2] < r).any())
                out = self.O.pair_step(self.osc, self.q, self.v, n, dt=dt, restitution=e, friction=mu, tol=self.tol,
                                       dtype=self.dtype, record=rec)
                if self.split:
                    self.touch.append((bool(out[2][0].sum() > 0), ground))
            else:
                out = self.O.step(self.osc, self.q, self.v, n, dt=dt, restitution=e, friction=mu, threshold=thr,
                                  dtype=self.dtype, xfrc=self.xfrc, record=rec)
                if self.split:
                    par = out[2][1]
                    self.touch.append((bool((par >= 0).any()), bool((par < 0).any())))
            self.q, self.v = out[0], out[1]
            if rec and self.record:
                self.last_record = out[2]

    # -- the calls
    def do(self, op):
        name, a = op.name, op.args
        assert name in self.legal_kinds(), f"illegal op {op!r} (legal: {self.legal_kinds()})"
        return getattr(self, "_op_" + name)(*a)

    def _op_step(self, k, p, sync=True):
        if self.twin == "param_reuse":
            p = self.first_params.setdefault(k, p)
        self.mirror = None
        self.stepped_since_handed = True
        if self.timing:
            self.t_n += k
        if self.poison:
            self.poison = 3 if sync else 2
            self.last_record = None       # (the failed step wrote the record buffers)
            return ("err", EDOM) if sync else ("ok",)
        if self.xfrc_cleared == 1 and self.law == "mujoco" and not self.poison:
            self.xfrc_cleared = 2
        if k >= 2 and self.law == "mujoco" and self.xfrc is None and not self.timing and not self.record:
            self.tileable += k
        if not self.dry:
            self._advance(k, p)
        elif self.record:
            self.last_record = True
        return ("ok",)

    def _op_step_async(self, k, p):
        return self._op_step(k, p, sync=False)

    def _op_sync(self):
        if self.poison == 2:
            self.poison = 3
            return ("err", EDOM)
        return ("ok",)

    def _op_get_state(self):
        self.have_handed, self.stepped_since_handed = True, False
        if self.dry:
            return None
        self.handed = (self.q.copy(), self.v.copy())
        self.mirror = (self.handed[0].tobytes(), self.handed[1].tobytes())
        return ("state", self.handed[0], self.handed[1])

    def _op_get_part(self, which):
        self.mirror = None            # rb_get_state with one array: the staging no longer mirrors the state
        if self.dry:
            return None
        return (which, (self.q if which == "qpos" else self.v).copy())

    def _op_set_state(self, *ref):
        self._set_state(ref)
        if ref[0] in ("pool", "moved"):
            self.stepped_since_handed = True      # (the handed-out arrays are no longer the state)
        self.poison = 0
        return ("ok",)

    def _op_set_state_nan(self, i, body):
        self._set_state(("nan", i, body))
        self.poison = 1
        return ("ok",)

    def _op_set_xfrc(self, ref):
        if ref is None and self.twin == "xfrc_keep":
            return ("ok",)
        if ref is None and self.xfrc is not None and self.xfrc_cleared == 0:
            self.xfrc_cleared = 1
        self.xfrc = ref if self.dry else resolve_xfrc(ref, self.xf)
        return ("ok",)

    def _op_record(self, on):
        self.record, self.last_record = bool(on), None
        return ("ok",)

    def _op_contacts(self):
        if self.dry:
            return None
        r = self.last_record
        return ("contacts",) + tuple(r[:2] if self.law == "balls" else r)

    def _op_law(self, law, tol):
        self.law, self.tol = law, tol
        self.mirror, self.last_record = None, None
        self.stepped_since_handed = True      # (state_version moves: the handed-out arrays upload again)
        return ("ok",)

    def _op_stream(self, which):
        self.stream = which
        return ("ok",)

    def _op_timing(self, on):
        n = self.t_n
        if on and not self.timing:
            self.t_n = 0
        self.timing = bool(on)
        return ("timing", n)

    def _op_stats(self):
        return ("stats", self.io[0], self.io[1], self.cfg["max_partners"])

    def _op_refused(self, what):
        return ("err", EUNSUPPORTED if what == "law" else EINVAL)

    def close(self):
        pass


# ---------------------------------------------------------------- the device
class DeviceWorld:
    """The same calls on rbhip.World.  The caller has set the variant's
    environment (RBHIP_*) before this is built."""

    def __init__(self, variant):
        import rbhip
        self.rb = rbhip
        self.cfg = WORLD_VARIANTS[variant]
        self.sc, self.pool, self.xf = world_fixture(self.cfg["scene"])
        self.w = rbhip.World(self.sc, dtype=self.cfg["dtype"], max_partners=self.cfg["max_partners"])
        self.handed = None
        self.torch_stream = None

    def _call(self, fn, *a, **kw):
        try:
            fn(*a, **kw)
        except self.rb.RbError as exc:
            return ("err", exc.code)
        return ("ok",)

    def do(self, op):
        return getattr(self, "_op_" + op.name)(*op.args)

    def _kw(self, p):
        dt, e, mu, thr = step_params(self.sc, p)
        return dict(dt=dt, restitution=e, friction=mu, threshold=thr)

    def _op_step(self, k, p):
        return self._call(self.w.step, k, **self._kw(p))

    def _op_step_async(self, k, p):
        return self._call(self.w.step_async, k, **self._kw(p))

    def _op_sync(self):
        return self._call(self.w.sync)

    def _op_get_state(self):
        self.handed = self.w.get_state()
        return ("state", self.handed[0].copy(), self.handed[1].copy())

    def _op_get_part(self, which):
        from rbhip import _lib
        a = np.zeros((self.sc.n, 7 if which == "qpos" else 6))
        args = (_lib.ptr(a), None) if which == "qpos" else (None, _lib.ptr(a))
        _lib.check(self.w._L.rb_get_state(self.w._h, *args), "rb_get_state")
        return (which, a)

    def _op_set_state(self, *ref):
        return self._call(self.w.set_state, *resolve_state(ref, self.pool, self.handed))

    def _op_set_state_nan(self, i, body):
        return self._call(self.w.set_state, *resolve_state(("nan", i, body), self.pool, None))

    def _op_set_xfrc(self, ref):
        return self._call(self.w.set_xfrc, resolve_xfrc(ref, self.xf))

    def _op_record(self, on):
        return self._call(self.w.record_contacts, on)

    def _op_contacts(self):
        c = self.w.contacts()
        return ("contacts",) + tuple(c[:2] if self.w.law == "balls" else c)

    def _op_law(self, law, tol):
        return self._call(self.w.set_contact_law, law, tol)

    def _op_stream(self, which):
        if which == "torch":
            import torch
            if self.torch_stream is None:
                self.torch_stream = torch.cuda.Stream()
            return self._call(self.w.set_stream, self.torch_stream.cuda_stream)
        return self._call(self.w.set_stream, 0)

    def _op_timing(self, on):
        return ("timing", self.w.kernel_timing(on)[1])

    def _op_stats(self):
        st = self.w.stats()
        return ("stats", st["io_skipped"], st["io_uploads"], st["max_partners"])

    def _op_refused(self, what):
        if what == "nsteps":
            return self._call(self.w.step, -1)
        if what == "async_nsteps":
            return self._call(self.w.step_async, -3)
        if what == "dt0":
            return self._call(self.w.step, 3, dt=0.0)
        if what == "dtneg":
            return self._call(self.w.step, 17, dt=-0.01)
        return self._call(self.w.set_contact_law, "balls", 0.01)

    def close(self):
        self.w.close()


# ---------------------------------------------------------------- the generator
def _world_candidate(kind, m, rng, cfg, n_bodies, spheres, used):
    """One op of `kind` with drawn arguments, legal in model state m; a first
    argument the variant's seeds have not used yet goes first."""
    def pick(options, p=None):
        new = [o for o in options if (kind, o) not in used]
        o = new[0] if new else options[int(rng.choice(len(options), p=p))]
        used.add((kind, o))
        return o
    if kind in ("step", "step_async"):
        k = pick(POISON_STEP_COUNTS) if m.poison else pick(STEP_COUNTS, STEP_WEIGHTS)
        return Op(kind, (k, int(rng.choice(N_STEP_PARAMS, p=STEP_PARAM_WEIGHTS))))
    if kind in ("sync", "get_state", "contacts", "stats"):
        return Op(kind, ())
    if kind == "get_part":
        return Op(kind, (pick(("qpos", "qvel")),))
    if kind == "set_state":
        forms = ["pool"]
        if m.have_handed and m.poison == 0:
            forms += ["moved"] + ["stale" if m.stepped_since_handed else "same"] * 3
        f = pick(forms)
        if f == "pool":
            return Op(kind, ("pool", int(rng.integers(0, 4))))
        if f == "moved":
            return Op(kind, ("moved", int(rng.integers(0, n_bodies)), 0.01))
        return Op(kind, (f,))
    if kind == "set_state_nan":
        return Op(kind, (int(rng.integers(0, 4)), int(spheres[int(rng.integers(0, len(spheres)))])))
    if kind == "set_xfrc":
        if m.law == "balls":
            return Op(kind, (None,))
        # forces set: mostly cleared next, so that "none" is stepped after "some"
        return Op(kind, (pick((0, 1, "zeros", None), (0.3, 0.3, 0.2, 0.2) if m.xfrc is None else (0.1, 0.1, 0.1, 0.7)),))
    if kind == "record":
        return Op(kind, (bool(rng.random() < 0.75) if m.record else True,))
    if kind == "law":
        if m.law == "mujoco" and m.xfrc is None:
            return Op(kind, ("balls", TOLS[int(rng.integers(0, 2))]))
        return Op(kind, ("mujoco", 0.01))
    if kind == "stream":
        return Op(kind, ("torch" if m.stream != "torch" else "null",))
    if kind == "timing":
        return Op(kind, (not m.timing,))
    if kind == "refused":
        what = ["nsteps", "async_nsteps", "dt0", "dtneg"] + ([] if cfg["law"] else ["law", "law"])
        return Op(kind, (pick(what),))
    raise KeyError(kind)


def _scene_bodies(scene):
    """(body count, ids of the sphere bodies) without building the scene's pool."""
    if scene == "boxes":
        from rbhip import scenes
        kind = scenes.box_pile(6, 6, 3, seed=0).kind
        return int(kind.size), np.flatnonzero(kind == 0)
    return 37 * 29, np.arange(37 * 29)


def _greedy_sequences(variant, vi, nseeds, kinds, pair_legal, new_model, candidate, n_ops, busy, closers,
                      steer=None, finish=None):
    """Seeds 0 .. nseeds-1 of a variant, in order.  Greedy: the next op prefers
    an ordered pair (previous kind, this kind) no seed of the variant has had
    yet, and among those the kind out of which most pairs are still open.
    Legal by construction: the dry model's state says what may follow."""
    seen, used, out = set(), set(), []
    for seed in range(nseeds):
        rng = np.random.default_rng([vi, seed])
        m = new_model()
        ops, prev = [], None
        while len(ops) < n_ops or busy(m):
            legal = [k for k in m.legal_kinds() if k in kinds]
            if len(ops) >= n_ops:                           # wrap up: only what ends an open episode
                legal = [k for k in legal if k not in ("set_state_nan", "poison")]
            fresh = [k for k in legal if prev is not None and (prev, k) not in seen]

            def gain(k):        # pairs still open out of k: prefer the kind that leads somewhere new
                return sum(1 for b in kinds if pair_legal(k, b) and (k, b) not in seen)
            pick_from = fresh or legal
            best = max(gain(k) for k in pick_from)
            pick_from = [k for k in pick_from if gain(k) == best] if fresh or best > 0 else pick_from
            kind = pick_from[int(rng.integers(0, len(pick_from)))]
            if steer is not None and not fresh and len(ops) < n_ops:
                kind = steer(m, legal, seen) or kind
            op = candidate(kind, m, rng, used)
            m.do(op)
            if prev is not None:
                seen.add((prev, kind))
            ops.append(op)
            prev = kind
        if finish is not None:
            for op in finish(m):
                m.do(op)
                ops.append(op)
        ops += closers
        out.append(tuple(ops))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _generate_world(variant, nseeds):
    cfg = WORLD_VARIANTS[variant]
    kinds = world_kinds(variant)
    n_bodies, spheres = _scene_bodies(cfg["scene"])
    open_pairs = [(a, b) for a in kinds for b in kinds if "contacts" in (a, b) and world_pair_legal(variant, a, b)]

    def steer(m, legal, seen):      # towards a state in which contacts() is legal
        if m.poison == 0 and "contacts" not in legal and any(pr not in seen for pr in open_pairs):
            return "step" if m.record else "record"
        return None

    def finish(m):
        ops = []
        if m.xfrc_cleared < 2:          # every sequence steps with forces and then without them
            ops += ([Op("law", ("mujoco", 0.01))] if m.law == "balls" else []) + \
                   [Op("set_xfrc", (0,)), Op("step", (2, 0)), Op("set_xfrc", (None,)), Op("step", (2, 0))]
        if "RBHIP_TILE" in cfg["env"] and m.tileable == 0:      # the tile form gets at least one run
            ops += [Op("set_xfrc", (None,)), Op("timing", (False,)), Op("record", (False,)),
                    Op("law", ("mujoco", 0.01)), Op("step", (17, 0))]
        return ops

    return _greedy_sequences(
        variant, list(WORLD_VARIANTS).index(variant), nseeds, kinds, lambda a, b: world_pair_legal(variant, a, b),
        lambda: ModelWorld(variant, dry=True),
        lambda kind, m, rng, used: _world_candidate(kind, m, rng, cfg, n_bodies, spheres, used),
        WORLD_OPS, lambda m: m.poison != 0, [Op("sync", ()), Op("stats", ()), Op("get_state", ())], steer, finish)


# ================================================================ batches
# A batch is E environments of M bodies; the model holds one scene per
# environment and steps each with the oracle on its own scene.
BATCH_VARIANTS = {
    "b_multi4": dict(template="multi4", E=37, dtype="f64", law=False),
    "b_multi4_f32": dict(template="multi4", E=37, dtype="f32", law=False),
    "b_cube": dict(template="cube", E=37, dtype="f64", law=False),
    "b_pile": dict(template="pile", E=37, dtype="f64", law=False),
    "b_pile_f32": dict(template="pile", E=37, dtype="f32", law=False),
    "b_balls16": dict(template="balls", E=37, dtype="f64", law=True, start="balls"),
    "b_mixed64": dict(template="mixed64", E=5, dtype="f64", law=False),
}
BATCH_SEEDS = 8
BATCH_OPS = 46
BATCH_STEPS = (1, 3, 40, 300)            # 300 crosses RB_BATCH_CHUNK (256)
BATCH_STEP_WEIGHTS = (0.35, 0.35, 0.22, 0.08)
BATCH_KINDS = ("set_params", "set_bodies", "set_planes", "set_gravity", "set_xfrc", "set_state", "get_state", "step",
               "step_async", "sync", "run_sampled", "contacts", "status", "law", "stream", "poison", "refused")


def batch_kinds(variant):
    return tuple(k for k in BATCH_KINDS if k != "law" or BATCH_VARIANTS[variant]["law"])


def batch_pair_legal(variant, a, b):
    """Every call of a batch may follow every other: a failed environment
    freezes alone and the rest of the batch goes on."""
    kinds = batch_kinds(variant)
    if (a, b) == ("poison", "contacts"):      # the query of a NaN state not yet marked failed by a step: left open
        return False
    return a in kinds and b in kinds


@functools.lru_cache(maxsize=None)
def batch_fixture(template, E):
    """The template scene, three pools of per-environment states taken from
    oracle runs once bodies touch, and the per-environment constants the ops
    refer to by index."""
    from oracle import oracle as O
    from rbhip import scenes
    rng = np.random.default_rng(5150)
    balls = False
    if template == "multi4":
        # the four balls in a bowl of four planes (tilt 0.2 rad), so that they roll together and stay in
        # touch; e 0.5, mu 0.3 so that they settle
        a = 0.2
        bowl = np.array([[np.sin(a), 0, np.cos(a), 0, 0, 0], [-np.sin(a), 0, np.cos(a), 0, 0, 0],
                         [0, np.sin(a), np.cos(a), 0, 0, 0], [0, -np.sin(a), np.cos(a), 0, 0, 0]], np.float64)
        sc = scenes.multi_sphere4().with_(threshold=1e-4, restitution=0.5, friction=0.3, planes=bowl)
        q = np.zeros((E, 4, 7))
        q[:, :, 0:2] = np.sign(sc.qpos0[:, 0:2]) * 0.095 + rng.uniform(-0.01, 0.01, (E, 4, 2))
        q[:, :, 2] = 0.3 + 0.2 * rng.uniform(0.0, 1.0, (E, 4))
        q[:, :, 3] = 1.0
        v = np.concatenate([rng.normal(0.0, 0.3, (E, 4, 3)), rng.normal(0.0, 1.0, (E, 4, 3))], axis=2)
        at = (60, 90, 120)
    elif template == "cube":
        sc = scenes.cube_incline()
        q = np.broadcast_to(sc.qpos0, (E, 1, 7)).copy()
        q[:, 0, 2] += rng.uniform(0.0, 0.05, E)
        v = np.concatenate([np.zeros((E, 1, 3)), rng.normal(0.0, 0.3, (E, 1, 3))], axis=2)
        at = (20, 40, 60)
    elif template == "pile":
        scs = [scenes.box_pile(1, 1, 3, seed=k) for k in range(E)]
        sc = scs[0]
        q, v = np.stack([x.qpos0 for x in scs]), np.stack([x.qvel0 for x in scs])
        at = (40, 70, 100)
    elif template == "balls":
        scs = [scenes.balls_pile(4, 4, seed=k, spacing=0.19) for k in range(E)]
        sc, balls = scs[0].with_(restitution=0.1), True       # (nearly inelastic: the cluster does not bounce apart)
        # a tight cluster that stays one: hardly any sideways velocity, and (below) no sideways gravity;
        # without walls a pile thrown apart never touches again
        q, v = np.stack([x.qpos0 for x in scs]), np.stack([x.qvel0 for x in scs]) * 0.05
        at = (60, 80, 100)
    else:
        sc = scenes.mixed_spheres(8, 8, seed=0)
        scs = [scenes.mixed_spheres(8, 8, seed=k) for k in range(E)]
        q, v = np.stack([x.qpos0 for x in scs]), np.stack([x.qvel0 for x in scs])
        at = (100, 120, 140)
    M = sc.n
    osc = O.OracleScene(sc, max_partners=32)
    pool, t = [], 0
    for s in at:
        for k in range(E):
            q[k], v[k] = (O.pair_step(osc, q[k], v[k], s - t) if balls else O.step(osc, q[k], v[k], s - t))
        t = s
        pool.append((q.copy(), v.copy()))
    P = sc.planes.shape[0]
    planes = np.broadcast_to(sc.planes, (E, P, 6)).copy()
    if P:
        planes[:, :, 0:2] += rng.uniform(-0.05, 0.05, (E, P, 2))
        planes[:, :, 0:3] /= np.linalg.norm(planes[:, :, 0:3], axis=2)[:, :, None]
    mass, inertia, size = (np.broadcast_to(a, (E,) + a.shape).copy() for a in (sc.mass, sc.inertia, sc.size))
    fx = dict(sc=sc, E=E, M=M, pool=pool, e=rng.uniform(0.0, 0.2, E) if balls else rng.uniform(0.2, 1.0, E),
              mu=rng.uniform(0.0, 0.8, E),
              bodies=[(mass, inertia, size),
                      (mass * rng.uniform(0.8, 1.2, (E, M)), inertia * rng.uniform(0.8, 1.2, (E, M, 1)), None),
                      (mass * rng.uniform(0.9, 1.1, (E, M)), inertia.copy(), size * rng.uniform(0.97, 1.0, (E, M, 1)))],
              planes=planes,
              gravity=np.stack([rng.uniform(-0.3, 0.3, E) * (not balls), rng.uniform(-0.3, 0.3, E) * (not balls),
                                -9.8 * rng.uniform(0.8, 1.2, E)], 1),
              xf=[np.concatenate([rng.normal(0.0, 0.2, (E, M, 3)), rng.normal(0.0, 0.01, (E, M, 3))], 2) * sc.mass[:, None]
                  for _ in range(2)])
    for a in [x for pr in pool for x in pr] + [fx["e"], fx["mu"], planes, fx["gravity"]] + fx["xf"] + \
            [x for b in fx["bodies"] for x in b if x is not None]:
        a.setflags(write=False)
    return fx


def batch_step_params(sc, p):
    if p == 0:
        return sc.dt, sc.restitution, sc.friction, sc.threshold
    return sc.dt * 0.5, min(0.5, sc.restitution), 0.7, 2e-4


def batch_state(ref_pool, nan, fx):
    """Pool state i, with a NaN height at (env, body) when nan is given."""
    q, v = fx["pool"][ref_pool]
    if nan is not None:
        q = q.copy()
        q[nan[0], nan[1], 2] = np.nan
    return q, v


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def dense_contacts(lists, M, R):
    """oracle.contacts()' CSR lists of one environment in the dense layout of
    rb_batch_contacts: the first R records of each body, kind -1 and zeros past them."""
    cnt, par, kin, dis, pos, frm = lists
    out = [cnt.astype(np.int32), np.zeros((M, R), np.int32), np.full((M, R), -1, np.int32), np.zeros((M, R)),
           np.zeros((M, R, 3)), np.zeros((M, R, 3))]
    at = 0
    for b in range(M):
        k = min(int(cnt[b]), R)
        for dst, src in zip(out[1:], (par, kin, dis, pos, frm)):
            dst[b, :k] = src[at:at + k]
        at += int(cnt[b])
    return out


class ModelBatch:
    """A BatchWorld as include/rbhip.h describes it.  dry / split / twin as
    ModelWorld; twins: "reset_keeps_status" (a subset set_state does not clear
    code / steps_done), "planes_keep" (set_planes(None) keeps the earlier planes)."""

    def __init__(self, variant, oracle=None, dry=False, split=False, twin=None):
        self.cfg = BATCH_VARIANTS[variant]
        self.O, self.dry, self.split, self.twin = oracle, dry, split, twin
        self.dtype = self.cfg["dtype"]
        self.E = self.cfg["E"]
        self.fx = None if dry else batch_fixture(self.cfg["template"], self.E)
        self.e = self.mu = self.planes = self.gravity = self.xfrc = None
        self.bodies = None
        self.law, self.tol = self.cfg.get("start", "mujoco"), 0.01
        self.stream = "own"
        self.poisoned = set()
        self.pending_nan = False      # a NaN state set and no step since (its environment is not yet failed)
        self.touch = []
        self._osc = {}
        if not dry:
            self.M = self.fx["M"]
            self.bodies = list(self.fx["bodies"][0])
            self.code, self.done = np.zeros(self.E, np.int32), np.zeros(self.E, np.int64)
            self.q, self.v = (self._in(a) for a in self.fx["pool"][0])

    def legal_kinds(self):
        out = ["set_params", "set_bodies", "set_planes", "set_gravity", "set_xfrc", "set_state", "get_state", "step",
               "step_async", "sync", "run_sampled", "status", "stream", "poison", "refused"]
        if self.law == "mujoco" and not self.pending_nan:
            out.append("contacts")
        if self.cfg["law"]:
            out.append("law")
        return out

    def _in(self, a):
        return _f32(a) if self.dtype == "f32" else np.array(a, np.float64)

    def _scene(self, k, p):
        key = (k, p)
        if key not in self._osc:
            sc = self.fx["sc"]
            dt, e, mu, thr = batch_step_params(sc, p)
            kw = dict(restitution=e if self.e is None else float(self.e[k]),
                      friction=mu if self.mu is None else float(self.mu[k]),
                      mass=self.bodies[0][k], inertia=self.bodies[1][k], size=self.bodies[2][k])
            if self.planes is not None:
                kw["planes"] = self.planes[k]
            if self.gravity is not None:
                kw["gravity"] = self.gravity[k]
            self._osc[key] = self.O.OracleScene(sc.with_(**kw), max_partners=32)
        return self._osc[key]

    def _advance(self, n, p):
        sc = self.fx["sc"]
        dt, _, _, thr = batch_step_params(sc, p)
        for steps in ([1] * n if self.split else [n]):
            pair = plane = False
            for k in range(self.E):
                if self.code[k]:
                    continue
                if not np.isfinite(self.q[k, :, 0:3]).all():
                    self.code[k] = EDOM           # frozen at the start state of the failing step
                    continue
                osc = self._scene(k, p)
                kw = dict(dt=dt, restitution=osc.sc.restitution, friction=osc.sc.friction, dtype=self.dtype,
                          record=self.split)
                if self.law == "balls":
                    if self.split:
                        plane |= bool((self.q[k, :, 2] < osc.sc.size[:, 0]).any())
                    out = self.O.pair_step(osc, self.q[k], self.v[k], steps, tol=self.tol, **kw)
                    pair |= self.split and bool(out[2][0].sum() > 0)
                else:
                    out = self.O.step(osc, self.q[k], self.v[k], steps, threshold=thr,
                                      xfrc=None if self.xfrc is None else self.xfrc[k], **kw)
                    if self.split:
                        pair |= bool((out[2][1] >= 0).any())
                        plane |= bool((out[2][1] < 0).any())
                self.q[k], self.v[k] = out[0], out[1]
                self.done[k] += steps
            if self.split:
                self.touch.append((pair, plane))
        return int((self.code != 0).sum())

    def _failed(self):
        return int((self.code != 0).sum())

    def do(self, op):
        assert op.name in self.legal_kinds(), f"illegal op {op!r}"
        if op.name == "poison":
            self.pending_nan = True
        elif op.name in ("step", "step_async", "run_sampled"):
            self.pending_nan = False
        elif op.name == "set_state" and not self.poisoned - (set(range(self.E)) if op.args[2] is None else set(op.args[2])):
            self.pending_nan = False
        if self.dry:
            return self._dry(op)
        return getattr(self, "_op_" + op.name)(*op.args)

    def _dry(self, op):
        name, a = op.name, op.args
        if name == "law":
            self.law = a[0]
        elif name == "set_planes":
            self.planes = a[0]
        elif name == "set_xfrc":
            self.xfrc = a[1] if a[0] == "dev" else a[0]
        elif name == "stream":
            self.stream = a[0]
        elif name == "poison":
            self.poisoned.add(a[0])
        elif name == "set_state":
            self.poisoned -= set(range(self.E)) if a[2] is None else set(a[2])
        return None

    # -- constants
    def _op_set_params(self, which):
        self.e = self.fx["e"] if which in ("both", "e") else None
        self.mu = self.fx["mu"] if which in ("both", "mu") else None
        self._osc.clear()
        return ("ok",)

    def _op_set_bodies(self, i):
        for j, a in enumerate(self.fx["bodies"][i]):
            if a is not None:
                self.bodies[j] = a
        self._osc.clear()
        return ("ok",)

    def _op_set_planes(self, on):
        if on is None and self.twin == "planes_keep":
            return ("ok",)
        self.planes = self.fx["planes"] if on else None
        self._osc.clear()
        return ("ok",)

    def _op_set_gravity(self, on):
        self.gravity = self.fx["gravity"] if on else None
        self._osc.clear()
        return ("ok",)

    def _op_set_xfrc(self, form, ref=None, io="f64"):
        if form == "dev":
            x = self.fx["xf"][ref]
            self.xfrc = _f32(x) if io == "f32" else x
        else:
            self.xfrc = None if form is None else np.zeros_like(self.fx["xf"][0]) if form == "zeros" else self.fx["xf"][form]
        return ("ok",)

    # -- state
    def _op_set_state(self, form, i, ids, io="f64", nan=None):
        q, v = batch_state(i, nan, self.fx)
        if form in ("dev", "dev_mask") and io == "f32":
            q, v = _f32(q), _f32(v)
        rows = list(range(self.E)) if ids is None else list(ids)
        if nan is None:
            self.poisoned -= set(rows)
        for t, k in enumerate(rows):
            src = t if form == "subset" else k        # a subset call passes the listed environments' rows, in order
            self.q[k], self.v[k] = self._in(q[src]), self._in(v[src])
            if not (self.twin == "reset_keeps_status" and form == "subset"):
                self.code[k], self.done[k] = 0, 0
        return ("ok",)

    def _op_poison(self, env, body, i):
        self.poisoned.add(env)
        return self._op_set_state("subset_nan", i, (env,), nan=(env, body))

    def _op_get_state(self, form, arg=None):
        if form == "subset":
            ids = list(arg)
            return ("state", self.q[ids].copy(), self.v[ids].copy())
        if form == "dev" and arg == "f32":
            return ("state", _f32(self.q), _f32(self.v))
        return ("state", self.q.copy(), self.v.copy())

    def _op_status(self, form):
        return ("status", self.code.copy(), self.done.copy())

    # -- stepping
    def _op_step(self, k, p):
        return ("failed", self._advance(k, p))

    def _op_step_async(self, k, p):
        self._advance(k, p)
        return ("ok",)

    def _op_sync(self):
        return ("failed", self._failed())

    def _op_run_sampled(self, form, n, every, vel, p):
        S = n // every
        qs, vs = np.zeros((S, self.E, self.M, 7)), np.zeros((S, self.E, self.M, 6))
        for s_ in range(S):
            self._advance(every, p)
            qs[s_], vs[s_] = self.q, self.v
        self._advance(n - S * every, p)
        out = ("samples", qs) + ((vs,) if vel else ())
        return out + (self._failed(),) if form == "host" else out

    def max_records(self, R):
        if R is not None:
            return R
        sc = self.fx["sc"]
        mixed = self.M > 1 and bool(np.any(sc.kind != 0))
        return min(16, 4 * sc.planes.shape[0] + (4 if mixed else 1) * (self.M - 1))

    def _op_contacts(self, form, ids, R):
        R = self.max_records(R)
        rows = list(range(self.E)) if ids is None else list(ids)
        per = []
        for k in rows:
            if self.code[k]:
                empty = (np.zeros(self.M, np.int32),) + (np.zeros(0),) * 3 + (np.zeros((0, 3)),) * 2
                per.append(dense_contacts(empty, self.M, R))
                per[-1][0][:] = -1                # a failed environment: count -1, unused slots only
            else:
                per.append(dense_contacts(self.O.contacts(self._scene(k, 0), self.q[k], dtype=self.dtype), self.M, R))
        out = [np.stack([x[j] for x in per]) for j in range(6)]
        if R == 0:
            out = out[:1]
        trunc = int((out[0] > R).sum())
        return ("contacts",) + tuple(out) + ((trunc,) if form == "host" else ())

    # -- law, stream, refusals
    def _op_law(self, law, tol):
        self.law, self.tol = law, tol
        return ("ok",)

    def _op_stream(self, which):
        return ("ok",)

    def _op_refused(self, what):
        return ("err", EUNSUPPORTED if what.startswith("u_") else EINVAL)

    def close(self):
        pass


class DeviceBatch:
    """The same calls on rbhip.BatchWorld; device arrays are torch tensors."""

    def __init__(self, variant):
        import rbhip
        import torch
        self.rb, self.torch = rbhip, torch
        self.cfg = BATCH_VARIANTS[variant]
        self.E = self.cfg["E"]
        self.fx = batch_fixture(self.cfg["template"], self.E)
        self.M = self.fx["M"]
        self.b = rbhip.BatchWorld(self.fx["sc"], self.E, dtype=self.cfg["dtype"], law=self.cfg.get("start", "mujoco"))
        self.b.set_state(*self.fx["pool"][0])
        self.keep = []
        self.torch_stream = None

    def _call(self, fn, *a, **kw):
        try:
            r = fn(*a, **kw)
        except self.rb.RbError as exc:
            return ("err", exc.code)
        return ("ok",) if r is None else r

    def _dev(self, a, io="f64"):
        t = self.torch.from_numpy(np.array(a, np.float32 if io == "f32" else np.float64)).to("cuda")
        self.keep.append(t)
        return t

    def _host(self, t):
        self.torch.cuda.synchronize()
        a = t.cpu().numpy()
        return a.astype(np.float64) if a.dtype == np.float32 else a

    def _kw(self, p):
        dt, e, mu, thr = batch_step_params(self.fx["sc"], p)
        return dict(dt=dt, restitution=e, friction=mu, threshold=thr)

    def do(self, op):
        return getattr(self, "_op_" + op.name)(*op.args)

    def _op_set_params(self, which):
        return self._call(self.b.set_params, self.fx["e"] if which in ("both", "e") else None,
                          self.fx["mu"] if which in ("both", "mu") else None)

    def _op_set_bodies(self, i):
        return self._call(self.b.set_bodies, *self.fx["bodies"][i])

    def _op_set_planes(self, on):
        return self._call(self.b.set_planes, self.fx["planes"] if on else None)

    def _op_set_gravity(self, on):
        return self._call(self.b.set_gravity, self.fx["gravity"] if on else None)

    def _op_set_xfrc(self, form, ref=None, io="f64"):
        if form == "dev":
            return self._call(self.b.set_xfrc_device, self._dev(self.fx["xf"][ref], io))
        x = None if form is None else np.zeros_like(self.fx["xf"][0]) if form == "zeros" else self.fx["xf"][form]
        return self._call(self.b.set_xfrc, x)

    def _op_set_state(self, form, i, ids, io="f64", nan=None):
        q, v = batch_state(i, nan, self.fx)
        if form == "all":
            return self._call(self.b.set_state, q, v)
        if form in ("subset", "subset_nan"):
            rows = list(ids)
            src = rows if form == "subset_nan" else list(range(len(rows)))
            return self._call(self.b.set_state, q[src], v[src], envs=rows)
        mask = None
        if ids is not None:
            m = np.zeros(self.E, np.uint8)
            m[list(ids)] = 1
            mask = self.torch.from_numpy(m).to("cuda")
            self.keep.append(mask)
        return self._call(self.b.set_state_device, self._dev(q, io), self._dev(v, io), mask)

    def _op_poison(self, env, body, i):
        return self._op_set_state("subset_nan", i, (env,), nan=(env, body))

    def _op_get_state(self, form, arg=None):
        if form == "all":
            return ("state",) + self.b.get_state()
        if form == "subset":
            return ("state",) + self.b.get_state(list(arg))
        q, v = self.b.get_state_device(dtype=arg)
        return ("state", self._host(q), self._host(v))

    def _op_status(self, form):
        if form == "host":
            return ("status",) + self.b.status()
        c, d = self.b.status_device()
        return ("status", self._host(c), self._host(d))

    def _op_step(self, k, p):
        r = self._call(self.b.step, k, **self._kw(p))
        return r if isinstance(r, tuple) else ("failed", r)

    def _op_step_async(self, k, p):
        return self._call(self.b.step_async, k, **self._kw(p))

    def _op_sync(self):
        r = self._call(self.b.sync)
        return r if isinstance(r, tuple) else ("failed", r)

    def _op_run_sampled(self, form, n, every, vel, p):
        if form == "host":
            q, v, nf = self.b.run_sampled(n, every, velocities=vel, **self._kw(p))
            return ("samples", q) + ((v,) if vel else ()) + (nf,)
        q, v = self.b.run_sampled_device(n, every, velocities=vel, **self._kw(p))
        return ("samples", self._host(q)) + ((self._host(v),) if vel else ())

    def _op_contacts(self, form, ids, R):
        if form == "host":
            c = self.b.contacts(None if ids is None else list(ids), max_records=R)
            f = [c.counts] if c.partner is None else [c.counts, c.partner, c.kind, c.dist, c.pos, c.frame]
            return ("contacts",) + tuple(f) + (c.truncated,)
        c = self.b.contacts_device(max_records=R)
        f = [c.counts] if c.partner is None else [c.counts, c.partner, c.kind, c.dist, c.pos, c.frame]
        return ("contacts",) + tuple(self._host(x) for x in f)

    def _op_law(self, law, tol):
        return self._call(self.b.set_contact_law, law, tol)

    def _op_stream(self, which):
        if which == "torch":
            if self.torch_stream is None:
                self.torch_stream = self.torch.cuda.Stream()
            return self._call(self.b.use_stream, self.torch_stream.cuda_stream)
        return self._call(self.b.use_stream, 0)

    def _op_refused(self, what):
        b = self.b
        if what == "nsteps":
            return self._call(b.step, -1)
        if what == "dt0":
            return self._call(b.step_async, 3, dt=0.0)
        if what == "every0":
            return self._call(b.run_sampled, 7, 0)
        if what == "maxrec_neg":
            return self._call(b.contacts, None, max_records=-1)
        if what == "twice":
            return self._call(b.contacts, [1, 0, 1], max_records=2)
        if what == "u_law":
            return self._call(b.set_contact_law, "balls", 0.01)
        if what == "u_planes":
            return self._call(b.set_planes, self.fx["planes"])
        if what == "u_xfrc":
            return self._call(b.set_xfrc, self.fx["xf"][0])
        if what == "u_contacts":
            return self._call(b.contacts, None, max_records=0)
        raise KeyError(what)

    def close(self):
        self.torch.cuda.synchronize()
        self.b.close()


def _batch_candidate(kind, m, rng, cfg, fxdims, used):
    E, M, P, spheres = fxdims

    def pick(options, p=None):
        new = [o for o in options if (kind, o) not in used]
        o = new[0] if new else options[int(rng.choice(len(options), p=p))]
        used.add((kind, o))
        return o

    def subset():
        n = int(rng.integers(1, min(E, 6) + 1))
        ids = [int(x) for x in rng.permutation(E)[:n]]
        if m.poisoned and rng.random() < 0.7:         # a reset that names a failed environment
            bad = sorted(m.poisoned)[0]
            ids = [bad] + [x for x in ids if x != bad][:n - 1]
        return tuple(ids)
    balls = m.law == "balls"
    if kind == "set_params":
        return Op(kind, (pick(("both", "e", "mu", "none")),))
    if kind == "set_bodies":
        return Op(kind, (pick((1, 2, 0)),))
    if kind == "set_planes":
        return Op(kind, (None if balls or P == 0 else pick((True, None)),))
    if kind == "set_gravity":
        return Op(kind, (pick((True, None)),))
    if kind == "set_xfrc":
        if balls:
            return Op(kind, (None,))
        f = pick((0, "zeros", None, "dev32", "dev64", 1))
        return Op(kind, ("dev", 1, "f32") if f == "dev32" else ("dev", 0, "f64") if f == "dev64" else (f,))
    if kind == "set_state":
        f = pick(("all", "subset", "dev", "dev_mask", "dev32", "dev_mask32"))
        i = int(rng.integers(0, 3))
        if f == "all":
            return Op(kind, ("all", i, None))
        if f == "subset":
            return Op(kind, ("subset", i, subset()))
        return Op(kind, ("dev_mask" if "mask" in f else "dev", i, subset() if "mask" in f else None,
                         "f32" if f.endswith("32") else "f64"))
    if kind == "get_state":
        f = pick(("all", "subset", "dev64", "dev32"))
        return Op(kind, ("subset", subset()) if f == "subset" else ("dev", "f" + f[3:]) if f.startswith("dev") else ("all",))
    if kind in ("step", "step_async"):
        return Op(kind, (pick(BATCH_STEPS, BATCH_STEP_WEIGHTS), int(rng.integers(0, 2))))
    if kind == "sync":
        return Op(kind, ())
    if kind == "run_sampled":
        f = pick(("host", "dev"))
        every = pick((1, 7)) if f == "host" else int(rng.choice((1, 7)))
        return Op(kind, (f, int(rng.choice((3, 20, 40))), every, bool(rng.random() < 0.7), int(rng.integers(0, 2))))
    if kind == "contacts":
        f = pick(("host", "host_subset", "dev"))
        R = (None, 2, 0)[int(rng.integers(0, 3))]
        return Op(kind, ("dev", None, R) if f == "dev" else ("host", subset() if f == "host_subset" else None, R))
    if kind == "status":
        return Op(kind, (pick(("host", "dev")),))
    if kind == "law":
        if not balls and m.planes is None and m.xfrc is None:
            return Op(kind, ("balls", TOLS[int(rng.integers(0, 2))]))
        return Op(kind, ("mujoco", 0.01))
    if kind == "stream":
        return Op(kind, ("torch" if m.stream != "torch" else "null",))
    if kind == "poison":
        return Op(kind, (int(rng.integers(0, E)), int(spheres[int(rng.integers(0, len(spheres)))]), int(rng.integers(0, 3))))
    if kind == "refused":
        what = ["nsteps", "dt0", "every0"]
        if balls:
            what += ["u_planes", "u_xfrc", "u_contacts"] if P else ["u_xfrc", "u_contacts"]
        else:
            what += ["maxrec_neg", "twice"]
            if not cfg["law"] or m.planes is not None or m.xfrc is not None:
                what.append("u_law")
        return Op(kind, (pick(tuple(what)),))
    raise KeyError(kind)


_BATCH_DIMS = {"multi4": (4, 4, None), "cube": (1, 1, None), "pile": (4, 1, (3,)), "balls": (16, 1, None),
               "mixed64": (64, 3, None)}


@functools.lru_cache(maxsize=None)
def _generate_batch(variant, nseeds):
    cfg = BATCH_VARIANTS[variant]
    M, P, sph = _BATCH_DIMS[cfg["template"]]
    dims = (cfg["E"], M, P, tuple(range(M)) if sph is None else sph)
    kinds = batch_kinds(variant)
    return _greedy_sequences(
        variant, 100 + list(BATCH_VARIANTS).index(variant), nseeds, kinds, lambda a, b: batch_pair_legal(variant, a, b),
        lambda: ModelBatch(variant, dry=True), lambda kind, m, rng, used: _batch_candidate(kind, m, rng, cfg, dims, used),
        BATCH_OPS, lambda m: False, [Op("sync", ()), Op("status", ("host",)), Op("get_state", ("all",))])


def generate(variant, seed):
    """The op list of (variant, seed); deterministic."""
    if variant in WORLD_VARIANTS:
        return list(_generate_world(variant, seed + 1)[seed])
    return list(_generate_batch(variant, seed + 1)[seed])


# ---------------------------------------------------------------- running and comparing
def run(ops, target):
    """Play ops on target; the observations, one per op."""
    return [target.do(Op(*op)) for op in ops]


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_observation(a, b):
    """Floats as 64-bit words (signs of zero and NaN rows count), integers and tags equal."""
    if type(a) is not type(b):
        return False
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_observation(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_words(a), _words(b))
    return a == b


def first_difference(obs_a, obs_b):
    for i, (a, b) in enumerate(zip(obs_a, obs_b)):
        if not same_observation(a, b):
            return i
    return None if len(obs_a) == len(obs_b) else min(len(obs_a), len(obs_b))


def _brief(o):
    if isinstance(o, tuple):
        return "(" + ", ".join(_brief(x) for x in o) + ")"
    if isinstance(o, np.ndarray):
        return f"<{o.dtype}{list(o.shape)}>"
    return repr(o)


def describe_failure(variant, seed, ops, i, obs_a, obs_b):
    """Variant, seed, index of the first differing observation, the last ten ops as a literal."""
    lines = [f"variant {variant!r} seed {seed}: observation {i} differs at op {ops[i]!r}",
             f"  device: {_brief(obs_a[i]) if i < len(obs_a) else None}",
             f"  model:  {_brief(obs_b[i]) if i < len(obs_b) else None}"]
    a, b = (obs_a[i], obs_b[i]) if i < min(len(obs_a), len(obs_b)) else ((), ())
    if isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b):
        for x, y in zip(a, b):
            if isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.shape == y.shape and \
                    not same_observation(x, y):
                rows = np.flatnonzero((_words(x) != _words(y)).reshape(x.shape[0], -1).any(1)) if x.ndim else []
                lines.append(f"  {len(rows)} rows differ, first {list(rows[:8])}")
    lo = max(0, i - 9)
    lines.append(f"  ops[{lo}:{i + 1}] = {[tuple(o) for o in ops[lo:i + 1]]!r}")
    lines.append(f"  replay: call_sequences.replay({variant!r}, {seed}, upto={i + 1})")
    return "\n".join(lines)


def make_model(variant, oracle, **kw):
    return (ModelWorld if variant in WORLD_VARIANTS else ModelBatch)(variant, oracle, **kw)


def make_device(variant):
    return (DeviceWorld if variant in WORLD_VARIANTS else DeviceBatch)(variant)


def replay(variant, seed, upto=None, ops=None):
    """The first `upto` ops of (variant, seed) on the device and on the model:
    (device observations, model observations).  Sets the variant's RBHIP_*
    switches for the world it builds and restores the environment."""
    from oracle import oracle as O
    ops = (generate(variant, seed) if ops is None else list(ops))[:upto]
    cfg = WORLD_VARIANTS.get(variant, {"env": {}})
    saved = {k: os.environ.get(k) for k in FORM_ENV_KEYS}
    try:
        for k in FORM_ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(cfg["env"])
        dev = make_device(variant)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    try:
        obs_d = run(ops, dev)
    finally:
        dev.close()
    return obs_d, run(ops, make_model(variant, O))
