"""BatchWorld: many small independent scenes on one MI355X, one launch per
step chunk (rb_batch_* in include/rbhip.h).

The reference's scenes hold 1 to 4 bodies and are studied one knob per run
(src/config/sim_overrides.py; the velocity variants under
data/plots/single_sphere/).  A BatchWorld is n_envs replicas of one such
scene, each with its own restitution, friction, body constants and state,
and (set_planes / set_gravity / set_xfrc, or one Scene per environment
through from_scenes) its own planes, gravity and applied forces: the incline
angle of cube_incline.py, model.opt.gravity, data.xfrc_applied.  Every
environment steps bit-identically to a World of the same scene, under the
default contact law or the two-ball law of ball_collision.py.  A scene may
mix spheres and boxes (scenes.box_pile: stacks of cubes), box-involved pairs
included; from_scenes over a list of seeds is an ensemble of piles.  A
scene holds up to 256 bodies: up to 64 an environment is (a part of) one
wave, from 65 on one workgroup of 2 to 4 waves (a wide batch), with the same
interface and the same bits; only the two-ball law stops at 64.
The environments need not hold the same scene shape: a population
(set_population, from_ragged_scenes) gives every environment its own body
count (1..M) and its own kinds.  Bodies past an environment's count are
absent: their rows are storage that no step reads or writes, sampled runs
hold zeros there and the contact query gives them count 0.
contacts() lists every body's contacts of the current state; impulses() is the
contact-force sensor: what the next step does to every body, contact by
contact (jn and jt of collision.py:7-48, the velocity the solve leaves, the
net contact impulse), without stepping.
Arrays are environment-major: (E, M, 7) / (E, M, 6).  run_sampled() returns
the curves the reference plots (logger_base.py, data_logger.py,
multi_sphere_logger.py), one per environment, sampled on the device;
run_sampled_impulses() adds the force curve of the same run, each body's
contact impulse summed over every sampling window inside the step loop.

The *_device methods keep all of that in device memory: they take any object
with __cuda_array_interface__ (a torch tensor on the batch's GPU), enqueue on
the batch's stream (use_stream) and return without waiting; sync() waits.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np

from . import _lib
from ._devarray import (_CONTACT_FIELDS, _IMPULSE_FIELDS, _IO_CODES, _device_array, _host_arrays, _new_tensor,
                        _pair_typestr, _resolve_out)
from .scenes import Scene


class BatchContacts:
    """The contact lists of a batch's state (BatchWorld.contacts /
    contacts_device): dense arrays, R = max_records slots per body.

    counts (n, M) int32: the true number of contacts of each body, also where
    it exceeds R (then only the first R records are kept); -1 for every body
    of a failed environment.  partner, kind (n, M, R) int32 and dist (n, M, R):
    partner is the other body's id within the environment or -1 - plane, kind
    an RB_CK_* code.  pos, frame (n, M, R, 3), or None without geometry: frame
    is the raw normal from geom1 to geom2 (geom1: the plane; the lower id of
    two spheres or two boxes; the sphere of a sphere-box pair).  Slots at or
    past a body's count hold kind -1 and zeros.  truncated: the number of
    bodies with count > R (None for the device form, which does not wait).
    With max_records 0 only counts is set.  An absent body (a slot past its
    environment's body count: BatchWorld.set_population) has count 0 and
    unused slots only, and is nobody's partner."""

    def __init__(self, max_records, counts, partner, kind, dist, pos, frame, truncated):
        self.max_records = max_records
        self.counts, self.partner, self.kind, self.dist = counts, partner, kind, dist
        self.pos, self.frame = pos, frame
        self.truncated = truncated

    def lists(self, i: int):
        """Row i's contacts in the CSR shape of World.contacts(): (counts (M,),
        partner, kind, dist, pos, frame), the last five flat over the kept
        records, body by body (pos / frame None without geometry).  Host
        arrays only."""
        if self.partner is None:
            raise ValueError("lists(): a counts-only query (max_records 0) holds no records")
        cnt = np.asarray(self.counts[i])
        keep = np.arange(self.max_records)[None, :] < np.minimum(cnt, self.max_records)[:, None]

        def pick(a):
            return None if a is None else np.asarray(a[i])[keep]
        return cnt.copy(), pick(self.partner), pick(self.kind), pick(self.dist), pick(self.pos), pick(self.frame)


@dataclass
class BatchImpulses:
    """What the next step does to every body, contact by contact
    (BatchWorld.impulses / impulses_device): dense arrays, R slots per body
    (partner.shape[-1]; 0 and None records for the "sensor only" call).

    counts (n, M), partner, kind, dist (n, M, R): word for word the fields of
    BatchContacts for the same state and R.  jn (n, M, R), jt (n, M, R, 3):
    the two return values of compute_collision_impulse_friction
    (collision.py:7-48) for the contact, 0 where the step skips it or it
    separates.  vel (n, M, 6): (v, omega) after gravity, applied forces and all
    the body's contacts, the step's qvel.  net (n, M, 6): the body's net contact
    impulse and net angular impulse about its centre; net[..., :3] / dt is the
    average contact force of the step.  vel and net do not depend on R.  A
    failed environment: counts -1, zeros elsewhere; an absent body: 0 and zeros.
    truncated: the bodies with count > R (None for the device form)."""
    counts: Any
    partner: Any
    kind: Any
    dist: Any
    jn: Any
    jt: Any
    vel: Any
    net: Any
    truncated: Optional[int]


class BatchWorld:
    def __init__(self, scene: Scene, n_envs: int, device: int = 0, dtype: str = "f64",
                 normal_convention: Optional[str] = None, law: str = "mujoco", tol: float = 0.01):
        """scene: the template environment (1..256 bodies, spheres and boxes
        in any mix: scenes.box_pile), replicated n_envs times with the
        scene's initial state.  More than 64 bodies make a wide batch
        (rb_batch_create_wide): everything works as on any other batch but
        law="balls", which is refused (RbError, RB_EUNSUPPORTED).

        law: "mujoco" (the per-body law of collision.py /
        multi_sphere_bounce.py) or "balls" (the symmetric two-ball law of
        ball_collision.py: spheres only, no plane or the z = 0 ground; tol is
        its contact margin, ball_collision.py:102).  See set_contact_law()."""
        L = _lib.load()
        self.scene = scene
        self.dtype = dtype
        self.n_envs, self.n_bodies = int(n_envs), scene.n
        self.device = device
        nc = normal_convention or scene.normal_convention
        kind = np.ascontiguousarray(scene.kind, np.int32)
        mass = np.ascontiguousarray(scene.mass, np.float64)
        inertia = np.ascontiguousarray(scene.inertia, np.float64)
        size = np.ascontiguousarray(scene.size, np.float64)
        planes = np.ascontiguousarray(scene.planes, np.float64)
        d = _lib.SceneDesc()
        d.n_bodies = scene.n
        d.n_planes = planes.shape[0]
        d.dtype = _lib.RB_F64 if dtype == "f64" else _lib.RB_F32
        d.normal_convention = _lib.RB_NORMAL_RAW if nc == "raw" else _lib.RB_NORMAL_ORIENTED
        d.device, d.rank, d.world_size = device, 0, 1
        d.kind, d.mass = _lib.ptr(kind), _lib.ptr(mass)
        d.inertia, d.size = _lib.ptr(inertia), _lib.ptr(size)
        d.planes = _lib.ptr(planes) if d.n_planes else None
        for k in range(3):
            d.gravity[k] = float(scene.gravity[k])
        h = C.c_void_p()
        self._h = None
        # a box among several bodies: the entry point that steps box-involved pairs
        mixed = scene.n > 1 and bool(np.any(kind != 0))
        create = "rb_batch_create_mixed" if mixed else "rb_batch_create"
        if scene.n > 64:        # an environment across several waves
            create = "rb_batch_create_wide"
        _lib.check(getattr(L, create)(C.byref(h), C.byref(d), self.n_envs), create)
        self._h = h
        self._L = L
        self._population = None
        E, M = self.n_envs, self.n_bodies
        if law != "mujoco":
            try:
                self.set_contact_law(law, tol)
            except Exception:
                self.close()
                raise
        self.set_state(np.broadcast_to(scene.qpos0, (E, M, 7)), np.broadcast_to(scene.qvel0, (E, M, 6)))

    @classmethod
    def from_scenes(cls, scenes, **kw):
        """A batch with one environment per Scene of `scenes` (an angle sweep:
        [scenes.cube_incline(a) for a in angles]).  The template is
        scenes[0]; planes, gravity, restitution, friction, mass, inertia,
        size and the initial state are taken from every scene.  The scenes
        must agree in body count, kinds, plane count, dt, threshold and
        normal convention (ValueError naming the first scene that does not).
        kw: the constructor's (device, dtype, ...)."""
        scenes = list(scenes)
        if not scenes:
            raise ValueError("from_scenes: no scene given")
        t = scenes[0]
        for k, sc in enumerate(scenes[1:], 1):
            for what, same in (("body count", sc.n == t.n),
                               ("body kinds", sc.n == t.n and np.array_equal(sc.kind, t.kind)),
                               ("plane count", np.shape(sc.planes)[0] == np.shape(t.planes)[0]),
                               ("dt", sc.dt == t.dt), ("threshold", sc.threshold == t.threshold),
                               ("normal convention", sc.normal_convention == t.normal_convention)):
                if not same:
                    raise ValueError(f"from_scenes: scene {k} ({sc.name!r}) differs from scene 0 in its {what}")
        return cls._apply_scenes(t, scenes, kw, None, np.stack([sc.mass for sc in scenes]),
                                 np.stack([sc.inertia for sc in scenes]), np.stack([sc.size for sc in scenes]),
                                 np.stack([sc.qpos0 for sc in scenes]), np.stack([sc.qvel0 for sc in scenes]))

    @classmethod
    def _apply_scenes(cls, t, scenes, kw, population, mass, inertia, size, qpos, qvel):
        """The batch of template t with an environment per scene: the
        population (None: none), the scenes' planes, gravity and parameters,
        the given constants and state.  Closed again if any is refused."""
        b = cls(t, len(scenes), **kw)
        try:
            if population is not None:
                b.set_population(*population)
            if np.shape(t.planes)[0]:
                b.set_planes(np.stack([np.asarray(sc.planes, np.float64) for sc in scenes]))
            b.set_gravity(np.stack([np.asarray(sc.gravity, np.float64) for sc in scenes]))
            b.set_params(restitution=[sc.restitution for sc in scenes], friction=[sc.friction for sc in scenes])
            b.set_bodies(mass=mass, inertia=inertia, size=size)
            b.set_state(qpos, qvel)
        except Exception:
            b.close()
            raise
        return b

    @classmethod
    def from_ragged_scenes(cls, scenes, **kw):
        """A batch with one environment per Scene of `scenes`, which may
        differ in body count and kinds (an ensemble of piles of 1 to 8
        bodies; single_sphere, single_cube and multi_sphere4 side by side).
        M is the largest body count and the template the first scene of that
        size; every environment's population is its scene's count and kinds
        (set_population).  Shorter scenes are padded with absent bodies: mass
        and inertia 1, the template's size row, pose (0, 0, 0, 1, 0, 0, 0),
        zero velocity, the template's kind.  Everything from_scenes takes per
        scene is taken here too.  The scenes must agree in plane count, dt,
        threshold and normal convention (ValueError naming the first scene
        that does not, before any batch is created).  kw: the constructor's."""
        scenes = list(scenes)
        if not scenes:
            raise ValueError("from_ragged_scenes: no scene given")
        M = max(sc.n for sc in scenes)
        t = next(sc for sc in scenes if sc.n == M)
        for k, sc in enumerate(scenes):
            for what, same in (("plane count", np.shape(sc.planes)[0] == np.shape(t.planes)[0]),
                               ("dt", sc.dt == t.dt), ("threshold", sc.threshold == t.threshold),
                               ("normal convention", sc.normal_convention == t.normal_convention)):
                if not same:
                    raise ValueError(f"from_ragged_scenes: scene {k} ({sc.name!r}) differs from the template "
                                     f"({t.name!r}) in its {what}")
        E = len(scenes)
        n = np.array([sc.n for sc in scenes], np.int32)
        kinds = np.tile(np.asarray(t.kind, np.int32), (E, 1))
        mass, inertia = np.ones((E, M)), np.ones((E, M, 3))
        size = np.tile(np.asarray(t.size, np.float64), (E, 1, 1))
        qpos, qvel = np.zeros((E, M, 7)), np.zeros((E, M, 6))
        qpos[:, :, 3] = 1.0
        for e, sc in enumerate(scenes):
            kinds[e, :sc.n], mass[e, :sc.n], inertia[e, :sc.n], size[e, :sc.n] = sc.kind, sc.mass, sc.inertia, sc.size
            qpos[e, :sc.n], qvel[e, :sc.n] = sc.qpos0, sc.qvel0
        return cls._apply_scenes(t, scenes, kw, (n, kinds), mass, inertia, size, qpos, qvel)

    # ---- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.rb_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- contact law --------------------------------------------------------
    def set_contact_law(self, law: str, tol: float = 0.01):
        """"mujoco" or "balls" (as World.set_contact_law).  Under "balls" the
        threshold given to step() and the inertia rows of set_bodies() are
        ignored: the law derives the inverse inertia from mass and radius
        (ball_collision.py:39-41).  The law may be switched between calls.
        "balls" on a batch of more than 64 bodies per environment is refused
        (RbError, RB_EUNSUPPORTED) and changes nothing."""
        code = {"mujoco": _lib.RB_LAW_MUJOCO, "balls": _lib.RB_LAW_BALLS}.get(law, law)
        if not isinstance(code, int):
            raise ValueError(f"unknown contact law {law!r}")
        _lib.check(self._L.rb_batch_set_contact_law(self._h, code, float(tol)), "rb_batch_set_contact_law")

    # ---- per-environment constants ----------------------------------------
    def _arr(self, a, shape):
        return None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), shape))

    def set_params(self, restitution=None, friction=None):
        """Per-environment restitution / friction, (E,) each; None: the
        scalar given to step()."""
        e = self._arr(restitution, (self.n_envs,))
        mu = self._arr(friction, (self.n_envs,))
        _lib.check(self._L.rb_batch_set_params(self._h, _lib.ptr(e), _lib.ptr(mu)), "rb_batch_set_params")

    def set_bodies(self, mass=None, inertia=None, size=None):
        """Per-environment body constants: mass (E, M), inertia (E, M, 3),
        size (E, M, 3); None: keep."""
        E, M = self.n_envs, self.n_bodies
        m, i, s = self._arr(mass, (E, M)), self._arr(inertia, (E, M, 3)), self._arr(size, (E, M, 3))
        _lib.check(self._L.rb_batch_set_bodies(self._h, _lib.ptr(m), _lib.ptr(i), _lib.ptr(s)), "rb_batch_set_bodies")

    def set_population(self, n_bodies=None, kinds=None):
        """Per-environment body counts n_bodies (E,) in 1..M (None: M
        everywhere) and kinds (E, M), 0 sphere / 1 box (None: the template's
        in every environment).  Bodies 0..n_e-1 of environment e are present
        and step bit-identically to a World of those bodies alone; the rest
        are absent: storage that set_* / get_* write and return as ever and
        that no step reads or writes.  Both None: no population again.  May
        be called between any two calls; it changes no state.  Not under
        "balls" (RbError, RB_EUNSUPPORTED)."""
        E, M = self.n_envs, self.n_bodies
        n = None if n_bodies is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_bodies, np.int32), (E,)))
        k = None if kinds is None else np.ascontiguousarray(np.broadcast_to(np.asarray(kinds, np.int32), (E, M)))
        _lib.check(self._L.rb_batch_set_population(self._h, _lib.ptr(n), _lib.ptr(k)), "rb_batch_set_population")
        if n is None and k is None:
            self._population = None
        else:
            self._population = (np.full(E, M, np.int32) if n is None else n.copy(),
                                np.tile(np.asarray(self.scene.kind, np.int32), (E, 1)) if k is None else k.copy())

    @property
    def population(self):
        """(n_bodies (E,) int32, kinds (E, M) int32) as last set, or None
        without a population."""
        pop = getattr(self, "_population", None)
        return None if pop is None else (pop[0].copy(), pop[1].copy())

    def set_planes(self, planes):
        """Per-environment planes (E, P, 6): normal xyz, point xyz; P is the
        template's plane count.  None: the template's planes again.  The
        values persist across steps and set_state().  Not under "balls"."""
        P = np.shape(self.scene.planes)[0]
        a = self._arr(planes, (self.n_envs, P, 6))
        _lib.check(self._L.rb_batch_set_planes(self._h, _lib.ptr(a)), "rb_batch_set_planes")

    def set_gravity(self, gravity):
        """Per-environment gravity (E, 3); None: the template's.  Honoured
        under both contact laws."""
        a = self._arr(gravity, (self.n_envs, 3))
        _lib.check(self._L.rb_batch_set_gravity(self._h, _lib.ptr(a)), "rb_batch_set_gravity")

    def set_xfrc(self, xfrc):
        """Per-body applied force and torque (E, M, 6) as World.set_xfrc
        (data.xfrc_applied, collision.py:66-70); None: none.  While set, every
        body takes the applied-force path, all-zero rows included.  Not under
        "balls"."""
        a = self._arr(xfrc, (self.n_envs, self.n_bodies, 6))
        _lib.check(self._L.rb_batch_set_xfrc(self._h, _lib.ptr(a)), "rb_batch_set_xfrc")

    # ---- state --------------------------------------------------------------
    def _envs(self, envs):
        if envs is None:
            return None, self.n_envs
        ids = np.ascontiguousarray(envs, np.int64).reshape(-1)
        return ids, ids.shape[0]

    def set_state(self, qpos, qvel, envs=None):
        """qpos (n, M, 7), qvel (n, M, 6) for the environments in envs (None:
        all, in order).  Clears the failed status of those environments."""
        ids, n = self._envs(envs)
        q = np.ascontiguousarray(qpos, np.float64).reshape(n, self.n_bodies, 7)
        v = np.ascontiguousarray(qvel, np.float64).reshape(n, self.n_bodies, 6)
        _lib.check(self._L.rb_batch_set_state(self._h, _lib.ptr(ids), n, _lib.ptr(q), _lib.ptr(v)),
                   "rb_batch_set_state")

    def get_state(self, envs=None):
        """(qpos (n, M, 7), qvel (n, M, 6)) of the environments in envs (None: all)."""
        ids, n = self._envs(envs)
        q = np.zeros((n, self.n_bodies, 7))
        v = np.zeros((n, self.n_bodies, 6))
        _lib.check(self._L.rb_batch_get_state(self._h, _lib.ptr(ids), n, _lib.ptr(q), _lib.ptr(v)),
                   "rb_batch_get_state")
        return q, v

    # ---- stepping -----------------------------------------------------------
    def _params(self, dt, restitution, friction, threshold):
        sc = self.scene
        return (sc.dt if dt is None else dt, sc.restitution if restitution is None else restitution,
                sc.friction if friction is None else friction,
                sc.threshold if threshold is None else threshold)

    def step(self, nsteps: int = 1, dt=None, restitution=None, friction=None, threshold=None) -> int:
        """Step every healthy environment nsteps times; returns how many
        environments have failed so far (status())."""
        p = self._params(dt, restitution, friction, threshold)
        nf = C.c_int64()
        _lib.check(self._L.rb_batch_step(self._h, int(nsteps), *p, C.byref(nf)), "rb_batch_step")
        return nf.value

    def run_sampled(self, nsteps: int, every: int, velocities: bool = True, dt=None, restitution=None,
                    friction=None, threshold=None):
        """Step nsteps times as step() does and record every environment's
        state after every every-th step, on the device: one launch per 256
        steps instead of one launch, one sync and one download per sample.
        Returns (qpos (S, E, M, 7), qvel (S, E, M, 6) or None, n_failed) with
        S = nsteps // every; sample s is the state after step (s + 1) * every
        of this call, word for word what step(every) + get_state() returns.  A
        failed environment's rows repeat its frozen state."""
        p = self._params(dt, restitution, friction, threshold)
        nsteps, every = int(nsteps), int(every)
        S = nsteps // every if every >= 1 and nsteps >= 0 else 0
        q = np.zeros((S, self.n_envs, self.n_bodies, 7))
        v = np.zeros((S, self.n_envs, self.n_bodies, 6)) if velocities else None
        nf = C.c_int64()
        _lib.check(self._L.rb_batch_run_sampled(self._h, nsteps, every, *p, _lib.ptr(q), _lib.ptr(v), C.byref(nf)),
                   "rb_batch_run_sampled")
        return q, v, nf.value

    def run_sampled_impulses(self, nsteps: int, every: int, positions: bool = True, velocities: bool = True, dt=None,
                             restitution=None, friction=None, threshold=None):
        """run_sampled() that also records the contact-impulse curve of the
        run.  Returns (qpos (S, E, M, 7) or None, qvel (S, E, M, 6) or None,
        net (S, E, M, 6), n_failed).  net[s, e, k] is the contact impulse
        (0:3) and angular impulse about its centre (3:6) that body k of
        environment e received over steps s * every + 1 .. (s + 1) * every of
        this call: the sum, in step order, of the `net` row impulses() gives
        before each committed step.  net[..., 0:3] / (every * dt) is the
        window's average contact force.  A failed environment's windows after
        the failure are zeros, absent bodies' rows are zeros.  positions=False,
        velocities=False is the force curve alone.  Not under "balls"."""
        p = self._params(dt, restitution, friction, threshold)
        nsteps, every = int(nsteps), int(every)
        S = nsteps // every if every >= 1 and nsteps >= 0 else 0
        q = np.zeros((S, self.n_envs, self.n_bodies, 7)) if positions else None
        v = np.zeros((S, self.n_envs, self.n_bodies, 6)) if velocities else None
        net = np.zeros((S, self.n_envs, self.n_bodies, 6))
        nf = C.c_int64()
        _lib.check(self._L.rb_batch_run_sampled_impulses(self._h, nsteps, every, *p, _lib.ptr(q), _lib.ptr(v),
                                                         _lib.ptr(net), C.byref(nf)), "rb_batch_run_sampled_impulses")
        return q, v, net, nf.value

    def status(self):
        """(code (E,) int32: 0 or RB_EDOM (-33); steps_done (E,) int64)."""
        code = np.zeros(self.n_envs, np.int32)
        done = np.zeros(self.n_envs, np.int64)
        _lib.check(self._L.rb_batch_status(self._h, _lib.ptr(code), _lib.ptr(done)), "rb_batch_status")
        return code, done

    # ---- contact lists --------------------------------------------------------
    def _max_records(self, max_records):
        """The scene's bound 4 planes' corners + every other body (4 points
        each in a mixed template), capped at 16."""
        if max_records is not None:
            return int(max_records)
        M, P = self.n_bodies, int(np.shape(self.scene.planes)[0])
        mixed = M > 1 and bool(np.any(np.asarray(self.scene.kind) != 0))
        if self.population is not None:
            mixed = M > 1 and bool(np.any(self.population[1] != 0))
        return min(16, 4 * P + (4 if mixed else 1) * (M - 1))

    def contacts(self, envs=None, max_records=None, geometry=True) -> BatchContacts:
        """The contact list of every body of the environments in envs (None:
        all) for the batch's current state, as mj_forward generates it for the
        environment's scene (data.contact, collision.py:57, :72-76), in the
        canonical order of World.contacts().  It steps nothing and changes
        nothing.  max_records: slots per body (None: the scene's bound, at
        most 16; 0: counts only); geometry=False leaves pos and frame out.
        Not under "balls"."""
        ids, n = self._envs(envs)
        R, M = self._max_records(max_records), self.n_bodies
        a = _host_arrays(_CONTACT_FIELDS, (n, M), R, skip=() if geometry else ("pos", "frame"))
        nt = C.c_int64()
        _lib.check(self._L.rb_batch_contacts(self._h, _lib.ptr(ids), n, R, *(_lib.ptr(v) for v in a.values()),
                                             C.byref(nt)), "rb_batch_contacts")
        return BatchContacts(R, *a.values(), nt.value)

    # ---- the device-resident boundary ---------------------------------------
    # Arrays are objects with __cuda_array_interface__ on the batch's device,
    # float64 or float32 whatever the batch's dtype (converted by a cast).
    # Every method but sync() enqueues on the batch's stream and returns.
    def use_stream(self, handle):
        """All later work of the batch goes to the HIP stream `handle` (an
        integer; None or 0: the null stream), after the work on the old one
        finished.  use_stream(torch.cuda.current_stream().cuda_stream) makes
        torch's allocator and the batch agree; the stream stays the caller's."""
        _lib.check(self._L.rb_batch_set_stream(self._h, C.c_void_p(int(handle)) if handle else None),
                   "rb_batch_set_stream")

    def step_async(self, nsteps: int = 1, dt=None, restitution=None, friction=None, threshold=None):
        """step() without the wait and the report (sync())."""
        p = self._params(dt, restitution, friction, threshold)
        _lib.check(self._L.rb_batch_step_async(self._h, int(nsteps), *p), "rb_batch_step_async")

    def sync(self) -> int:
        """Wait for the batch's stream; returns how many environments have
        failed so far.  Raises RbError (EINVAL) naming the environment and the
        body if a set_xfrc_device() since the last sync() held a non-finite
        value: that upload wrote nothing."""
        nf = C.c_int64()
        _lib.check(self._L.rb_batch_sync(self._h, C.byref(nf)), "rb_batch_sync")
        return nf.value

    def set_state_device(self, qpos, qvel, mask=None):
        """set_state() from device arrays qpos (E, M, 7), qvel (E, M, 6) of one
        element type.  mask (E,) bool or uint8 on the device: only the
        environments where it is set are written and reset (None: all); the
        rows of the others are not read."""
        E, M = self.n_envs, self.n_bodies
        ts = _pair_typestr(self.dtype, ("qpos", "qvel"), (qpos, qvel), None)
        q, _ = _device_array("qpos", qpos, (E, M, 7), (ts,))
        v, _ = _device_array("qvel", qvel, (E, M, 6), (ts,))
        m = None if mask is None else _device_array("mask", mask, (E,), ("|b1", "|u1"))[0]
        _lib.check(self._L.rb_batch_set_state_dev(self._h, m, q, v, _IO_CODES[ts]), "rb_batch_set_state_dev")

    def get_state_device(self, out_qpos=None, out_qvel=None, dtype=None):
        """(qpos (E, M, 7), qvel (E, M, 6)) of all environments, written into
        out_qpos / out_qvel, or into new torch tensors of `dtype` ("f64" /
        "f32"; None: the batch's), valid on the batch's stream."""
        E, M = self.n_envs, self.n_bodies
        ts = _pair_typestr(self.dtype, ("out_qpos", "out_qvel"), (out_qpos, out_qvel), dtype)
        q = _new_tensor((E, M, 7), ts, self.device) if out_qpos is None else out_qpos
        v = _new_tensor((E, M, 6), ts, self.device) if out_qvel is None else out_qvel
        qp, _ = _device_array("out_qpos", q, (E, M, 7), (ts,), out=True)
        vp, _ = _device_array("out_qvel", v, (E, M, 6), (ts,), out=True)
        _lib.check(self._L.rb_batch_get_state_dev(self._h, qp, vp, _IO_CODES[ts]), "rb_batch_get_state_dev")
        return q, v

    def set_xfrc_device(self, xfrc):
        """set_xfrc() from a device array (E, M, 6).  A non-finite value is
        found on the device: the upload then writes nothing and the next
        sync() raises; the batch counts as having forces set either way
        (set_xfrc(None) clears them).  Not under "balls"."""
        ts = _pair_typestr(self.dtype, ("xfrc",), (xfrc,), None)
        x, _ = _device_array("xfrc", xfrc, (self.n_envs, self.n_bodies, 6), (ts,))
        _lib.check(self._L.rb_batch_set_xfrc_dev(self._h, x, _IO_CODES[ts]), "rb_batch_set_xfrc_dev")

    def status_device(self, out_code=None, out_steps=None):
        """status() into device arrays: (code (E,) int32, steps_done (E,) int64)."""
        E = self.n_envs
        code = _new_tensor((E,), "<i4", self.device) if out_code is None else out_code
        done = _new_tensor((E,), "<i8", self.device) if out_steps is None else out_steps
        cp, _ = _device_array("out_code", code, (E,), ("<i4",), out=True)
        dp, _ = _device_array("out_steps", done, (E,), ("<i8",), out=True)
        _lib.check(self._L.rb_batch_status_dev(self._h, cp, dp), "rb_batch_status_dev")
        return code, done

    def run_sampled_device(self, nsteps: int, every: int, velocities: bool = True, out_qpos=None, out_qvel=None,
                           dtype=None, dt=None, restitution=None, friction=None, threshold=None):
        """run_sampled() with the samples in device memory: returns (qpos
        (S, E, M, 7), qvel (S, E, M, 6) or None), written into out_qpos /
        out_qvel or new torch tensors of `dtype`, without waiting (sync()
        reports the failed environments)."""
        p = self._params(dt, restitution, friction, threshold)
        nsteps, every = int(nsteps), int(every)
        S = nsteps // every if every >= 1 and nsteps >= 0 else 0
        E, M = self.n_envs, self.n_bodies
        if not velocities and out_qvel is not None:
            raise ValueError("out_qvel: given with velocities=False")
        ts = _pair_typestr(self.dtype, ("out_qpos", "out_qvel"), (out_qpos, out_qvel), dtype)
        q = _new_tensor((S, E, M, 7), ts, self.device) if out_qpos is None else out_qpos
        v = None if not velocities else _new_tensor((S, E, M, 6), ts, self.device) if out_qvel is None else out_qvel
        qp, _ = _device_array("out_qpos", q, (S, E, M, 7), (ts,), out=True)
        vp = None if v is None else _device_array("out_qvel", v, (S, E, M, 6), (ts,), out=True)[0]
        if S > 0 and v is not None and vp is None:
            raise ValueError("out_qvel: null device pointer")
        _lib.check(self._L.rb_batch_run_sampled_dev(self._h, nsteps, every, *p, qp, vp, _IO_CODES[ts]),
                   "rb_batch_run_sampled_dev")
        return q, v

    def run_sampled_impulses_device(self, nsteps: int, every: int, positions: bool = True, velocities: bool = True,
                                    out_qpos=None, out_qvel=None, out_net=None, dtype=None, dt=None, restitution=None,
                                    friction=None, threshold=None):
        """run_sampled_impulses() with the samples in device memory: returns
        (qpos (S, E, M, 7) or None, qvel (S, E, M, 6) or None, net (S, E, M,
        6)), written into out_qpos / out_qvel / out_net or new torch tensors of
        `dtype`, without waiting (sync() reports the failed environments)."""
        p = self._params(dt, restitution, friction, threshold)
        nsteps, every = int(nsteps), int(every)
        S = nsteps // every if every >= 1 and nsteps >= 0 else 0
        E, M = self.n_envs, self.n_bodies
        if not positions and out_qpos is not None:
            raise ValueError("out_qpos: given with positions=False")
        if not velocities and out_qvel is not None:
            raise ValueError("out_qvel: given with velocities=False")
        names = ("out_qpos", "out_qvel", "out_net")
        ts = _pair_typestr(self.dtype, names, (out_qpos, out_qvel, out_net), dtype)
        shapes = ((S, E, M, 7), (S, E, M, 6), (S, E, M, 6))
        want = (positions, velocities, True)
        # the arrays that were given are checked before any is allocated
        arrays = [a if w else None for a, w in zip((out_qpos, out_qvel, out_net), want)]
        for name, a, shape in zip(names, arrays, shapes):
            if a is not None:
                _device_array(name, a, shape, (ts,), out=True)
        arrays = [_new_tensor(shape, ts, self.device) if w and a is None else a
                  for a, w, shape in zip(arrays, want, shapes)]
        ptrs = [None if a is None else _device_array(name, a, shape, (ts,), out=True)[0]
                for name, a, shape in zip(names, arrays, shapes)]
        for name, a, ptr in zip(names, arrays, ptrs):
            if S > 0 and a is not None and ptr is None:
                raise ValueError(f"{name}: null device pointer")
        _lib.check(self._L.rb_batch_run_sampled_impulses_dev(self._h, nsteps, every, *p, *ptrs, _IO_CODES[ts]),
                   "rb_batch_run_sampled_impulses_dev")
        return tuple(arrays)

    def contacts_device(self, max_records=None, geometry=True, dtype=None, out=None) -> BatchContacts:
        """contacts() of all environments into device memory, enqueued on the
        batch's stream without waiting: a BatchContacts whose fields are the
        arrays of `out` (a BatchContacts of an earlier call, or a mapping
        with the fields' names; its max_records and geometry hold) or new
        torch tensors: counts, partner and kind int32, dist, pos and frame of
        `dtype` ("f64" / "f32"; None: the arrays', else the batch's).
        truncated is None: nothing is read back."""
        R, ts, given, ptrs = _resolve_out(
            _CONTACT_FIELDS, (self.n_envs, self.n_bodies), ("partner", "kind", "dist"),
            "partner, kind and dist: all three are required with max_records > 0", out, max_records, dtype,
            self.dtype, self.device, lambda: self._max_records(max_records), skip=() if geometry else ("pos", "frame"))
        _lib.check(self._L.rb_batch_contacts_dev(self._h, R, *ptrs.values(), _IO_CODES[ts]), "rb_batch_contacts_dev")
        return BatchContacts(R, *given.values(), None)      # (with R == 0 the library takes counts alone)

    # ---- the impulses of the next step ------------------------------------------
    def impulses(self, envs=None, max_records=None, dt=None, restitution=None, friction=None,
                 threshold=None) -> BatchImpulses:
        """What the next step(1, dt, restitution, friction, threshold) does to
        every body of the environments in envs (None: all), contact by contact:
        the contact list of contacts(), jn and jt of every record
        (collision.py:7-48, :72-88), the velocity the solve leaves and the
        body's net contact impulse.  It steps nothing and changes nothing.
        max_records as for contacts() (0: counts, vel and net only); the step
        parameters default to the scene's, as for step().  Not under "balls"."""
        ids, n = self._envs(envs)
        p = self._params(dt, restitution, friction, threshold)
        R, M = self._max_records(max_records), self.n_bodies
        a = _host_arrays(_IMPULSE_FIELDS, (n, M), R)
        nt = C.c_int64()
        _lib.check(self._L.rb_batch_impulses(self._h, _lib.ptr(ids), n, R, *p, *(_lib.ptr(v) for v in a.values()),
                                             C.byref(nt)), "rb_batch_impulses")
        return BatchImpulses(*a.values(), nt.value)

    def impulses_device(self, max_records=None, dtype=None, out=None, dt=None, restitution=None, friction=None,
                        threshold=None) -> BatchImpulses:
        """impulses() of all environments into device memory, enqueued on the
        batch's stream without waiting, with the conventions of
        contacts_device(): a BatchImpulses whose fields are the arrays of `out`
        (a BatchImpulses of an earlier call, or a mapping with the fields'
        names; its max_records holds; vel and net may be left out) or new
        torch tensors: counts, partner and kind int32, the rest of `dtype`
        ("f64" / "f32"; None: the arrays', else the batch's).  truncated is
        None: nothing is read back."""
        p = self._params(dt, restitution, friction, threshold)
        R, ts, given, ptrs = _resolve_out(
            _IMPULSE_FIELDS, (self.n_envs, self.n_bodies), ("partner", "kind", "dist", "jn", "jt"),
            "partner, kind, dist, jn and jt: all five with max_records > 0, none with 0", out, max_records, dtype,
            self.dtype, self.device, lambda: self._max_records(max_records), exclusive=True)
        _lib.check(self._L.rb_batch_impulses_dev(self._h, R, *p, *ptrs.values(), _IO_CODES[ts]), "rb_batch_impulses_dev")
        return BatchImpulses(*given.values(), None)
