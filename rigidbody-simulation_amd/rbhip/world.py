"""World: a scene resident on one MI355X, stepped by librbhip.so.

Host side of the drop-in boundary.  It replaces the MuJoCo model/data pair
the reference step functions mutate (collision.py:56, time_integeration.py:13,
multi_sphere_bounce.py:42) with explicit arrays; the state crosses the
boundary in the reference's own layout (qpos stride 7, qvel stride 6).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _lib
from ._devarray import (_CONTACT_FIELDS, _IMPULSE_FIELDS, _IO_CODES, _device_array, _host_arrays, _new_tensor,
                        _pair_typestr, _resolve_out)
from .scenes import Scene

COMM_ID_BYTES = 128      # ncclUniqueId (rccl.h NCCL_UNIQUE_ID_BYTES)
QUERY_PARTNERS = 32      # the partner list of the contact query's search (rb_query_contacts)
QUERY_NO_LIST = -2       # counts of a body whose list could not be built


class WorldContacts:
    """The contact lists of a world's state (World.query_contacts /
    query_contacts_device): the fields of BatchContacts for one row, dense
    arrays with R = max_records slots per body.

    counts (1, count) int32: the true number of contacts of each listed body,
    also where it exceeds R (then only the first R records are kept); -2 for a
    body whose list could not be built (more than 32 partners in reach, a
    non-finite or out-of-range position, or the query's table overflowed).
    partner, kind (1, count, R) int32 and dist (1, count, R): partner is a
    global body id or -1 - plane, kind an RB_CK_* code.  pos, frame
    (1, count, R, 3), or None without geometry: frame is the raw normal from
    geom1 to geom2 (geom1: the plane; the lower id of two spheres or two
    boxes; the sphere of a sphere-box pair).  Slots at or past a body's count
    hold kind -1 and zeros.  truncated: the number of bodies with count > R
    (None for the device form, which does not wait).  With max_records 0 only
    counts is set.  first: the id of the first listed body."""

    def __init__(self, max_records, counts, partner, kind, dist, pos, frame, truncated, first=0):
        self.max_records = max_records
        self.counts, self.partner, self.kind, self.dist = counts, partner, kind, dist
        self.pos, self.frame = pos, frame
        self.truncated = truncated
        self.first = first

    def to_csr(self):
        """The lists in the CSR shape of World.contacts(): (counts (count,),
        partner, kind, dist, pos, frame), the last five flat over the kept
        records, body by body (pos / frame None without geometry; all five
        None with max_records 0).  counts stays as returned: past max_records
        for a truncated body (min(counts, max_records) records are kept), -2
        for a body without a list (none).  Host arrays only."""
        cnt = np.asarray(self.counts).reshape(-1)
        if self.partner is None:
            return cnt.copy(), None, None, None, None, None
        R = self.max_records
        keep = np.arange(R)[None, :] < np.clip(cnt, 0, R)[:, None]
        out = [cnt.copy()]
        for a in (self.partner, self.kind, self.dist, self.pos, self.frame):
            out.append(None if a is None else np.asarray(a).reshape((cnt.size, R) + np.shape(a)[3:])[keep])
        return tuple(out)


class WorldImpulses:
    """What the next step does to each listed body of a world, contact by
    contact (World.query_impulses / query_impulses_device): the fields of
    BatchImpulses for one row, dense arrays with R = max_records slots per body.

    counts (1, count), partner, kind, dist (1, count, R): word for word the
    fields of WorldContacts for the same state, range and R (-2 in counts for a
    body without a list).  jn (1, count, R), jt (1, count, R, 3): the two
    return values of compute_collision_impulse_friction (collision.py:7-48)
    for the contact, 0 where the step skips it or it separates.  vel
    (1, count, 6): (v, omega) after gravity, applied forces and all the body's
    contacts, the qvel of the next step(1).  net (1, count, 6): the body's net
    contact impulse and net angular impulse about its centre.  vel and net do
    not depend on R; a body without a list has zero rows.  With max_records 0
    the five record fields are None (the "sensor only" call).  truncated: the
    bodies with count > R (None for the device form, which does not wait).
    first: the id of the first listed body."""

    def __init__(self, counts, partner, kind, dist, jn, jt, vel, net, truncated, first=0):
        self.counts, self.partner, self.kind, self.dist = counts, partner, kind, dist
        self.jn, self.jt, self.vel, self.net = jn, jt, vel, net
        self.truncated = truncated
        self.first = first

    @property
    def max_records(self) -> int:
        return 0 if self.partner is None else int(self.partner.shape[-1])


class World:
    def __init__(self, scene: Scene, device: int = 0, dtype: str = "f64", rank: int = 0,
                 world_size: int = 1, max_partners: int = 16, bucket_capacity: int = 0,
                 normal_convention: Optional[str] = None, law: str = "mujoco", tol: float = 0.01):
        """law: "mujoco" — the per-body Gauss-Seidel law of collision.py /
        multi_sphere_bounce.py; "balls" — the two-ball law of
        ball_collision.py:73-125 (tol: its contact tolerance, :102)."""
        L = _lib.load()
        self.scene = scene
        self.dtype, self.device = dtype, device
        self.rank, self.world_size = rank, world_size
        nc = normal_convention or scene.normal_convention
        self._kind = np.ascontiguousarray(scene.kind, np.int32)
        self._mass = np.ascontiguousarray(scene.mass, np.float64)
        self._inertia = np.ascontiguousarray(scene.inertia, np.float64)
        self._size = np.ascontiguousarray(scene.size, np.float64)
        self._planes = np.ascontiguousarray(scene.planes, np.float64)
        d = _lib.SceneDesc()
        d.n_bodies = scene.n
        d.n_planes = self._planes.shape[0]
        d.dtype = _lib.RB_F64 if dtype == "f64" else _lib.RB_F32
        d.normal_convention = _lib.RB_NORMAL_RAW if nc == "raw" else _lib.RB_NORMAL_ORIENTED
        d.device, d.rank, d.world_size = device, rank, world_size
        d.max_partners, d.bucket_capacity = max_partners, bucket_capacity
        d.kind, d.mass = _lib.ptr(self._kind), _lib.ptr(self._mass)
        d.inertia, d.size = _lib.ptr(self._inertia), _lib.ptr(self._size)
        d.planes = _lib.ptr(self._planes) if d.n_planes else None
        for k in range(3):
            d.gravity[k] = float(scene.gravity[k])
        h = C.c_void_p()
        _lib.check(L.rb_world_create(C.byref(h), C.byref(d)), "rb_world_create")
        self._h = h
        self._L = L
        # records per body (rb_world_create): 4 per plane, 1 per sphere
        # partner, up to 4 per partner in scenes with boxes; max_partners can
        # grow in a guarded chunk (16 -> 32), so contacts() recomputes it
        self._n_planes = d.n_planes
        self._any_box = bool(np.any(self._kind != 0))
        self.maxrec = self._maxrec(max_partners)
        # the bound of rb_query_contacts' staging buffer, read when the world is created
        try:
            self._stage_limit = int(os.environ.get("RBHIP_CONTACT_STAGE_BYTES", "0"))
        except ValueError:
            self._stage_limit = 0
        if self._stage_limit <= 0:
            self._stage_limit = 256 << 20
        n_owned, bpb = C.c_int64(), C.c_int64()
        _lib.check(L.rb_query(h, C.byref(n_owned), C.byref(bpb)), "rb_query")
        self.n_owned = n_owned.value
        self.bytes_per_body_step = bpb.value
        S = -(-scene.n // world_size)
        self.lo = S * rank
        self.hi = min(self.lo + S, scene.n)
        self.law = "mujoco"
        if law != "mujoco":
            self.set_contact_law(law, tol)
        self.set_state(scene.qpos0, scene.qvel0)

    def _maxrec(self, max_partners: int) -> int:
        return 4 * self._n_planes + (4 if self._any_box else 1) * max_partners

    def set_contact_law(self, law: str, tol: float = 0.01):
        """Switch between the default law and the two-ball law (rb_set_contact_law)."""
        code = {"mujoco": _lib.RB_LAW_MUJOCO, "balls": _lib.RB_LAW_BALLS}[law]
        _lib.check(self._L.rb_set_contact_law(self._h, code, float(tol)), "rb_set_contact_law")
        self.law, self.tol = law, float(tol)

    # ---- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.rb_world_destroy(self._h)
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

    # ---- state --------------------------------------------------------------
    def set_state(self, qpos, qvel):
        q = np.ascontiguousarray(qpos, np.float64).reshape(self.scene.n, 7)
        v = np.ascontiguousarray(qvel, np.float64).reshape(self.scene.n, 6)
        _lib.check(self._L.rb_set_state(self._h, _lib.ptr(q), _lib.ptr(v)), "rb_set_state")

    def get_state(self, qpos=None, qvel=None):
        """Returns global (N,7)/(N,6) arrays; only this shard's rows are filled."""
        q = np.zeros((self.scene.n, 7)) if qpos is None else qpos
        v = np.zeros((self.scene.n, 6)) if qvel is None else qvel
        _lib.check(self._L.rb_get_state(self._h, _lib.ptr(q), _lib.ptr(v)), "rb_get_state")
        return q, v

    def set_xfrc(self, xfrc):
        x = None if xfrc is None else np.ascontiguousarray(xfrc, np.float64).reshape(self.scene.n, 6)
        _lib.check(self._L.rb_set_xfrc(self._h, _lib.ptr(x)), "rb_set_xfrc")

    def set_stream(self, stream_handle: int):
        """Enqueue all later work on this hipStream_t (0 = HIP's null stream,
        which is torch's default stream)."""
        _lib.check(self._L.rb_set_stream(self._h, C.c_void_p(stream_handle or None)), "rb_set_stream")

    # ---- the device-resident boundary ---------------------------------------
    # Arrays are objects with __cuda_array_interface__ on the world's device
    # (torch tensors), float64 or float32 whatever the world's dtype (converted
    # by a cast).  Every call is enqueued on the world's stream (set_stream)
    # and returns without waiting, but for the cases each docstring names;
    # sync() waits.  One rank only (a shard's boundary is gpos_buffer()).
    def get_state_device(self, out_qpos=None, out_qvel=None, dtype=None):
        """(qpos (N, 7), qvel (N, 6)) written into out_qpos / out_qvel, or
        into new torch tensors of `dtype` ("f64" / "f32"; None: the world's),
        valid on the world's stream.  After a run in the tile form it waits
        for that run's check, like every reader of the state."""
        n = self.scene.n
        ts = _pair_typestr(self.dtype, ("out_qpos", "out_qvel"), (out_qpos, out_qvel), dtype)
        q = _new_tensor((n, 7), ts, self.device) if out_qpos is None else out_qpos
        v = _new_tensor((n, 6), ts, self.device) if out_qvel is None else out_qvel
        qp, _ = _device_array("out_qpos", q, (n, 7), (ts,), out=True)
        vp, _ = _device_array("out_qvel", v, (n, 6), (ts,), out=True)
        _lib.check(self._L.rb_get_state_dev(self._h, qp, vp, _IO_CODES[ts]), "rb_get_state_dev")
        return q, v

    def set_state_device(self, qpos, qvel, refit=True):
        """set_state() from device arrays qpos (N, 7), qvel (N, 6) of one
        element type.  refit=True fits the broadphase layout to the new
        positions as set_state() does, through one read-back of the positions
        (it waits: for a new scene); refit=False keeps the layout and only
        enqueues (a reset inside the extent the world was fitted for).  The
        layout decides speed, never bits."""
        n = self.scene.n
        ts = _pair_typestr(self.dtype, ("qpos", "qvel"), (qpos, qvel), None)
        q, _ = _device_array("qpos", qpos, (n, 7), (ts,))
        v, _ = _device_array("qvel", qvel, (n, 6), (ts,))
        _lib.check(self._L.rb_set_state_dev(self._h, q, v, _IO_CODES[ts], 1 if refit else 0), "rb_set_state_dev")

    def set_xfrc_device(self, xfrc):
        """set_xfrc() from a device array (N, 6).  The first call after "no
        forces" allocates the force rows (as set_xfrc does); later calls only
        enqueue.  set_xfrc(None) clears the forces."""
        ts = _pair_typestr(self.dtype, ("xfrc",), (xfrc,), None)
        x, _ = _device_array("xfrc", xfrc, (self.scene.n, 6), (ts,))
        _lib.check(self._L.rb_set_xfrc_dev(self._h, x, _IO_CODES[ts]), "rb_set_xfrc_dev")

    def run_sampled_device(self, nsteps: int, every: int, velocities: bool = True, out_qpos=None, out_qvel=None,
                           dtype=None, dt=None, restitution=None, friction=None, threshold=None):
        """nsteps steps, the state sampled after every `every` of them into
        device memory: returns (qpos (S, N, 7), qvel (S, N, 6) or None),
        S = nsteps // every, written into out_qpos / out_qvel or new torch
        tensors of `dtype`.  Sample s is what step(every) + get_state() returns
        at that point; the steps left over are taken at the end.  A
        composition of step_async() and get_state_device(): nothing waits
        (but a tile-form run's check, as in get_state_device)."""
        nsteps, every = int(nsteps), int(every)
        if every < 1 or nsteps < 0:
            raise ValueError(f"nsteps {nsteps}, every {every}: expected nsteps >= 0 and every >= 1")
        if not velocities and out_qvel is not None:
            raise ValueError("out_qvel: given with velocities=False")
        S, n = nsteps // every, self.scene.n
        ts = _pair_typestr(self.dtype, ("out_qpos", "out_qvel"), (out_qpos, out_qvel), dtype)
        q = _new_tensor((S, n, 7), ts, self.device) if out_qpos is None else out_qpos
        v = None if not velocities else _new_tensor((S, n, 6), ts, self.device) if out_qvel is None else out_qvel
        qp, _ = _device_array("out_qpos", q, (S, n, 7), (ts,), out=True)
        vp = None if v is None else _device_array("out_qvel", v, (S, n, 6), (ts,), out=True)[0]
        if S > 0 and n > 0 and (qp is None or (v is not None and vp is None)):
            raise ValueError("out_qpos / out_qvel: null device pointer")
        p = self._params(dt, restitution, friction, threshold)
        esz = 8 if ts == "<f8" else 4
        for s in range(S):
            _lib.check(self._L.rb_step_async(self._h, every, *p), "rb_step_async")
            qs = C.c_void_p(qp.value + s * n * 7 * esz)
            vs = None if vp is None else C.c_void_p(vp.value + s * n * 6 * esz)
            _lib.check(self._L.rb_get_state_dev(self._h, qs, vs, _IO_CODES[ts]), "rb_get_state_dev")
        if nsteps - S * every:
            _lib.check(self._L.rb_step_async(self._h, nsteps - S * every, *p), "rb_step_async")
        return q, v

    # ---- stepping -----------------------------------------------------------
    def _params(self, dt, restitution, friction, threshold):
        sc = self.scene
        return (sc.dt if dt is None else dt, sc.restitution if restitution is None else restitution,
                sc.friction if friction is None else friction,
                sc.threshold if threshold is None else threshold)

    def step(self, nsteps: int = 1, dt=None, restitution=None, friction=None, threshold=None):
        p = self._params(dt, restitution, friction, threshold)
        _lib.check(self._L.rb_step(self._h, int(nsteps), *p), "rb_step")

    def step_async(self, nsteps: int = 1, dt=None, restitution=None, friction=None, threshold=None):
        p = self._params(dt, restitution, friction, threshold)
        _lib.check(self._L.rb_step_async(self._h, int(nsteps), *p), "rb_step_async")

    def sync(self):
        _lib.check(self._L.rb_sync(self._h), "rb_sync")

    # ---- sharded stepping ---------------------------------------------------
    def shard_step(self, dt=None, restitution=None, friction=None, threshold=None):
        p = self._params(dt, restitution, friction, threshold)
        _lib.check(self._L.rb_shard_step(self._h, *p), "rb_shard_step")

    def shard_exchange_done(self):
        _lib.check(self._L.rb_shard_exchange_done(self._h), "rb_shard_exchange_done")

    def gpos_buffer(self):
        """(device pointer, elements per shard, bytes per element) of the
        replicated [P][S][4] position buffer."""
        p, n, b = C.c_void_p(), C.c_int64(), C.c_int32()
        _lib.check(self._L.rb_gpos_buffer(self._h, C.byref(p), C.byref(n), C.byref(b)), "rb_gpos_buffer")
        return p.value, n.value, b.value

    def gquat_buffer(self):
        """(device pointer, elements per shard, bytes per element) of the
        replicated [P][S][4] orientation buffer the same exchange fills in
        box worlds; (None, 0, esz) for sphere-only worlds."""
        p, n, b = C.c_void_p(), C.c_int64(), C.c_int32()
        _lib.check(self._L.rb_gquat_buffer(self._h, C.byref(p), C.byref(n), C.byref(b)), "rb_gquat_buffer")
        return p.value, n.value, b.value

    # ---- in-library exchange (RCCL communicator owned by the world) ---------
    @staticmethod
    def comm_unique_id() -> bytes:
        """A new communicator id (rank 0 makes it, every rank joins with it)."""
        L = _lib.load()
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _lib.check(L.rb_comm_unique_id(buf, COMM_ID_BYTES), "rb_comm_unique_id")
        return buf.raw

    def shard_comm_init(self, uid: bytes):
        """Join the world's ranks in one RCCL communicator (blocks until all have)."""
        if len(uid) != COMM_ID_BYTES:
            raise ValueError(f"communicator id must be {COMM_ID_BYTES} bytes")
        _lib.check(self._L.rb_shard_comm_init(self._h, C.c_char_p(uid), COMM_ID_BYTES), "rb_shard_comm_init")

    def p2p_handles(self) -> bytes:
        """This rank's IPC handles for the peer-to-peer exchange."""
        n = C.c_int64()
        _lib.check(self._L.rb_p2p_handles(self._h, None, 0, C.byref(n)), "rb_p2p_handles")
        buf = C.create_string_buffer(n.value)
        _lib.check(self._L.rb_p2p_handles(self._h, buf, n.value, C.byref(n)), "rb_p2p_handles")
        return buf.raw

    def p2p_connect(self, all_handles: bytes):
        """Map every peer's buffers (all ranks' handles concatenated in rank
        order); collective: no rank may step before all have connected."""
        _lib.check(self._L.rb_p2p_connect(self._h, C.c_char_p(all_handles), len(all_handles)), "rb_p2p_connect")

    def p2p_halo(self, enable: bool = True):
        """Halo mode of the peer-to-peer exchange (push only the bodies a peer
        can reach); collective, after p2p_connect."""
        _lib.check(self._L.rb_p2p_halo(self._h, 1 if enable else 0), "rb_p2p_halo")

    def shard_run(self, nsteps: int = 1, dt=None, restitution=None, friction=None, threshold=None):
        """nsteps sharded steps with the in-library exchange (enqueued only)."""
        p = self._params(dt, restitution, friction, threshold)
        _lib.check(self._L.rb_shard_run(self._h, int(nsteps), *p), "rb_shard_run")

    # ---- parity support -----------------------------------------------------
    def record_contacts(self, enable: bool = True):
        _lib.check(self._L.rb_record_contacts(self._h, int(bool(enable))), "rb_record_contacts")

    # ---- the contact query ---------------------------------------------------
    def _query_range(self, first, count, max_records, per_slot, per_body=4):
        """per_slot, per_body: the bytes of one record slot and of one body's
        own words in the host form's staging buffer."""
        n = self.scene.n
        first = int(first)
        count = n - first if count is None else int(count)
        if max_records is None:
            # the scene's bound, as long as one body's slots fit the staging
            # buffer of the host form (rb_query_contacts, rb_query_impulses)
            R = 4 * self._n_planes + (4 if self._any_box else 1) * QUERY_PARTNERS
            R = max(0, min(R, (self._stage_limit - per_body) // per_slot))
        else:
            R = int(max_records)
        return first, count, R

    def query_contacts(self, first=0, count=None, max_records=None, geometry=True, strict=True) -> WorldContacts:
        """The contact list of bodies [first, first + count) (count None: up
        to the last) for the world's current state, as mj_forward generates it
        (data.contact, collision.py:57, :72-76), in the canonical order of
        contacts(), with pos and frame.  It steps nothing and changes nothing
        a step can see; like get_state() it first finishes the world's pending
        work.  max_records: slots per body (None: the scene's bound, 4 per
        plane + 32 partners' records; 0: counts only); geometry=False leaves
        pos and frame out.  A body whose list cannot be built (WorldContacts)
        raises RbError (EOVERFLOW / EDOM) if strict; with strict=False the
        arrays are returned with -2 in its counts.  One rank, not under
        "balls"."""
        first, count, R = self._query_range(first, count, max_records, 8 * (7 if geometry else 1) + 8)
        c = max(count, 0)
        a = _host_arrays(_CONTACT_FIELDS, (1, c), R, skip=() if geometry else ("pos", "frame"))
        nt = C.c_int64()
        rc = self._L.rb_query_contacts(self._h, first, count, R, *(_lib.ptr(v) for v in a.values()), C.byref(nt))
        # (EOVERFLOW / EDOM of a query with valid arguments: a body without a list, every array written)
        if rc != _lib.RB_OK and (strict or rc not in (-75, -33)):
            _lib.check(rc, "rb_query_contacts")
        return WorldContacts(R, *a.values(), nt.value, first)

    def query_contacts_device(self, first=0, count=None, max_records=None, geometry=True, dtype=None,
                              out=None) -> WorldContacts:
        """query_contacts() into device memory, enqueued on the world's stream
        without waiting (but a tile-form run's check, as get_state_device): a
        WorldContacts whose fields are the arrays of `out` (a WorldContacts of
        an earlier call, or a mapping with the fields' names; its max_records
        and geometry hold) or new torch tensors: counts, partner and kind
        int32, dist, pos and frame of `dtype` ("f64" / "f32"; None: the
        arrays', else the world's).  truncated is None: nothing is read back,
        and a body without a list shows as -2 in counts alone."""
        # (with `out` its partner sets R: only first and count are taken here, `bound` is unused)
        first, count, bound = self._query_range(first, count, max_records if out is None else 0,
                                                8 * (7 if geometry else 1) + 8)
        c = max(count, 0)
        R, ts, given, ptrs = _resolve_out(
            _CONTACT_FIELDS, (1, c), ("partner", "kind", "dist") if c > 0 else (),
            "partner, kind and dist: all three are required with max_records > 0", out, max_records, dtype,
            self.dtype, self.device, lambda: bound, skip=() if geometry else ("pos", "frame"))
        _lib.check(self._L.rb_query_contacts_dev(self._h, first, count, R, *ptrs.values(), _IO_CODES[ts]),
                   "rb_query_contacts_dev")
        return WorldContacts(R, *given.values(), None, first)   # (with R == 0 the library takes counts alone)

    # ---- the impulses of the next step ----------------------------------------
    _IMPULSE_SLOT, _IMPULSE_BODY = 5 * 8 + 8, 4 + 2 * 6 * 8      # staging bytes: a record slot; counts, vel and net

    def query_impulses(self, first=0, count=None, max_records=None, dt=None, restitution=None, friction=None,
                       threshold=None, strict=True) -> WorldImpulses:
        """What the next step(1, dt, restitution, friction, threshold) does to
        bodies [first, first + count) (count None: up to the last), contact by
        contact: the contact list of query_contacts(), jn and jt of every
        record (collision.py:7-48, :72-88), the velocity the solve leaves and
        the body's net contact impulse, applied forces (set_xfrc) included.
        It steps nothing and changes nothing a step can see; like get_state()
        it first finishes the world's pending work.  max_records as for
        query_contacts() (0: counts, vel and net only); the step parameters
        default to the scene's, as for step().  A body whose list cannot be
        built raises RbError if strict, as query_contacts() does.  One rank,
        not under "balls"."""
        first, count, R = self._query_range(first, count, max_records, self._IMPULSE_SLOT, self._IMPULSE_BODY)
        p = self._params(dt, restitution, friction, threshold)
        a = _host_arrays(_IMPULSE_FIELDS, (1, max(count, 0)), R)
        nt = C.c_int64()
        rc = self._L.rb_query_impulses(self._h, first, count, R, *p, *(_lib.ptr(v) for v in a.values()), C.byref(nt))
        # (EOVERFLOW / EDOM of a query with valid arguments: a body without a list, every array written)
        if rc != _lib.RB_OK and (strict or rc not in (-75, -33)):
            _lib.check(rc, "rb_query_impulses")
        return WorldImpulses(*a.values(), nt.value, first)

    def query_impulses_device(self, first=0, count=None, max_records=None, dt=None, restitution=None, friction=None,
                              threshold=None, dtype=None, out=None) -> WorldImpulses:
        """query_impulses() into device memory, enqueued on the world's stream
        without waiting, with the conventions of query_contacts_device(): a
        WorldImpulses whose fields are the arrays of `out` (a WorldImpulses of
        an earlier call, or a mapping with the fields' names; its max_records
        holds; vel and net may be left out) or new torch tensors: counts,
        partner and kind int32, the rest of `dtype` ("f64" / "f32"; None: the
        arrays', else the world's).  truncated is None: nothing is read back,
        and a body without a list shows as -2 in counts alone."""
        first, count, bound = self._query_range(first, count, max_records if out is None else 0, self._IMPULSE_SLOT,
                                                self._IMPULSE_BODY)
        p = self._params(dt, restitution, friction, threshold)
        c = max(count, 0)
        R, ts, given, ptrs = _resolve_out(
            _IMPULSE_FIELDS, (1, c), ("partner", "kind", "dist", "jn", "jt") if c > 0 else (),
            "partner, kind, dist, jn and jt: all five with max_records > 0, none with 0", out, max_records, dtype,
            self.dtype, self.device, lambda: bound, exclusive=True)
        _lib.check(self._L.rb_query_impulses_dev(self._h, first, count, R, *p, *ptrs.values(), _IO_CODES[ts]),
                   "rb_query_impulses_dev")
        return WorldImpulses(*given.values(), None, first)

    def contacts(self):
        """Contact list of the most recent step, CSR over owned bodies:
        (counts, partner, kind, dist)."""
        n = self.n_owned
        self.maxrec = self._maxrec(self.stats()["max_partners"])   # (the library may have grown it)
        cap = max(1, n * self.maxrec)
        cnt = np.zeros(n, np.int32)
        par = np.zeros(cap, np.int32)
        kin = np.zeros(cap, np.int32)
        dis = np.zeros(cap)
        tot = C.c_int64()
        _lib.check(self._L.rb_get_contacts(self._h, _lib.ptr(cnt), _lib.ptr(par), _lib.ptr(kin),
                                           _lib.ptr(dis), cap, C.byref(tot)), "rb_get_contacts")
        t = tot.value
        return cnt, par[:t], kin[:t], dis[:t]

    def stats(self) -> dict:
        """Counters of the world (rb_world_stats, include/rbhip.h RB_STAT_*):
        the step kernel form, tile-form runs and roll-backs, refits, ..."""
        n = len(_lib.STAT_NAMES)
        buf = (C.c_int64 * n)()
        rc = self._L.rb_world_stats(self._h, buf, n)
        if rc < 0:
            _lib.check(rc, "rb_world_stats")
        return {k: int(buf[i]) for i, k in enumerate(_lib.STAT_NAMES[:rc])}

    def kernel_timing(self, enable: bool):
        """Toggle per-launch HIP-event timing of the step kernel; returns the
        (average ms, launches) collected since it was last enabled."""
        avg, n = C.c_double(), C.c_int64()
        _lib.check(self._L.rb_kernel_timing(self._h, int(bool(enable)), C.byref(avg), C.byref(n)),
                   "rb_kernel_timing")
        return avg.value, n.value


def kat_impulse(inp: np.ndarray, dtype: str = "f64", device: int = 0) -> np.ndarray:
    """Device known-answer entry: a1 (collision.py:7-48) then a2
    (physics_utils.py:25-49) per row of inp[:, 24] -> out[:, 10]."""
    L = _lib.load()
    inp = np.ascontiguousarray(inp, np.float64).reshape(-1, 24)
    out = np.zeros((inp.shape[0], 10))
    _lib.check(L.rb_kat_impulse(device, _lib.RB_F64 if dtype == "f64" else _lib.RB_F32, inp.shape[0],
                                _lib.ptr(inp), _lib.ptr(out)), "rb_kat_impulse")
    return out


def kat_inertia(inp: np.ndarray, dtype: str = "f64", device: int = 0) -> np.ndarray:
    """Device known-answer entry: compute_inertia_tensor_world (collision.py:51-53)
    and its inverse per row of inp[:, 7] -> out[:, 18]."""
    L = _lib.load()
    inp = np.ascontiguousarray(inp, np.float64).reshape(-1, 7)
    out = np.zeros((inp.shape[0], 18))
    _lib.check(L.rb_kat_inertia(device, _lib.RB_F64 if dtype == "f64" else _lib.RB_F32, inp.shape[0],
                                _lib.ptr(inp), _lib.ptr(out)), "rb_kat_inertia")
    return out


def kat_apply(inp: np.ndarray, dtype: str = "f64", device: int = 0) -> np.ndarray:
    """Device entry for apply_impulse_friction (physics_utils.py:25-49) with
    given impulses, per row of inp[:, 26] -> out[:, 6] = v', w'."""
    L = _lib.load()
    inp = np.ascontiguousarray(inp, np.float64).reshape(-1, 26)
    out = np.zeros((inp.shape[0], 6))
    _lib.check(L.rb_kat_apply(device, _lib.RB_F64 if dtype == "f64" else _lib.RB_F32, inp.shape[0],
                              _lib.ptr(inp), _lib.ptr(out)), "rb_kat_apply")
    return out


def kat_pair_impulse(inp: np.ndarray, dtype: str = "f64", device: int = 0) -> np.ndarray:
    """Device known-answer entry: compute_collision_impulse (ball_collision.py:53-68)
    per row of inp[:, 27] = m, e, mu, v, w, r, n, I_inv(9) -> out[:, 3]."""
    L = _lib.load()
    inp = np.ascontiguousarray(inp, np.float64).reshape(-1, 27)
    out = np.zeros((inp.shape[0], 3))
    _lib.check(L.rb_kat_pair_impulse(device, _lib.RB_F64 if dtype == "f64" else _lib.RB_F32, inp.shape[0],
                                     _lib.ptr(inp), _lib.ptr(out)), "rb_kat_pair_impulse")
    return out


def kat_narrow(inp: np.ndarray, dtype: str = "f64", device: int = 0) -> np.ndarray:
    """Device entry for the box-involved narrowphase (rb_boxes.hpp; SURVEY
    §8f row 4) per row of inp[:, 22] = kind1, kind2, c1, q1, s1, c2, q2, s2
    -> out[:, 33] = count, then per contact dist, pos[3], frame[3], kind."""
    L = _lib.load()
    inp = np.ascontiguousarray(inp, np.float64).reshape(-1, 22)
    out = np.zeros((inp.shape[0], 33))
    _lib.check(L.rb_kat_narrow(device, _lib.RB_F64 if dtype == "f64" else _lib.RB_F32, inp.shape[0],
                               _lib.ptr(inp), _lib.ptr(out)), "rb_kat_narrow")
    return out
