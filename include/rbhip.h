/*
 * rbhip.h — C-ABI of librbhip.so, the MI355X-native (gfx950) many-body
 * rigid-body stepper that sits behind the src/physics / src/simulation call
 * surface of pratyay2510/RigidBody-Simulation.
 *
 * The reference has no FFI: every entry point below replaces a Python call
 * site of the reference (cited per function, paths relative to the reference
 * repository root).  The ctypes binding a maintainer would add on the
 * reference side is shown in INTEGRATION.md; the in-tree binding is
 * rigidbody-simulation_amd/rbhip/_lib.py.
 *
 * Conventions
 *   - Every function returns 0 on success or a negative errno-style code
 *     (RB_E*); rb_last_error() returns a thread-local message for the last
 *     failure on the calling thread.
 *   - Host buffers are owned by the caller and never retained past a call.
 *     Device buffers are owned by the library (a world).
 *   - A world handle is not thread-safe: one world per host thread.
 *   - Results are deterministic: independent of launch geometry, of the
 *     number of ranks a scene is sharded over, and of run-to-run scheduling.
 *   - State layout at the boundary is the reference's MuJoCo layout:
 *     qpos stride 7 (x y z qw qx qy qz), qvel stride 6 (vx vy vz wx wy wz),
 *     body k (0-based among free bodies) at qpos[7k], qvel[6k]
 *     (multi_sphere_bounce.py:50-51 with the SURVEY D1 off-by-one fixed).
 *     Inside the library the state is struct-of-arrays in HBM.
 */
#ifndef RBHIP_H
#define RBHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------- */
#define RB_OK            0
#define RB_EINVAL      (-22)  /* bad argument / descriptor                      */
#define RB_ENOMEM      (-12)  /* device or host allocation failed               */
#define RB_ENODEV      (-19)  /* no HIP device / HIP runtime failure            */
#define RB_EOVERFLOW   (-75)  /* contact or broadphase-bucket capacity exceeded */
#define RB_EUNSUPPORTED (-95) /* unsupported combination (e.g. the two-ball law in a sharded world) */
#define RB_EDOM        (-33)  /* non-finite or out-of-range body position       */

/* ---- enums ------------------------------------------------------------- */
#define RB_BODY_SPHERE   0    /* size = (radius, -, -)                          */
#define RB_BODY_BOX      1    /* size = half extents (hx, hy, hz)               */

#define RB_F64           0
#define RB_F32           1

/* MuJoCo stores one normal per contact, pointing geom1 -> geom2.
 * RAW applies it unchanged to both bodies (what collision.py:27 does);
 * ORIENTED flips it for the body that is geom1 so it always points toward
 * the body being solved.  Plane contacts are identical in both modes. */
#define RB_NORMAL_ORIENTED 0
#define RB_NORMAL_RAW      1

/* contact laws (rb_set_contact_law) */
#define RB_LAW_MUJOCO    0    /* the per-body Gauss-Seidel law of collision.py / multi_sphere_bounce.py (default) */
#define RB_LAW_BALLS     1    /* the symmetric two-ball law of ball_collision.py */

/* contact kinds reported by rb_get_contacts */
#define RB_CK_PLANE_SPHERE   0
#define RB_CK_PLANE_BOX0     1   /* 1 + corner index (0..7, corner bits i&1,i&2,i&4) */
#define RB_CK_SPHERE_SPHERE 16
/* Box-involved kinds are this project's restatement of MuJoCo's sphere-box /
 * box-box primitives (not available offline): parity against MuJoCo is
 * UNPINNED (the reference's only box, models/cube.xml:35, never meets
 * another box or a sphere).  Known divergence: a face contact keeps at most
 * the 4 deepest clipped points, where mjc_BoxBox may return more and select
 * differently. */
#define RB_CK_SPHERE_BOX    17   /* sphere = geom1 (MuJoCo dispatches by geom type) */
#define RB_CK_BOX_BOX0      32   /* 32 + k: k-th face-clip point of a box pair (k < 4) */
#define RB_CK_BOX_EDGE      40   /* edge-edge point of a box pair */

/* ---- scene descriptor -------------------------------------------------- */
typedef struct rb_scene_desc {
    int64_t n_bodies;          /* global body count N                                  */
    int32_t n_planes;          /* <= RB_MAX_PLANES static half-spaces                   */
    int32_t dtype;             /* RB_F64 | RB_F32 (arithmetic type of the path)        */
    int32_t normal_convention; /* RB_NORMAL_ORIENTED | RB_NORMAL_RAW                   */
    int32_t device;            /* HIP device ordinal                                   */
    int32_t rank;              /* shard index: owns bodies [rank*S, rank*S+S) ∩ [0,N)  */
    int32_t world_size;        /* shard count P; S = ceil(N / P)                       */
    int32_t max_partners;      /* sphere-sphere contacts per body (0 = default 16; a guarded rb_step chunk raises 16 to 32 on overflow) */
    int32_t bucket_capacity;   /* reserved (0): a broadphase bucket holds 30 ids       */
    const int32_t *kind;       /* [N]   RB_BODY_*                                      */
    const double  *mass;       /* [N]   model.body_mass of each free body              */
    const double  *inertia;    /* [N*3] model.body_inertia (principal, body frame)     */
    const double  *size;       /* [N*3] sphere: (r, 0, 0); box: half extents           */
    const double  *planes;     /* [n_planes*6] (normal xyz, point xyz), world frame    */
    double         gravity[3]; /* model.opt.gravity                                    */
} rb_scene_desc;

#define RB_MAX_PLANES 8

typedef struct rb_world rb_world;

/* ---- lifetime ---------------------------------------------------------- */
/* Replaces the MjModel/MjData pair the reference step functions receive
 * (collision.py:56, time_integeration.py:13, multi_sphere_bounce.py:42):
 * masses, inertias, geometry and gravity become explicit SoA device arrays. */
int  rb_world_create(rb_world **out, const rb_scene_desc *desc);
void rb_world_destroy(rb_world *w);
const char *rb_last_error(void);
const char *rb_version(void);

/* Bind the world to a caller-owned HIP stream (hipStream_t; NULL is HIP's
 * default null stream, e.g. torch's default stream).  Until this is called
 * the world uses a private non-blocking stream.  All later work of this
 * world is enqueued on the bound stream. */
int rb_set_stream(rb_world *w, void *hip_stream);

/* ---- state transfer (the only AoS<->SoA transposes) --------------------- */
/* Global arrays: qpos [N*7], qvel [N*6] (host).  set: every rank passes the
 * whole scene; the world keeps all positions and its own shard of the rest.
 * get: writes the rows of the bodies this world owns, leaves others alone.
 * Replaces the reads/writes of data.qpos/data.qvel at collision.py:60-65,
 * :97-100 and multi_sphere_bounce.py:50-51, :85-88. */
int rb_set_state(rb_world *w, const double *qpos, const double *qvel);
int rb_get_state(rb_world *w, double *qpos, double *qvel);
/* optional data.xfrc_applied [N*6] (force xyz, torque xyz); NULL = zero
 * (collision.py:66-67).  Host pointer, copied. */
int rb_set_xfrc(rb_world *w, const double *xfrc);

/* ---- the device-resident boundary (world_size 1) ------------------------ */
/* The same three transfers with the caller's arrays in device memory on the
 * world's device: qpos [N][7], qvel [N][6], xfrc [N][6], of doubles or floats
 * (io_dtype RB_F64 | RB_F32) whatever the world's real type; conversion is a
 * C cast.  An array may start at any element (16-byte aligned ones move 16
 * bytes per lane).  Every call is enqueued on the world's stream
 * (rb_set_stream) and does not wait, but for the cases named below: a caller
 * on that stream (a controller, a force field, a renderer in torch) exchanges
 * state and forces with the world without a copy across PCIe and without a
 * host synchronisation; rb_sync waits.  Replaces, for such a caller, the host
 * round trip of data.qpos / data.qvel / data.xfrc_applied
 * (multi_sphere_bounce.py:50-51, :85-88; collision.py:66-67).
 * All three return RB_EINVAL for a null world, a null array or an unknown
 * io_dtype and RB_EUNSUPPORTED for a world with world_size > 1 (a shard's
 * boundary is rb_gpos_buffer), before any device call.
 *   rb_get_state_dev: writes qpos and qvel; either may be NULL, not both.
 *     Like every reader of the state it first runs the check of a run that
 *     awaits one: after steps in the tile form it waits for that run.  Under
 *     RB_LAW_BALLS the positions are the state's own (as rb_get_state).
 *   rb_set_state_dev: rb_set_state from device memory, with its bookkeeping
 *     (the next step rebuilds the broadphase table; a later rb_set_state is
 *     never skipped as unchanged).  refit != 0: the broadphase layout is then
 *     fitted to the new positions, as rb_set_state fits it to the host copy,
 *     through one read-back of the positions: it waits, and is meant for a
 *     new scene.  refit == 0: the layout stays and the call is enqueued only,
 *     for resets inside the extent the world was fitted for.  The layout
 *     decides speed, never bits, and a synchronous rb_step still refits when
 *     a bucket overflows.
 *   rb_set_xfrc_dev: rb_set_xfrc from device memory.  The first call after
 *     "no forces" allocates the force rows and drops the captured graphs as
 *     rb_set_xfrc does (it waits); later calls are enqueued only, ordered
 *     after the steps in flight.  rb_set_xfrc(w, NULL) clears the forces. */
int rb_get_state_dev(rb_world *w, void *qpos, void *qvel, int32_t io_dtype);
int rb_set_state_dev(rb_world *w, const void *qpos, const void *qvel,
                     int32_t io_dtype, int32_t refit);
int rb_set_xfrc_dev(rb_world *w, const void *xfrc, int32_t io_dtype);

/* ---- the contact query of a world (additive to librbhip 0.4) ----------------
 * For the world's current state, the contact list of the bodies [first,
 * first + count) exactly as rb_batch_contacts (below) defines it for one
 * environment: what the reference reads as data.contact[i].dist / pos / frame
 * / geom1 / geom2 after mj_forward (collision.py:57, :72-76), without a step.
 * Every generated contact is listed (the step's skip rules, dist < 0 and the
 * threshold, are not applied), in the canonical per-body order of
 * rb_get_contacts: the planes in plane order, a box's corners in bit order
 * with at most 4 per plane, then the partners by ascending body id, a box
 * pair's points in generation order.  frame is the raw normal from geom1 to
 * geom2 (no normal convention applied); geom1 is the plane of a plane contact,
 * the lower id of two spheres or two boxes, the sphere of a sphere-box pair.
 *
 * Layout: dense, R = max_records slots per body.  counts [count]; partner,
 * kind and dist [count][R]; pos and frame [count][R][3].  counts[k] is the
 * true number of contacts of body first + k, also past R (the first R records
 * are kept); partner is a global body id or -1 - plane.  Slots at or past the
 * count hold kind -1 and zeros elsewhere, so every word of the output is
 * defined.  pos and frame may be NULL, singly or together; partner, kind and
 * dist only all together, with max_records 0: a counts-only query, for sizing.
 *
 * A body whose list cannot be built has counts[k] == -2 and unused slots
 * only: one with more than 32 partners in reach (the query searches with a
 * partner list of 32 whatever the world's max_partners), one with a
 * non-finite or out-of-range position, and every body of the call if the
 * query's own broadphase table overflowed.  The host form then returns
 * RB_EOVERFLOW (RB_EDOM for the position case) with a message naming the
 * lowest such body, all arrays written; the device form reports through
 * counts alone.  Neither sets any sticky state, neither touches the world's
 * error word.
 *
 * The query is pure: it steps nothing and changes nothing a step can see
 * (state, broadphase tables and generations, captured graphs, the layout fit,
 * rb_world_stats, the rb_set_state mirror, recorded contacts).  A run of steps
 * gives the same bits and stats with any number of queries between its calls.
 * It searches a broadphase table of its own, allocated at the first query and
 * filled from the current positions by every call.
 *
 * RB_EINVAL, nothing enqueued or changed: a null world or counts;
 * max_records < 0; max_records 0 with a record array given, or > 0 without;
 * first < 0, count < 0 or first + count > n_bodies; in the device form an
 * unknown io_dtype, a host pointer or memory of another device.  count 0 is
 * RB_OK.  RB_EUNSUPPORTED before any device call: world_size > 1; RB_LAW_BALLS
 * (that law has no contact list); the device form under a stream capture.
 *
 * rb_query_contacts: host arrays, synchronous; like rb_get_state it finishes
 * the world's pending work first.  *n_truncated (may be NULL) = the listed
 * bodies with count > max_records.  The lists are staged in a device buffer
 * owned by the world, allocated on first use and freed with it, of at most
 * RBHIP_CONTACT_STAGE_BYTES bytes (read at rb_world_create; default 256 MiB);
 * a request that does not fit is cut into launches over sub-ranges (RB_EINVAL
 * if one body's slots alone do not fit).
 * rb_query_contacts_dev: the arrays are device memory on the world's device;
 * dist, pos and frame of io_dtype (RB_F64 | RB_F32), converted by a C cast.
 * Enqueued on the world's stream without waiting, but that like every reader
 * of the state it first runs the check of a tile-form run that awaits one. */
int rb_query_contacts(rb_world *w, int64_t first, int64_t count, int32_t max_records,
                      int32_t *counts, int32_t *partner, int32_t *kind,
                      double *dist, double *pos, double *frame, int64_t *n_truncated);
int rb_query_contacts_dev(rb_world *w, int64_t first, int64_t count, int32_t max_records,
                          int32_t *counts, int32_t *partner, int32_t *kind,
                          void *dist, void *pos, void *frame, int32_t io_dtype);

/* ---- the impulses of the next step -------------------------------------- */
/* rb_batch_impulses (below) for one environment that is the world: for the
 * world's current state and the step parameters of the call, what the next
 * rb_step(w, 1, dt, ...) does to each body of [first, first + count).  jn, jt,
 * vel and net mean what they mean there (the skip rules, a separating contact,
 * the step's normal, the sums of net from +0; vel: the words the next
 * rb_step(1, ...) writes into the body's qvel, whichever step form runs it).
 * Applied forces (rb_set_xfrc, rb_set_xfrc_dev) are honoured by the path the
 * step takes: once forces are set, the applied-force path for all-zero rows too.
 *
 * Layout: rb_query_contacts', dense, R = max_records slots per body.  counts
 * [count]; partner, kind, dist and jn [count][R]; jt [count][R][3]; vel and
 * net [count][6].  counts, partner, kind and dist are word for word what
 * rb_query_contacts writes for the same state, range and R (the true count
 * past R; kind -1 and zeros in the unused slots, in jn and jt as well).
 * Truncation drops records only: vel and net do not depend on R.  partner,
 * kind, dist, jn and jt are given all together with R > 0, or are all NULL
 * with R 0 (the "sensor only" call); counts is required; vel and net may each
 * be NULL.
 *
 * A body without a list (rb_query_contacts' three conditions) has counts -2,
 * unused slots, and zero rows in vel and net.  The host form returns what
 * rb_query_contacts returns there, all arrays written; the device form reports
 * through counts alone; nothing sticky is set and the world's error word is
 * untouched.  The query is pure exactly as rb_query_contacts is, and shares
 * its table and its staging buffer.
 *
 * RB_EINVAL, nothing enqueued: every case of rb_query_contacts (the five record
 * arrays all together or none); what rb_step refuses (dt not positive, a
 * negative restitution, friction or contact_threshold, NaN); a non-finite dt,
 * restitution, friction or contact_threshold.  RB_EUNSUPPORTED: world_size > 1;
 * RB_LAW_BALLS; the device form under a stream capture.  count 0 is RB_OK.
 *
 * rb_query_impulses: host arrays, synchronous, staged and cut into sub-ranges
 * of bodies as rb_query_contacts is (RBHIP_CONTACT_STAGE_BYTES); *n_truncated
 * (may be NULL) = the listed bodies with count > max_records.
 * rb_query_impulses_dev: device arrays, enqueued on the world's stream as
 * rb_query_contacts_dev is; pointers are checked on the host; reals are of
 * io_dtype, converted by a C cast.
 *
 * Not covered: sharded worlds; the two-ball law; impulses recorded inside a
 * sampled run of a world (a batch records the per-body net impulse:
 * rb_batch_run_sampled_impulses; per-contact records jn, jt inside a sampled
 * run are open for both). */
int rb_query_impulses(rb_world *w, int64_t first, int64_t count, int32_t max_records,
                      double dt, double restitution, double friction, double contact_threshold,
                      int32_t *counts, int32_t *partner, int32_t *kind, double *dist,
                      double *jn, double *jt, double *vel, double *net, int64_t *n_truncated);
int rb_query_impulses_dev(rb_world *w, int64_t first, int64_t count, int32_t max_records,
                          double dt, double restitution, double friction, double contact_threshold,
                          int32_t *counts, int32_t *partner, int32_t *kind, void *dist,
                          void *jn, void *jt, void *vel, void *net, int32_t io_dtype);

/* ---- the hot path ------------------------------------------------------ */
/* nsteps reference steps: contact generation (mj_forward's role,
 * collision.py:57), gravity (collision.py:66-70), the per-contact
 * Gauss-Seidel impulse solve with Coulomb friction (collision.py:72-88 ->
 * compute_collision_impulse_friction collision.py:7-48 ->
 * apply_impulse_friction physics_utils.py:25-49) and the semi-implicit
 * position/quaternion integration (collision.py:90-100).  Jacobi across
 * bodies (one contact pass per step, multi_sphere_bounce.py:43-46).
 * contact_threshold: contacts with |dist| < threshold are skipped
 * (collision.py:79-80; 0 there, 1e-4 in time_integeration.py:13).
 * Synchronous: returns after the device finished, with any device-side
 * error (overflow, unsupported pair, non-finite position) reported. */
int rb_step(rb_world *w, int64_t nsteps, double dt, double restitution,
            double friction, double contact_threshold);
/* Same, enqueued only (no host sync, no error check).  rb_sync waits and
 * returns the accumulated device-side error. */
int rb_step_async(rb_world *w, int64_t nsteps, double dt, double restitution,
                  double friction, double contact_threshold);
int rb_sync(rb_world *w);

/* ---- sharded stepping (world_size > 1) ---------------------------------- */
/* One step of the owned bodies; their new positions land in this rank's
 * slice of the replicated position buffer of the next step.  The caller then
 * all-gathers that buffer (RCCL over xGMI via torch.distributed, or any
 * transport) and calls rb_shard_exchange_done, which publishes the other
 * ranks' positions to the next step's broadphase.  Both calls are enqueued
 * only. */
int rb_shard_step(rb_world *w, double dt, double restitution, double friction,
                  double contact_threshold);
int rb_shard_exchange_done(rb_world *w);
/* Device view of the position buffer the pending exchange fills (valid
 * between rb_shard_step and rb_shard_exchange_done; two buffers alternate
 * step by step).  Layout [P][S][4] of the world's dtype — (x, y, z,
 * bounding radius) per body, bodies in global id order; this rank's slice
 * is the contiguous [rank][S][4] (shard_elems = 4*S elements). */
int rb_gpos_buffer(rb_world *w, void **dev_ptr, int64_t *shard_elems,
                   int32_t *elem_bytes);
/* Worlds with box bodies: the orientation buffer the same exchange fills
 * alongside (layout [P][S][4], (w, x, y, z) per body in global id order, rows
 * of box bodies meaningful) — all-gather it like the position buffer.  A
 * sphere-only world returns *dev_ptr = NULL and *shard_elems = 0 (nothing
 * to exchange: a sphere's contacts never read its orientation).  No reference
 * counterpart (the reference is single-process; its box body is
 * models/cube.xml:35). */
int rb_gquat_buffer(rb_world *w, void **dev_ptr, int64_t *shard_elems,
                    int32_t *elem_bytes);

/* In-library exchange: the library owns an RCCL communicator over the
 * world's ranks (RCCL is loaded at first use; the single-GPU path never
 * needs it) and runs the per-step exchange itself, so K sharded steps --
 * step kernel, in-place all-gather of the position buffer over xGMI, remote
 * insert -- replay from one captured HIP graph with no host work per step.
 * Replaces the per-frame loop of custom_step_multi_sphere
 * (multi_sphere_bounce.py:42-92) on a body-range sharded scene.
 *   rb_comm_unique_id: rank 0 creates the communicator id (bytes >= 128)
 *     and hands it to every rank (e.g. torch.distributed broadcast);
 *   rb_shard_comm_init: every rank joins (blocks until all have); the
 *     world's device, rank and world_size define the communicator;
 *   rb_shard_run: nsteps sharded steps, enqueued only; every rank must make
 *     the same calls with the same nsteps.  Bit-identical to rb_shard_step +
 *     all-gather + rb_shard_exchange_done, and to rb_step for world_size 1. */
int rb_comm_unique_id(void *id, int32_t bytes);
int rb_shard_comm_init(rb_world *w, const void *id, int32_t bytes);
int rb_shard_run(rb_world *w, int64_t nsteps, double dt, double restitution,
                 double friction, double contact_threshold);

/* Peer-to-peer exchange (SURVEY §7 hard part 4), in place of the RCCL
 * all-gather: after its step kernel each rank flags "step done" into every
 * peer's flag word, and its exchange kernel reads the other ranks' fresh
 * slices straight from their buffers over xGMI (IPC mappings) once they
 * have flagged, then inserts them.  Waits are bounded: a peer missing for
 * 5 s raises RB_ENODEV at the next rb_sync instead of hanging.
 *   rb_p2p_handles: this rank's IPC handles (*len bytes; out = NULL to ask
 *     the size); every rank passes the concatenation of all ranks' handles,
 *     in rank order, to
 *   rb_p2p_connect (collective: no rank may step before all have connected).
 * rb_shard_run then uses this transport; bit-identical to the others. */
int rb_p2p_handles(rb_world *w, void *out, int64_t cap, int64_t *len);
int rb_p2p_connect(rb_world *w, const void *all, int64_t len);

/* Halo mode of the peer-to-peer exchange, for large shards (no reference
 * counterpart: the reference is single-process).  Instead of reading every
 * peer's whole slice, the step kernel of each rank pushes to each peer only
 * its bodies whose new cell lies within two cells of that peer's own
 * bodies' cell bounds of the step before (a superset of everything the
 * peer's next contact searches can reach while no body moves more than one
 * broadphase cell per step; one that does fails the run with RB_EDOM), into
 * the peer's inbox; one insert kernel per step then publishes the bounds
 * and counts and inserts what the peers pushed.  No host work; still
 * bit-identical to every other transport.  Collective: every rank must make
 * the same call, after rb_p2p_connect and before stepping.  enable = 0
 * returns to full reads. */
int rb_p2p_halo(rb_world *w, int32_t enable);

/* ---- the two-ball law -------------------------------------------------- */
/* Switch a world to RB_LAW_BALLS (or back to RB_LAW_MUJOCO), replacing
 * step_with_custom_collisions (ball_collision.py:73-125): gravity v += g dt;
 * ground contact against z = 0 when z < r (impulse, then z = r); ball-ball
 * contact when |p_b - p_a| < r_a + r_b + tol with the full-effective-mass
 * impulse compute_collision_impulse (ball_collision.py:53-68) and half-overlap
 * position correction; x += v dt; quaternions untouched.  Two balls step
 * exactly as the reference; N balls evaluate every pair from the post-ground
 * state of both and accumulate per ball in ascending partner id.  Requires
 * spheres only, world_size 1, and either no plane or exactly the ground
 * plane (normal (0,0,1) through the origin); tol >= 0 (the reference: 0.01).
 * rb_step's contact_threshold is ignored under this law. */
int rb_set_contact_law(rb_world *w, int32_t law, double tol);

/* ---- parity support ---------------------------------------------------- */
/* Record the contact list generated during the most recent step (off by
 * default: recording costs HBM traffic).  Canonical per-body order: plane
 * contacts (plane order; box corners in bit order), then partners by
 * ascending body id (a box-involved partner: its contacts in generation
 * order, RB_CK_SPHERE_BOX / RB_CK_BOX_BOX0 + k / RB_CK_BOX_EDGE), in
 * sharded worlds as well (their exchange carries the boxes' orientations:
 * rb_gquat_buffer).  Output is CSR over the owned bodies: counts[n_owned];
 * partner (body id, or -1-plane_index), kind (RB_CK_*), dist.  cap is the
 * capacity of the flat arrays; total receives the number of records. */
int rb_record_contacts(rb_world *w, int enable);
int rb_get_contacts(rb_world *w, int32_t *counts, int32_t *partner,
                    int32_t *kind, double *dist, int64_t cap, int64_t *total);

/* Known-answer entries, run as device kernels on `device`.
 * rb_kat_impulse: per case in[24] = m, e, mu, v[3], w[3], r[3], n[3],
 * inertia_world[9] (row-major) -> out[10] = jn, jt[3], v'[3], w'[3]:
 * compute_collision_impulse_friction (collision.py:7-48) followed by
 * apply_impulse_friction (physics_utils.py:25-49).  dtype RB_F64|RB_F32.
 * rb_kat_inertia: per case in[7] = inertia_diag[3], q[4] (wxyz) ->
 * out[18] = inertia_world[9], inv(inertia_world)[9]
 * (compute_inertia_tensor_world collision.py:51-53 + np.linalg.inv). */
int rb_kat_impulse(int32_t device, int32_t dtype, int64_t n, const double *in,
                   double *out);
int rb_kat_inertia(int32_t device, int32_t dtype, int64_t n, const double *in,
                   double *out);
/* rb_kat_pair_impulse: per case in[27] = m, e, mu, v[3], w[3], r[3], n[3],
 * I_inv[9] (row-major) -> out[3] = impulse: compute_collision_impulse
 * (ball_collision.py:53-68). */
int rb_kat_pair_impulse(int32_t device, int32_t dtype, int64_t n, const double *in,
                        double *out);
/* rb_kat_narrow: the box-involved narrowphase (this
 * project's restatement of MuJoCo's sphere-box / box-box primitives, which
 * are not available offline — parity against MuJoCo is unpinned):
 * per case in[22] = kind1, kind2 (RB_BODY_*), c1[3], q1[4] (wxyz), size1[3],
 * c2[3], q2[4], size2[3] (body 1 = the lower id) -> out[33] = count, then
 * per contact dist, pos[3], frame[3] (geom1 -> geom2; a sphere is geom1 of
 * a sphere-box pair), kind (RB_CK_*). */
int rb_kat_narrow(int32_t device, int32_t dtype, int64_t n, const double *in, double *out);
/* rb_kat_apply: apply_impulse_friction alone (physics_utils.py:25-49) with
 * caller-given impulses: in[26] = m, v[3], w[3], r[3], n[3], jn, jt[3],
 * inertia_world[9] -> out[6] = v'[3], w'[3]. */
int rb_kat_apply(int32_t device, int32_t dtype, int64_t n, const double *in,
                 double *out);

/* Introspection for measurement: per-body algorithmic HBM bytes of one
 * step (state read+write + constants), number of owned bodies, and the
 * average device duration (ms) of the step kernel over the launches timed
 * since the last reset (HIP events on the world's stream; enable first). */
int rb_query(rb_world *w, int64_t *n_owned, int64_t *bytes_per_body_step);

/* Counters for tests and measurement; fills out[0 .. min(n, RB_STATS_COUNT))
 * and returns how many.
 * ABI note: librbhip 0.3 (rb_version) renumbered the counters of 0.2 — the
 * round-4 block counters were removed and RB_STAT_FORM, _BUCKETS,
 * _MAX_PARTNERS and _IO_* moved (8 -> 1, 19 -> 6, 20 -> 7, 27/28 -> 8/9;
 * RB_STATS_COUNT 30 -> 18, then 19 with RB_STAT_HASHED_FORM appended).  A
 * consumer built against the 0.2 header must be rebuilt; from 0.3 on new
 * counters are only appended. */
#define RB_STAT_GRAPHS          0   /* captured step graphs alive               */
#define RB_STAT_FORM            1   /* step kernel form of the next run: 0 one-lane, 1 cooperative, 2 wide,
                                       3 cooperative + helper, 4 wide + helper (hashed cells),
                                       5 cell-ordered tiles (rb_tiles.hip) */
#define RB_STAT_BOX_OPT         2   /* box worlds: chunks replayed without the box kernel */
#define RB_STAT_BOX_ROLLBACK    3   /* of which rolled back and replayed with it (a body was deferred) */
#define RB_STAT_REFITS          4   /* broadphase layout refits of a drifting scene (chunk rolled back, replayed) */
#define RB_STAT_TABLE_GROWS     5   /* of which with the bucket table doubled */
#define RB_STAT_BUCKETS         6   /* buckets per table now */
#define RB_STAT_MAX_PARTNERS    7   /* max_partners now (16 -> 32 after an overflow in a guarded chunk) */
#define RB_STAT_IO_SKIPPED      8   /* rb_set_state calls that were no-ops (the bytes rb_get_state handed out) */
#define RB_STAT_IO_UPLOADS      9   /* rb_set_state calls that uploaded          */
#define RB_STAT_TILE_RUNS      10   /* runs stepped in the cell-ordered tile form */
#define RB_STAT_TILE_STEPS     11   /* steps of those runs committed (checked)  */
#define RB_STAT_TILE_ROLLBACKS 12   /* tile runs rolled back and replayed by the hashed-cell forms */
#define RB_STAT_TILE_BUILDS    13   /* tile bins built from the id-ordered state */
#define RB_STAT_TILE_WHY       14   /* why bits of the rolled-back tile runs (OR; 1 bin capacity, 2 window
                                       capacity, 4 far list, 8 partners, 16 position) */
#define RB_STAT_TILE_SLOTS     15   /* tile slots of the periodic tile grid (workgroups per step) */
#define RB_STAT_TILE_COLS      16   /* columns per tile edge                    */
#define RB_STAT_TILE_ON        17   /* the next run of >= 2 steps would use the tile form */
#define RB_STAT_HASHED_FORM    18   /* the hashed-cell form (0-4, as RB_STAT_FORM) the world steps with when
                                       the tile form does not */
/* Append epochs (appended counters; sphere-only worlds on one rank stepped by a
 * wide form): a broadphase table is read by up to RBHIP_TABLE_EPOCH
 * consecutive steps; all but the last only append the bodies that changed
 * cell, the last rebuilds the next table from every body.  Worlds without
 * epochs report 0 for both step counters (and do not wait for the device).
 * The counters count launches: the steps of a guarded chunk that was rolled
 * back and replayed are counted twice. */
#define RB_STAT_APPEND_STEPS   19   /* steps that appended to the table they read */
#define RB_STAT_REBUILD_STEPS  20   /* steps of a world with epochs that rebuilt the next table */
#define RB_STAT_TABLE_EPOCH    21   /* RBHIP_TABLE_EPOCH: the longest epoch (1: every step rebuilds) */
#define RB_STAT_GRID_LAYOUT    22   /* the cell -> bucket layout word: group shape bits of x, y, z in nibbles
                                       0-2; bit 24: linear layout, periodic in 2^lx x 2^ly x 2^lz groups
                                       (nibbles 3-5); bits 25-26: log2 bucket heads per line */
#define RB_STAT_HELP_SEARCH    23   /* 1: the world's hashed form is wide + helper and shares the contact
                                       search between its two waves (RBHIP_HELP_SEARCH; 0 in worlds with a
                                       box body and in every other form) */
#define RB_STATS_COUNT         24
int rb_world_stats(rb_world *w, int64_t *out, int32_t n);
int rb_kernel_timing(rb_world *w, int enable, double *avg_ms, int64_t *launches);

/* ---- batched worlds (librbhip 0.4) ---------------------------------------- */
/* Many small independent scenes ("environments") stepped by one launch: a
 * parameter sweep, an ensemble of initial conditions, a domain-randomised
 * batch of the reference's scenes (1 to 4 bodies each).  A batch is n_envs
 * replicas of a template environment of M = n_bodies <= 64 bodies
 * (rb_batch_create, rb_batch_create_mixed) or <= RB_BATCH_MAX_BODIES = 256
 * bodies (rb_batch_create_wide); the
 * plane count, dt, the contact threshold and the normal convention are per
 * batch; restitution / friction / body constants / state and, additive to
 * 0.4 (rb_version is unchanged), the planes' values, gravity and applied
 * forces (rb_batch_set_planes / _gravity / _xfrc) are per environment.
 * An environment steps bit-identically to an rb_world of the same scene,
 * under either contact law (rb_batch_set_contact_law).
 * Arrays are environment-major: body k of environment e at row e*M + k.
 * Not covered (use rb_world): contacts recorded inside a step (a batch is
 * asked for the contact list of its current state: rb_batch_contacts, and for
 * the impulses of its next step: rb_batch_impulses; a sampled run records
 * each body's net contact impulse per window: rb_batch_run_sampled_impulses;
 * per-contact records jn, jt inside a sampled run are open), sharding,
 * per-environment plane counts, more than 256 bodies per
 * environment; under RB_LAW_BALLS also per-environment planes, applied
 * forces, the contact query, environments of more than 64 bodies and
 * per-environment body counts and kinds (rb_batch_set_population).
 * A batch handle is not thread-safe; every call that takes host arrays is
 * synchronous (the device-resident boundary below only enqueues).
 *
 * A step launch runs at most RB_BATCH_CHUNK steps (a bound on kernel duration
 * on a shared device); longer runs are several launches, with the same
 * result however a run is cut into launches or calls. */
#define RB_BATCH_CHUNK 256
/* Most bodies of an environment (rb_batch_create_wide). */
#define RB_BATCH_MAX_BODIES 256
typedef struct rb_batch rb_batch;
/* Replaces one MjModel/MjData pair per scene variant (as rb_world_create:
 * collision.py:56, multi_sphere_bounce.py:42).  scene: the template
 * environment (n_bodies = M in 1..64, world_size 1, rank 0; max_partners and
 * bucket_capacity unused: every body may touch all others), replicated
 * n_envs times.  RB_EUNSUPPORTED for a template with a box body and more
 * than one body (rb_batch_create_mixed takes it). */
int  rb_batch_create(rb_batch **out, const rb_scene_desc *scene, int64_t n_envs);
/* rb_batch_create that also accepts any mix of spheres and boxes in a
 * template of 2..64 bodies (a column or pile of cubes: the reference's
 * stated goal is stacking): box-involved pairs are evaluated inside the
 * batch, every environment bit-identically to an rb_world of its scene with
 * max_partners 32.  Additive to 0.4 (rb_version is unchanged).  A sphere-only
 * or one-box template gives exactly the batch rb_batch_create gives.  Every
 * other rb_batch_* call works on such a batch as on any other (sizes set by
 * rb_batch_set_bodies are per environment, the kinds stay the template's
 * unless rb_batch_set_population gives every environment its own);
 * rb_batch_set_contact_law(RB_LAW_BALLS) is RB_EUNSUPPORTED: that law takes
 * spheres only. */
int  rb_batch_create_mixed(rb_batch **out, const rb_scene_desc *scene, int64_t n_envs);
/* rb_batch_create_mixed for a template of 1..RB_BATCH_MAX_BODIES bodies
 * (box_pile(4, 4, 4): 70 bodies; a 16 x 16 sphere field: 256).  Additive to
 * 0.4 (rb_version is unchanged).  Up to 64 bodies it gives exactly the batch
 * rb_batch_create_mixed gives: same kernels, same bits.  From 65 bodies on the
 * batch is wide: an environment is one workgroup of 2 to 4 waves instead of
 * (a part of) one wave, every body still testing every other body of its
 * environment in ascending id, so an environment steps bit-identically to an
 * rb_world of its scene wherever the world's partner lists (max_partners <=
 * 32) hold the scene; the batch itself has no partner bound.  Every other
 * rb_batch_* call works on a wide batch as on any other, failure semantics
 * included: a failing body freezes its whole environment, bodies in other
 * waves too, and no other environment.  Validation and codes are
 * rb_batch_create's (RB_EINVAL for 0 or 257 bodies).  Not covered on a wide
 * batch: rb_batch_set_contact_law(RB_LAW_BALLS) returns RB_EUNSUPPORTED and
 * changes nothing (the two-ball law across waves is not implemented). */
int  rb_batch_create_wide(rb_batch **out, const rb_scene_desc *scene, int64_t n_envs);
void rb_batch_destroy(rb_batch *b);
/* Per-environment restitution / friction, [n_envs] each; NULL = use the
 * scalar given to rb_batch_step.  Replaces the per-scene constants of
 * src/config/sim_overrides.py:1-28 (one run of the reference per value). */
int  rb_batch_set_params(rb_batch *b, const double *restitution, const double *friction);
/* Per-environment body constants: mass [E*M], inertia [E*M*3], size [E*M*3]
 * (as rb_scene_desc; kinds stay the template's, or the population's:
 * rb_batch_set_population); NULL = keep.  Replaces
 * model.body_mass / body_inertia / geom_size of a per-variant model
 * (collision.py:58-62). */
int  rb_batch_set_bodies(rb_batch *b, const double *mass, const double *inertia, const double *size);
/* The population of a batch: per environment a body count and a kind for each
 * of its M body slots, so that one batch holds scenes of different shapes (an
 * ensemble of piles of 1 to 8 bodies; single_sphere, single_cube and
 * multi_sphere4 side by side).  Additive to 0.4 (rb_version is unchanged).
 * n_bodies [n_envs] (1..M; NULL: every environment holds M bodies);
 * kind [n_envs*M] RB_BODY_* (NULL: the template's kinds in every environment).
 * Both NULL: no population; the batch steps with the kernels it stepped with before.
 *
 * Bodies 0 .. n_e-1 of environment e are present, slots n_e .. M-1 absent.
 * Every environment steps bit-identically to an rb_world of its own scene:
 * the present bodies alone, with their own kinds, under max_partners 32.
 * Present bodies are a prefix, so body and partner ids are those of the
 * smaller world.  A uniform population (all counts M, the template's kinds)
 * gives the same words as no population.
 *
 * Absent slots are ordinary storage: the set calls write their rows of state,
 * constants and forces (validated as ever over all n_envs*M rows) and the get
 * calls return them bit for bit.  No step reads or writes them: they are
 * nobody's partner, take no plane contact and cannot fail an environment (a
 * NaN position there is harmless).  In sampled runs their rows hold zeros in
 * every sample; in the contact query an absent body has count 0 and unused
 * slots only (a failed environment still reports -1 for all M bodies).
 * Bounding radii (here and in rb_batch_set_bodies) follow the population's
 * kinds; the batch's largest radius skips absent bodies.
 *
 * Synchronous: pending work finishes first, under the population it was
 * enqueued with.  The call touches no state, status or step count and may come
 * between any two calls; no state is converted.  Any batch accepts it,
 * whatever its creator and M; a batch of rb_batch_create may receive boxes
 * this way.  RB_EINVAL for a count outside 1..M or a kind other than
 * RB_BODY_SPHERE / RB_BODY_BOX in any of the n_envs*M slots (the message names
 * the environment and the body); RB_EUNSUPPORTED under RB_LAW_BALLS, and
 * rb_batch_set_contact_law(RB_LAW_BALLS) is RB_EUNSUPPORTED while a
 * population is set.  A refused call changes nothing.
 * Not covered: a device-side form of this call (a reset that changes an
 * environment's body count without the host), the two-ball law,
 * per-environment plane counts, more than 256 bodies. */
int  rb_batch_set_population(rb_batch *b, const int32_t *n_bodies, const int32_t *kind);
/* qpos [n*M*7], qvel [n*M*6] for the environments listed in env_ids[n]
 * (distinct; NULL = all n_envs, in order, n = n_envs).  set clears the listed
 * environments' failed status and step count (a per-environment reset).
 * Replaces the reads/writes of data.qpos / data.qvel at collision.py:60-65,
 * :97-100 and multi_sphere_bounce.py:50-51, :85-88, per environment. */
int  rb_batch_set_state(rb_batch *b, const int64_t *env_ids, int64_t n, const double *qpos, const double *qvel);
int  rb_batch_get_state(rb_batch *b, const int64_t *env_ids, int64_t n, double *qpos, double *qvel);
/* nsteps reference steps of every environment: the per-frame loop of
 * custom_step_multi_sphere (multi_sphere_bounce.py:42-92), i.e.
 * custom_step_with_contacts (collision.py:56-102) per body, per environment.
 * Synchronous.  An environment with a non-finite or out-of-range body
 * position (the check of rb_step) fails alone: it is not advanced by that
 * step or any later one — its state stays the start state of the failing
 * step — until rb_batch_set_state resets it.  Healthy environments are
 * always stepped to the end.  *n_failed = environments failed so far; with
 * n_failed == NULL a failed environment makes the call return RB_EDOM (after
 * stepping the rest). */
int  rb_batch_step(rb_batch *b, int64_t nsteps, double dt, double restitution, double friction,
                   double contact_threshold, int64_t *n_failed);
/* code [n_envs] (RB_OK | RB_EDOM), steps_done [n_envs] (steps completed since
 * the environment's last rb_batch_set_state); either may be NULL.  No
 * reference counterpart (the reference raises from inside its one scene). */
int  rb_batch_status(rb_batch *b, int32_t *code, int64_t *steps_done);
/* Switch a batch to RB_LAW_BALLS (or back to RB_LAW_MUJOCO): every
 * environment then steps as step_with_custom_collisions
 * (ball_collision.py:73-125) with compute_collision_impulse
 * (ball_collision.py:53-68), exactly as rb_set_contact_law describes it for a
 * world; an environment of N > 2 balls evaluates every pair (a < b) from the
 * post-ground state of both and accumulates per ball in ascending partner id
 * (no partner cap: every ball may touch all others).  Same conditions and
 * codes as rb_set_contact_law: spheres only and either no plane or exactly
 * the z = 0 ground plane, else RB_EUNSUPPORTED; tol finite and >= 0 (the
 * reference: 0.01, ball_collision.py:102) and a known law, else RB_EINVAL; a
 * refused call changes nothing.  Under RB_LAW_BALLS the contact_threshold of
 * rb_batch_step is ignored, and so are the inertia rows of
 * rb_batch_set_bodies: the law derives I^-1 from mass and radius
 * (compute_inverse_inertia, ball_collision.py:39-41).  Per-environment
 * restitution / friction (rb_batch_set_params) apply to the ground and the
 * pair impulses.  The law may be switched between calls: the quaternion is
 * never touched under RB_LAW_BALLS and no state is converted. */
int  rb_batch_set_contact_law(rb_batch *b, int32_t law, double tol);
/* rb_batch_step that also records the curves the reference logs while it
 * steps (logger_base.py, data_logger.py, multi_sphere_logger.py: height
 * against time and the 3-D trajectory of every run): after every every-th step
 * of this call the state of every body of every environment, S = nsteps /
 * every samples (rounded down; the steps after the last sample are still
 * run).  Sample s is the state after step (s + 1) * every of this call, at
 * qpos [S][n_envs][M][7] and qvel [S][n_envs][M][6] (host arrays of the
 * caller; qvel NULL: positions and quaternions only) — word for word what a
 * loop of rb_batch_step(every) + rb_batch_get_state(all) returns, a failed
 * environment's rows repeating its frozen state; final state, status and
 * steps_done are those of rb_batch_step(nsteps).  The samples are taken
 * inside the step kernel's register loop (launches still run at most
 * RB_BATCH_CHUNK steps, the sampling period running on across them) into a
 * device buffer owned by the batch, allocated on first use, of at most
 * RBHIP_BATCH_SAMPLE_BYTES bytes (environment variable read by
 * rb_batch_create; default 256 MiB); one sample takes n_envs * M * rows *
 * (sizeof(real) + 8) bytes, rows = 13, or 7 without qvel.  A run whose
 * samples do not fit is cut into shorter launches with the buffer downloaded
 * in between.  RB_EINVAL (nothing stepped): every < 1, nsteps < 0, qpos NULL
 * with S > 0, or a buffer bound below one sample. */
int  rb_batch_run_sampled(rb_batch *b, int64_t nsteps, int64_t every, double dt, double restitution,
                          double friction, double contact_threshold, double *qpos, double *qvel,
                          int64_t *n_failed);
/* Per-environment planes, gravity and applied forces (additive to librbhip
 * 0.4).  Each call is synchronous; the values persist across steps and
 * across rb_batch_set_state (a reset does not touch them) and are converted
 * to the batch's real type as the template's are.  A non-finite value is
 * RB_EINVAL (the message names the environment, and the plane or body); a
 * refused call changes nothing.  While any of the three is set, steps and
 * sampled runs launch the per-environment instances of the step kernels;
 * failure semantics (rb_batch_step) are the same.
 *
 * planes [n_envs][n_planes][6] (normal xyz, point xyz), n_planes = the
 * template's; NULL = every environment uses the template's planes again.
 * RB_EINVAL for a non-NULL array when the template has no plane.  Replaces
 * the model's plane rewritten from INCLINE_ANGLE_RAD (cube_incline.py:28-34;
 * sim_overrides.py), one model per angle. */
int  rb_batch_set_planes(rb_batch *b, const double *planes);
/* gravity [n_envs][3]; NULL = the template's.  Replaces model.opt.gravity of
 * a per-variant model (collision.py:66; ball_collision.py:78).  Honoured
 * under both contact laws. */
int  rb_batch_set_gravity(rb_batch *b, const double *gravity);
/* xfrc [n_envs*M][6] (force xyz, torque xyz) as rb_set_xfrc; NULL = none.
 * Replaces data.xfrc_applied (collision.py:66-70).  While set, every body of
 * every environment takes the applied-force path of the step, all-zero rows
 * included (which matters for the sign of zeros), as a world with rb_set_xfrc
 * does.
 * Under RB_LAW_BALLS rb_batch_set_planes and rb_batch_set_xfrc with a non-NULL
 * array, and rb_batch_set_contact_law(RB_LAW_BALLS) while either is set,
 * return RB_EUNSUPPORTED and change nothing. */
int  rb_batch_set_xfrc(rb_batch *b, const double *xfrc);

/* ---- the device-resident boundary of a batch (additive to librbhip 0.4) ----
 * The state, the applied forces and the samples of a batch in device memory
 * of the caller, on a stream of the caller: a closed loop (read the state,
 * compute data.xfrc_applied from it, collision.py:66-70, step, reset the
 * environments that are done) without a download, an upload or a host
 * synchronisation per iteration.  io_dtype (RB_F64 | RB_F32) is the element
 * type of the caller's arrays, whatever the batch's real type; conversion is a
 * C cast.  Layouts are those of the host calls: [n_envs][M][7] qpos,
 * [n_envs][M][6] qvel and xfrc.  Every array must be device memory on the
 * batch's device (checked on the host): a host pointer, or memory of another
 * device, is RB_EINVAL with nothing enqueued.  Every call below except
 * rb_batch_sync enqueues on the batch's stream and returns without waiting;
 * argument errors are returned at once and a refused call changes nothing.
 * Stepping a batch under a stream capture of the caller (hipGraph,
 * torch.cuda.graph) is not supported and not attempted.
 *
 * rb_batch_set_stream: as rb_set_stream for a world.  Waits for the work on
 * the old stream; all later work of the batch, the synchronous entries above
 * included, is enqueued on hip_stream (a hipStream_t; NULL = the null stream).
 * The batch keeps its own stream and destroys only that one. */
int  rb_batch_set_stream(rb_batch *b, void *hip_stream);
/* The launches of rb_batch_step, without its report (arguments checked alike). */
int  rb_batch_step_async(rb_batch *b, int64_t nsteps, double dt, double restitution,
                         double friction, double contact_threshold);
/* Waits for the batch's stream, then reports as rb_batch_step: *n_failed =
 * environments failed so far, or RB_EDOM with n_failed == NULL.  Also reports
 * and clears a refused rb_batch_set_xfrc_dev (below): RB_EINVAL, the message
 * naming the environment and the body (*n_failed is still written). */
int  rb_batch_sync(rb_batch *b, int64_t *n_failed);
/* rb_batch_set_state from full-size device arrays.  mask [n_envs] bytes on the
 * device (NULL = all): where mask[e] != 0, environment e's state and snapshot
 * are written and its status and step count cleared (the per-environment
 * reset), in one kernel; the rows of other environments are not read. */
int  rb_batch_set_state_dev(rb_batch *b, const uint8_t *mask, const void *qpos,
                            const void *qvel, int32_t io_dtype);
/* All environments; either output may be NULL, not both. */
int  rb_batch_get_state_dev(rb_batch *b, void *qpos, void *qvel, int32_t io_dtype);
/* rb_batch_set_xfrc from a device array (RB_EUNSUPPORTED under RB_LAW_BALLS).
 * The host cannot see the values, so a non-finite one is refused on the
 * device: the upload writes nothing, the rows keep their earlier contents
 * (zeros before the first upload), and the next rb_batch_sync returns
 * RB_EINVAL.  Until that rb_batch_sync, later uploads write nothing either.
 * The wrinkle: the call itself returns RB_OK, and from it on the batch counts
 * as having applied forces set (steps launch the per-environment instances;
 * all-zero rows matter for the sign of zeros) whether or not the upload was
 * refused; rb_batch_set_xfrc(b, NULL) clears that, as ever.  The synchronous
 * entries neither report nor clear a refusal. */
int  rb_batch_set_xfrc_dev(rb_batch *b, const void *xfrc, int32_t io_dtype);
/* rb_batch_status into device arrays; either may be NULL, not both. */
int  rb_batch_status_dev(rb_batch *b, int32_t *code, int64_t *steps_done);
/* rb_batch_run_sampled with the samples written into device arrays of the
 * caller, qpos [S][n_envs][M][7] and qvel [S][n_envs][M][6] (NULL: positions
 * and quaternions only), by a transpose kernel per drain of the sample
 * buffer: no host synchronisation between launches, no copy.  The buffer
 * holds the slots alone, n_envs * M * rows * sizeof(real) bytes per sample
 * (rows = 13, or 7), under the same RBHIP_BATCH_SAMPLE_BYTES bound.  Final
 * state, status and steps_done are those of rb_batch_step(nsteps); no
 * report (rb_batch_sync).  RB_EINVAL as rb_batch_run_sampled. */
int  rb_batch_run_sampled_dev(rb_batch *b, int64_t nsteps, int64_t every, double dt,
                              double restitution, double friction, double contact_threshold,
                              void *qpos, void *qvel, int32_t io_dtype);

/* ---- the contact query of a batch (additive to librbhip 0.4) -------------------
 * For the batch's current state, each body's contact list exactly as
 * mj_forward generates it for that environment's scene: what the reference
 * reads as data.contact[i].dist / pos / frame / geom1 / geom2 (collision.py:57,
 * :72-76), per environment.  A pure function of the state and the batch's
 * constants (sizes, planes per environment where rb_batch_set_planes is set):
 * it steps nothing and changes nothing.  The list holds every generated
 * contact; the skip rules of the step (dist < 0, the contact threshold) are
 * not applied.
 *
 * Order (the canonical per-body order of rb_get_contacts): the planes in plane
 * order, a sphere's one contact per plane, a box's corners in bit order with
 * at most 4 per plane; then the other bodies of the environment by ascending
 * id, a box pair's points in generation order.
 *
 * Layout: dense, R = max_records slots per body.  counts [n][M]; partner, kind
 * and dist [n][M][R]; pos and frame [n][M][R][3].  counts[t][k] is the true
 * number of contacts of body k of listed environment t, also where it exceeds
 * R: the records past R are dropped, the first R kept.  A record: partner = the
 * other body's id within the environment, or -1 - plane; kind = RB_CK_*; dist,
 * pos and frame as MuJoCo's mjContact has them.  frame is the raw normal from
 * geom1 to geom2 (as rb_kat_narrow reports it; no normal convention applied).
 * geom1 is the plane of a plane contact; the lower id of two spheres or of two
 * boxes; the sphere of a sphere-box pair.  Slots at or past the count hold
 * kind -1 and zeros elsewhere, so every word of the output is defined.  An
 * environment whose status is failed (rb_batch_status) has count -1 for each
 * of its bodies, and unused slots only.
 *
 * pos and frame may be NULL, together or singly.  partner, kind and dist may
 * be NULL only all together, with max_records 0: a counts-only query.  counts
 * is required.
 *
 * RB_EINVAL, with nothing enqueued: max_records < 0; max_records 0 with a
 * record array given, or > 0 without; n < 0; env_ids out of range or listing
 * an environment twice; in the device form a host pointer or memory of another
 * device.  RB_EUNSUPPORTED under RB_LAW_BALLS: that law has no contact list
 * (its hit test carries a tolerance of its own).
 *
 * rb_batch_contacts: host arrays, for the environments env_ids[n] (NULL = all
 * n_envs in order, n = n_envs), synchronous: like rb_batch_get_state it
 * finishes the batch's pending work first.  *n_truncated (may be NULL) = the
 * listed bodies with count > max_records.  The lists are staged in a device
 * buffer owned by the batch, allocated on first use and freed with it, of at
 * most RBHIP_BATCH_SAMPLE_BYTES bytes; a request that does not fit is cut into
 * several launches over ranges of the listed environments (RB_EINVAL if one
 * environment's lists alone do not fit). */
int  rb_batch_contacts(rb_batch *b, const int64_t *env_ids, int64_t n, int32_t max_records,
                       int32_t *counts, int32_t *partner, int32_t *kind,
                       double *dist, double *pos, double *frame, int64_t *n_truncated);
/* The same into device arrays of the caller, all environments, enqueued on the
 * batch's stream without waiting (the rules of the device-resident boundary
 * above).  dist, pos and frame are of io_dtype (RB_F64 | RB_F32), converted
 * from the batch's real type by a C cast. */
int  rb_batch_contacts_dev(rb_batch *b, int32_t max_records, int32_t *counts, int32_t *partner,
                           int32_t *kind, void *dist, void *pos, void *frame, int32_t io_dtype);

/* ---- the impulse query of a batch (additive to librbhip 0.4) -------------------
 * What the next rb_batch_step(1, dt, restitution, friction, contact_threshold)
 * does to every body, contact by contact: the two return values jn and jt of
 * compute_collision_impulse_friction (collision.py:7-48) for every contact of
 * the per-body Gauss-Seidel loop (collision.py:72-88), the velocity that
 * apply_impulse_friction (physics_utils.py:25-49) leaves behind, and the body's
 * net contact impulse.  The reference computes jn and jt and drops them; this
 * call replaces reading them out of those call sites.  A pure function of the
 * batch's current state, the step parameters of the call and the batch's
 * constants: it steps nothing, fails nothing (the position check of a step is
 * not run) and changes nothing.
 *
 * Layout: rb_batch_contacts', dense, R = max_records slots per body.  counts
 * [n][M]; partner, kind, dist and jn [n][M][R]; jt [n][M][R][3]; vel and net
 * [n][M][6].
 *
 * counts, partner, kind and dist are word for word what rb_batch_contacts
 * writes for the same state and the same R: the same canonical order (geom1
 * as defined there), the true count past R, kind -1 and zeros in the unused
 * slots (in jn and jt as well), count -1 for every body of a failed
 * environment, count 0 for an absent body of a population.
 *
 * jn, jt: the solve visits the contacts of a body in list order, from the
 * velocity that gravity, the applied forces and the earlier contacts of this
 * body have left.  A contact the step skips (dist not below 0, or |dist| <
 * contact_threshold) has jn 0 and jt 0; so has a separating one (u_rel_n >= 0),
 * as the reference function returns it.  The normal is the step's: the frame
 * flipped for the geom1 body under RB_NORMAL_ORIENTED, raw under RB_NORMAL_RAW.
 *
 * vel: (v, omega) of the body after gravity, applied forces and all its
 * contacts: for every environment the step commits, the words
 * rb_batch_step(1, ...) writes into qvel.
 * net: the body's net contact impulse and net angular impulse about its
 * centre, sum of P and sum of r x P over its applied contacts in list order
 * from +0, P = jn n + jt as apply_impulse_friction evaluates it; gravity and
 * applied forces are not part of it.  net[0:3] / dt is the average contact
 * force of the step.
 * Truncation drops records only: the solve runs over every contact, vel and
 * net do not depend on R.  The vel and net rows of failed environments and of
 * absent bodies are zeros.
 *
 * restitution and friction are the scalars of the call unless
 * rb_batch_set_params set per-environment values; per-environment planes,
 * gravity and applied forces are honoured as the step honours them (the
 * applied-force path for all-zero rows once forces are set), and so is a
 * population.
 *
 * counts is required.  partner, kind, dist, jn and jt are given all together
 * with R > 0, or are all NULL with R 0 (the cheap "sensor only" call).  vel and
 * net may each be NULL.
 *
 * RB_EINVAL, with nothing enqueued: every case of rb_batch_contacts; what
 * rb_batch_step refuses (dt not positive, a negative restitution, friction or
 * contact_threshold, NaN); a non-finite dt, restitution, friction or
 * contact_threshold.  RB_EUNSUPPORTED under RB_LAW_BALLS.
 *
 * rb_batch_impulses: host arrays, the listed environments, synchronous (it
 * finishes the batch's pending work first), staged in rb_batch_contacts'
 * buffer under RBHIP_BATCH_SAMPLE_BYTES and cut into launches over ranges of
 * the listed environments alike (RB_EINVAL if one environment alone does not
 * fit).  *n_truncated (may be NULL) = the listed bodies with count > R.
 * rb_batch_impulses_dev: device arrays of the caller, all environments,
 * enqueued on the batch's stream without waiting; pointers are checked on the
 * host; reals are of io_dtype, converted by a C cast.  Not offered under a
 * stream capture.
 *
 * Not covered: the same query for an rb_world of more than one rank (a world
 * of one rank has it: rb_query_impulses); per-contact records (jn, jt) inside
 * a sampled run (the per-body net impulse is recorded there:
 * rb_batch_run_sampled_impulses), and either for an rb_world; the two-ball
 * law. */
int  rb_batch_impulses(rb_batch *b, const int64_t *env_ids, int64_t n, int32_t max_records,
                       double dt, double restitution, double friction, double contact_threshold,
                       int32_t *counts, int32_t *partner, int32_t *kind, double *dist,
                       double *jn, double *jt, double *vel, double *net, int64_t *n_truncated);
int  rb_batch_impulses_dev(rb_batch *b, int32_t max_records,
                           double dt, double restitution, double friction, double contact_threshold,
                           int32_t *counts, int32_t *partner, int32_t *kind, void *dist,
                           void *jn, void *jt, void *vel, void *net, int32_t io_dtype);

/* ---- contact-impulse curves of a sampled run (additive to librbhip 0.4) --------
 * rb_batch_run_sampled that also records what the contacts did to every body
 * between two samples: the force curve of the run (the ground reaction of a
 * bouncing ball, the load on the bottom cube of a stack) beside the curves the
 * reference's loggers plot.  Stepping, the S = nsteps / every samples, qpos
 * [S][n_envs][M][7], qvel [S][n_envs][M][6], final state, status, steps_done and
 * failure semantics are rb_batch_run_sampled's, word for word.
 *
 * net [S][n_envs][M][6]: row (s, e, k) is the contact impulse (components 0-2)
 * and the angular impulse about its centre (3-5) that body k of environment e
 * received in the window of sample s, steps s * every + 1 .. (s + 1) * every of
 * this call.  It is defined by rb_batch_impulses: for each committed step of
 * the window, that step's net row for the state the step starts from (the sum
 * of P = jn n + jt, the two return values of compute_collision_impulse_friction,
 * collision.py:7-48, and of r x P, over the applied contacts of the per-body
 * loop, collision.py:72-88, in list order from +0, P as
 * apply_impulse_friction evaluates it, physics_utils.py:25-49); these rows
 * added component by component, in step order, from +0, in the batch's real
 * type.  net[s][e][k][0:3] / (every * dt) is the window's average contact force;
 * with every == 1 a row is the word rb_batch_impulses returns before that step.
 * A step that is not committed contributes nothing (the failing step of an
 * environment and every later one): the window that holds the failure keeps the
 * sum of its committed steps, later windows are rows of +0.  Rows of absent
 * bodies of a population are +0.  Steps after the last sample are run and
 * belong to no window.  Step parameters, per-environment parameters, planes,
 * gravity, applied forces and a population are honoured as the step honours
 * them.
 *
 * The sums are kept in the step kernel's register loop and do not depend on
 * how the run is cut into launches (RB_BATCH_CHUNK steps at most, fewer where
 * the sample buffer fills): a window left open by a launch is carried in a
 * per-batch device buffer of 6 * n_envs * M reals.
 *
 * net is required when S > 0.  qpos and qvel may each be NULL: a sample takes
 * rows = 6 + (qpos ? 7 : 0) + (qvel ? 6 : 0) struct-of-arrays rows of the
 * buffer, n_envs * M * rows * (sizeof(real) + 8) bytes in the host form and
 * n_envs * M * rows * sizeof(real) in the device form, under
 * RBHIP_BATCH_SAMPLE_BYTES.
 * RB_EINVAL (nothing stepped) as rb_batch_run_sampled, with net in the place
 * of qpos: every < 1, nsteps < 0, what rb_batch_step refuses, net NULL with
 * S > 0, a buffer bound below one sample; in the device form a host pointer or
 * memory of another device, or an unknown io_dtype.  RB_EUNSUPPORTED under
 * RB_LAW_BALLS, changing nothing.
 *
 * rb_batch_run_sampled_impulses: host arrays, synchronous, reports through
 * n_failed as rb_batch_run_sampled does.
 * rb_batch_run_sampled_impulses_dev: device arrays of io_dtype (converted by a
 * C cast), enqueued on the batch's stream without waiting, no report
 * (rb_batch_sync).  Not offered under a stream capture.
 *
 * Not covered: per-contact records (jn, jt) inside a sampled run; the same
 * for an rb_world; the two-ball law. */
int  rb_batch_run_sampled_impulses(rb_batch *b, int64_t nsteps, int64_t every, double dt, double restitution,
                                   double friction, double contact_threshold,
                                   double *qpos, double *qvel, double *net, int64_t *n_failed);
int  rb_batch_run_sampled_impulses_dev(rb_batch *b, int64_t nsteps, int64_t every, double dt, double restitution,
                                       double friction, double contact_threshold,
                                       void *qpos, void *qvel, void *net, int32_t io_dtype);

/* Retired (kept for ABI compatibility with librbhip 0.2): the round-3 tile
 * blocks' configuration.  mode -1 (auto) and 0 (off) are accepted and do
 * nothing; mode 1 returns RB_EUNSUPPORTED.  The step forms are chosen by the
 * library (RB_STAT_FORM); RBHIP_TILE selects the tile form for tests. */
int rb_tile_config(rb_world *w, int32_t mode, int32_t kmax, double band, int64_t owned);

#ifdef __cplusplus
}
#endif
#endif /* RBHIP_H */
