// rb_batch_wide.hip — batched worlds whose environments span several waves
// (rb_batch_create_wide, 65..256 bodies per environment): the step kernel and
// the contact query of a wide batch.
//
// One environment per workgroup, one lane per body: the block is
// 64 * ceil(M / 64) threads (128, 192 or 256) and lane = body id.  Lanes at or
// past M are idle as in the one-wave kernels (rb_batch.hip): they run along on
// slot 0's data, visit no partner, store nothing and raise no failure, and
// they reach every barrier (nothing returns before the step loop ends).
//
// A step is batch_step_body (rb_batch_body.hpp), one text for this unit's and
// rb_batch_ragged.hip's step kernels: batch_mixed_kernel's sequence (BOXES) or
// batch_step_kernel's sphere path (!BOXES; rb_batch.hip), partners in
// ascending id over the whole environment, step-start snapshots (BOXES:
// orientations too) ping-pong in LDS, one __syncthreads() per step, state in
// registers for up to RB_BATCH_CHUNK steps.  So an environment steps
// bit-identically to a world of its scene, whichever waves its bodies sit in.
// The kernel below is the mapping alone.
//
// What the workgroup barrier changes against the one-wave kernels is the
// failure flag.  Waves leave a barrier at different times: a wave that is
// already in step s + 1 may raise the flag before a slower wave has read it
// for step s, which would freeze the two at different steps.  The flag
// therefore ping-pongs as the snapshots do: step s raises and reads word
// s & 1, which nobody writes again before the barrier of step s + 1.  A word
// is never cleared: once it is read as set every lane is failed for good.
// (batch_step_body does this for every block of more than one wave.)
//
// LDS scales with the block (a template parameter): BOXES at f64 takes 69,128 /
// 103,688 / 138,248 bytes at 128 / 192 / 256 threads, of which the clipping
// polygon (a column of 48 reals per lane, stride BLOCK) is 48 * BLOCK * 8.
// BOXES is built as batch_mixed_kernel is: one wave per SIMD.
// Built once per real type: RB_INST = 1 fp64, 2 fp32.
#include "rb_batch_body.hpp"
#include "rb_contacts.hpp"

namespace rb {
namespace {

// BOXES: the template holds a box (a lane's kind is the template's kind of its
// body); else spheres only: no polygon, orientation, extent or kind LDS
// REC: the recording instance of a sampled run
// ENVS: per-environment planes, gravity or applied forces are set
// BLOCK: threads per workgroup, 64 * ceil(M / 64)
template <typename T, bool BOXES, bool REC, bool ENVS, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, BOXES ? 1 : 8)))
void batch_wide_kernel(BatchParams<T> p) {
    static_assert(BLOCK % 64 == 0 && BLOCK > BATCH_BLOCK && BLOCK <= BATCH_WIDE_MAX, "one lane per body, whole waves");
    const int lane = threadIdx.x;                // = body id
    const int M = p.M;
    // idle lanes run along on slot 0's data, visit no partner and store nothing
    const bool active = lane < M;
    const int b = active ? lane : 0;
    const int64_t env = blockIdx.x;              // (the grid is p.E workgroups)
    const int64_t g = active ? env * M + b : 0;
    const int nj = active ? M : 0;               // bodies whose pairs this lane evaluates

    int32_t kind = 0;
    if constexpr (BOXES) kind = p.cs.kind[b];            // [M]: the template's kinds
    // one environment per block: column 0 of a planes block of stride 1
    batch_step_body<T, BOXES, REC, ENVS, BLOCK>(p, active, g, env, b, 0, nj, kind, 0, 1,
                                                [&](T *blk) { env_planes_fill(p, blk, lane, 1); });
}

// ---- the contact query of a wide batch ------------------------------------------
// contacts_body of rb_batch_contacts.hip with this file's mapping: a workgroup
// takes one row of the query, lane = body id.  The list, its order and its
// layout are that file's.

template <typename T, bool BOXES, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, BOXES ? 1 : 8)))
void wide_contacts_kernel(BatchParams<T> p, ContactQuery q) {
    __shared__ Snap<T> s_snap[BLOCK];

    const int lane = threadIdx.x;                // = body id
    const int M = p.M;
    // idle lanes load slot 0's data and leave after the barrier
    const bool active = lane < M;
    const int b = active ? lane : 0;
    const int64_t row = blockIdx.x;              // (the grid is q.n workgroups)
    const int64_t env = q.ids ? q.ids[row] : q.env0 + row;
    const int64_t g = active ? env * M + b : 0;

    // ---- load once ---------------------------------------------------------
    int32_t kind = 0;
    if constexpr (BOXES) kind = p.cs.kind[b];
    const Snap<T> self = p.snap[g];
    const V3<T> x = {self.x, self.y, self.z};
    const T bi = self.r;
    const V3<T> sz = {p.cs.sx()[g], kind != 0 ? p.cs.sy()[g] : T(0), kind != 0 ? p.cs.sz()[g] : T(0)};
    Q4<T> qt = {T(1), T(0), T(0), T(0)};
    if (kind != 0) qt = {p.st.qw()[g], p.st.qx()[g], p.st.qy()[g], p.st.qz()[g]};
    const bool failed = p.code[env] != 0;

    // what the partners read
    s_snap[lane] = self;
    T *poly = nullptr;
    const Q4<T> *s_q = nullptr;
    const T *s_e = nullptr;
    const int32_t *s_k = nullptr;
    if constexpr (BOXES) {
        __shared__ Q4<T> s_quat[BLOCK];
        __shared__ T s_ext[3 * BLOCK];           // half extents (a sphere: its radius, 0, 0)
        __shared__ int32_t s_kind[BLOCK];
        __shared__ T s_poly[48 * BLOCK];         // box-box face clipping: 2 x 8 vertices x 3 per lane
        s_quat[lane] = qt;
        s_ext[lane] = sz.x; s_ext[BLOCK + lane] = sz.y; s_ext[2 * BLOCK + lane] = sz.z;
        s_kind[lane] = kind;
        poly = s_poly + lane;
        s_q = s_quat; s_e = s_ext; s_k = s_kind;
    }
    __syncthreads();
    if (!active) return;

    const int32_t R = q.R;
    const int64_t slot0 = (row * M + b) * (int64_t)R;
    int32_t n = 0;
    auto emit = [&](int32_t partner, int32_t ck, const Contact<T> &con) {
        if (n < R) put_record(q, slot0 + n, partner, ck, con.dist, con.pos, con.frame);
        ++n;
    };

    if (!failed) {
        // ---- planes, plane order: a sphere's one, a box's corners in bit order, at most 4 ----
        M3<T> Mi;
        if (kind != 0) Mi = mj_body_mat(qt);
        for (int a = 0; a < p.n_planes; ++a) {
            V3<T> pn = {p.pn[a][0], p.pn[a][1], p.pn[a][2]};
            V3<T> pp = {p.pp[a][0], p.pp[a][1], p.pp[a][2]};
            if (p.env_planes) {                  // [n_planes][6][E]
                const T *r = p.env_planes + (int64_t)a * 6 * p.E + env;
                pn = {r[0], r[p.E], r[2 * p.E]};
                pp = {r[3 * p.E], r[4 * p.E], r[5 * p.E]};
            }
            Contact<T> con;
            if (kind == 0) {
                if (plane_sphere(pn, pp, x, sz.x, con)) emit(-1 - a, 0, con);
            } else {
                const V3<T> dif = {x.x - pp.x, x.y - pp.y, x.z - pp.z};
                const T dist = mj_dot(dif, pn);
                int cnt = 0;
                for (int c = 0; c < 8 && cnt < 4; ++c) {
                    if (!plane_box_corner(pn, x, dist, Mi, sz, c, con)) continue;
                    ++cnt;
                    emit(-1 - a, 1 + c, con);
                }
            }
        }

        // ---- every other body of the environment, ascending id -------------------
        for (int j = 0; j < M; ++j) {
            if (j == b) continue;
            const Snap<T> sj = s_snap[j];
            const V3<T> cj = {sj.x, sj.y, sj.z};
            int32_t kj = 0;
            if constexpr (BOXES) kj = s_k[j];
            if (kind == 0 && kj == 0) {
                if (!sphere_sphere_hit(x, sz.x, cj, sj.r)) continue;
                Contact<T> con;
                if (b < j) sphere_sphere(x, sz.x, cj, sj.r, con);      // geom1: the lower id
                else sphere_sphere(cj, sj.r, x, sz.x, con);
                emit(j, 16, con);
                continue;
            }
            if constexpr (BOXES) {
                // box-involved: overlapping bounding spheres (candidate_hit, rb_step.hpp)
                const V3<T> dd = {x.x - cj.x, x.y - cj.y, x.z - cj.z};
                if (!(sqroot(mj_dot(dd, dd)) <= bi + sj.r)) continue;
                const V3<T> hj = {s_e[j], s_e[BLOCK + j], s_e[2 * BLOCK + j]};
                M3<T> Mj;
                if (kj != 0) Mj = mj_body_mat(s_q[j]);
                // geom1: the sphere of a sphere-box pair, else the lower id (solve_box_pair)
                const bool g1 = (kind == 0 && kj != 0) || (kind != 0 && kj != 0 && b < j);
                const V3<T> p1 = g1 ? x : cj, p2 = g1 ? cj : x;
                const V3<T> h1 = g1 ? sz : hj, h2 = g1 ? hj : sz;
                M3<T> M1, M2;
#pragma unroll
                for (int c = 0; c < 9; ++c) { M1.a[c] = g1 ? Mi.a[c] : Mj.a[c]; M2.a[c] = g1 ? Mj.a[c] : Mi.a[c]; }
                if (kind == 0 || kj == 0) {
                    Contact<T> con;
                    if (sphere_box(p1, g1 ? sz.x : sj.r, p2, M2, h2, con)) emit(j, CK_SPHERE_BOX, con);
                } else {
                    box_box(p1, M1, h1, p2, M2, h2, poly, BLOCK, [&](const Contact<T> &c, int ck) { emit(j, ck, c); });
                }
            }
        }
    }

    // ---- the count, and the fill of the unused slots ------------------------------
    q.counts[row * M + b] = failed ? -1 : n;
    const V3<T> zero = {T(0), T(0), T(0)};
    for (int32_t s = failed ? 0 : n; s < R; ++s) put_record(q, slot0 + s, 0, -1, T(0), zero, zero);
}

}  // namespace

template <typename T> hipError_t launch_batch_wide(const BatchParams<T> &p, bool boxes, bool rec, hipStream_t s) {
    if (p.E <= 0 || p.k <= 0) return hipSuccess;
    if (p.M <= BATCH_BLOCK || p.M > BATCH_WIDE_MAX || p.n_planes < 0 || p.n_planes > MAX_PLANES) return hipErrorInvalidValue;
    if (boxes && !p.cs.kind) return hipErrorInvalidValue;
    if (rec && !rec_ok(p)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)p.E;       // one environment per workgroup
    with_block(p.M, [&](auto BLOCK) {
        as_constant(boxes, [&](auto BOXES) {
            as_constant(rec, [&](auto REC) {
                as_constant(p.env_planes || p.env_g || p.env_xfrc, [&](auto ENVS) {
                    // ENVS: the environment's planes in LDS, [n_planes][6]
                    const size_t lds = ENVS.value ? (size_t)p.n_planes * 6 * sizeof(T) : 0;
                    hipLaunchKernelGGL((batch_wide_kernel<T, BOXES.value, REC.value, ENVS.value, BLOCK.value>), dim3(blocks),
                                       dim3(BLOCK.value), lds, s, p);
                });
            });
        });
    });
    return hipGetLastError();
}

template <typename T>
hipError_t launch_batch_wide_contacts(const BatchParams<T> &p, const ContactQuery &q, bool boxes, hipStream_t s) {
    if (q.n <= 0) return hipSuccess;
    if (!query_ok(p, q, BATCH_BLOCK + 1, BATCH_WIDE_MAX) || (boxes && !p.cs.kind)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)q.n;       // one row per workgroup
    with_block(p.M, [&](auto BLOCK) {
        as_constant(boxes, [&](auto BOXES) {
            hipLaunchKernelGGL((wide_contacts_kernel<T, BOXES.value, BLOCK.value>), dim3(blocks), dim3(BLOCK.value), 0, s, p, q);
        });
    });
    return hipGetLastError();
}

#if RB_INST == 1
using Real = double;
#elif RB_INST == 2
using Real = float;
#else
#error "RB_INST: 1 (fp64) or 2 (fp32)"
#endif
template hipError_t launch_batch_wide<Real>(const BatchParams<Real> &, bool, bool, hipStream_t);
template hipError_t launch_batch_wide_contacts<Real>(const BatchParams<Real> &, const ContactQuery &, bool, hipStream_t);

}  // namespace rb
