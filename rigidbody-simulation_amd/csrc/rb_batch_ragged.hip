// rb_batch_ragged.hip — batched worlds with a population
// (rb_batch_set_population; rb_batch_ragged.hpp): per environment a body count
// n_e in 1..M and a kind for each body slot.  Bodies 0..n_e-1 are present,
// the rest absent: they have no lane (one-wave batches) or an idle one (wide
// batches and the queries), are nobody's partner, take no plane contact,
// cannot fail their environment and are never stored.
//
// A step is batch_step_body (rb_batch_body.hpp), one text for this unit's and
// rb_batch_wide.hip's step kernels, with the population's kind and count handed in:
// partners in ascending id over the present bodies of the environment, which
// are a prefix, so the ids are those of a world of the present bodies alone
// and an environment steps bit-identically to it.  The two step kernels below
// are their mappings alone.
//
// One-wave batches (M <= 64), ragged_step_kernel: the lanes are packed by the
// host's plan (rb_laneplan.hpp).  A lane reads its row e * M + b from the
// per-lane table (-1: idle); the b == 0 lanes of the wave, by ballot, give a
// lane its environment's index within the wave; the environment's bodies sit
// in the n_e LDS slots from lane - b.  Idle lanes run along on row 0's data,
// visit nobody and store nothing.
//
// Wide batches (65..256 bodies), ragged_wide_kernel: batch_wide_kernel's
// mapping (rb_batch_wide.hip), one environment per workgroup, lane = body id,
// lanes at or past n_e idle; whole idle waves still reach every barrier; the
// failure word ping-pongs as there.
//
// Per-environment planes, gravity and forces are not a template parameter
// here: the planes are always read from the wave's block in dynamic LDS
// (filled from the batch's rows, or with the template's planes), gravity and
// forces are tested at run time: the body's ENVS instances.
//
// The queries (ragged_contacts_kernel, ragged_wide_contacts_kernel) keep the
// fixed E x M mapping of rb_batch_contacts.hip / rb_batch_wide.hip: a query is
// one pass into a dense (n, M, R) layout; an absent body writes count 0 (-1 in
// a failed environment) and unused slots.
// Built once per real type: RB_INST = 1 fp64, 2 fp32.
#include "rb_batch_body.hpp"
#include "rb_contacts.hpp"
#include "rb_batch_ragged.hpp"

namespace rb {
namespace {

// The planes of `count` environments from `env0` on into the block
// [plane][component][stride] (EnvPlanes): lane l < count fills environment
// env0 + l, from the batch's rows or with the template's planes.
template <typename T>
__device__ __forceinline__ void ragged_planes_fill(const BatchParams<T> &p, T *blk, int lane, int64_t env0, int count,
                                                   int stride) {
    if (lane >= count) return;
    const int64_t env = env0 + lane;             // (< p.E: the plan's ranges end at E)
    for (int a = 0; a < p.n_planes; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            T n = p.pn[a][c], o = p.pp[a][c];
            if (p.env_planes) {
                n = p.env_planes[((int64_t)a * 6 + c) * p.E + env];
                o = p.env_planes[((int64_t)a * 6 + 3 + c) * p.E + env];
            }
            blk[(a * 6 + c) * stride + lane] = n;
            blk[(a * 6 + 3 + c) * stride + lane] = o;
        }
    }
}

// BOXES: a present body of some environment is a box (a lane's kind is the
// population's kind of its row); else spheres only: no polygon, orientation,
// extent or kind LDS, two waves per SIMD and more
// REC: the recording instance of a sampled run
template <typename T, bool BOXES, bool REC>
__global__ __launch_bounds__(BATCH_BLOCK) __attribute__((amdgpu_waves_per_eu(1, BOXES ? 1 : 8)))
void ragged_step_kernel(BatchParams<T> p, Population pop) {
    const int lane = threadIdx.x;
    const int M = p.M;
    // the plan: this lane's row (the grid is pop.waves workgroups of one wave)
    const int32_t row = pop.lane_row[(int64_t)blockIdx.x * BATCH_BLOCK + lane];
    // idle lanes run along on row 0's data, visit no partner and store nothing
    const bool active = row >= 0;
    const int64_t g = active ? row : 0;
    const int64_t env = g / M;
    const int b = (int)(g - env * M);            // body within the environment
    // the environment within the wave: the b == 0 lanes up to this one
    const unsigned long long heads = __ballot(active && b == 0);
    const int el = active ? __popcll(heads & (~0ull >> (63 - lane))) - 1 : 0;
    const int ebase = active ? lane - b : 0;     // the environment's first lane
    const int nj = active ? pop.n_bodies[env] : 0;   // bodies whose pairs this lane evaluates
    const int64_t env0 = pop.wave_env0[blockIdx.x];
    const int nenv = (int)(pop.wave_env0[blockIdx.x + 1] - env0);

    int32_t kind = 0;
    if constexpr (BOXES) kind = pop.kind[g];
    const int stride = pop.epw_max;
    batch_step_body<T, BOXES, REC, true, BATCH_BLOCK>(p, active, g, env, b, ebase, nj, kind, el, stride, [&](T *blk) {
        ragged_planes_fill(p, blk, lane, env0, nenv, stride);
    });
}

// BLOCK: threads per workgroup, 64 * ceil(M / 64)
template <typename T, bool BOXES, bool REC, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, BOXES ? 1 : 8)))
void ragged_wide_kernel(BatchParams<T> p, Population pop) {
    static_assert(BLOCK % 64 == 0 && BLOCK > BATCH_BLOCK && BLOCK <= BATCH_WIDE_MAX, "one lane per body, whole waves");
    const int lane = threadIdx.x;                // = body id
    const int M = p.M;
    const int64_t env = blockIdx.x;              // (the grid is p.E workgroups)
    const int ne = pop.n_bodies[env];            // present bodies (<= M <= BLOCK)
    // idle lanes (absent bodies, lanes past M) run along on the environment's
    // body 0, visit no partner and store nothing
    const bool active = lane < ne;
    const int b = active ? lane : 0;
    const int64_t g = env * M + b;
    const int nj = active ? ne : 0;              // bodies whose pairs this lane evaluates

    int32_t kind = 0;
    if constexpr (BOXES) kind = pop.kind[g];
    // one environment per block: column 0 of a planes block of stride 1
    batch_step_body<T, BOXES, REC, true, BLOCK>(p, active, g, env, b, 0, nj, kind, 0, 1,
                                                [&](T *blk) { ragged_planes_fill(p, blk, lane, env, 1, 1); });
}

// ---- the contact query -----------------------------------------------------------
// contacts_body of rb_batch_contacts.hip / wide_contacts_kernel of
// rb_batch_wide.hip with the population: lane `lane` of a workgroup of BLOCK
// threads is body b of the environment whose first lane is ebase, `in_range`
// where that environment is a row of the query.  The list, its order and its
// layout are those files'.
template <typename T, bool BOXES, int BLOCK>
__device__ __forceinline__ void ragged_contacts_body(const BatchParams<T> &p, const Population &pop, const ContactQuery &q,
                                                     bool in_range, int64_t row_raw, int b, int ebase) {
    __shared__ Snap<T> s_snap[BLOCK];

    const int lane = threadIdx.x;
    const int M = p.M;
    // lanes without a row load slot 0's data and leave after the barrier
    const int64_t row = in_range ? row_raw : 0;
    const int64_t env = !in_range ? 0 : q.ids ? q.ids[row] : q.env0 + row;
    const int ne = pop.n_bodies[env];
    const int64_t g = in_range ? env * M + b : 0;
    const bool present = in_range && b < ne;

    // ---- load once ---------------------------------------------------------
    int32_t kind = 0;
    if constexpr (BOXES) kind = pop.kind[g];
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
    if (!in_range) return;

    const int32_t R = q.R;
    const int64_t slot0 = (row * M + b) * (int64_t)R;
    int32_t n = 0;
    auto emit = [&](int32_t partner, int32_t ck, const Contact<T> &con) {
        if (n < R) put_record(q, slot0 + n, partner, ck, con.dist, con.pos, con.frame);
        ++n;
    };

    if (!failed && present) {
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

        // ---- every other present body of the environment, ascending id -----------
        for (int j = 0; j < ne; ++j) {
            if (j == b) continue;
            const Snap<T> sj = s_snap[ebase + j];
            const V3<T> cj = {sj.x, sj.y, sj.z};
            int32_t kj = 0;
            if constexpr (BOXES) kj = s_k[ebase + j];
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
                const V3<T> hj = {s_e[ebase + j], s_e[BLOCK + ebase + j], s_e[2 * BLOCK + ebase + j]};
                M3<T> Mj;
                if (kj != 0) Mj = mj_body_mat(s_q[ebase + j]);
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

    // ---- the count (an absent body: 0), and the fill of the unused slots -------------
    q.counts[row * M + b] = failed ? -1 : n;
    const V3<T> zero = {T(0), T(0), T(0)};
    for (int32_t s = failed ? 0 : n; s < R; ++s) put_record(q, slot0 + s, 0, -1, T(0), zero, zero);
}

// M <= 64: floor(64 / M) rows of the query per one-wave workgroup (rb_batch_contacts.hip)
template <typename T, bool BOXES>
__global__ __launch_bounds__(BATCH_BLOCK) __attribute__((amdgpu_waves_per_eu(1, BOXES ? 1 : 8)))
void ragged_contacts_kernel(BatchParams<T> p, Population pop, ContactQuery q) {
    const int lane = threadIdx.x;
    const int M = p.M;
    const int epw = BATCH_BLOCK / M;
    const int el = lane / M;
    const int64_t row = (int64_t)blockIdx.x * epw + el;
    const bool in_range = el < epw && row < q.n;
    ragged_contacts_body<T, BOXES, BATCH_BLOCK>(p, pop, q, in_range, row, lane - el * M, in_range ? el * M : 0);
}

// 65..256 bodies: one row per workgroup, lane = body id (rb_batch_wide.hip)
template <typename T, bool BOXES, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, BOXES ? 1 : 8)))
void ragged_wide_contacts_kernel(BatchParams<T> p, Population pop, ContactQuery q) {
    static_assert(BLOCK % 64 == 0 && BLOCK > BATCH_BLOCK && BLOCK <= BATCH_WIDE_MAX, "one lane per body, whole waves");
    const int lane = threadIdx.x;
    const bool in_range = lane < p.M;
    ragged_contacts_body<T, BOXES, BLOCK>(p, pop, q, in_range, blockIdx.x, in_range ? lane : 0, 0);
}

bool pop_ok(const Population &pop, bool boxes, bool wide) {
    if (!pop.n_bodies || (boxes && !pop.kind)) return false;
    return wide || (pop.wave_env0 && pop.lane_row && pop.waves >= 1 && pop.epw_max >= 1 && pop.epw_max <= BATCH_BLOCK);
}

}  // namespace

template <typename T>
hipError_t launch_ragged_step(const BatchParams<T> &p, const Population &pop, bool boxes, bool rec, hipStream_t s) {
    if (p.E <= 0 || p.k <= 0) return hipSuccess;
    if (p.M < 1 || p.M > BATCH_WIDE_MAX || p.n_planes < 0 || p.n_planes > MAX_PLANES) return hipErrorInvalidValue;
    const bool wide = p.M > BATCH_BLOCK;
    if (!pop_ok(pop, boxes, wide)) return hipErrorInvalidValue;
    if (rec && !rec_ok(p)) return hipErrorInvalidValue;
    as_constant(boxes, [&](auto BOXES) {
        as_constant(rec, [&](auto REC) {
            if (wide) {
                // one environment per workgroup; its planes in LDS, [n_planes][6]
                const size_t lds = (size_t)p.n_planes * 6 * sizeof(T);
                with_block(p.M, [&](auto BLOCK) {
                    hipLaunchKernelGGL((ragged_wide_kernel<T, BOXES.value, REC.value, BLOCK.value>), dim3((unsigned)p.E),
                                       dim3(BLOCK.value), lds, s, p, pop);
                });
            } else {
                // the wave's planes in LDS, [n_planes][6][most environments of a wave]
                const size_t lds = (size_t)pop.epw_max * (size_t)p.n_planes * 6 * sizeof(T);
                hipLaunchKernelGGL((ragged_step_kernel<T, BOXES.value, REC.value>), dim3((unsigned)pop.waves),
                                   dim3(BATCH_BLOCK), lds, s, p, pop);
            }
        });
    });
    return hipGetLastError();
}

template <typename T>
hipError_t launch_ragged_contacts(const BatchParams<T> &p, const Population &pop, const ContactQuery &q, bool boxes,
                                  hipStream_t s) {
    if (q.n <= 0) return hipSuccess;
    if (!query_ok(p, q, 1, BATCH_WIDE_MAX) || !pop_ok(pop, boxes, true)) return hipErrorInvalidValue;
    as_constant(boxes, [&](auto BOXES) {
        if (p.M > BATCH_BLOCK) {
            with_block(p.M, [&](auto BLOCK) {
                hipLaunchKernelGGL((ragged_wide_contacts_kernel<T, BOXES.value, BLOCK.value>), dim3((unsigned)q.n),
                                   dim3(BLOCK.value), 0, s, p, pop, q);
            });
        } else {
            const int64_t epw = BATCH_BLOCK / p.M;
            const unsigned blocks = (unsigned)((q.n + epw - 1) / epw);
            hipLaunchKernelGGL((ragged_contacts_kernel<T, BOXES.value>), dim3(blocks), dim3(BATCH_BLOCK), 0, s, p, pop, q);
        }
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
template hipError_t launch_ragged_step<Real>(const BatchParams<Real> &, const Population &, bool, bool, hipStream_t);
template hipError_t launch_ragged_contacts<Real>(const BatchParams<Real> &, const Population &, const ContactQuery &, bool,
                                                 hipStream_t);

}  // namespace rb
