// rb_batch_contacts.hip — the contact query of a batch (rb_batch_contacts.hpp):
// the kernel that emits the contact list the batch step kernels consume.
//
// The lane mapping is the batch step kernels' (rb_batch.hip): one lane per
// body, floor(64 / M) whole environments per one-wave workgroup, idle lanes
// store nothing; a workgroup takes floor(64 / M) rows of the query.  One pass:
// a lane loads its snapshot, quaternion, half extents and kind, puts what its
// partners read into LDS (one barrier), walks the planes in plane order and
// then every other body of its environment in ascending id with the tests of
// the step kernels (sphere_sphere_hit; for a box-involved pair overlapping
// bounding spheres), and writes one record per generated contact straight
// into the caller's layout.  None of the solve's skip rules (dist < 0, the
// threshold) applies: this is the list mj_forward generates, not the part of
// it a step acts on.  The planes come from the parameter block, or, where
// rb_batch_set_planes is set, from the environment's rows in global memory (a
// single pass reads each once: no block in LDS, no instance of its own).
//
// The instance of a mixed template holds the box narrowphase and is built as
// batch_mixed_kernel is (rb_batch_boxes.hip): one wave per SIMD, register
// arrays indexed by compile-time constants only, the clipping polygon of
// box_box a column of 48 reals per lane in LDS.
#include "rb_device.hpp"
#include "rb_boxes.hpp"
#include "rb_batch_contacts.hpp"
#include "rb_contacts.hpp"
#include "rb_batch_checks.hpp"

namespace rb {
namespace {

// MIXED: the template mixes spheres and boxes (a lane's kind is the
// template's kind of its body); else spheres only, or (q.box) the one box
template <typename T, bool MIXED>
__device__ __forceinline__ void contacts_body(const BatchParams<T> &p, const ContactQuery &q) {
    __shared__ Snap<T> s_snap[BATCH_BLOCK];

    const int lane = threadIdx.x;
    const int M = p.M;
    const int epw = BATCH_BLOCK / M;             // whole environments (rows) per wave
    const int el_raw = lane / M;
    const int b = lane - el_raw * M;             // body within the environment
    const int64_t row_raw = (int64_t)blockIdx.x * epw + el_raw;
    // lanes past the wave's last whole environment, or past the query, are
    // idle: they load slot 0's data and leave after the barrier
    const bool active = el_raw < epw && row_raw < q.n;
    const int el = active ? el_raw : 0;
    const int64_t row = active ? row_raw : 0;
    const int64_t env = !active ? 0 : q.ids ? q.ids[row] : q.env0 + row;
    const int64_t g = active ? env * M + b : 0;
    const int ebase = el * M;                    // the environment's first lane

    // ---- load once ---------------------------------------------------------
    int32_t kind = q.box ? 1 : 0;
    if constexpr (MIXED) kind = p.cs.kind[active ? b : 0];
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
    if constexpr (MIXED) {
        __shared__ Q4<T> s_quat[BATCH_BLOCK];
        __shared__ T s_ext[3 * BATCH_BLOCK];     // half extents (a sphere: its radius, 0, 0)
        __shared__ int32_t s_kind[BATCH_BLOCK];
        __shared__ T s_poly[48 * BATCH_BLOCK];   // box-box face clipping: 2 x 8 vertices x 3 per lane
        s_quat[lane] = qt;
        s_ext[lane] = sz.x; s_ext[BATCH_BLOCK + lane] = sz.y; s_ext[2 * BATCH_BLOCK + lane] = sz.z;
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
            const Snap<T> sj = s_snap[ebase + j];
            const V3<T> cj = {sj.x, sj.y, sj.z};
            int32_t kj = kind;                   // (not MIXED: spheres only; the one box has no partner)
            if constexpr (MIXED) kj = s_k[ebase + j];
            if (kind == 0 && kj == 0) {
                if (!sphere_sphere_hit(x, sz.x, cj, sj.r)) continue;
                Contact<T> con;
                if (b < j) sphere_sphere(x, sz.x, cj, sj.r, con);      // geom1: the lower id
                else sphere_sphere(cj, sj.r, x, sz.x, con);
                emit(j, 16, con);
                continue;
            }
            if constexpr (MIXED) {
                // box-involved: overlapping bounding spheres (candidate_hit, rb_step.hpp)
                const V3<T> dd = {x.x - cj.x, x.y - cj.y, x.z - cj.z};
                if (!(sqroot(mj_dot(dd, dd)) <= bi + sj.r)) continue;
                const V3<T> hj = {s_e[ebase + j], s_e[BATCH_BLOCK + ebase + j], s_e[2 * BATCH_BLOCK + ebase + j]};
                M3<T> Mj;
                if (kj != 0) Mj = mj_body_mat(s_q[ebase + j]);
                // geom1: the sphere of a sphere-box pair, else the lower id
                // (one call of each primitive, operands selected: solve_box_pair, rb_batch_boxes.hip)
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
                    box_box(p1, M1, h1, p2, M2, h2, poly, BATCH_BLOCK, [&](const Contact<T> &c, int ck) { emit(j, ck, c); });
                }
            }
        }
    }

    // ---- the count, and the fill of the unused slots ------------------------------
    q.counts[row * M + b] = failed ? -1 : n;
    const V3<T> zero = {T(0), T(0), T(0)};
    for (int32_t s = failed ? 0 : n; s < R; ++s) put_record(q, slot0 + s, 0, -1, T(0), zero, zero);
}

template <typename T>
__global__ __launch_bounds__(BATCH_BLOCK) void batch_contacts_kernel(BatchParams<T> p, ContactQuery q) {
    contacts_body<T, false>(p, q);
}

template <typename T>
__global__ __launch_bounds__(BATCH_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
void batch_contacts_boxes_kernel(BatchParams<T> p, ContactQuery q) {
    contacts_body<T, true>(p, q);
}

}  // namespace

template <typename T>
hipError_t launch_batch_contacts(const BatchParams<T> &p, const ContactQuery &q, bool mixed, hipStream_t s) {
    if (q.n <= 0) return hipSuccess;
    if (!query_ok(p, q, 1, BATCH_BLOCK)) return hipErrorInvalidValue;
    if (mixed ? !p.cs.kind || p.M < 2 : q.box && p.M != 1) return hipErrorInvalidValue;
    const int64_t epw = BATCH_BLOCK / p.M;
    const unsigned blocks = (unsigned)((q.n + epw - 1) / epw);
    if (mixed) hipLaunchKernelGGL((batch_contacts_boxes_kernel<T>), dim3(blocks), dim3(BATCH_BLOCK), 0, s, p, q);
    else hipLaunchKernelGGL((batch_contacts_kernel<T>), dim3(blocks), dim3(BATCH_BLOCK), 0, s, p, q);
    return hipGetLastError();
}

template hipError_t launch_batch_contacts<double>(const BatchParams<double> &, const ContactQuery &, bool, hipStream_t);
template hipError_t launch_batch_contacts<float>(const BatchParams<float> &, const ContactQuery &, bool, hipStream_t);

}  // namespace rb
