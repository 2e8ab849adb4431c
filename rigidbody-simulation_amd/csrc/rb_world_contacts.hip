// rb_world_contacts.hip — the contact query of a world (rb_world_contacts.hpp):
// the kernel that joins the hashed-grid search of the step kernels with the
// narrowphase, without a solve.
//
// One lane per queried body, one wave per workgroup.  A lane loads its
// snapshot, kind, half extents and (a box) orientation, searches the 2 x 2 x 2
// neighbourhood of its cell in the query's own table with the step kernels'
// one-lane search (rb_grid.hpp search_buckets, a partner list of QUERY_MAXP
// ids kept ascending in the lane's LDS column) and their candidate test
// (rb_step.hpp candidate_hit), then walks the planes in plane order and the
// partners in ascending id exactly as the batch's query does
// (rb_contacts.hpp) and writes one record per generated contact straight into
// the caller's layout: a lane's R slots are contiguous, so its records fill
// whole lines by themselves.  None of the solve's skip rules applies.
//
// Nothing of the world is written.  A lane whose list cannot be built (more
// than QUERY_MAXP partners, a position no cell holds, or a table that
// overflowed while it was filled) stores QUERY_NO_LIST and unused slots, and
// the reason goes to the query's own error word (sp.err), never the world's.
//
// Two instances per real type: spheres only (no box code, no occupancy cap),
// and the one with the box narrowphase, built as batch_contacts_boxes_kernel
// is: one wave per SIMD, the clipping polygon of box_box a column of 48 reals
// per lane in LDS; a partner's orientation and half extents are read by id
// from the state rows and the constants.
#include "rb_step.hpp"
#include "rb_contacts.hpp"
#include "rb_world_contacts.hpp"

namespace rb {
namespace {

static_assert(STEP_BLOCK == 64, "one wave per workgroup: search_buckets strides the LDS columns by STEP_BLOCK");

template <typename T, bool BOXES>
__device__ __forceinline__ void world_contacts_body(const WorldContactQuery<T> &q) {
    __shared__ int32_t s_id[QUERY_MAXP * STEP_BLOCK];

    const int tid = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * STEP_BLOCK + tid;
    if (k >= q.count) return;                    // (no barrier below: lanes past the range store nothing)
    const StepParams<T> &p = q.sp;
    const int32_t i = (int32_t)(q.first + k);

    // ---- load once ---------------------------------------------------------
    int32_t kind = 0;
    if constexpr (BOXES) kind = p.cs.kind[i];
    const Snap<T> self = p.snap_cur[i];
    const V3<T> x = {self.x, self.y, self.z};
    const T bi = self.r;
    const V3<T> sz = {p.cs.sx()[i], kind != 0 ? p.cs.sy()[i] : T(0), kind != 0 ? p.cs.sz()[i] : T(0)};
    Q4<T> qt = {T(1), T(0), T(0), T(0)};
    if (kind != 0) qt = {p.st.qw()[i], p.st.qx()[i], p.st.qy()[i], p.st.qz()[i]};
    T *poly = nullptr;
    if constexpr (BOXES) {
        __shared__ T s_poly[48 * STEP_BLOCK];    // box-box face clipping: 2 x 8 vertices x 3 per lane
        poly = s_poly + tid;
    }
    // the table's fill overflowed (the insert kernel ran before this one; no
    // lane of this kernel raises that bit): no body of the call has a list
    const bool no_table = (__hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ERR_BUCKET_OVERFLOW) != 0;

    // ---- the partners, ascending id, in the lane's column of s_id ------------
    int32_t cx, cy, cz;
    const bool in_grid = cell_of(x.x, x.y, x.z, p.grid.inv_cs, cx, cy, cz);
    if (!in_grid) atomicOr(p.err, ERR_DOMAIN);
    int32_t np_ = 0, hits = 0;
    if (in_grid && !no_table) {
        bool defer = false;
        // every body is in the table once and every bucket is visited once, so
        // the hits are distinct: more of them than the list holds is an overflow
        // (search_buckets raises ERR_PARTNER_OVERFLOW in sp.err itself)
        np_ = search_buckets<T, QUERY_MAXP, LAYOUT_ANY>(p, i, x, s_id, tid, *p.cur.gen, [&](uint32_t tj, const Snap<T> &s) {
            const bool h = candidate_hit<T, BOXES>(p, i, kind, x, sz.x, bi, tj, s, defer);
            hits += h ? 1 : 0;
            return h;
        });
    }
    const bool listed = in_grid && !no_table && hits <= QUERY_MAXP;

    const int32_t R = q.R;
    const int64_t slot0 = k * (int64_t)R;
    int32_t n = 0;
    auto emit = [&](int32_t partner, int32_t ck, const Contact<T> &con) {
        if (n < R) put_record(q, slot0 + n, partner, ck, con.dist, con.pos, con.frame);
        ++n;
    };

    if (listed) {
        M3<T> Mi;
        if (kind != 0) Mi = mj_body_mat(qt);
        contacts_planes<T>(p.n_planes, [&](int a, V3<T> &pn, V3<T> &pp) {
            pn = {p.pn[a][0], p.pn[a][1], p.pn[a][2]};
            pp = {p.pp[a][0], p.pp[a][1], p.pp[a][2]};
        }, kind, x, sz, Mi, emit);
        for (int u = 0; u < np_; ++u) {
            const int32_t j = s_id[u * STEP_BLOCK + tid];
            int32_t kj = 0;
            if constexpr (BOXES) kj = p.cs.kind[j];
            contacts_pair<T, BOXES>(
                i, j, kind, kj, x, sz, bi, Mi, p.snap_cur[j],
                [&] { return V3<T>{p.cs.sx()[j], p.cs.sy()[j], p.cs.sz()[j]}; },
                [&] { return Q4<T>{p.st.qw()[j], p.st.qx()[j], p.st.qy()[j], p.st.qz()[j]}; }, poly, STEP_BLOCK, emit);
        }
    }

    // ---- the count, and the fill of the unused slots ------------------------------
    q.counts[k] = listed ? n : QUERY_NO_LIST;
    fill_records<T>(q, slot0, listed ? n : 0, R);
}

template <typename T>
__global__ __launch_bounds__(STEP_BLOCK) void world_contacts_kernel(WorldContactQuery<T> q) {
    world_contacts_body<T, false>(q);
}

template <typename T>
__global__ __launch_bounds__(STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
void world_contacts_boxes_kernel(WorldContactQuery<T> q) {
    world_contacts_body<T, true>(q);
}

}  // namespace

template <typename T> hipError_t launch_world_contacts(const WorldContactQuery<T> &q, bool boxes, hipStream_t s) {
    if (q.count <= 0) return hipSuccess;
    const StepParams<T> &p = q.sp;
    if (q.first < 0 || q.first + q.count > p.n_global || p.n_global > INT32_MAX || q.R < 0 || !q.counts)
        return hipErrorInvalidValue;
    if (q.R > 0 && (!q.partner || !q.kind || !q.dist)) return hipErrorInvalidValue;
    if (!p.snap_cur || !p.st.base || !p.cs.base || !p.cur.line || !p.cur.gen || !p.err || p.next.line) return hipErrorInvalidValue;
    if (p.n_planes < 0 || p.n_planes > MAX_PLANES || p.grid.H <= 0 || (boxes && !p.cs.kind)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((q.count + STEP_BLOCK - 1) / STEP_BLOCK);
    if (boxes) hipLaunchKernelGGL((world_contacts_boxes_kernel<T>), dim3(blocks), dim3(STEP_BLOCK), 0, s, q);
    else hipLaunchKernelGGL((world_contacts_kernel<T>), dim3(blocks), dim3(STEP_BLOCK), 0, s, q);
    return hipGetLastError();
}

template hipError_t launch_world_contacts<double>(const WorldContactQuery<double> &, bool, hipStream_t);
template hipError_t launch_world_contacts<float>(const WorldContactQuery<float> &, bool, hipStream_t);

}  // namespace rb
