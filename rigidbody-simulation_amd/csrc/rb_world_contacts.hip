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
#include "rb_world_list.hpp"

namespace rb {
namespace {

// (the load, the search and the walk: rb_world_list.hpp, shared with the impulse query)
template <typename T, bool BOXES>
__device__ __forceinline__ void world_contacts_body(const WorldContactQuery<T> &q) {
    __shared__ int32_t s_id[QUERY_MAXP * STEP_BLOCK];

    const int tid = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * STEP_BLOCK + tid;
    if (k >= q.count) return;                    // (no barrier below: lanes past the range store nothing)
    const StepParams<T> &p = q.sp;
    const int32_t i = (int32_t)(q.first + k);
    T *poly = nullptr;
    if constexpr (BOXES) {
        __shared__ T s_poly[48 * STEP_BLOCK];    // box-box face clipping: 2 x 8 vertices x 3 per lane
        poly = s_poly + tid;
    }
    const WorldBody<T> b = world_list<T, BOXES>(p, i, false, s_id, tid);

    const int32_t R = q.R;
    const int64_t slot0 = k * (int64_t)R;
    int32_t n = 0;
    if (b.listed) {
        world_walk<T, BOXES>(p, i, b, s_id, tid, poly, [&](int32_t partner, int32_t ck, const Contact<T> &con, bool) {
            if (n < R) put_record(q, slot0 + n, partner, ck, con.dist, con.pos, con.frame);
            ++n;
        });
    }

    // ---- the count, and the fill of the unused slots ------------------------------
    q.counts[k] = b.listed ? n : QUERY_NO_LIST;
    fill_records<T>(q, slot0, b.listed ? n : 0, R);
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
