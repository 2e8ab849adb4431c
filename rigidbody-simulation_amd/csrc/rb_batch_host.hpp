// rb_batch_host.hpp — what the host units of the batched worlds share
// (rb_api_batch.hip, rb_api_batch_dev.hip, rb_api_batch_query.hip): the batch
// and the functions that cross those units.  Not part of the public interface.
#pragma once
#include "rb_batch_ragged.hpp"
#include "rb_batch_sensed.hpp"
#include "rb_host.hpp"
#include "rb_sampleplan.hpp"

struct rb_batch {
    int dtype = RB_F64, esz = 8, device = 0;
    hipStream_t stream = nullptr;      // where the batch's work is enqueued: own_stream, or the caller's
    hipStream_t own_stream = nullptr;  // created with the batch, destroyed with it
    int64_t E = 0, N = 0;              // environments, body slots (E * M)
    int32_t M = 0, n_planes = 0, oriented = 1;
    bool box = false;                  // the template is one box
    bool mixed = false;                // a box among several bodies (rb_batch_create_mixed): batch_mixed_kernel
    bool wide = false;                 // more than 64 bodies (rb_batch_create_wide): the kernels of rb_batch_wide.hip
    int32_t *d_kind = nullptr;         // [M] the template's kinds on the device (mixed)
    std::vector<int32_t> kind;         // [M] the template's kinds
    double planes[RB_MAX_PLANES][6] = {};
    double g[3] = {};
    double inv_cs = 1.0;
    void *snap = nullptr, *state = nullptr, *consts = nullptr;
    void *env_e = nullptr, *env_mu = nullptr;   // [E] reals; used while have_*
    bool have_e = false, have_mu = false;
    // per-environment planes [n_planes][6][E], gravity [3][E] and applied
    // forces [6][E * M] (reals; allocated by the first call that sets them,
    // used while have_*): any of them selects the ENVS step instances
    void *env_planes = nullptr, *env_g = nullptr, *env_xfrc = nullptr;
    bool have_planes = false, have_g = false, have_xfrc = false;
    int32_t *code = nullptr, *count = nullptr;
    int64_t *steps_done = nullptr;
    // grow-only device buffers (rb::host::grow), each with its capacity in
    // bytes: the staging of the AoS rows, the copy of an env_ids list
    double *io_q = nullptr, *io_v = nullptr;
    size_t io_q_bytes = 0, io_v_bytes = 0;
    int64_t *ids = nullptr;
    size_t ids_bytes = 0;
    // contact law (rb_batch_set_contact_law)
    int32_t law = RB_LAW_MUJOCO;
    double tol = 0.01;
    double rmax = 0.0;                          // largest bounding radius
    // sampled runs (rb_batch_run_sampled): one allocation, first the sample
    // slots the recording kernels fill (the batch's real type), then the
    // boundary rows of as many samples (double), allocated on first use
    char *samp = nullptr;
    size_t samp_bytes = 0;                      // allocated
    size_t samp_limit = (size_t)256 << 20;      // RBHIP_BATCH_SAMPLE_BYTES
    // rb_batch_set_xfrc_dev: the smallest body slot an upload was refused for
    // (DEV_NO_SLOT: none), sticky until rb_batch_sync reports and clears it
    uint32_t *refused = nullptr;
    // the host forms of the queries: device staging of the answers for a range
    // of listed environments (allocated on first use, at most samp_limit bytes)
    char *con = nullptr;
    size_t con_bytes = 0;
    // rb_batch_run_sampled_impulses: the running window's partial sums, [6][E * M]
    // reals, zeroed at the start of a call and carried from launch to launch
    void *sense = nullptr;
    size_t sense_bytes = 0;
    // the sizes last given (rb_batch_create, rb_batch_set_bodies): [E * M * 3];
    // a change of population derives the bounding radii from them again
    std::vector<double> size;
    // the population (rb_batch_set_population): while pop.set, the kernels of
    // rb_batch_ragged.hip step and query the batch.  A struct of its own: a
    // change of population commits, and rolls back, by one swap
    struct Pop {
        bool set = false;
        bool boxes = false;            // a present body of some environment is a box
        bool absent = false;           // some environment holds fewer than M bodies
        std::vector<int32_t> n, kind;  // [E], [E * M]
        int32_t *tables = nullptr;     // one allocation: n_bodies [E], kind [E * M], wave_env0 [waves + 1], lane_row [waves * 64]
        int32_t waves = 0, epw = 0;
    } pop;
};

namespace rb {
namespace host __attribute__((visibility("hidden"))) {

// ---- rb_api_batch.hip --------------------------------------------------------
int batch_check_step(const rb_batch *b, int64_t nsteps, double dt, double e, double mu, double thr);
// env_ids == NULL: all environments (n must be n_envs); else n ids in range
int batch_check_ids(const rb_batch *b, const int64_t *env_ids, int64_t n);
// an env_ids list onto the device (b->ids), enqueued
int batch_put_ids(rb_batch *b, const int64_t *env_ids, int64_t n);
// the environments failed so far, as rb_batch_step reports them (waits for the stream)
int batch_report(rb_batch *b, int64_t *n_failed);

// ---- rb_api_batch_dev.hip ----------------------------------------------------
// what the kernels of one launch read: k steps with these step parameters
template <typename T> BatchParams<T> batch_params(rb_batch *b, int32_t k, double dt, double e, double mu, double thr);
// the population's device tables
Population batch_population(const rb_batch *b);
// nsteps steps in launches of at most RB_BATCH_CHUNK steps
int batch_enqueue_steps(rb_batch *b, int64_t nsteps, double dt, double e, double mu, double thr);

// A sampled run before its first launch, host form (io_dtype NULL) or device form: the
// arguments' checks, the device and, if it records, the sample buffer of `fit` slots of per(b, rows) bytes.
struct SampledRun {
    int rows = 7;       // struct-of-arrays rows a sample holds: 13 with velocities
    int64_t fit = 1;    // samples the buffer holds
};
int batch_sampled_prelude(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu, double thr,
                          const void *qpos, const void *qvel, const int32_t *io_dtype,
                          size_t (*per)(const rb_batch *, int rows), SampledRun &r);
// launch l of a sampled run's plan, recording into the r.fit slots at `slots`
int batch_enqueue_sampled(rb_batch *b, const SampleLaunch &l, char *slots, const SampledRun &r, int64_t every, double dt,
                          double e, double mu, double thr);

// The same two for a run that records impulse curves (rb_batch_run_sampled_impulses, _dev): net is the
// required array, qpos and qvel may each be NULL; r.rows: sensed_rows(qpos, qvel).  RB_EUNSUPPORTED under
// the two-ball law.  With samples to record the prelude also allocates the carry rows (b->sense); the
// caller zeroes them before the first launch.  Every launch of the plan runs the sensing kernel.
int batch_sensed_prelude(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu, double thr,
                         const void *qpos, const void *qvel, const void *net, const int32_t *io_dtype,
                         size_t (*per)(const rb_batch *, int rows), SampledRun &r);
int batch_enqueue_sensed(rb_batch *b, const SampleLaunch &l, char *slots, const SampledRun &r, const SensedRun &sr,
                         int64_t every, double dt, double e, double mu, double thr);
// the slot layout of such a run for this batch
SensedRun batch_sensed_run(const rb_batch *b, bool want_q, bool want_v);

int batch_check_io(int32_t io_dtype);

}  // namespace host
}  // namespace rb
