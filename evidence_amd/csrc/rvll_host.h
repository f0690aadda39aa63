// rvll_host.h — what the host-side translation units of librvll.so share: the handle behind the C-ABI's opaque
// pointer, the error macro, and the helpers of rvll_api.hip the other units call.  Internal; not part of the ABI.
//   rvll_api.hip        the ABI core: create / destroy, priors, launch geometry, resident batch calls, scalar-call server, curves,
//                       self tests
//   rvll_batch.hip      the host-buffer batch calls and their transports, streamed host batches, resident uploads and download
//   rvll_batch_route.h  which transport a host-buffer call takes and where its bytes lie: arithmetic without a HIP call
//   rvll_walk_host.hip  the sampler's proposal step: the device walk in its forms (rvll_slice_walk*)
//   rvll_walk_plan.h    the walk's switches, geometry, arena layout and row order: arithmetic without a HIP call
//   rvll_live_host.hip  the resident live set and ensemble (rvll_live_*, rvll_live_runs_*): the stages of a resident step
//   rvll_step_groups.h  the walker groups of a resident ensemble step: index arithmetic without a HIP call
//   rvll_comm.hip       multi-GPU: RCCL communicators, lanes, all-gathers
//   rvll_cluster_host.hip  MLFriends clustering of many row sets (rvll_cluster_runs)
//   rvll_region.hip     MLFriends region sampling (rvll_region_draw_runs): kernels and host side
//   rvll_celerite.hip   log-L under correlated noise (rvll_celerite_loglike_batch): kernel and host side
//   rvll_celerite_predict.hip  GP prediction under correlated noise (rvll_celerite_predict_batch): kernels and host side
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

// the C-ABI entry points are the only exported symbols (built with -fvisibility=hidden)
#pragma GCC visibility push(default)
#include "rvll.h"
#pragma GCC visibility pop
#include "rvll_kernels.h"
#include "rvll_copypool.h"
#include "rvll_batch_route.h"   // kPinBytes, kSplit*, kStream*, kDownloadStagedMin

namespace rvll {
// sets the thread's last-error string (rvll_last_error) and returns `code`
int report_error(int code, const char* fmt, ...);
}  // namespace rvll

#define HIP_TRY(expr)                                                               \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess)                                                       \
            return ::rvll::report_error(e_ == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),      \
                        __FILE__, __LINE__);                                        \
    } while (0)

// a host-unit call that has reported its own error: pass its code on
#define RVLL_TRY(expr)                                                              \
    do {                                                                            \
        const int rc_ = (expr);                                                     \
        if (rc_) return rc_;                                                        \
    } while (0)

namespace rvll {
namespace host {
template <typename T>
void dev_free(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }
}  // namespace host
}  // namespace rvll

constexpr int kMaxLanes = 4;
constexpr int kWalkWords = 14;                // counters of the walk kernel: calls, tile slots, 4 phase bins + workgroups + longest life + 4 tile phases (diagnostic build), the queue
constexpr long long kFusedMaxPoints = 4096;   // rvll_prior_loglike_batch: one launch up to here, two beyond

using rvll::CopyPool;
constexpr int kStageSlots = 4;              // pinned staging blocks each way of a streamed host batch (stream_host_batch)

struct rvll_handle {
    int device = 0;
    hipStream_t compute = nullptr;          // lane 0: every single-GPU call runs here
    hipStream_t lanes[kMaxLanes] = {};      // lanes[0] == compute; further pipeline lanes of the multi-GPU step (rvll_allgather_logl)
    int      nlanes_dev = 2;                // lanes rvll_dev_flip_lane cycles through

    // layout (host mirror, then device copies)
    rvll_layout L{};
    std::vector<rvll_planet> planets;
    std::vector<rvll_inst>   insts;
    std::vector<rvll_slot>   linslots;
    rvll_planet* d_planets = nullptr;
    rvll_inst*   d_insts = nullptr;
    rvll_slot*   d_linslots = nullptr;
    double*      d_layblob = nullptr;       // planets, insts, linslots, drift[4], tref back to back: staged into LDS by the kernels
    int          form_override = 0;         // RVLL_FORM: 1 = tile kernel only, 2 = CU-wide kernel wherever it fits

    // resident epoch table
    int Ne = 0;
    double*  d_t = nullptr;
    double*  d_y = nullptr;
    double*  d_s2 = nullptr;
    int32_t* d_inst = nullptr;
    double*  d_linpar = nullptr;
    double   cte = 0.;
    double   tmin = 0., tmax = 0.;              // range of the epoch times

    // priors
    bool have_priors = false;
    rvll_prior* d_priors = nullptr;
    int32_t* d_heavy = nullptr;
    int n_heavy = 0;
    std::vector<double*> d_tables;
    std::vector<double> table_err;              // measured quintic-interpolant error per parameter (NaN: no table)
    std::vector<int> table_direct;              // per parameter: evaluated by verified interpolation alone
    bool priors_rowwise = false;                // some prior reads other coordinates of its row (the sorted kinds)
    bool all_direct = true;                     // every Beta / Gamma prior has a verified table: the slim prior stage applies
    double slim_umax = 0.;                      // |logit q| range the slim stage takes (rvll_set_slim_table_range; default: the table's)
    int* pin_defer = nullptr;                   // mapped pinned word the slim stage sets when it defers an element
    int* pin_defer_dev = nullptr;
    long long fused_pending = 0;                // rows of a one-launch cube -> log-L batch whose defer word has not been looked at yet

    // batch buffers
    long long cap = 0;
    double*  d_theta = nullptr;
    double*  d_cube = nullptr;
    double*  d_logL2[kMaxLanes] = {};           // one log-L buffer per pipeline lane
    int      logl_cur = 0;                      // lane the next device-resident launch uses
    int      logl_last = 0;                     // lane the last launch used (download source)
    bool     theta_async = false;               // theta was (re)written asynchronously on lane 0's stream
    bool     pipelined = false;                 // launches alternate lanes: two are in flight, no kernel-end tail
    int32_t* d_flags2[kMaxLanes] = {};          // per lane, like log-L

    // pinned host staging for small transfers (scalar / small-batch callbacks)
    static constexpr size_t kPinBytes = ::kPinBytes;
    void* pin_in = nullptr;
    void* pin_out = nullptr;
    void* pin_in_dev = nullptr;      // device-visible aliases of the two pinned buffers (zero-copy path)
    void* pin_out_dev = nullptr;

    // large host batches (stream_host_batch): worker threads for the host's copies, pinned staging blocks, one event per block
    CopyPool* pool = nullptr;
    void* stage_in[kStageSlots] = {};
    void* stage_out[kStageSlots] = {};
    size_t stage_in_bytes = 0, stage_out_bytes = 0;
    hipEvent_t stage_ev[kStageSlots] = {};      // a chunk's results are in its pinned block
    hipEvent_t stage_up[kStageSlots] = {}, stage_done[kStageSlots] = {};   // ... its rows are on the device / its kernels have run
    hipStream_t stream_up = nullptr, stream_down = nullptr;                // the two copy directions, beside lane 0's kernels (stream_reserve)

    // scalar-call server (rvll_scalar_server): persistent one-workgroup kernel + host-coherent control block
    rvll::ServerCtl* srv = nullptr;             // pinned, mapped, coherent
    rvll::ServerCtl* srv_dev = nullptr;         // its device address
    hipStream_t srv_stream = nullptr;
    bool srv_enabled = false, srv_running = false, srv_dead = false;
    unsigned long long srv_seq = 0;             // request numbers (low 32 bits travel)
    unsigned long long srv_last = 0;            // the last request word that was answered
    double*  d_srv_out = nullptr;               // device-local {logL, flags} the server's tile writes
    unsigned long long srv_idle_ticks = 500000; // 5 ms of the 100 MHz constant clock

    // device-resident slice-sampling walk (rvll_slice_walk)
    long long walk_cap = 0;                     // rows
    double *d_walk_u = nullptr, *d_walk_theta = nullptr, *d_walk_logl = nullptr, *d_walk_chol = nullptr;
    int32_t* d_walk_wrapped = nullptr;
    unsigned long long* d_walk_ncalls = nullptr;
    int32_t *d_walk_steps = nullptr, *d_walk_wid = nullptr, *d_walk_start = nullptr;   // [walk_cap] each
    int32_t *d_walk_cost = nullptr, *d_walk_order = nullptr;                            // [walk_cap] each (two-part walks)
    int32_t* d_walk_wflag = nullptr;            // [walk_cap] 1: the walker's last accepted candidate had a wandering solve (redo_wandering puts its log-L right)
    // run mode of the walk (rvll_slice_walk_runs): per row its run (its index inside the run goes in d_walk_wid), per run
    // lstar, seed and whitening factor
    long long runs_rows_cap = 0, runs_cap = 0;
    int32_t* d_walk_run = nullptr;              // [runs_rows_cap]
    double* d_run_lstar = nullptr;              // [runs_cap]
    unsigned long long* d_run_seed = nullptr;   // [runs_cap]
    double* d_run_chol = nullptr;               // [runs_cap, ndim, ndim]
    int32_t* d_run_nsteps = nullptr;            // [runs_cap] per-run step counts (rvll_slice_walk_runs_steps)
    int wander_exact = 1;                       // wandering solves are redone with correctly rounded sin / cos (rvll_set_wander_exact; RVLL_WANDER_EXACT)
    int walk_spec = 4;                          // candidates a walker may evaluate ahead per iteration (rvll_set_walk_speculation)
    int walk_prop = 0;                          // the walk's proposal (rvll_set_walk_proposal): RVLL_PROPOSAL_CHORD / _STEPOUT ...
    double walk_width = 1.;                     // ... and the stepout bracket's width
    double* d_walk_basis = nullptr;             // stepout: [slots, ndim, ndim] the basis of every walker slot (basis_for)
    size_t walk_basis_cap = 0;                  // ... in doubles
    // the walk as rounds of launches (rvll_rounds.hip; walk_rounds in rvll_walk_host.hip): one arena with every group's walker
    // state, candidate slots and counters (rounds_arena, rvll_walk_plan.h); a progress word per group in mapped pinned memory
    int walk_spec_rounds = 8;                   // ... and per round of the rounds form, while a round is below the latency floor
    void* d_rounds = nullptr;
    double* d_walk_dirs = nullptr;              // [K, nsteps, D] the directions of all moves of the walk in progress
    size_t walk_dirs_cap = 0;                   // in doubles
    size_t rounds_bytes = 0;
    unsigned long long* pin_rounds = nullptr;   // [kMaxLanes]
    unsigned long long* pin_rounds_dev = nullptr;
    hipEvent_t ev_rounds = nullptr;             // orders the groups' streams behind lane 0
    hipEvent_t ev_chain[kMaxLanes] = {};        // group g's step of a round has been issued to the device (the next group's step waits for it)
    hipStream_t rounds_streams[kMaxLanes] = {}; // the groups' streams, at DIFFERENT priorities (rounds_streams)
    int walk_rounds_used = 0;                   // rounds the last walk took (0: it ran in one of the single-kernel forms)
    long long walk_evaluated = 0;               // tile slots the last rvll_slice_walk evaluated (>= its ncalls)
    unsigned long long walk_phase[6] = {};      // diagnostic build (make walktrace): 100 MHz ticks per phase, summed over workgroups; workgroups

    // device-resident live set (rvll_live_*): nested sampling's live points, and the points that died, stay in HBM
    long long live_n = 0, live_cap = 0;
    double *d_live_u = nullptr, *d_live_theta = nullptr, *d_live_logl = nullptr;
    double* d_live_birth = nullptr;             // [live_cap] every live row's birth contour: -inf from the load, else the lstar it was drawn above
    int32_t* d_live_idx = nullptr;              // [2 * live_cap] order, then start rows, of the current step
    double *d_live_mom = nullptr;               // scratch, mean, covariance of the whitening
    // the order on the device (rvll_live_sort): keys in / out, rows in (the order itself lands in d_live_idx), rocPRIM's scratch
    unsigned long long* d_sort_keys = nullptr;  // [2 * live_cap]
    int32_t* d_sort_rows = nullptr;             // [live_cap]
    void* d_sort_temp = nullptr;
    size_t sort_temp_bytes = 0;
    long long sorted_kdead = -1;                // kdead of the rvll_live_sort whose order d_live_idx holds (-1: none, or used up)
    double sorted_lstar = 0.;
    long long dead_n = 0, dead_cap = 0;
    double *d_dead_theta = nullptr, *d_dead_logl = nullptr, *d_dead_birth = nullptr;   // [dead_cap, ndim], [dead_cap] x 2
    // the resident ensemble (rvll_live_runs_*): R live sets of n rows in d_live_u / _theta / _logl (run r = rows r n .. r n + n - 1;
    // live_n is 0 meanwhile, so the one-run calls refuse them, and rvll_live_init sets runs_R to 0); the dead store holds the dying
    // rows of every step in one block of A kdead rows, run a's kdead at a kdead, and runs_dead[r] lists run r's pieces in death order
    long long runs_R = 0, runs_n = 0;
    int32_t* d_runs_idx = nullptr;              // [runs_idx_cap]: order [R n] | ranks, dying rows, start rows [R n each] | runs, segments [2 R + 1]
    long long runs_idx_cap = 0;                 // in ints
    double* d_runs_mom = nullptr;               // [R] x (moments scratch | mean [D] | covariance [D, D])
    long long runs_mom_cap = 0;                 // in runs
    std::vector<int32_t> runs_sorted;           // the runs of the rvll_live_runs_sort whose order d_runs_idx holds (empty: none, or used up)
    long long runs_sorted_kdead = -1;
    std::vector<double> runs_sorted_lstar;
    std::vector<std::vector<std::pair<long long, long long>>> runs_dead;   // [R] (first row in the store, rows)

    // clustering (rvll_cluster_runs): grow-only device blocks for the packed inputs, the forest and per-run maxima, the packed outputs
    void* d_cl_in = nullptr;
    void* d_cl_work = nullptr;
    void* d_cl_out = nullptr;
    size_t cl_in_cap = 0, cl_work_cap = 0, cl_out_cap = 0;   // bytes
    // the step-count adaptation's distances (rvll_walk_distances_runs): one grow-only block of inputs, tiles, partials, outputs
    void* d_adapt = nullptr;
    size_t adapt_cap = 0;                                     // bytes
    void* d_adapt_in = nullptr;                               // rvll_walk_distances_runs' inputs; the resident step's walker start rows
    size_t adapt_in_cap = 0;                                  // bytes
    // region sampling (rvll_region_draw_runs): one grow-only block of inputs, per-candidate work, per-run state, outputs, trace
    void* d_region = nullptr;
    size_t region_cap = 0;                                    // bytes
    // correlated noise (rvll_celerite_loglike_batch, rvll_celerite_predict_batch): one grow-only block of the epoch tables in time order and a chunk's
    // residuals, variances and results; the host's copy of the epoch times (fetched at the first call)
    void* d_cel = nullptr;
    size_t cel_cap = 0;                                       // bytes
    std::vector<double> cel_times;
    // the clustered step of the resident ensemble (rvll_live_runs_step_clustered): grow-only block of the per-(run, cluster) segments
    // — (offset, rows) [S][2], fold scales [S][2], mean [S][D], covariance [S][D, D] — and what the last clustered step found, for
    // rvll_live_runs_clusters: per listed run the survivors' labels in rank order [A m], the metric scale [A D], the cluster count,
    // the factors the walk used (one per cluster, or the run's own when it has one cluster), and the seconds between its syncs
    void* d_clseg = nullptr;
    size_t clseg_cap = 0;                       // bytes
    int32_t cl_A = 0;                           // listed runs of the last clustered step (0: none since the ensemble was loaded)
    long long cl_m = 0;                         // survivors per run
    std::vector<int32_t> cl_labels, cl_ncl;
    std::vector<double> cl_scale;
    std::vector<std::vector<double>> cl_factors;
    double cl_phase_s[3] = {0., 0., 0.};        // clustering + label sort, per-cluster moments, walk

    hipEvent_t marks[2] = {nullptr, nullptr};   // rvll_dev_mark: HIP events on lane 0's stream

    // geometry
    int pb_override = 0;
    std::unordered_map<long long, int> geo;     // batch size -> points per workgroup chosen for it
    std::unordered_map<size_t, int> occ_by_lds; // dynamic LDS bytes -> resident workgroups per CU
    int chunk_items = rvll::kTileWindow;
    int n_cu = 256;

    // multi-GPU
    void* nccl_comm[kMaxLanes] = {};            // one communicator per lane (all but the first by ncclCommSplit)
    int nranks = 1, rank = 0;
    int nlanes = 1;
    long long gather_cap = 0;
    double* d_gather2[kMaxLanes] = {};
    double *d_gather_host_in = nullptr, *d_gather_host_out = nullptr;   // rvll_allgather_host: grow-only staging
    long long gather_host_cap = 0;              // in doubles
    double* d_gather_theta = nullptr;           // [nranks * B_local, D] (rvll_allgather_theta)
    long long gather_theta_cap = 0;             // in rows
    int gather_last = 0;
};

namespace rvll {
namespace host {
// A grow-only device buffer: *p holds *cap elements (of a void buffer: bytes); fewer than `need` of them: lane 0 is waited for (what
// it has queued may use the old buffer), the buffer freed and one of `room` elements (0: need) allocated.  *cap is 0 in between,
// so that a failed allocation leaves an empty buffer behind, not a stale capacity.
template <typename T, typename N>
int grow(rvll_handle* h, T** p, N* cap, size_t need, size_t room = 0)
{
    if (need <= (size_t)*cap) return RVLL_OK;
    HIP_TRY(hipStreamSynchronize(h->compute));
    dev_free(*p);
    *cap = 0;
    room = room ? room : need;
    HIP_TRY(hipMalloc(p, room * sizeof(std::conditional_t<std::is_void<T>::value, char, T>)));
    *cap = (N)room;
    return RVLL_OK;
}
// ... one of several buffers that share a capacity (zeroed by the caller meanwhile): anew, n elements
template <typename T>
int renew(rvll_handle* h, T** p, size_t n)
{
    size_t none = 0;
    return grow(h, p, &none, n);
}
}  // namespace host

// rvll_gls.hip: res = datum - model and var = svrad^2 (+ jitter^2) of every (row, epoch) of a.theta, the planets of include_mask
// subtracted (rvll_residuals_batch's values); asynchronous on `stream`
struct DriftSlots { rvll_slot s[5]; };                    // lin, quad, cub, quar, tref
hipError_t launch_residuals(const LoglikeArgs& a, const DriftSlots& ds, unsigned include_mask, double* res, double* var,
                            hipStream_t stream);
DriftSlots drift_slots(const rvll_handle* h);

// rvll_celerite.hip, shared with rvll_celerite_predict.hip: the checks and the plan of the noise terms, the epoch tables in time
// order, the grow-only block h->d_cel, and the factor sweep (with ws: the sweep that also stores what the prediction needs)
struct CelPlan;
constexpr int kCelRows = 64;                              // rows a workgroup: one wave
constexpr long long kCelChunkBytes = 256ll << 20;         // what a chunk of rows may take on the device
size_t cel_up8(size_t n);
int cel_make_plan(rvll_handle* h, const rvll_noise_term* terms, int32_t n_terms, CelPlan& plan, int& J);
int cel_time_tables(rvll_handle* h, const int32_t* order, std::vector<int32_t>& ord, std::vector<double>& tab);
int cel_reserve(rvll_handle* h, size_t total);
hipError_t launch_celerite_factor(int J, const double* theta, int D, long long R, const double* res, const double* var, int Ne,
                                  const int32_t* ord, const double* ts, const double* dts, const CelPlan& plan, double cte,
                                  double* logl, int32_t* flags, double* ws, long long rp, hipStream_t stream);
}  // namespace rvll

namespace rvll {
namespace host {

// helpers of rvll_api.hip the other host units use
int use_device(rvll_handle* h);                     // select the device, stop a running scalar-call server, settle a pending one-launch batch
int sync_other_lanes(rvll_handle* h);
int build_args(rvll_handle* h, const double* d_theta, double* d_logL, int32_t* d_flags, long long B, rvll::LoglikeArgs* out,
               int* cu_grid = nullptr);
void make_fused(const rvll_handle* h, const double* d_cube, double* d_theta_out, rvll::LoglikeArgs* a);
hipError_t launch_form(const rvll::LoglikeArgs& a, int cu_grid, hipStream_t stream);   // the tile form, or the CU-wide form on cu_grid > 0 workgroups
// one request through the scalar-call server (started on demand): op is a kServer* request of rvll_kernels.h
int scalar_call(rvll_handle* h, unsigned op, const double* theta, double* logL, int32_t* flags, double* theta_out);
// a batch size of the device-resident forms: least .. reserved capacity
inline int check_capacity(const rvll_handle* h, long long B, long long least = 0)
{
    if (B >= least && B <= h->cap) return RVLL_OK;
    return report_error(RVLL_E_INVALID, "B %lld outside reserved capacity %lld", B, h->cap);
}
// rvll_batch.hip
int download_rows(rvll_handle* h, void* dst, const void* src_dev, size_t bytes);   // a large device array into pageable host memory
void stream_free(rvll_handle* h);                   // the copy workers, staging blocks, events and streams of the streamed transports
void comm_release(rvll_handle* h);                  // rvll_comm.hip: destroy the handle's communicators
// rvll_cluster_host.hip: the clustering's device blocks (d_cl_in: cube, scale, run_start, seeds, block table; d_cl_work: forest,
// per-run maxima; d_cl_out: radius2, nclusters, labels) and its core on inputs already there (asynchronous)
struct ClusterLayout {
    size_t o_cube, o_scale, o_start, o_seed, o_blk, in_bytes;
    size_t w_slots, work_bytes;
    size_t p_ncl, p_lab, out_bytes;
    long long N, R, nblocks;
};
std::vector<int32_t> cluster_blocks(const int64_t* run_start, int64_t R);   // (run, first row) of every 64 rows of one run
ClusterLayout cluster_layout(int64_t N, int64_t R, int D, size_t block_ints);
int cluster_reserve(rvll_handle* h, const ClusterLayout& L, const char* who);
rvll::ClusterArgs cluster_args(rvll_handle* h, const ClusterLayout& L, int D, int nboot, const int32_t* wrapped);
int cluster_core(rvll_handle* h, const rvll::ClusterArgs& a);
// rvll_adapt.hip: the step-count adaptation's distances on device pointers.  Group g's members are rows (d_idx ? d_idx[gofs[g] + i]
// : gofs[g] + i) of d_rows, i < gcnt[g]; its factor is d_factors[g]; walker k went from d_starts[k] to d_ends[k] in group
// d_walker_group[k].  Leaves pair [G] and move [K] in *d_pair / *d_move (h->d_adapt) behind the launches on the compute stream;
// `tables` (and gofs, gcnt) must live until the stream has passed them.  adapt_in_reserve: the grow-only block d_adapt_in.
int walk_distances_core(rvll_handle* h, const double* d_rows, const int32_t* d_idx, const std::vector<int64_t>& gofs,
                        const std::vector<int64_t>& gcnt, const double* d_factors, unsigned long long wmask, const double* d_starts,
                        const double* d_ends, const int32_t* d_walker_group, int64_t K, double** d_pair, double** d_move,
                        std::vector<int32_t>& tables);
int adapt_in_reserve(rvll_handle* h, size_t bytes);
inline unsigned long long wrapped_mask(const int32_t* wrapped, int D)
{
    unsigned long long m = 0;
    if (wrapped) for (int d = 0; d < D && d < 64; ++d) if (wrapped[d]) m |= 1ull << d;
    return m;
}
constexpr size_t kDeadStagedMin = 8u << 20;

// rvll_walk_host.hip: what the resident live set (rvll_live_host.hip) needs of the walk
// Run mode of a walk (rvll_slice_walk_runs): the walkers of several independent runs in one walk.  Every row's run is in
// d_walk_run and its index inside the run in d_walk_wid (the random-number counter index the one-run walk of that run gives
// it); per run lstar, seed and whitening factor are in d_run_lstar / d_run_seed / d_run_chol.  Every launch of the walk counts
// the calls of each row in d_walk_cost (the single-kernel forms' per-row cost, the rounds step's per-walker count), and the
// host adds them up per row: the calls of a run are then those its own walk would report, whichever forms the rows took.
// With a per-run step-count table (rvll_slice_walk_runs_steps; nsteps != null, d_run_nsteps uploaded) the nsteps of the walk
// is the largest count and a row stops after its run's own: the single-kernel forms read the table (WalkArgs::run_nsteps),
// the rounds form, whose direction table has nsteps rows per walker, is not taken.
struct RunWalk {
    const int32_t* run;                // [K] host copy of d_walk_run
    const int32_t* rid;                // [K] host copy of d_walk_wid
    std::vector<long long> row_calls;  // [K] out: likelihood calls every row consumed
    const int32_t* nsteps = nullptr;   // [R] or null: host copy of d_run_nsteps
};
int walk_reserve(rvll_handle* h, int64_t K);                 // device buffers of the walk for K rows (grown on demand)
int runs_reserve(rvll_handle* h, int64_t K, int64_t R);      // ... in run mode, and the tables of R runs
int walk_check_args(rvll_handle* h, int64_t K, int32_t nsteps, int32_t max_rounds, int64_t walker_base, const int32_t* wrapped);
int walk_upload_frame(rvll_handle* h, const double* chol, const int32_t* wrapped);   // chol may be null (run mode); synchronises
// the walk of the K rows in the walk's buffers (rw: run mode, else null); synchronises the compute stream
int walk_core(rvll_handle* h, int64_t K, double lstar, int32_t nsteps, int32_t max_rounds, uint64_t seed, int64_t walker_base,
              int64_t* ncalls, RunWalk* rw);
int steps_range(const char* who, const int32_t* nsteps, int32_t n, int32_t* most, bool* uniform);

}  // namespace host
}  // namespace rvll
