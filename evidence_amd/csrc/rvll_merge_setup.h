// What the merged-run entry points share (rvll_merge.hip, rvll_posterior.hip, rvll_fip_merged.hip, rvll_marginal.hip,
// rvll_draws.hip): the setup
// of a merge by birth contours (keys, two radix sorts, placement and the event stream), the replicate kernel, the argument checks
// and the driver of a call that reduces replicates of the merged run block by block.  rvll_merge_setup.hip defines them, once
// for the library; rvll_merge.hip's header comment describes the kernels; DESIGN §4j.  This header declares them and holds the
// small inline helpers that the reducers' own kernels use.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <functional>
#include <vector>
#include <cstring>

#pragma GCC visibility push(default)
#include "rvll.h"
#pragma GCC visibility pop
#include "rvll_keys.h"
#include "rvll_math.h"

namespace rvll {
int report_error(int code, const char* fmt, ...);

namespace merge {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kPer = 4;                                   // stream entries a lane holds per tile
constexpr long long kTile = (long long)kThreads * kPer;
constexpr int kMaxBlocks = 8192;
constexpr long long kMaxGroups = 1ll << 22;               // replicates per launch (grid x * 256 threads < 2^32)
constexpr long long kDefaultBlockBytes = 512ll << 20;     // rvll_merge_replicates: device bound on a block of weights
// The default block of weights of the reducers.  A block holds bound / (8 N) replicates and the replicate kernel runs one workgroup a
// replicate, so a small block leaves most of the device idle: at 2.6e6 rows, 512 MiB (24 replicates) took 2.8 s for the weights of
// 1000 replicates and 8 GiB 0.24 s (profiles/posterior_probe.txt).  Only min(nsamples, bound / (8 N)) replicates are allocated.
constexpr long long kDefaultWeightBytes = 8ll << 30;
constexpr unsigned long long kSeedMul = 0xD1B54A32D192ED03ull;   // replicate s has the seed seed + s * kSeedMul

typedef unsigned long long u64;

// a failed HIP call ends the entry point: RVLL_E_NOMEM or RVLL_E_HIP with the call's text
int report_hip(hipError_t e, const char* expr, const char* file, int line);

#define MRG_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return rvll::merge::report_hip(e_, #expr, __FILE__, __LINE__);            \
    } while (0)

#define MRG_OK(expr) do { const int rc_ = (expr); if (rc_ != RVLL_OK) return rc_; } while (0)

inline int blocks_for(long long total, int per_block)
{
    const long long b = (total + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > kMaxBlocks ? kMaxBlocks : b);
}

// inclusive 64-lane scan
template <typename T>
__device__ __forceinline__ T wave_scan(T v, int lane)
{
    for (int off = 1; off < kWave; off <<= 1) {
        const T o = __shfl_up(v, off, kWave);
        if (lane >= off) v += o;
    }
    return v;
}

// the sum of v over the wave, in every lane
__device__ __forceinline__ long long wave_sum(long long v)
{
    for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// the sum of v over the workgroup, in every thread: butterfly inside a wave, then the waves in order
__device__ inline double block_sum(double v, double* sh)
{
    for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double r = sh[0];
    for (int w = 1; w < kWaves; ++w) r += sh[w];
    __syncthreads();
    return r;
}

int check_common(const double* logl, const double* birth, int64_t n_rows, const int64_t* run_start, int32_t n_runs);
// what every replicate entry point asks of nsamples, mode, bootstrap and block_bytes
int check_replicate_args(int32_t nsamples, int32_t mode, int32_t bootstrap, int32_t n_runs, int64_t block_bytes);
int check_finite_values(const double* values, int64_t n_rows, int32_t n_cols);

// The fixed point of the weights of `reps` replicates of n slots each: every entry exp(logwt) becomes m = rint(p 2^62)
// as int64 in place (0 for a row without weight) and msum[replicate], zeroed by the caller, receives the integer sum of its m.
hipError_t launch_fixed(double* w, long long n, long long reps, unsigned long long* msum, hipStream_t stream);

struct Replicates;

// The device tables of one merge and the four launches that fill them (keys, two sorts, place).  After launch() the merged order
// (order), L, rho, nlive and the event stream ev are final; kl, kb, sl, sb, run, rb and temp are scratch a caller may reuse, and
// idx still holds 0 .. n - 1.  The tables belong to the call (owner) and go with it.
struct MergeSetup {
    double *logl = nullptr, *birth = nullptr, *L = nullptr;
    u64 *kl = nullptr, *kb = nullptr, *sl = nullptr, *sb = nullptr;
    int32_t *idx = nullptr, *order = nullptr, *run = nullptr, *rb = nullptr, *rho = nullptr, *ev = nullptr;
    long long *rs = nullptr, *nlive = nullptr;
    char* temp = nullptr;
    size_t temp_bytes = 0;

    hipError_t query(long long n);
    hipError_t alloc(Replicates& owner, long long n, int n_runs);
    hipError_t upload(const double* h_logl, const double* h_birth, const int64_t* run_start, long long n, int n_runs,
                      hipStream_t stream);
    // four launches
    hipError_t launch(long long n, int n_runs, hipStream_t stream);
    // one launch sequence: the stable rocPRIM radix sort of n 64-bit keys carrying int32 values, in temp
    hipError_t sort(u64* keys_in, u64* keys_out, int32_t* vals_in, int32_t* vals_out, long long n, hipStream_t stream);
};

// One call that reduces replicates of a merged run: the device, the stream and the events, every device buffer, the setup, the
// blocks of replicates and their timing.  A caller (checks done) goes through plan_blocks, begin, its own alloc and uploads on
// `stream`, setup, free_now of what only the setup needed, run_blocks and finish, and returns at the first status that is not
// RVLL_OK: the destructor frees every buffer, destroys the stream and the events and restores the device.
struct Replicates {
    // a step of a block of sb replicates from s0 whose weights are in d_w; it queues on stream
    typedef std::function<hipError_t(long long s0, long long sb, double* d_w, hipStream_t stream)> Step;

    Replicates(int32_t device, const double* logl, const double* birth, long long n, const int64_t* run_start, int n_runs,
               int nsamples, int expected, int bootstrap, uint64_t seed);
    ~Replicates();
    Replicates(const Replicates&) = delete;

    // s_blk = min(nsamples, max_reps, (bound - tables) / per_rep) with bound = block_bytes or, when that is 0, default_bound.
    // RVLL_E_NOMEM when tables + per_rep is above the bound: "<tables_name> (.. bytes) and one replicate of <rep_name> (.. bytes)
    // are above ..", or without tables_name "one replicate of <rep_name> needs .. bytes, above ..".  weights = false: no block of
    // weights and no bound.
    int plan_blocks(int64_t block_bytes, long long default_bound, long long tables, long long per_rep, long long max_reps,
                    const char* tables_name, const char* rep_name, bool weights = true);
    int begin();
    // device memory that lives until the call ends, or until free_now
    template <class T>
    hipError_t alloc(T*& p, size_t count)
    {
        return alloc_bytes(reinterpret_cast<void**>(&p), sizeof(T) * count);
    }
    template <class T>
    hipError_t free_now(T*& p)
    {
        return free_bytes(reinterpret_cast<void**>(&p));
    }
    // event 0, the merge's launches, own(), event 1, synchronise: setup_ms
    int setup(const std::function<hipError_t()>& own);
    // per block: before (untimed), event 0, replicate_kernel, event 1, reduce, event 2, after (untimed: the block's downloads),
    // one synchronise: weights_ms and reduce_ms.  An empty step is skipped.
    int run_blocks(const Step& before, const Step& reduce, const Step& after);
    int finish(double* logz, double* info);
    double elapsed_ms() const;                            // since the constructor: total_ms
    // the fields that the timing structs with the three phases share; what else a struct has is its entry point's
    template <class T>
    void report(T* t) const
    {
        if (!t) return;
        t->kernel_ms = setup_ms + weights_ms + reduce_ms;
        t->total_ms = elapsed_ms();
        t->setup_ms = setup_ms;
        t->weights_ms = weights_ms;
        t->reduce_ms = reduce_ms;
        t->rows = n;
        t->elements = n * (long long)nsamples;
        t->launches = launches;
        t->blocks = blocks;
    }

    MergeSetup su;
    hipStream_t stream = nullptr;
    double *d_logz = nullptr, *d_info = nullptr, *d_w = nullptr;
    long long s_blk = 0;
    double setup_ms = 0., weights_ms = 0., reduce_ms = 0.;
    int launches = 0, blocks = 0;                         // the driver counts its own launches, the caller adds its own

private:
    hipError_t alloc_bytes(void** p, size_t bytes);
    hipError_t free_bytes(void** p);

    const int32_t device;
    const double *logl, *birth;
    const long long n;
    const int64_t* run_start;
    const int n_runs, nsamples, expected, bootstrap;
    const uint64_t seed;
    const std::chrono::steady_clock::time_point t_start;
    int prev_device = -1;
    bool weights = true;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    std::vector<void*> owned;
};

}  // namespace merge
}  // namespace rvll
