// MLFriends region sampling on gfx950 (rvll_region_draw_runs; include/rvll.h).  evidence_amd/region.py holds the
// numpy definition: candidate c of run r takes its random numbers from uniform01(seed_r, c << 8 | draw), so it is the same
// candidate whatever block, launch or call handles it.
//
// Device work per round (every run that is still short proposes `block` candidates, c0 .. c0 + block - 1):
//     propose   one 256-thread workgroup per (run, 256 candidates), one candidate per thread, its coordinates in registers (the
//               loops over dimensions unrolled to a compile-time bound on ndim): centre, offset (walk_normal, the walk's own
//               Box-Muller), folding, the OUTSIDE test.  The run's survivors pass through LDS in tiles of kRegionTileDoubles /
//               ndim rows (one tile when they fit); every thread counts the survivors within radius2 of its candidate
//               (clustering.pair_d2's operations, -ffp-contract=off: exact), an integer.  Thinning: kept iff U n < 1.  The
//               workgroup scans its kept flags: a rank per candidate, a count per workgroup.
//     offsets   one workgroup scans the workgroups' counts in order: where each workgroup's kept candidates start, and the total.
//     pack      the kept candidates' rows go to the batch cube buffer at offset + rank: candidate order inside a run, runs in
//               the order of the call.
//     log-L     the existing prior and log-L kernels on that buffer (rvll_dev_prior_loglike): the bits of rvll_prior_loglike_batch.
//     select    one workgroup per run scans accepted (log-L > lstar) and kept flags in candidate order: the first
//               (kdraw - found) accepted candidates are taken, ncalls counts the kept ones up to the last taken.
// Counts and ranks are integers and every scan has a fixed order: no atomics of any kind, and a run's results depend on its own
// rows, seed and contour alone.
#include "rvll_host.h"
#include "rvll_tile.h"

using rvll::report_error;
using namespace rvll::host;

namespace {

constexpr int kRegionThreads = 256;
constexpr int kRegionMaxDims = 64;
constexpr int kRegionTileDoubles = 5120;                 // 40 KiB of survivors in LDS at a time
constexpr int kFlagOutside = 1, kFlagLost = 2, kFlagKept = 4, kFlagAccepted = 8;
constexpr unsigned kDrawCentre = 128, kDrawRadius = 129, kDrawThin = 130;
constexpr size_t kRegionMaxBytes = (size_t)4 << 30;

struct RegionArgs {
    const double* surv;                // [N, D]
    const long long* run_start;        // [R + 1]
    const double* scale;               // [R, D]
    const double* radius2;             // [R]
    const double* lstar;               // [R]
    const unsigned long long* seeds;   // [R]
    const int32_t* act;                // [A] the runs of this round
    unsigned long long wmask;
    int D, block, chunks, kdraw;       // chunks: workgroups per run
    long long c0, cend, first;         // this round's first candidate; one past the last candidate of the call; the call's first
    // per slot s = a * block + i (candidate c0 + i of the a-th run of the round)
    double* cand;                      // [S, D]
    int32_t* flag;                     // [S]
    int32_t* count;                    // [S] neighbours
    int32_t* rank;                     // [S] rank among the workgroup's kept candidates, -1 when not kept
    int32_t* pos;                      // [S] row in the batch, -1 when not kept
    int32_t* wg_count;                 // [A * chunks]
    int32_t* wg_offset;                // [A * chunks + 1] (the last entry: the total)
    // the batch (the handle's buffers)
    double* batch_cube;
    const double* batch_theta;
    const double* batch_logl;
    // per run
    int32_t* nfound;                   // [R]
    long long* ncalls;                 // [R]
    double* out_cube;                  // [R, kdraw, D]
    double* out_theta;                 // [R, kdraw, D]
    double* out_logl;                  // [R, kdraw]
    long long trace_cap;               // candidates per run (0: no trace)
    double* trace_cube;                // [R, trace_cap, D]
    int32_t* trace_flags;              // [R, trace_cap]
    int32_t* trace_n;                  // [R, trace_cap]
    double* trace_logl;                // [R, trace_cap]
};

// inclusive scan of one int per thread over the workgroup, in thread order
__device__ __forceinline__ int block_scan_inclusive(int v, int* buf)
{
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int ofs = 1; ofs < kRegionThreads; ofs <<= 1) {
        const int add = tid >= ofs ? buf[tid - ofs] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    const int out = buf[tid];
    __syncthreads();
    return out;
}

template <int DM>
__global__ __launch_bounds__(kRegionThreads)
void region_propose_kernel(const RegionArgs p)
{
    __shared__ double tile[kRegionTileDoubles];
    __shared__ int scan[kRegionThreads];
    const int D = p.D, tid = threadIdx.x;
    const int a = blockIdx.x / p.chunks, q = blockIdx.x % p.chunks;
    const int r = p.act[a];
    const int local = q * kRegionThreads + tid;
    const long long c = p.c0 + local;
    const bool exists = local < p.block && c < p.cend;
    const long long s = (long long)a * p.block + local;
    const long long rs = p.run_start[r];
    const int m = (int)(p.run_start[r + 1] - rs);
    const double* u = p.surv + rs * D;
    const double* sc = p.scale + (long long)r * D;
    const unsigned long long seed = p.seeds[r];
    const double r2 = p.radius2[r];
    const unsigned long long base = (unsigned long long)c << 8;

    double x[DM];
    bool outside = false;
    if (exists) {
        const double fi = floor(rvll::uniform01(seed, base | kDrawCentre) * (double)m);
        const int i = (int)fmin(fi, (double)(m - 1));
        double norm2 = 0.0;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
            if (k < D) {
                x[k] = rvll::walk_normal(seed, base | (unsigned)(2 * k));
                norm2 = norm2 + x[k] * x[k];
            }
        }
        const double rho = pow(rvll::uniform01(seed, base | kDrawRadius), 1.0 / (double)D);
        const double f = sqrt(r2) * rho / sqrt(norm2);
        const long long tc = c - p.first;
        const bool traced = tc < p.trace_cap;
#pragma unroll
        for (int k = 0; k < DM; ++k) {
            if (k < D) {
                double v = u[(long long)i * D + k] + (f * x[k]) / sc[k];
                if ((p.wmask >> k) & 1ull) {
                    v = v - floor(v);
                    if (v >= 1.0) v = 0.0;
                } else if (!(v >= 0.0 && v < 1.0)) {
                    outside = true;
                }
                x[k] = v;
                p.cand[s * D + k] = v;
                if (traced) p.trace_cube[((long long)r * p.trace_cap + tc) * D + k] = v;
            }
        }
    }

    // the survivors within radius2 of the candidate, tile by tile
    const int tile_rows = kRegionTileDoubles / D;
    int n = 0;
    for (int t0 = 0; t0 < m; t0 += tile_rows) {
        const int rows = min(tile_rows, m - t0);
        __syncthreads();
        for (int e = tid; e < rows * D; e += kRegionThreads) tile[e] = u[(long long)t0 * D + e];
        __syncthreads();
        if (exists && !outside) {
            for (int j = 0; j < rows; ++j) {
                const double* uj = tile + j * D;
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < DM; ++k) {
                    if (k < D) {
                        double delta = x[k] - uj[k];
                        if ((p.wmask >> k) & 1ull) delta = delta - rint(delta);
                        const double t = delta * sc[k];
                        acc = acc + t * t;
                    }
                }
                n += acc <= r2 ? 1 : 0;
            }
        }
    }

    bool kept = false;
    int flag = 0;
    if (exists) {
        if (outside) flag = kFlagOutside;
        else if (n == 0) flag = kFlagLost;
        else kept = rvll::uniform01(seed, base | kDrawThin) * (double)n < 1.0;
    }
    const int incl = block_scan_inclusive(kept ? 1 : 0, scan);
    if (local < p.block) {
        p.flag[s] = flag;
        p.count[s] = n;
        p.rank[s] = kept ? incl - 1 : -1;
        if (exists) {
            const long long tc = c - p.first;
            if (tc < p.trace_cap) p.trace_n[(long long)r * p.trace_cap + tc] = n;
        }
    }
    if (tid == kRegionThreads - 1) p.wg_count[blockIdx.x] = incl;
}

// exclusive scan of the workgroups' counts in order; the total behind them
__global__ __launch_bounds__(kRegionThreads)
void region_offsets_kernel(const int32_t* wg_count, int32_t* wg_offset, int W)
{
    __shared__ int scan[kRegionThreads];
    int carry = 0;
    for (int w0 = 0; w0 < W; w0 += kRegionThreads) {
        const int w = w0 + threadIdx.x;
        const int v = w < W ? wg_count[w] : 0;
        const int incl = block_scan_inclusive(v, scan);
        if (w < W) wg_offset[w] = carry + incl - v;
        __shared__ int total;
        if (threadIdx.x == kRegionThreads - 1) total = incl;
        __syncthreads();
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) wg_offset[W] = carry;
}

__global__ __launch_bounds__(kRegionThreads)
void region_pack_kernel(const RegionArgs p)
{
    const int a = blockIdx.x / p.chunks, q = blockIdx.x % p.chunks;
    const int local = q * kRegionThreads + threadIdx.x;
    if (local >= p.block) return;
    const long long s = (long long)a * p.block + local;
    const int rk = p.rank[s];
    int at = -1;
    if (rk >= 0) {
        at = p.wg_offset[blockIdx.x] + rk;
        for (int k = 0; k < p.D; ++k) p.batch_cube[(long long)at * p.D + k] = p.cand[s * p.D + k];
    }
    p.pos[s] = at;
}

__global__ __launch_bounds__(kRegionThreads)
void region_select_kernel(const RegionArgs p)
{
    __shared__ int scan[kRegionThreads];
    __shared__ int tot, last_calls;
    const int D = p.D, tid = threadIdx.x;
    const int a = blockIdx.x;
    const int r = p.act[a];
    const double lstar = p.lstar[r];
    const int found0 = p.nfound[r];
    const int need = p.kdraw - found0;
    int carry_acc = 0, carry_kept = 0;
    if (tid == 0) last_calls = 0;
    __syncthreads();
    for (int i0 = 0; i0 < p.block; i0 += kRegionThreads) {
        const int local = i0 + tid;
        const long long s = (long long)a * p.block + local;
        const long long c = p.c0 + local;
        const bool exists = local < p.block && c < p.cend;
        const int at = exists ? p.pos[s] : -1;
        const bool kept = at >= 0;
        const double ll = kept ? p.batch_logl[at] : __builtin_nan("");
        const bool acc = kept && ll > lstar;
        // accepted flags in the high half, kept flags in the low half: both scans at once (each at most 256 a pass)
        const int incl = block_scan_inclusive((acc ? 1 << 16 : 0) | (kept ? 1 : 0), scan);
        const int acc_excl = carry_acc + (incl >> 16) - (acc ? 1 : 0);
        const int kept_incl = carry_kept + (incl & 0xffff);
        if (acc && acc_excl < need) {
            const long long o = (long long)r * p.kdraw + found0 + acc_excl;
            for (int k = 0; k < D; ++k) {
                p.out_cube[o * D + k] = p.cand[s * D + k];
                p.out_theta[o * D + k] = p.batch_theta[(long long)at * D + k];
            }
            p.out_logl[o] = ll;
            if (acc_excl == need - 1) last_calls = kept_incl;
        }
        if (exists) {
            const long long tc = c - p.first;
            if (tc < p.trace_cap) {
                p.trace_flags[(long long)r * p.trace_cap + tc] = p.flag[s] | (kept ? kFlagKept : 0) | (acc ? kFlagAccepted : 0);
                p.trace_logl[(long long)r * p.trace_cap + tc] = ll;
            }
        }
        if (tid == kRegionThreads - 1) tot = incl;
        __syncthreads();
        carry_acc += tot >> 16;
        carry_kept += tot & 0xffff;
        __syncthreads();
    }
    if (tid == 0) {
        if (carry_acc >= need) {
            p.nfound[r] = p.kdraw;
            p.ncalls[r] += last_calls;
        } else {
            p.nfound[r] = found0 + carry_acc;
            p.ncalls[r] += carry_kept;
        }
    }
}

template <int DM>
void launch_propose(const RegionArgs& p, int A, hipStream_t st)
{
    hipLaunchKernelGGL(region_propose_kernel<DM>, dim3((unsigned)(A * p.chunks)), dim3(kRegionThreads), 0, st, p);
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int rvll_region_tile_rows(int32_t ndim, int32_t* rows)
{
    if (!rows || ndim < 1 || ndim > kRegionMaxDims) return report_error(RVLL_E_INVALID, "rvll_region_tile_rows: bad arguments");
    *rows = kRegionTileDoubles / ndim;
    return RVLL_OK;
}

int rvll_region_draw_runs(rvll_handle* h, const double* survivors, const int64_t* run_start, int64_t R, const double* scale,
                          const double* radius2, const double* lstar, const uint64_t* seeds, const int32_t* wrapped,
                          int32_t kdraw, int64_t first, int64_t max_candidates, int32_t block, double* cube_out,
                          double* theta_out, double* logl_out, int32_t* nfound, int64_t* ncalls, int64_t trace_cap,
                          double* trace_cube, int32_t* trace_flags, int32_t* trace_n, double* trace_logl, int64_t* trace_count,
                          int32_t* rounds)
{
    if (!h) return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: null handle");
    int rc = use_device(h);
    if (rc) return rc;
    if (!h->have_priors) return report_error(RVLL_E_NOPRIORS, "rvll_region_draw_runs: rvll_set_priors has not been called");
    if (R < 0 || !run_start) return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: bad run table");
    if (run_start[0] != 0) return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: run_start[0] must be 0");
    for (int64_t r = 0; r < R; ++r)
        if (run_start[r + 1] < run_start[r])
            return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: run_start decreases at run %lld", (long long)r);
    const int64_t N = run_start[R];
    if (N >= (1LL << 31) || R >= (1LL << 24)) return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: too many rows or runs");
    if (kdraw < 0 || first < 0 || max_candidates < 0 || first + max_candidates >= (1LL << 55))
        return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: kdraw, first or max_candidates out of range");
    if (block < 1 || block > (1 << 20)) return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: block = %d is outside [1, 2^20]", block);
    if (trace_cap < 0 || (trace_cap > 0 && (!trace_cube || !trace_flags || !trace_n || !trace_logl || !trace_count)))
        return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: bad trace buffers");
    if (rounds) *rounds = 0;
    if (R == 0) return RVLL_OK;
    if (!scale || !radius2 || !lstar || !seeds || !nfound || !ncalls || (N > 0 && !survivors) ||
        (kdraw > 0 && (!cube_out || !theta_out || !logl_out)))
        return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: null buffer");
    const int D = h->L.ndim;
    if (D < 1 || D > kRegionMaxDims)
        return report_error(RVLL_E_UNSUPPORTED, "rvll_region_draw_runs: %d parameters (region sampling takes 1 .. %d)", D, kRegionMaxDims);
    for (int64_t k = 0; k < R * D; ++k)
        if (!(std::isfinite(scale[k]) && scale[k] > 0.0))
            return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: scale[%lld] is not finite and positive", (long long)k);
    for (int64_t r = 0; r < R; ++r) {
        if (!(std::isfinite(radius2[r]) && radius2[r] >= 0.0))
            return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: radius2[%lld] is not finite and non-negative", (long long)r);
        if (std::isnan(lstar[r])) return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: lstar[%lld] is NaN", (long long)r);
    }
    const unsigned long long wmask = wrapped_mask(wrapped, D);

    // the runs that draw at all: survivors, and no wrapped dimension in which the ball meets its own image
    std::vector<int32_t> act;
    for (int64_t r = 0; r < R; ++r) {
        bool ok = run_start[r + 1] > run_start[r] && kdraw > 0 && max_candidates > 0;
        for (int k = 0; ok && k < D; ++k)
            if (((wmask >> k) & 1ull) && std::sqrt(radius2[r]) / scale[r * D + k] >= 0.5) ok = false;
        if (ok) act.push_back((int32_t)r);
    }
    std::vector<int32_t> found((size_t)R, 0);
    std::vector<long long> calls((size_t)R, 0);
    std::vector<long long> evaluated((size_t)R, 0);

    const int chunks = (block + kRegionThreads - 1) / kRegionThreads;
    const size_t A0 = act.size();
    const size_t S = A0 * (size_t)block, W = A0 * (size_t)chunks;
    if (S >= ((size_t)1 << 31)) return report_error(RVLL_E_INVALID, "rvll_region_draw_runs: runs x block must stay below 2^31");
    const size_t K = (size_t)R * (size_t)kdraw, T = (size_t)R * (size_t)trace_cap;
    // one device block: inputs | per-slot work | per-run state | outputs | trace
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = up16(o + bytes); return at; };
    const size_t o_surv = take(sizeof(double) * (size_t)N * D), o_scale = take(sizeof(double) * (size_t)R * D);
    const size_t o_r2 = take(sizeof(double) * (size_t)R), o_lstar = take(sizeof(double) * (size_t)R);
    const size_t o_start = take(sizeof(int64_t) * (size_t)(R + 1)), o_seed = take(sizeof(uint64_t) * (size_t)R);
    const size_t in_bytes = o;
    const size_t o_act = take(sizeof(int32_t) * (size_t)R);
    const size_t o_cand = take(sizeof(double) * S * D), o_flag = take(sizeof(int32_t) * S), o_count = take(sizeof(int32_t) * S);
    const size_t o_rank = take(sizeof(int32_t) * S), o_pos = take(sizeof(int32_t) * S);
    const size_t o_wgc = take(sizeof(int32_t) * W), o_wgo = take(sizeof(int32_t) * (W + 1));
    const size_t o_state = o;
    const size_t o_found = take(sizeof(int32_t) * (size_t)R), o_calls = take(sizeof(long long) * (size_t)R);
    const size_t state_bytes = o - o_state;
    const size_t o_out = o;
    const size_t o_ocube = take(sizeof(double) * K * D), o_otheta = take(sizeof(double) * K * D), o_ologl = take(sizeof(double) * K);
    const size_t out_bytes = o - o_out;
    const size_t o_trace = o;
    const size_t o_tcube = take(sizeof(double) * T * D), o_tlogl = take(sizeof(double) * T);
    const size_t o_tflags = take(sizeof(int32_t) * T), o_tn = take(sizeof(int32_t) * T);
    const size_t trace_bytes = o - o_trace;
    const size_t total = o;
    if (total > kRegionMaxBytes)
        return report_error(RVLL_E_NOMEM, "rvll_region_draw_runs: %zu bytes of device memory exceed the region sampler's budget", total);
    RVLL_TRY(grow(h, &h->d_region, &h->region_cap, total));
    // the batch buffers take every kept candidate of a round (reserved now: growing them frees them)
    rc = rvll_dev_reserve(h, (int64_t)std::max<size_t>(S, 1));
    if (rc) return rc;
    rc = sync_other_lanes(h);
    if (rc) return rc;

    hipStream_t st = h->compute;
    char* dev = static_cast<char*>(h->d_region);
    std::vector<char> in(in_bytes);
    if (N > 0) memcpy(in.data() + o_surv, survivors, sizeof(double) * (size_t)N * D);
    memcpy(in.data() + o_scale, scale, sizeof(double) * (size_t)R * D);
    memcpy(in.data() + o_r2, radius2, sizeof(double) * (size_t)R);
    memcpy(in.data() + o_lstar, lstar, sizeof(double) * (size_t)R);
    memcpy(in.data() + o_start, run_start, sizeof(int64_t) * (size_t)(R + 1));
    memcpy(in.data() + o_seed, seeds, sizeof(uint64_t) * (size_t)R);
    HIP_TRY(hipMemcpyAsync(dev, in.data(), in_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dev + o_state, 0, state_bytes, st));
    if (out_bytes) HIP_TRY(hipMemsetAsync(dev + o_out, 0xff, out_bytes, st));              // rows never found: NaN
    if (trace_bytes) {
        HIP_TRY(hipMemsetAsync(dev + o_tcube, 0xff, o_tflags - o_tcube, st));
        HIP_TRY(hipMemsetAsync(dev + o_tflags, 0, o - o_tflags, st));
    }

    RegionArgs p{};
    p.surv = reinterpret_cast<const double*>(dev + o_surv);
    p.run_start = reinterpret_cast<const long long*>(dev + o_start);
    p.scale = reinterpret_cast<const double*>(dev + o_scale);
    p.radius2 = reinterpret_cast<const double*>(dev + o_r2);
    p.lstar = reinterpret_cast<const double*>(dev + o_lstar);
    p.seeds = reinterpret_cast<const unsigned long long*>(dev + o_seed);
    p.act = reinterpret_cast<const int32_t*>(dev + o_act);
    p.wmask = wmask;
    p.D = D; p.block = block; p.chunks = chunks; p.kdraw = kdraw;
    p.first = first; p.cend = first + max_candidates;
    p.cand = reinterpret_cast<double*>(dev + o_cand);
    p.flag = reinterpret_cast<int32_t*>(dev + o_flag);
    p.count = reinterpret_cast<int32_t*>(dev + o_count);
    p.rank = reinterpret_cast<int32_t*>(dev + o_rank);
    p.pos = reinterpret_cast<int32_t*>(dev + o_pos);
    p.wg_count = reinterpret_cast<int32_t*>(dev + o_wgc);
    p.wg_offset = reinterpret_cast<int32_t*>(dev + o_wgo);
    p.nfound = reinterpret_cast<int32_t*>(dev + o_found);
    p.ncalls = reinterpret_cast<long long*>(dev + o_calls);
    p.out_cube = reinterpret_cast<double*>(dev + o_ocube);
    p.out_theta = reinterpret_cast<double*>(dev + o_otheta);
    p.out_logl = reinterpret_cast<double*>(dev + o_ologl);
    p.trace_cap = trace_cap;
    p.trace_cube = reinterpret_cast<double*>(dev + o_tcube);
    p.trace_flags = reinterpret_cast<int32_t*>(dev + o_tflags);
    p.trace_n = reinterpret_cast<int32_t*>(dev + o_tn);
    p.trace_logl = reinterpret_cast<double*>(dev + o_tlogl);

    int nrounds = 0;
    std::vector<char> state(state_bytes);
    for (long long c0 = first; !act.empty() && c0 < p.cend; c0 += block) {
        const int A = (int)act.size();
        const int Wr = A * chunks;
        p.c0 = c0;
        HIP_TRY(hipMemcpyAsync(dev + o_act, act.data(), sizeof(int32_t) * (size_t)A, hipMemcpyHostToDevice, st));
        p.batch_cube = h->d_cube;
        if (D <= 8) launch_propose<8>(p, A, st);
        else if (D <= 16) launch_propose<16>(p, A, st);
        else if (D <= 32) launch_propose<32>(p, A, st);
        else launch_propose<64>(p, A, st);
        hipLaunchKernelGGL(region_offsets_kernel, dim3(1), dim3(kRegionThreads), 0, st, p.wg_count, p.wg_offset, Wr);
        hipLaunchKernelGGL(region_pack_kernel, dim3((unsigned)Wr), dim3(kRegionThreads), 0, st, p);
        HIP_TRY(hipGetLastError());
        int32_t B = 0;
        HIP_TRY(hipMemcpyAsync(&B, p.wg_offset + Wr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (B < 0 || (size_t)B > S) return report_error(RVLL_E_HIP, "rvll_region_draw_runs: the pack count %d is out of range", B);
        if (B > 0) {
            rc = rvll_dev_prior_loglike(h, B);
            if (rc) return rc;
            rc = use_device(h);                                   // a one-launch batch that deferred elements is redone here
            if (rc) return rc;
        }
        p.batch_theta = h->d_theta;
        p.batch_logl = h->d_logL2[h->logl_last];
        if (h->logl_last != 0) HIP_TRY(hipStreamSynchronize(h->lanes[h->logl_last]));
        hipLaunchKernelGGL(region_select_kernel, dim3((unsigned)A), dim3(kRegionThreads), 0, st, p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(state.data(), dev + o_state, state_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        memcpy(found.data(), state.data() + (o_found - o_state), sizeof(int32_t) * (size_t)R);
        memcpy(calls.data(), state.data() + (o_calls - o_state), sizeof(long long) * (size_t)R);
        ++nrounds;
        const long long done = std::min<long long>(c0 + block, p.cend) - first;
        std::vector<int32_t> next;
        for (int32_t r : act) {
            evaluated[(size_t)r] = done;
            if (found[(size_t)r] < kdraw) next.push_back(r);
        }
        act.swap(next);
    }

    if (out_bytes) {
        std::vector<char> out(out_bytes);
        HIP_TRY(hipMemcpyAsync(out.data(), dev + o_out, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        memcpy(cube_out, out.data() + (o_ocube - o_out), sizeof(double) * K * D);
        memcpy(theta_out, out.data() + (o_otheta - o_out), sizeof(double) * K * D);
        memcpy(logl_out, out.data() + (o_ologl - o_out), sizeof(double) * K);
    }
    if (trace_bytes) {
        std::vector<char> tr(trace_bytes);
        HIP_TRY(hipMemcpyAsync(tr.data(), dev + o_trace, trace_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        memcpy(trace_cube, tr.data() + (o_tcube - o_trace), sizeof(double) * T * D);
        memcpy(trace_logl, tr.data() + (o_tlogl - o_trace), sizeof(double) * T);
        memcpy(trace_flags, tr.data() + (o_tflags - o_trace), sizeof(int32_t) * T);
        memcpy(trace_n, tr.data() + (o_tn - o_trace), sizeof(int32_t) * T);
    }
    for (int64_t r = 0; r < R; ++r) {
        nfound[r] = found[(size_t)r];
        ncalls[r] = calls[(size_t)r];
        if (trace_count) trace_count[r] = std::min<long long>(evaluated[(size_t)r], trace_cap);
    }
    if (rounds) *rounds = nrounds;
    return RVLL_OK;
}

}  // extern "C"
