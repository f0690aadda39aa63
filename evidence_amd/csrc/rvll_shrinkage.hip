// Simulated shrinkage on gfx950: replicates of ln Z, H and the posterior weights of finished nested-sampling runs
// (evidence_amd/shrinkage.py holds the numpy definition).
//
// One 256-thread workgroup per (run, replicate).  The run's deaths go through in tiles of kThreads * kPer: lane t holds
// deaths t*kPer .. t*kPer + kPer - 1 of the tile in registers, regenerating each draw u from its counter (splitmix64,
// uniform01 of rvll_math.h) — nothing per death is stored.  Per tile:
//     log t_j            kPer logs (or -1/n_j in expected mode) and one lane sum
//     exclusive scan     of the lane sums: 64-lane shuffle scan, then the four wave totals through LDS (one barrier;
//                        the LDS slots alternate between tiles so the next tile's writes cannot meet this tile's reads)
//     logX, logw         the lane walks its kPer deaths from carry + its prefix: logw = (logl + logX_{j-1}) + log(-expm1(log t))
//     online sums        (max, sum e, sum e logl) of the dead rows, one exp per row, rescaled when the max rises
// then the final live rows (logX_last - log m) + logl, strided over the lanes into (max, sum e), and one workgroup
// reduction of both triples in a fixed tree.  With weights requested every lane writes its rows' logw to the caller's
// block and, once ln Z is known, subtracts it from the rows it wrote itself.
//
// A (run, replicate)'s result depends on its log-L, schedule, seed and replicate index only: the tile and the reduction
// trees are fixed, no atomics, and no workgroup reads another's data — alone or inside any batch, the bits are the same.
// The run's log-L array is read by all its replicates: consecutive workgroups belong to one run, so it stays in L2.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include <algorithm>

#pragma GCC visibility push(default)
#include "rvll.h"
#pragma GCC visibility pop
#include "rvll_math.h"

namespace rvll {
int report_error(int code, const char* fmt, ...);
}

namespace {

#ifndef RVLL_SHRINK_K
#define RVLL_SHRINK_K 4
#endif
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kPer = RVLL_SHRINK_K;                     // deaths a lane holds per tile
constexpr long long kTile = (long long)kThreads * kPer;
constexpr unsigned long long kSeedMul = 0xD1B54A32D192ED03ull;
constexpr long long kMaxGroups = 1ll << 22;              // workgroups per launch (grid x * 256 threads < 2^32)
constexpr long long kDefaultBlockBytes = 512ll << 20;   // device bound on a block of weights

#define SHR_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            status = rvll::report_error(e_ == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, \
                                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                        __FILE__, __LINE__);                                   \
            goto done;                                                                         \
        }                                                                                      \
    } while (0)

// (max, sum of exp(w - max), sum of exp(w - max) * logl) of a set of rows; m = -inf: no row with weight
struct Tri {
    double m, s, a;
};

__device__ __forceinline__ void tri_add(Tri& t, double w, double l)
{
    if (!(w > -INFINITY)) return;                        // a row of zero weight (or NaN) takes no part
    const double d = w - t.m;                            // t.m = -inf: d = +inf, x = 0
    const double x = exp(-fabs(d));
    const bool up = d > 0.0;
    t.s = up ? t.s * x + 1.0 : t.s + x;
    t.a = up ? t.a * x + l : t.a + x * l;
    t.m = up ? w : t.m;
}

__device__ __forceinline__ Tri tri_join(Tri p, Tri q)
{
    if (!(q.m > -INFINITY)) return p;
    if (!(p.m > -INFINITY)) return q;
    const double mx = fmax(p.m, q.m);
    const double cp = exp(p.m - mx), cq = exp(q.m - mx);
    return Tri{mx, p.s * cp + q.s * cq, p.a * cp + q.a * cq};
}

__device__ __forceinline__ Tri tri_shfl_xor(Tri t, int off)
{
    return Tri{__shfl_xor(t.m, off, kWave), __shfl_xor(t.s, off, kWave), __shfl_xor(t.a, off, kWave)};
}

// the workgroup's triple, every lane: butterfly inside each wave, then the four wave results in order 0..3
__device__ Tri tri_reduce(Tri t, Tri* sh)
{
    for (int off = 1; off < kWave; off <<= 1) t = tri_join(t, tri_shfl_xor(t, off));
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) sh[wave] = t;
    __syncthreads();
    Tri r = sh[0];
    for (int w = 1; w < kWaves; ++w) r = tri_join(r, sh[w]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kThreads) void shrink_kernel(
    const double* __restrict__ logl, const long long* __restrict__ run_start, const long long* __restrict__ n_dead,
    const int* __restrict__ nlive, const int* __restrict__ kbatch, const unsigned long long* __restrict__ seeds,
    int nsamples, int s0, int s_blk, int expected, double* __restrict__ logz, double* __restrict__ info,
    double* __restrict__ logw_out)
{
    __shared__ double sh_scan[2][kWaves];
    __shared__ Tri sh_tri[kWaves];
    __shared__ double sh_lnz;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int r = (int)(blockIdx.x / (unsigned)s_blk);
    const int s = s0 + (int)(blockIdx.x % (unsigned)s_blk);
    const long long base = run_start[r], rows = run_start[r + 1] - base, N = n_dead[r], m = rows - N;
    const int nl = nlive[r], kb = kbatch[r];
    const uint64_t seed = (uint64_t)seeds[r] + (uint64_t)s * kSeedMul;
    const double* ll = logl + base;
    double* wout = logw_out ? logw_out + (long long)s_blk * base + (long long)(s - s0) * rows : nullptr;

    Tri dead{-INFINITY, 0.0, 0.0};
    double carry = 0.0;                                  // logX before the tile
    int parity = 0;
    for (long long t0 = 0; t0 < N; t0 += kTile, parity ^= 1) {
        const long long j0 = t0 + (long long)tid * kPer;
        int ph = (int)(j0 % kb);                         // j mod kbatch, stepped below
        double lt[kPer];
        double lsum = 0.0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const long long j = j0 + k;
            const double n = (double)(nl - ph);
            ph = ph + 1 == kb ? 0 : ph + 1;
            lt[k] = j >= N ? 0.0 : expected ? -1.0 / n : log(1.0 - rvll::uniform01(seed, (uint64_t)j)) / n;
            lsum += lt[k];
        }
        double incl = lsum;
        for (int off = 1; off < kWave; off <<= 1) {
            const double o = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += o;
        }
        double excl = __shfl_up(incl, 1, kWave);
        if (lane == 0) excl = 0.0;
        if (lane == kWave - 1) sh_scan[parity][wave] = incl;
        __syncthreads();
        double before = 0.0, total = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const double v = sh_scan[parity][w];
            if (w < wave) before += v;
            total += v;
        }
        double lx = carry + (before + excl);
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const long long j = j0 + k;
            if (j < N) {
                const double l = ll[j];
                const double w = (l + lx) + log(-expm1(lt[k]));
                lx += lt[k];
                tri_add(dead, w, l);
                if (wout) wout[j] = w;
            }
        }
        carry += total;
    }
    const double live_off = carry - log((double)m);
    Tri live{-INFINITY, 0.0, 0.0};
    for (long long i = tid; i < m; i += kThreads) {
        const double w = live_off + ll[N + i];
        tri_add(live, w, 0.0);
        if (wout) wout[N + i] = w;
    }
    dead = tri_reduce(dead, sh_tri);
    live = tri_reduce(live, sh_tri);
    if (tid == 0) {
        const bool any = dead.m > -INFINITY;
        const double lnzd = any ? dead.m + log(dead.s) : -INFINITY;
        const double lnzl = live.m > -INFINITY ? live.m + log(live.s) : -INFINITY;
        const double hi = fmax(lnzd, lnzl), lo = fmin(lnzd, lnzl);
        const double lnz = hi == -INFINITY ? -INFINITY : hi + log1p(exp(lo - hi));
        logz[(long long)r * nsamples + s] = lnz;
        info[(long long)r * nsamples + s] = any ? dead.a / dead.s - lnzd : 0.0;
        sh_lnz = lnz;
    }
    if (!wout) return;
    __syncthreads();
    const double lnz = sh_lnz;
    for (long long t0 = 0; t0 < N; t0 += kTile)
        for (int k = 0; k < kPer; ++k) {
            const long long j = t0 + (long long)tid * kPer + k;
            if (j < N) wout[j] -= lnz;
        }
    for (long long i = tid; i < m; i += kThreads) wout[N + i] -= lnz;
}

}  // namespace

extern "C" int rvll_shrinkage_replicates(int32_t device, const double* logl, int64_t n_rows, const int64_t* run_start,
                                         int32_t n_runs, const int64_t* n_dead, const int32_t* nlive,
                                         const int32_t* kbatch, const uint64_t* seeds, int32_t nsamples, int32_t mode,
                                         double* logz, double* info, double* logwt, int64_t block_bytes,
                                         rvll_shrink_timing* timing)
{
    const auto t_start = std::chrono::steady_clock::now();
    if (n_runs < 0 || n_rows < 0) return rvll::report_error(RVLL_E_INVALID, "negative n_runs or n_rows");
    if (nsamples < 1) return rvll::report_error(RVLL_E_INVALID, "nsamples must be >= 1");
    if (mode != RVLL_SHRINK_RANDOM && mode != RVLL_SHRINK_EXPECTED)
        return rvll::report_error(RVLL_E_INVALID, "mode %d is neither RVLL_SHRINK_RANDOM nor RVLL_SHRINK_EXPECTED", mode);
    if (block_bytes < 0) return rvll::report_error(RVLL_E_INVALID, "negative block_bytes");
    if (timing) *timing = rvll_shrink_timing{0., 0., 0, 0, kThreads};
    if (n_runs == 0) return RVLL_OK;
    if (!run_start || !n_dead || !nlive || !kbatch || !seeds || !logz || !info || (n_rows > 0 && !logl))
        return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (n_runs > kMaxGroups) return rvll::report_error(RVLL_E_INVALID, "n_runs > %lld", kMaxGroups);
    if (run_start[0] != 0 || run_start[n_runs] != n_rows)
        return rvll::report_error(RVLL_E_INVALID, "run_start must run from 0 to n_rows = %lld", (long long)n_rows);
    for (int r = 0; r < n_runs; ++r) {
        const long long rows = run_start[r + 1] - run_start[r];
        if (rows < 0) return rvll::report_error(RVLL_E_INVALID, "run_start must be non-decreasing (run %d)", r);
        if (n_dead[r] < 0) return rvll::report_error(RVLL_E_INVALID, "n_dead[%d] < 0", r);
        if (kbatch[r] < 1 || kbatch[r] >= nlive[r])
            return rvll::report_error(RVLL_E_INVALID, "run %d: need 1 <= kbatch (%d) < nlive (%d)", r, kbatch[r], nlive[r]);
        if (n_dead[r] % kbatch[r] != 0)
            return rvll::report_error(RVLL_E_INVALID, "run %d: n_dead %lld is not a multiple of kbatch %d", r,
                                      (long long)n_dead[r], kbatch[r]);
        if (rows - n_dead[r] < 1)
            return rvll::report_error(RVLL_E_INVALID, "run %d: %lld rows leave no final live row after %lld dead", r, rows,
                                      (long long)n_dead[r]);
    }

    // replicates per launch: bounded by the grid, and with weights by the device block (one replicate of every run is
    // n_rows doubles; a request whose single replicate does not fit is refused before anything is allocated)
    long long s_blk = std::min<long long>(nsamples, std::max<long long>(1, kMaxGroups / n_runs));
    const long long bound = block_bytes > 0 ? block_bytes : kDefaultBlockBytes;
    if (logwt) {
        const long long per_rep = n_rows * (long long)sizeof(double);
        if (per_rep > bound)
            return rvll::report_error(RVLL_E_NOMEM, "one replicate of the weights needs %lld bytes, above the device block "
                                      "bound of %lld", per_rep, bound);
        if (n_rows > 0) s_blk = std::min<long long>(s_blk, bound / per_rep);
    }
    const long long nout = (long long)n_runs * nsamples;

    int status = RVLL_OK;
    int prev_device = -1;
    double *d_logl = nullptr, *d_logz = nullptr, *d_info = nullptr, *d_w = nullptr;
    long long *d_rs = nullptr, *d_nd = nullptr;
    int *d_nl = nullptr, *d_kb = nullptr;
    unsigned long long* d_seeds = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double kernel_ms = 0.;
    int launches = 0;

    SHR_TRY(hipGetDevice(&prev_device));
    if (device >= 0) SHR_TRY(hipSetDevice(device));
    SHR_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) SHR_TRY(hipEventCreate(&e));
    // every device block is allocated before the first launch: running out of memory fails the call before any work
    SHR_TRY(hipMalloc(&d_logl, sizeof(double) * (size_t)std::max<long long>(n_rows, 1)));
    SHR_TRY(hipMalloc(&d_rs, sizeof(long long) * (size_t)(n_runs + 1)));
    SHR_TRY(hipMalloc(&d_nd, sizeof(long long) * (size_t)n_runs));
    SHR_TRY(hipMalloc(&d_nl, sizeof(int) * (size_t)n_runs));
    SHR_TRY(hipMalloc(&d_kb, sizeof(int) * (size_t)n_runs));
    SHR_TRY(hipMalloc(&d_seeds, sizeof(unsigned long long) * (size_t)n_runs));
    SHR_TRY(hipMalloc(&d_logz, sizeof(double) * (size_t)nout));
    SHR_TRY(hipMalloc(&d_info, sizeof(double) * (size_t)nout));
    if (logwt) SHR_TRY(hipMalloc(&d_w, sizeof(double) * (size_t)std::max<long long>(s_blk * n_rows, 1)));
    if (n_rows > 0) SHR_TRY(hipMemcpyAsync(d_logl, logl, sizeof(double) * (size_t)n_rows, hipMemcpyHostToDevice, stream));
    SHR_TRY(hipMemcpyAsync(d_rs, run_start, sizeof(long long) * (size_t)(n_runs + 1), hipMemcpyHostToDevice, stream));
    SHR_TRY(hipMemcpyAsync(d_nd, n_dead, sizeof(long long) * (size_t)n_runs, hipMemcpyHostToDevice, stream));
    SHR_TRY(hipMemcpyAsync(d_nl, nlive, sizeof(int) * (size_t)n_runs, hipMemcpyHostToDevice, stream));
    SHR_TRY(hipMemcpyAsync(d_kb, kbatch, sizeof(int) * (size_t)n_runs, hipMemcpyHostToDevice, stream));
    SHR_TRY(hipMemcpyAsync(d_seeds, seeds, sizeof(unsigned long long) * (size_t)n_runs, hipMemcpyHostToDevice, stream));
    for (long long s0 = 0; s0 < nsamples; s0 += s_blk) {
        const long long sb = std::min<long long>(s_blk, nsamples - s0);
        SHR_TRY(hipEventRecord(ev[0], stream));
        hipLaunchKernelGGL(shrink_kernel, dim3((unsigned)(n_runs * sb)), dim3(kThreads), 0, stream, d_logl, d_rs, d_nd, d_nl,
                           d_kb, d_seeds, (int)nsamples, (int)s0, (int)sb, mode == RVLL_SHRINK_EXPECTED ? 1 : 0, d_logz, d_info,
                           d_w);
        SHR_TRY(hipGetLastError());
        SHR_TRY(hipEventRecord(ev[1], stream));
        ++launches;
        if (d_w) {
            // run r's block is contiguous on both sides: sb rows of its length at s_blk-strided offsets on the device,
            // at row s0 of its [nsamples, rows] slab in the caller's buffer
            for (int r = 0; r < n_runs; ++r) {
                const long long rows = run_start[r + 1] - run_start[r];
                if (rows == 0) continue;
                SHR_TRY(hipMemcpyAsync(logwt + (long long)nsamples * run_start[r] + s0 * rows, d_w + sb * run_start[r],
                                       sizeof(double) * (size_t)(sb * rows), hipMemcpyDeviceToHost, stream));
            }
        }
        SHR_TRY(hipEventSynchronize(ev[1]));
        float ms = 0.f;
        SHR_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        kernel_ms += ms;
    }
    SHR_TRY(hipMemcpyAsync(logz, d_logz, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, stream));
    SHR_TRY(hipMemcpyAsync(info, d_info, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, stream));
    SHR_TRY(hipStreamSynchronize(stream));
    if (timing) {
        timing->kernel_ms = kernel_ms;
        timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        timing->elements = n_rows * (long long)nsamples;
        timing->launches = launches;
        timing->threads = kThreads;
    }

done:
    for (void* p : {(void*)d_logl, (void*)d_rs, (void*)d_nd, (void*)d_nl, (void*)d_kb, (void*)d_seeds, (void*)d_logz,
                    (void*)d_info, (void*)d_w})
        if (p) (void)hipFree(p);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (prev_device >= 0 && device >= 0) (void)hipSetDevice(prev_device);
    return status;
}
