// Merging finished nested-sampling runs by their birth contours on gfx950, and replicates of the merged run (simulated
// shrinkage, optionally on top of a bootstrap of the runs).  evidence_amd/merge.py holds the numpy definition; DESIGN §4j.
//
// Once per call:
//     keys      the log-L and the (off-contour corrected) birth of every row as order-preserving uint64 keys (rvll_keys.h),
//               the row index and its run label
//     sorts     rocPRIM radix sort of the log-L keys carrying the row index (stable: ties keep the input order, which is
//               (run, position)) -> the merged order; radix sort of the birth keys carrying the run labels
//     place     per merged row i: L_i, rho_i, cntb_i = #{births < L_i} (binary search in the sorted births), n_i = cntb_i - i;
//               and one event stream of 2N entries, the births and deaths merged by value with deaths first on a tie: death i
//               sits at i + cntb_i, birth j at j + #{deaths with L <= b_j}.  Entry >= 0: the death of merged row i;
//               entry < 0: the birth of a row of run -1 - entry.
// Per replicate, one 256-thread workgroup walks the stream in tiles of 1024 entries (lane t holds entries 4t .. 4t + 3):
//     counts    w = the run's multiplicity (LDS; 1 without the bootstrap).  A birth adds +w to the live count, a death -w,
//               and a death adds w to the copies that died before.  Exclusive scan of both (int64) over the lane sums:
//               64-lane shuffle scan, the four wave totals through LDS, one barrier.  So every death learns
//               n_i = sum_{b < L_i} w - sum_{k < i} w and its first draw counter c without a second pass.
//     Delta     per death: w terms in the order q = 0 .. w - 1, expected -1 / (n - q) or log(1 - uniform01(seed_s, c + q)) / (n - q)
//     logX      exclusive scan of Delta as above (a second barrier); the carry between tiles is a compensated (two-sum) pair,
//               and a row's logX_{i-1} = carry_hi + (carry_lo + its offset inside the tile): one rounding at the magnitude of
//               logX, none accumulated over the tiles
//     sums      logw = (L + logX_{i-1}) + log(-expm1(Delta)) into an online (max, sum e, sum e L) triple, one exp per row
// then a fixed butterfly and four-wave fold of the triple.  With weights requested each lane writes its deaths' logw to the
// replicate's slot of the device block and, once ln Z is known, subtracts it from the rows it wrote itself.  The LDS slots of
// both scans alternate between tiles, so a tile's writes cannot meet the previous tile's reads.
//
// A replicate's result depends on the input, the seed and its index only: the tile and the trees are fixed, the bootstrap's
// LDS counts are integers, and no workgroup reads another's data — alone or inside any batch, the bits are the same.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <vector>
#include <cstring>
#include <rocprim/rocprim.hpp>

#pragma GCC visibility push(default)
#include "rvll.h"
#pragma GCC visibility pop
#include "rvll_keys.h"
#include "rvll_math.h"

namespace rvll {
int report_error(int code, const char* fmt, ...);
}

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kPer = 4;                                   // stream entries a lane holds per tile
constexpr long long kTile = (long long)kThreads * kPer;
constexpr int kMaxBlocks = 8192;
constexpr long long kMaxRows = (1ll << 30) - 1;           // 2N stream positions stay below 2^31
constexpr int kMaxBootRuns = 8192;                        // LDS multiplicities: 32 KiB
constexpr long long kMaxGroups = 1ll << 22;               // replicates per launch (grid x * 256 threads < 2^32)
constexpr long long kDefaultBlockBytes = 512ll << 20;     // device bound on a block of weights
constexpr unsigned long long kSeedMul = 0xD1B54A32D192ED03ull;
constexpr unsigned long long kBootXor = 0x5851F42D4C957F2Dull;

typedef unsigned long long u64;

#define MRG_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            status = rvll::report_error(e_ == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, \
                                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                        __FILE__, __LINE__);                                   \
            goto done;                                                                         \
        }                                                                                      \
    } while (0)

int blocks_for(long long total, int per_block)
{
    const long long b = (total + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > kMaxBlocks ? kMaxBlocks : b);
}

// keys of every row, its index and its run (the last r with run_start[r] <= g)
__global__ __launch_bounds__(kThreads)
void keys_kernel(const double* __restrict__ logl, const double* __restrict__ birth, long long n, const long long* __restrict__ rs,
                 int nruns, u64* __restrict__ kl, u64* __restrict__ kb, int32_t* __restrict__ idx, int32_t* __restrict__ run)
{
    for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < n; g += (long long)gridDim.x * kThreads) {
        const double l = logl[g], b = birth[g];
        kl[g] = rvll::key_of(l);
        kb[g] = rvll::key_of(l <= b ? nextafter(l, -INFINITY) : b);
        idx[g] = (int32_t)g;
        int lo = 0, hi = nruns;
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (rs[mid] <= g) lo = mid; else hi = mid;
        }
        run[g] = lo;
    }
}

// first position in s[0 .. n) whose key is > v (upper) or >= v (lower)
__device__ inline long long upper_bound(const u64* s, long long n, u64 v)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline long long lower_bound(const u64* s, long long n, u64 v)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// per merged row: L, rho, n (unweighted) and its death's place in the stream; per sorted birth: its place
__global__ __launch_bounds__(kThreads)
void place_kernel(const double* __restrict__ logl, const u64* __restrict__ sl, const int32_t* __restrict__ order,
                  const u64* __restrict__ sb, const int32_t* __restrict__ rb, const int32_t* __restrict__ run, long long n,
                  double* __restrict__ L, int32_t* __restrict__ rho, long long* __restrict__ nlive, int32_t* __restrict__ ev)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const int32_t g = order[i];
        L[i] = logl[g];
        rho[i] = run[g];
        const long long cntb = lower_bound(sb, n, sl[i]);     // #{birth < L_i}, >= i + 1
        nlive[i] = cntb - i;
        ev[i + cntb] = (int32_t)i;
        const long long dj = upper_bound(sl, n, sb[i]);       // #{deaths with L <= b_i}: the deaths before birth i
        ev[i + dj] = -1 - rb[i];
    }
}

// (max, sum of exp(w - max), sum of exp(w - max) * L); m = -inf: no row with weight
struct Tri {
    double m, s, a;
};

__device__ __forceinline__ void tri_add(Tri& t, double w, double l)
{
    if (!(w > -INFINITY)) return;
    const double d = w - t.m;
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

__device__ Tri tri_reduce(Tri t, Tri* sh)
{
    for (int off = 1; off < kWave; off <<= 1)
        t = tri_join(t, Tri{__shfl_xor(t.m, off, kWave), __shfl_xor(t.s, off, kWave), __shfl_xor(t.a, off, kWave)});
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) sh[wave] = t;
    __syncthreads();
    Tri r = sh[0];
    for (int w = 1; w < kWaves; ++w) r = tri_join(r, sh[w]);
    __syncthreads();
    return r;
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

__global__ __launch_bounds__(kThreads) void replicate_kernel(
    const int32_t* __restrict__ ev, const double* __restrict__ L, const int32_t* __restrict__ rho, long long n, int nruns,
    int s0, u64 seed, int expected, int bootstrap, double* __restrict__ logz, double* __restrict__ info,
    double* __restrict__ logw_out)
{
    extern __shared__ int32_t sh_w[];                     // bootstrap: the multiplicity of every run
    __shared__ long long sh_n[2][kWaves], sh_d[2][kWaves];
    __shared__ double sh_x[2][kWaves];
    __shared__ Tri sh_tri[kWaves];
    __shared__ double sh_lnz;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int s = s0 + (int)blockIdx.x;
    const u64 seed_s = seed + (u64)s * kSeedMul;
    const long long E = 2 * n;
    double* wout = logw_out ? logw_out + (long long)blockIdx.x * n : nullptr;

    if (bootstrap) {
        for (int r = tid; r < nruns; r += kThreads) sh_w[r] = 0;
        __syncthreads();
        const u64 bseed = seed_s ^ kBootXor;
        for (int t = tid; t < nruns; t += kThreads) {
            const int d = (int)fmin(floor(rvll::uniform01(bseed, (u64)t) * (double)nruns), (double)(nruns - 1));
            atomicAdd(&sh_w[d], 1);
        }
        __syncthreads();
    }

    Tri acc{-INFINITY, 0.0, 0.0};
    long long carry_n = 0, carry_d = 0;
    double carry_hi = 0.0, carry_lo = 0.0;               // logX before the tile, as a compensated pair
    int parity = 0;
    for (long long t0 = 0; t0 < E; t0 += kTile, parity ^= 1) {
        const long long e0 = t0 + (long long)tid * kPer;
        int32_t v[kPer];
        int wt[kPer];
        long long sn = 0, sd = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const long long e = e0 + k;
            v[k] = e < E ? ev[e] : INT32_MIN;
            const int r = v[k] >= 0 ? rho[v[k]] : v[k] == INT32_MIN ? -1 : -1 - v[k];
            wt[k] = r < 0 ? 0 : bootstrap ? sh_w[r] : 1;
            if (v[k] >= 0) { sn -= wt[k]; sd += wt[k]; } else sn += wt[k];
        }
        const long long in_n = wave_scan(sn, lane), in_d = wave_scan(sd, lane);
        if (lane == kWave - 1) { sh_n[parity][wave] = in_n; sh_d[parity][wave] = in_d; }
        __syncthreads();
        long long bn = 0, bd = 0, tn = 0, td = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const long long a = sh_n[parity][w], b = sh_d[parity][w];
            if (w < wave) { bn += a; bd += b; }
            tn += a;
            td += b;
        }
        long long nl = carry_n + bn + (in_n - sn), dl = carry_d + bd + (in_d - sd);
        double dt[kPer];
        double xs = 0.0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            dt[k] = 0.0;
            if (v[k] >= 0) {
                for (int q = 0; q < wt[k]; ++q) {
                    const double nn = (double)(nl - q);
                    dt[k] += expected ? -1.0 / nn : log(1.0 - rvll::uniform01(seed_s, (u64)(dl + q))) / nn;
                }
                nl -= wt[k];
                dl += wt[k];
            } else {
                nl += wt[k];
            }
            xs += dt[k];
        }
        carry_n += tn;
        carry_d += td;
        const double in_x = wave_scan(xs, lane);
        if (lane == kWave - 1) sh_x[parity][wave] = in_x;
        __syncthreads();
        double bx = 0.0, tx = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const double a = sh_x[parity][w];
            if (w < wave) bx += a;
            tx += a;
        }
        double loc = bx + (in_x - xs);
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (v[k] >= 0) {
                const double l = L[v[k]];
                const double lx = carry_hi + (carry_lo + loc);
                const double w = wt[k] > 0 ? (l + lx) + log(-expm1(dt[k])) : -INFINITY;
                tri_add(acc, w, l);
                if (wout) wout[v[k]] = w;
            }
            loc += dt[k];
        }
        // two-sum of carry_hi + tx
        const double sum = carry_hi + tx, bv = sum - carry_hi;
        carry_lo += (carry_hi - (sum - bv)) + (tx - bv);
        carry_hi = sum;
    }
    acc = tri_reduce(acc, sh_tri);
    if (tid == 0) {
        const bool any = acc.m > -INFINITY;
        const double lnz = any ? acc.m + log(acc.s) : -INFINITY;
        logz[s] = lnz;
        info[s] = any ? acc.a / acc.s - lnz : 0.0;
        sh_lnz = lnz;
    }
    if (!wout) return;
    __syncthreads();
    const double lnz = sh_lnz;
    for (long long t0 = 0; t0 < E; t0 += kTile)
        for (int k = 0; k < kPer; ++k) {
            const long long e = t0 + (long long)tid * kPer + k;
            if (e < E) {
                const int32_t i = ev[e];
                if (i >= 0) wout[i] -= lnz;
            }
        }
}

int check_common(const double* logl, const double* birth, int64_t n_rows, const int64_t* run_start, int32_t n_runs)
{
    if (n_runs < 1) return rvll::report_error(RVLL_E_INVALID, "n_runs must be >= 1");
    if (n_rows < 1 || n_rows > kMaxRows) return rvll::report_error(RVLL_E_INVALID, "n_rows must be in [1, %lld]", kMaxRows);
    if (!logl || !birth || !run_start) return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (run_start[0] != 0 || run_start[n_runs] != n_rows)
        return rvll::report_error(RVLL_E_INVALID, "run_start must run from 0 to n_rows = %lld", (long long)n_rows);
    for (int32_t r = 0; r < n_runs; ++r)
        if (run_start[r + 1] < run_start[r])
            return rvll::report_error(RVLL_E_INVALID, "run_start must be non-decreasing (run %d)", (int)r);
    for (int64_t i = 0; i < n_rows; ++i) {
        if (!std::isfinite(logl[i])) return rvll::report_error(RVLL_E_INVALID, "row %lld: log-L is not finite", (long long)i);
        if (std::isnan(birth[i])) return rvll::report_error(RVLL_E_INVALID, "row %lld: NaN birth", (long long)i);
    }
    return RVLL_OK;
}

// the whole call: checks done by the caller; nsamples replicates, or (merge != 0) the merged run with its order and counts
int run_merge(int32_t device, const double* logl, const double* birth, int64_t n, const int64_t* run_start, int32_t n_runs,
              int32_t nsamples, int expected, int bootstrap, uint64_t seed, double* logz, double* info, double* logwt,
              int64_t block_bytes, int64_t* order_out, int64_t* nlive_out, rvll_merge_timing* timing)
{
    const auto t_start = std::chrono::steady_clock::now();
    long long s_blk = std::min<long long>(nsamples, kMaxGroups);
    const long long bound = block_bytes > 0 ? block_bytes : kDefaultBlockBytes;
    if (logwt) {
        const long long per_rep = n * (long long)sizeof(double);
        if (per_rep > bound)
            return rvll::report_error(RVLL_E_NOMEM, "one replicate of the weights needs %lld bytes, above the device block "
                                      "bound of %lld", per_rep, bound);
        s_blk = std::min<long long>(s_blk, bound / per_rep);
    }
    int status = RVLL_OK;
    int prev_device = -1;
    double *d_logl = nullptr, *d_birth = nullptr, *d_L = nullptr, *d_logz = nullptr, *d_info = nullptr, *d_w = nullptr;
    u64 *d_kl = nullptr, *d_kb = nullptr, *d_sl = nullptr, *d_sb = nullptr;
    int32_t *d_idx = nullptr, *d_order = nullptr, *d_run = nullptr, *d_rb = nullptr, *d_rho = nullptr, *d_ev = nullptr;
    long long *d_rs = nullptr, *d_nlive = nullptr;
    void* d_temp = nullptr;
    size_t temp_bytes = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double kernel_ms = 0.;
    int launches = 0;
    const size_t shmem = bootstrap ? sizeof(int32_t) * (size_t)n_runs : 0;
    std::vector<int32_t> order32;

    {
        size_t b1 = 0;
        u64* k = nullptr;
        int32_t* o = nullptr;
        MRG_TRY(rocprim::radix_sort_pairs(nullptr, b1, k, k, o, o, (unsigned int)n, 0, 64, (hipStream_t) nullptr));
        temp_bytes = std::max<size_t>(b1, 1);
    }
    MRG_TRY(hipGetDevice(&prev_device));
    if (device >= 0) MRG_TRY(hipSetDevice(device));
    MRG_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) MRG_TRY(hipEventCreate(&e));
    // every device block before the first launch: running out of memory fails the call before any work
    MRG_TRY(hipMalloc(&d_logl, sizeof(double) * (size_t)n));
    MRG_TRY(hipMalloc(&d_birth, sizeof(double) * (size_t)n));
    MRG_TRY(hipMalloc(&d_L, sizeof(double) * (size_t)n));
    MRG_TRY(hipMalloc(&d_kl, sizeof(u64) * (size_t)n));
    MRG_TRY(hipMalloc(&d_kb, sizeof(u64) * (size_t)n));
    MRG_TRY(hipMalloc(&d_sl, sizeof(u64) * (size_t)n));
    MRG_TRY(hipMalloc(&d_sb, sizeof(u64) * (size_t)n));
    MRG_TRY(hipMalloc(&d_idx, sizeof(int32_t) * (size_t)n));
    MRG_TRY(hipMalloc(&d_order, sizeof(int32_t) * (size_t)n));
    MRG_TRY(hipMalloc(&d_run, sizeof(int32_t) * (size_t)n));
    MRG_TRY(hipMalloc(&d_rb, sizeof(int32_t) * (size_t)n));
    MRG_TRY(hipMalloc(&d_rho, sizeof(int32_t) * (size_t)n));
    MRG_TRY(hipMalloc(&d_ev, sizeof(int32_t) * (size_t)(2 * n)));
    MRG_TRY(hipMalloc(&d_nlive, sizeof(long long) * (size_t)n));
    MRG_TRY(hipMalloc(&d_rs, sizeof(long long) * (size_t)(n_runs + 1)));
    MRG_TRY(hipMalloc(&d_logz, sizeof(double) * (size_t)nsamples));
    MRG_TRY(hipMalloc(&d_info, sizeof(double) * (size_t)nsamples));
    if (logwt) MRG_TRY(hipMalloc(&d_w, sizeof(double) * (size_t)(s_blk * n)));
    MRG_TRY(hipMalloc(&d_temp, temp_bytes));
    MRG_TRY(hipMemcpyAsync(d_logl, logl, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_birth, birth, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_rs, run_start, sizeof(long long) * (size_t)(n_runs + 1), hipMemcpyHostToDevice, stream));

    MRG_TRY(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(keys_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, d_logl, d_birth, (long long)n, d_rs,
                       (int)n_runs, d_kl, d_kb, d_idx, d_run);
    MRG_TRY(hipGetLastError());
    MRG_TRY(rocprim::radix_sort_pairs(d_temp, temp_bytes, d_kl, d_sl, d_idx, d_order, (unsigned int)n, 0, 64, stream));
    MRG_TRY(rocprim::radix_sort_pairs(d_temp, temp_bytes, d_kb, d_sb, d_run, d_rb, (unsigned int)n, 0, 64, stream));
    hipLaunchKernelGGL(place_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, d_logl, d_sl, d_order, d_sb, d_rb,
                       d_run, (long long)n, d_L, d_rho, d_nlive, d_ev);
    MRG_TRY(hipGetLastError());
    MRG_TRY(hipEventRecord(ev[1], stream));
    launches += 4;
    MRG_TRY(hipEventSynchronize(ev[1]));
    {
        float ms = 0.f;
        MRG_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        kernel_ms += ms;
    }
    for (long long s0 = 0; s0 < nsamples; s0 += s_blk) {
        const long long sb = std::min<long long>(s_blk, nsamples - s0);
        MRG_TRY(hipEventRecord(ev[0], stream));
        hipLaunchKernelGGL(replicate_kernel, dim3((unsigned)sb), dim3(kThreads), shmem, stream, d_ev, d_L, d_rho, (long long)n,
                           (int)n_runs, (int)s0, (u64)seed, expected, bootstrap, d_logz, d_info, d_w);
        MRG_TRY(hipGetLastError());
        MRG_TRY(hipEventRecord(ev[1], stream));
        ++launches;
        if (d_w) MRG_TRY(hipMemcpyAsync(logwt + s0 * n, d_w, sizeof(double) * (size_t)(sb * n), hipMemcpyDeviceToHost, stream));
        MRG_TRY(hipEventSynchronize(ev[1]));
        float ms = 0.f;
        MRG_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        kernel_ms += ms;
    }
    MRG_TRY(hipMemcpyAsync(logz, d_logz, sizeof(double) * (size_t)nsamples, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(info, d_info, sizeof(double) * (size_t)nsamples, hipMemcpyDeviceToHost, stream));
    if (nlive_out) MRG_TRY(hipMemcpyAsync(nlive_out, d_nlive, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, stream));
    if (order_out) {
        order32.resize((size_t)n);
        MRG_TRY(hipMemcpyAsync(order32.data(), d_order, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    }
    MRG_TRY(hipStreamSynchronize(stream));
    if (order_out) std::copy(order32.begin(), order32.end(), order_out);
    if (timing) {
        timing->kernel_ms = kernel_ms;
        timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        timing->rows = n;
        timing->elements = n * (long long)nsamples;
        timing->launches = launches;
        timing->threads = kThreads;
    }

done:
    for (void* p : {(void*)d_logl, (void*)d_birth, (void*)d_L, (void*)d_logz, (void*)d_info, (void*)d_w, (void*)d_kl, (void*)d_kb,
                    (void*)d_sl, (void*)d_sb, (void*)d_idx, (void*)d_order, (void*)d_run, (void*)d_rb, (void*)d_rho, (void*)d_ev,
                    (void*)d_rs, (void*)d_nlive, d_temp})
        if (p) (void)hipFree(p);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (prev_device >= 0 && device >= 0) (void)hipSetDevice(prev_device);
    return status;
}

}  // namespace

extern "C" int rvll_merge_runs(int32_t device, const double* logl, const double* birth, int64_t n_rows, const int64_t* run_start,
                               int32_t n_runs, int64_t* order_out, int64_t* nlive_out, double* logz, double* info,
                               double* logwt_out, int64_t* n_off_contour, rvll_merge_timing* timing)
{
    const int rc = check_common(logl, birth, n_rows, run_start, n_runs);
    if (rc != RVLL_OK) return rc;
    if (!order_out || !nlive_out || !logz || !info || !logwt_out || !n_off_contour)
        return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (timing) *timing = rvll_merge_timing{0., 0., n_rows, n_rows, 0, kThreads};
    long long off = 0;
    for (int64_t i = 0; i < n_rows; ++i) off += logl[i] <= birth[i];
    *n_off_contour = off;
    return run_merge(device, logl, birth, n_rows, run_start, n_runs, 1, 1, 0, 0, logz, info, logwt_out, 0, order_out, nlive_out,
                     timing);
}

extern "C" int rvll_merge_replicates(int32_t device, const double* logl, const double* birth, int64_t n_rows,
                                     const int64_t* run_start, int32_t n_runs, int32_t nsamples, int32_t mode, int32_t bootstrap,
                                     uint64_t seed, double* logz, double* info, double* logwt, int64_t block_bytes,
                                     rvll_merge_timing* timing)
{
    const int rc = check_common(logl, birth, n_rows, run_start, n_runs);
    if (rc != RVLL_OK) return rc;
    if (nsamples < 1) return rvll::report_error(RVLL_E_INVALID, "nsamples must be >= 1");
    if (mode != RVLL_SHRINK_RANDOM && mode != RVLL_SHRINK_EXPECTED)
        return rvll::report_error(RVLL_E_INVALID, "mode %d is neither RVLL_SHRINK_RANDOM nor RVLL_SHRINK_EXPECTED", mode);
    if (bootstrap != 0 && bootstrap != 1) return rvll::report_error(RVLL_E_INVALID, "bootstrap must be 0 or 1");
    if (bootstrap && n_runs > kMaxBootRuns)
        return rvll::report_error(RVLL_E_INVALID, "the run bootstrap takes at most %d runs", kMaxBootRuns);
    if (block_bytes < 0) return rvll::report_error(RVLL_E_INVALID, "negative block_bytes");
    if (!logz || !info) return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (timing) *timing = rvll_merge_timing{0., 0., n_rows, 0, 0, kThreads};
    return run_merge(device, logl, birth, n_rows, run_start, n_runs, nsamples, mode == RVLL_SHRINK_EXPECTED ? 1 : 0, bootstrap,
                     seed, logz, info, logwt, block_bytes, nullptr, nullptr, timing);
}
