// Equal-weight draws of the replicates of a merged run on gfx950: per replicate ndraws rows of the input, drawn by systematic
// resampling from the weights that the replicate kernel of rvll_merge_setup.hip writes, with one uniform a replicate.  No weight
// leaves the device.  evidence_amd/draws.py holds the numpy definition; DESIGN §4o.
//
// Once per call:
//     setup     the merge's own (rvll_merge_setup.hip: keys, two sorts, place) -> the merged order
// Per block of replicates (as many as fit the block bound):
//     weights   replicate_kernel writes logw - lnZ into the replicate's slot
//     fixed     launch_fixed: every slot entry becomes m = rint(exp(logwt) 2^62) as int64 in place, M = sum m (§4m's integers)
//     scan      the inclusive int64 running sum C of every replicate's slots in place, reduce-then-scan in three launches:
//               sums of tiles of 1024 slots (one workgroup a tile), the inclusive scan of a replicate's tile sums (one workgroup
//               a replicate, 256 sums a step with a carry), and the scan inside every tile on top of the sum of the tiles before
//               it.  No workgroup waits for another: the launches are the only synchronisation.
//     pick      one thread per (replicate, draw k): Q = M / ndraws, O = (U Q) >> 53 from the high and the low word of the 116-bit
//               product, tau = k Q + O, and the first merged row with C > tau by a binary search of the tile sums and then of the
//               one tile; it writes that row's input row, or -1 throughout a replicate with M < ndraws.
// Every decision is an integer comparison on integer sums, so the rows do not depend on the tiling, the block bound or the other
// replicates of the call.  No floating-point atomics.
// The call itself (device, stream, buffers, blocks of replicates, timing) is rvll_merge_setup.h's Replicates.
#include "rvll_merge_setup.h"

using namespace rvll::merge;

namespace {

constexpr int kMaxDraws = 1 << 20;
constexpr long long kMaxBlockReps = 32768;                // grid y
constexpr unsigned long long kDrawXor = 0xA0761D6478BD642Full;   // the uniform of replicate s uses the seed seed_s ^ kDrawXor

// the 53-bit integer behind rvll::uniform01(seed, index), which returns it times 2^-53
__device__ __forceinline__ u64 uniform53(u64 seed, u64 index)
{
    u64 z = seed + 0x9E3779B97F4A7C15ull * (index + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return z >> 11;
}

// blockIdx.x: the tile, blockIdx.y: the replicate; tsum[replicate * ntiles + tile] = the sum of the tile's slots
__global__ __launch_bounds__(kThreads)
void tile_sum_kernel(const long long* __restrict__ slots, long long n, long long ntiles, long long* __restrict__ tsum)
{
    __shared__ long long sh[kWaves];
    const long long* __restrict__ m = slots + (long long)blockIdx.y * n;
    const long long i0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPer;
    long long acc = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (i0 + k < n) acc += m[i0 + k];
    acc = wave_sum(acc);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = sh[0];
        for (int k = 1; k < kWaves; ++k) t += sh[k];
        tsum[(long long)blockIdx.y * ntiles + blockIdx.x] = t;
    }
}

// one workgroup a replicate: its tile sums become their inclusive running sum, kThreads of them a step
__global__ __launch_bounds__(kThreads)
void tile_scan_kernel(long long* __restrict__ tsum, long long ntiles)
{
    __shared__ long long sh[2][kWaves];                   // alternating: a step's writes cannot meet the previous step's reads
    long long* __restrict__ t = tsum + (long long)blockIdx.x * ntiles;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    long long carry = 0;
    int parity = 0;
    for (long long base = 0; base < ntiles; base += kThreads, parity ^= 1) {    // uniform bounds: every thread meets the barrier
        const long long i = base + threadIdx.x;
        const long long v = i < ntiles ? t[i] : 0;
        const long long inc = wave_scan(v, lane);
        if (lane == kWave - 1) sh[parity][wave] = inc;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const long long a = sh[parity][w];
            if (w < wave) before += a;
            total += a;
        }
        if (i < ntiles) t[i] = carry + before + inc;
        carry += total;
    }
}

// blockIdx.x: the tile, blockIdx.y: the replicate; the tile's slots become C, on top of the scanned sum of the tiles before it
__global__ __launch_bounds__(kThreads)
void tile_add_kernel(long long* __restrict__ slots, long long n, long long ntiles, const long long* __restrict__ tsum)
{
    __shared__ long long sh[kWaves];
    long long* __restrict__ m = slots + (long long)blockIdx.y * n;
    const long long i0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPer;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    long long v[kPer];
    long long own = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        v[k] = i0 + k < n ? m[i0 + k] : 0;
        own += v[k];
    }
    const long long inc = wave_scan(own, lane);
    if (lane == kWave - 1) sh[wave] = inc;
    __syncthreads();
    long long run = blockIdx.x > 0 ? tsum[(long long)blockIdx.y * ntiles + blockIdx.x - 1] : 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) run += sh[w];
    run += inc - own;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        run += v[k];
        if (i0 + k < n) m[i0 + k] = run;
    }
}

// blockIdx.y: the replicate; one thread a draw
__global__ __launch_bounds__(kThreads)
void pick_kernel(const long long* __restrict__ slots, long long n, long long ntiles, const long long* __restrict__ tsum,
                 const int32_t* __restrict__ order, int ndraws, int s0, u64 seed, int32_t* __restrict__ rows)
{
    const int k = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (k >= ndraws) return;
    const long long* __restrict__ c = slots + (long long)blockIdx.y * n;
    const long long* __restrict__ t = tsum + (long long)blockIdx.y * ntiles;
    const u64 M = (u64)t[ntiles - 1];
    int32_t row = -1;
    if (M >= (u64)ndraws) {
        const u64 seed_s = seed + (u64)(s0 + (int)blockIdx.y) * kSeedMul;
        const u64 U = uniform53(seed_s ^ kDrawXor, 0);
        const u64 Q = M / (u64)ndraws;
        const u64 O = (__umul64hi(U, Q) << 11) | ((U * Q) >> 53);    // (U Q) >> 53 < Q: U < 2^53
        const long long tau = (long long)((u64)k * Q + O);           // < ndraws Q <= M: a tile and a row with C > tau exist
        long long lo = 0, hi = ntiles - 1;                           // the first tile whose scanned sum is above tau
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (t[mid] > tau) hi = mid; else lo = mid + 1;
        }
        const long long last = (lo + 1) * kTile < n ? (lo + 1) * kTile - 1 : n - 1;
        lo *= kTile;
        hi = last;                                                   // C[last] = t[tile] > tau
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (c[mid] > tau) hi = mid; else lo = mid + 1;
        }
        row = order[lo];
    }
    rows[(long long)blockIdx.y * ndraws + k] = row;
}

int run_draws(int32_t device, const double* logl, const double* birth, int64_t n, const int64_t* run_start, int32_t n_runs,
              int32_t ndraws, int32_t nsamples, int expected, int bootstrap, uint64_t seed, int32_t* rows, double* logz,
              double* info, int64_t* fixed, int64_t* msum, int64_t block_bytes, rvll_draw_timing* timing)
{
    const long long ntiles = (n + kTile - 1) / kTile;
    Replicates rep(device, logl, birth, n, run_start, n_runs, nsamples, expected, bootstrap, seed);
    MRG_OK(rep.plan_blocks(block_bytes, kDefaultWeightBytes, 0, n * (long long)sizeof(double), kMaxBlockReps, nullptr,
                           "the weights"));
    const long long s_blk = rep.s_blk;
    long long* d_tsum = nullptr;
    unsigned long long* d_msum = nullptr;
    int32_t* d_rows = nullptr;
    struct Events {                                       // the split of reduce_ms into scan and pick
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
    } events;
    hipEvent_t (&evs)[3] = events.e;
    float scan_ms = 0.f, pick_ms = 0.f;

    MRG_OK(rep.begin());
    const hipStream_t stream = rep.stream;
    MRG_TRY(rep.alloc(d_tsum, (size_t)(s_blk * ntiles)));
    MRG_TRY(rep.alloc(d_msum, (size_t)s_blk));
    MRG_TRY(rep.alloc(d_rows, (size_t)(s_blk * ndraws)));
    MRG_OK(rep.setup(nullptr));
    for (auto& e : evs) MRG_TRY(hipEventCreate(&e));
    const hipEvent_t ev_begin = evs[0], ev_scan = evs[1], ev_end = evs[2];
    MRG_OK(rep.run_blocks([&](long long, long long sb, double*, hipStream_t) -> hipError_t {
        return hipMemsetAsync(d_msum, 0, sizeof(unsigned long long) * (size_t)sb, stream);
    }, [&](long long s0, long long sb, double* d_w, hipStream_t) -> hipError_t {
        long long* slots = reinterpret_cast<long long*>(d_w);
        hipError_t e = hipEventRecord(ev_begin, stream);
        if (e != hipSuccess) return e;
        e = launch_fixed(d_w, (long long)n, sb, d_msum, stream);
        if (e != hipSuccess) return e;
        if (fixed) {                                      // m itself, before the scan overwrites it: a test's handle on the integers
            e = hipMemcpyAsync(fixed + s0 * n, d_w, sizeof(long long) * (size_t)(sb * n), hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) return e;
        }
        const dim3 tiles((unsigned)ntiles, (unsigned)sb);
        hipLaunchKernelGGL(tile_sum_kernel, tiles, dim3(kThreads), 0, stream, slots, (long long)n, ntiles, d_tsum);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(tile_scan_kernel, dim3((unsigned)sb), dim3(kThreads), 0, stream, d_tsum, ntiles);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(tile_add_kernel, tiles, dim3(kThreads), 0, stream, slots, (long long)n, ntiles, d_tsum);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(ev_scan, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(pick_kernel, dim3((unsigned)((ndraws + kThreads - 1) / kThreads), (unsigned)sb), dim3(kThreads), 0, stream,
                           slots, (long long)n, ntiles, d_tsum, rep.su.order, (int)ndraws, (int)s0, (u64)seed, d_rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        rep.launches += 5;
        return hipEventRecord(ev_end, stream);
    }, [&](long long s0, long long sb, double*, hipStream_t) -> hipError_t {
        hipError_t e = hipMemcpyAsync(rows + s0 * ndraws, d_rows, sizeof(int32_t) * (size_t)(sb * ndraws), hipMemcpyDeviceToHost,
                                      stream);
        if (e != hipSuccess) return e;
        if (msum) {
            e = hipMemcpyAsync(msum + s0, d_msum, sizeof(long long) * (size_t)sb, hipMemcpyDeviceToHost, stream);
            if (e != hipSuccess) return e;
        }
        if ((e = hipEventSynchronize(ev_end)) != hipSuccess) return e;
        float ms = 0.f;
        if ((e = hipEventElapsedTime(&ms, ev_begin, ev_scan)) != hipSuccess) return e;
        scan_ms += ms;
        if ((e = hipEventElapsedTime(&ms, ev_scan, ev_end)) != hipSuccess) return e;
        pick_ms += ms;
        return hipSuccess;
    }));
    MRG_OK(rep.finish(logz, info));
    rep.report(timing);
    if (timing) {
        timing->scan_ms = scan_ms;
        timing->pick_ms = pick_ms;
        timing->draws = (long long)ndraws * nsamples;
        timing->threads = kThreads;
        timing->tiles = (int32_t)ntiles;
    }
    return RVLL_OK;
}

}  // namespace

extern "C" int rvll_draw_replicates(int32_t device, const double* logl, const double* birth, int64_t n_rows,
                                    const int64_t* run_start, int32_t n_runs, int32_t ndraws, int32_t nsamples, int32_t mode,
                                    int32_t bootstrap, uint64_t seed, int32_t* rows, double* logz, double* info, int64_t* fixed,
                                    int64_t* msum, int64_t block_bytes, rvll_draw_timing* timing)
{
    MRG_OK(check_common(logl, birth, n_rows, run_start, n_runs));
    MRG_OK(check_replicate_args(nsamples, mode, bootstrap, n_runs, block_bytes));
    if (ndraws < 1 || ndraws > kMaxDraws) return rvll::report_error(RVLL_E_INVALID, "ndraws must be in [1, %d]", kMaxDraws);
    if (!rows || !logz || !info) return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (timing) *timing = rvll_draw_timing{0., 0., 0., 0., 0., 0., 0., n_rows, 0, 0, 0, kThreads, 0, 0};
    return run_draws(device, logl, birth, n_rows, run_start, n_runs, ndraws, nsamples, mode == RVLL_SHRINK_EXPECTED ? 1 : 0,
                     bootstrap, seed, rows, logz, info, fixed, msum, block_bytes, timing);
}
