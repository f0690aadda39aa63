// The true inclusion probability (TIP) of every frequency bin, for every replicate of a merged run, on gfx950: the FIP periodogram
// of the merged runs of one planet model, reduced on the device from the weights that the replicate kernel of rvll_merge_setup.hip
// writes.  No weight leaves the device.  evidence_amd/fip.py (merged_tip_arrays) holds the numpy definition; DESIGN §4l.
//
// Row i of the merged run covers the union of the spans [beg, end) of its periods (the two binary searches of fip_index_kernel,
// rvll_fip_search.h), written as disjoint, non-touching intervals.  With p the replicate's weights and P their sum,
//     TIP[b] = (A[b] - E[b]) / P,   A[b] = sum of p over the intervals with beg <= b,   E[b] = the same with end <= b,
// and both are running sums over event lists that do not depend on the replicate.
//
// Once per call:
//     setup     the merge's own (rvll_merge_setup.hip: keys, two sorts, place) -> the merged order and the event stream
//     spans     one thread per merged row: the spans of its np <= 8 periods, sorted by beg and merged in registers, written as
//               np start keys and np end keys at e = i * np + k (an unused slot: the sentinel bin nfreq) with the position i
//     sorts     per list one stable rocPRIM radix sort over ceil(log2(nfreq + 1)) key bits: the events by (bin, merged position)
//     counts    per list and bin b the number of events with bin <= b (one binary search a bin).  cnt_A[b] - cnt_E[b] is the number
//               of intervals open at b: the exact test for an uncovered bin; cnt[b] - 1 is where the running sum is read
//     tiles     per list and tile of 1024 events the first bin whose read position is at or after the tile's start
// Per block of replicates (as many as fit the block bound next to the tables):
//     weights   replicate_kernel writes logw - lnZ into the replicate's slot
//     exp_sum   one workgroup per replicate: p = exp(logwt) in place (0 for rows without weight) and P, four accumulators a
//               lane, a 64-lane butterfly and the four waves in order (the tree of the posterior summaries' P)
//     coverage  one 256-thread workgroup per (replicate, list): walks the list in tiles of 1024 (lane t holds events 4t .. 4t + 3),
//               gathers p[position] and runs the inclusive scan of the replicate kernel's logX (64-lane shuffle scan, wave totals
//               through LDS, compensated two-sum carry between tiles; every partial sum is built from earlier entries only, so
//               it is good relative to itself however steeply the weights rise).  The tile's 1024 inclusive sums go to LDS, and the lanes
//               stride over the contiguous range of bins that read inside the tile (from the tile table) and store A or E for
//               them: an empty stretch of the periodogram is no lane's serial loop, and a peak of any height is 1024 events a tile
//     tip       TIP = clamp((A - E) / P) in place of A, 0 where the counts say that no interval is open, NaN without weight
// No floating-point atomics, fixed reduction trees.  A (replicate, list) workgroup reads its replicate's slot and the per-call
// tables only, so a replicate's bits depend on the input, the seed and its index: the same alone, in any batch, from call to call.
// The call itself (device, stream, buffers, blocks of replicates, timing) is rvll_merge_setup.h's Replicates.
#include "rvll_merge_setup.h"
#include "rvll_fip_search.h"
#include <climits>
#include <rocprim/rocprim.hpp>

using namespace rvll::merge;

namespace {

constexpr int kMaxPlanets = RVLL_FIP_MAX_PLANETS;
constexpr int kMaxFreq = 1 << 30;
constexpr int kAcc = 4;

// per merged row: the union of its spans as disjoint, non-touching intervals in rising order
template <int NP>
__global__ __launch_bounds__(kThreads)
void span_kernel(const double* __restrict__ periods, const int32_t* __restrict__ order, long long n,
                 const double* __restrict__ nua, const double* __restrict__ nub, int nfreq, uint32_t* __restrict__ key_a,
                 uint32_t* __restrict__ key_e, int32_t* __restrict__ pos)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double* row = periods + (long long)order[i] * NP;
        int beg[NP], end[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const double f = 6.283185307179586 / row[j];
            beg[j] = rvll::count_le(nub, nfreq, f);
            end[j] = rvll::count_lt(nua, nfreq, f);
            if (!(beg[j] < end[j])) beg[j] = end[j] = INT_MAX;            // empty: sorts behind every span
        }
        // odd-even transposition sort by beg: NP passes, every index a constant
#pragma unroll
        for (int pass = 0; pass < NP; ++pass) {
#pragma unroll
            for (int j = pass & 1; j + 1 < NP; j += 2) {
                const bool sw = beg[j + 1] < beg[j];
                const int b0 = sw ? beg[j + 1] : beg[j], b1 = sw ? beg[j] : beg[j + 1];
                const int e0 = sw ? end[j + 1] : end[j], e1 = sw ? end[j] : end[j + 1];
                beg[j] = b0; beg[j + 1] = b1; end[j] = e0; end[j + 1] = e1;
            }
        }
        const long long base = i * NP;
        int cnt = 0, cb = beg[0], ce = end[0];
#pragma unroll
        for (int j = 1; j < NP; ++j) {
            if (beg[j] == INT_MAX) continue;
            if (beg[j] <= ce) {                                           // overlapping or adjacent
                ce = max(ce, end[j]);
            } else {
                key_a[base + cnt] = (uint32_t)cb;
                key_e[base + cnt] = (uint32_t)ce;
                ++cnt;
                cb = beg[j];
                ce = end[j];
            }
        }
        if (cb != INT_MAX) {
            key_a[base + cnt] = (uint32_t)cb;
            key_e[base + cnt] = (uint32_t)ce;
            ++cnt;
        }
        for (int k = cnt; k < NP; ++k) key_a[base + k] = key_e[base + k] = (uint32_t)nfreq;
        for (int k = 0; k < NP; ++k) pos[base + k] = (int32_t)i;
    }
}

// cnt[b] = the number of sorted keys <= b
__global__ __launch_bounds__(kThreads)
void count_kernel(const uint32_t* __restrict__ sorted, long long m, int nfreq, int32_t* __restrict__ cnt)
{
    for (int b = blockIdx.x * kThreads + threadIdx.x; b < nfreq; b += gridDim.x * kThreads) {
        long long lo = 0, hi = m;
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (sorted[mid] <= (uint32_t)b) lo = mid + 1; else hi = mid;
        }
        cnt[b] = (int32_t)lo;
    }
}

// first[t] = the first bin b with cnt[b] >= t * kTile + 1 (nfreq when there is none), t = 0 .. ntiles
__global__ __launch_bounds__(kThreads)
void tile_kernel(const int32_t* __restrict__ cnt, int nfreq, long long ntiles, int32_t* __restrict__ first)
{
    for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t <= ntiles; t += (long long)gridDim.x * kThreads) {
        const long long want = t * kTile + 1;
        int lo = 0, hi = nfreq;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cnt[mid] < want) lo = mid + 1; else hi = mid;
        }
        first[t] = lo;
    }
}

__global__ __launch_bounds__(kThreads)
void exp_sum_kernel(double* __restrict__ wblock, long long n, int s0, double* __restrict__ psum)
{
    __shared__ double sh_d[kWaves];
    const int tid = threadIdx.x;
    double* __restrict__ p = wblock + (long long)blockIdx.x * n;
    double ap[kAcc];
#pragma unroll
    for (int k = 0; k < kAcc; ++k) ap[k] = 0.0;
    for (long long i0 = tid; i0 < n; i0 += (long long)kThreads * kAcc) {
#pragma unroll
        for (int k = 0; k < kAcc; ++k) {
            const long long i = i0 + (long long)k * kThreads;
            if (i < n) {
                const double pi = exp(p[i]);
                p[i] = pi;
                ap[k] += pi;
            }
        }
    }
    double tp = ap[0];
#pragma unroll
    for (int k = 1; k < kAcc; ++k) tp += ap[k];
    const double P = block_sum(tp, sh_d);
    if (tid == 0) psum[s0 + (int)blockIdx.x] = P;
}

__global__ __launch_bounds__(kThreads) void coverage_kernel(
    const double* __restrict__ pblock, long long n, const int32_t* __restrict__ pos_a, const int32_t* __restrict__ pos_e,
    const int32_t* __restrict__ cnt_a, const int32_t* __restrict__ cnt_e, const int32_t* __restrict__ first_a,
    const int32_t* __restrict__ first_e, int nfreq, double* __restrict__ out_a, double* __restrict__ out_e)
{
    __shared__ double sh_x[kWaves];
    __shared__ double sh_s[kTile];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int sl = (int)(blockIdx.x >> 1), list = (int)(blockIdx.x & 1u);
    const double* __restrict__ p = pblock + (long long)sl * n;
    const int32_t* __restrict__ pos = list ? pos_e : pos_a;
    const int32_t* __restrict__ cnt = list ? cnt_e : cnt_a;
    const int32_t* __restrict__ first = list ? first_e : first_a;
    double* __restrict__ out = (list ? out_e : out_a) + (long long)sl * nfreq;
    const long long m = cnt[nfreq - 1];                   // the events that a bin can read: those with bin <= nfreq - 1

    int blo = first[0];                                   // bins before the first event
    for (int b = tid; b < blo; b += kThreads) out[b] = 0.0;
    double carry_hi = 0.0, carry_lo = 0.0;
    long long t = 0;
    for (long long t0 = 0; t0 < m; t0 += kTile, ++t) {
        const long long j0 = t0 + (long long)tid * kPer;
        double pv[kPer];
        double xs = 0.0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const long long j = j0 + k;
            pv[k] = j < m ? p[pos[j]] : 0.0;
            xs += pv[k];
        }
        const int bhi = first[t + 1];
        const double in_x = wave_scan(xs, lane);
        // the sum before this lane, from the lane below: in_x - xs would carry the rounding of the lane's own entries, which
        // in a steep tail of the posterior are many orders above everything before them
        const double up = __shfl_up(in_x, 1, kWave);
        const double ex_x = lane ? up : 0.0;
        if (lane == kWave - 1) sh_x[wave] = in_x;
        __syncthreads();
        double bx = 0.0, tot = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const double v = sh_x[w];
            if (w < wave) bx += v;
            tot += v;
        }
        if (blo < bhi) {                                  // uniform: some bin reads inside this tile
            double loc = bx + ex_x;
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                loc += pv[k];
                sh_s[tid * kPer + k] = carry_hi + (carry_lo + loc);
            }
        }
        __syncthreads();
        for (int b = blo + tid; b < bhi; b += kThreads) out[b] = sh_s[(long long)cnt[b] - 1 - t0];
        blo = bhi;
        // two-sum of carry_hi + tot
        const double sum = carry_hi + tot, bv = sum - carry_hi;
        carry_lo += (carry_hi - (sum - bv)) + (tot - bv);
        carry_hi = sum;
    }
}

__global__ __launch_bounds__(kThreads)
void tip_kernel(double* __restrict__ a, const double* __restrict__ e, const double* __restrict__ psum,
                const int32_t* __restrict__ cnt_a, const int32_t* __restrict__ cnt_e, int nfreq, int s0, long long total)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const long long sl = i / nfreq;
        const int b = (int)(i - sl * nfreq);
        const double P = psum[s0 + sl];
        double v;
        if (!(P > 0.0)) v = NAN;
        else if (cnt_a[b] == cnt_e[b]) v = 0.0;
        else v = fmin(fmax((a[i] - e[i]) / P, 0.0), 1.0);
        a[i] = v;
    }
}

template <int NP>
hipError_t launch_spans(const double* periods, const int32_t* order, long long n, const double* nua, const double* nub, int nfreq,
                        uint32_t* key_a, uint32_t* key_e, int32_t* pos, hipStream_t s)
{
    hipLaunchKernelGGL(span_kernel<NP>, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, s, periods, order, n, nua, nub, nfreq,
                       key_a, key_e, pos);
    return hipGetLastError();
}

int run_fip(int32_t device, const double* logl, const double* birth, int64_t n, const int64_t* run_start, int32_t n_runs,
            const double* periods, int32_t np, const double* nua, const double* nub, int32_t nfreq, int32_t nsamples, int expected,
            int bootstrap, uint64_t seed, double* logz, double* info, double* tip, int64_t block_bytes, rvll_fip_merged_timing* timing)
{
    const long long m = n * (long long)np;                                // events a list
    const long long ntiles = (m + kTile - 1) / kTile;
    const long long per_rep = n * (long long)sizeof(double) + 2ll * nfreq * (long long)sizeof(double);
    const long long tables = 2 * m * (long long)sizeof(int32_t) + 2ll * nfreq * (long long)sizeof(int32_t) +
                             2 * (ntiles + 1) * (long long)sizeof(int32_t);
    Replicates rep(device, logl, birth, n, run_start, n_runs, nsamples, expected, bootstrap, seed);
    MRG_OK(rep.plan_blocks(block_bytes, tables + kDefaultWeightBytes, tables, per_rep, kMaxGroups, "the event tables",
                           "the weights and of A and E"));
    const long long s_blk = rep.s_blk;
    int key_bits = 1;
    while ((1ll << key_bits) <= (long long)nfreq) ++key_bits;             // ceil(log2(nfreq + 1))
    double *d_psum = nullptr, *d_a = nullptr, *d_e = nullptr, *d_periods = nullptr, *d_nua = nullptr, *d_nub = nullptr;
    uint32_t *d_key_a = nullptr, *d_key_e = nullptr, *d_key_s = nullptr;
    int32_t *d_pos = nullptr, *d_pos_a = nullptr, *d_pos_e = nullptr, *d_cnt_a = nullptr, *d_cnt_e = nullptr, *d_first_a = nullptr,
            *d_first_e = nullptr;
    char* d_temp = nullptr;
    size_t temp_bytes = 0;
    const size_t fbytes = sizeof(double) * (size_t)nfreq;

    MRG_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, d_key_a, d_key_s, d_pos, d_pos_a, (unsigned int)m, 0, key_bits,
                                      (hipStream_t) nullptr));
    temp_bytes = std::max<size_t>(temp_bytes, 1);
    MRG_OK(rep.begin());
    MergeSetup& su = rep.su;
    const hipStream_t stream = rep.stream;
    MRG_TRY(rep.alloc(d_psum, (size_t)nsamples));
    MRG_TRY(rep.alloc(d_nua, (size_t)nfreq));
    MRG_TRY(rep.alloc(d_nub, (size_t)nfreq));
    MRG_TRY(rep.alloc(d_pos_a, (size_t)m));
    MRG_TRY(rep.alloc(d_pos_e, (size_t)m));
    MRG_TRY(rep.alloc(d_cnt_a, (size_t)nfreq));
    MRG_TRY(rep.alloc(d_cnt_e, (size_t)nfreq));
    MRG_TRY(rep.alloc(d_first_a, (size_t)(ntiles + 1)));
    MRG_TRY(rep.alloc(d_first_e, (size_t)(ntiles + 1)));
    MRG_TRY(rep.alloc(d_a, (size_t)nfreq * (size_t)s_blk));
    MRG_TRY(rep.alloc(d_e, (size_t)nfreq * (size_t)s_blk));
    // what only the setup needs: freed before the first block of replicates
    MRG_TRY(rep.alloc(d_periods, (size_t)m));
    MRG_TRY(rep.alloc(d_key_a, (size_t)m));
    MRG_TRY(rep.alloc(d_key_e, (size_t)m));
    MRG_TRY(rep.alloc(d_key_s, (size_t)m));
    MRG_TRY(rep.alloc(d_pos, (size_t)m));
    MRG_TRY(rep.alloc(d_temp, temp_bytes));
    MRG_TRY(hipMemcpyAsync(d_periods, periods, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_nua, nua, fbytes, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_nub, nub, fbytes, hipMemcpyHostToDevice, stream));

    MRG_OK(rep.setup([&]() -> hipError_t {
        static constexpr decltype(&launch_spans<1>) spans[] = {launch_spans<1>, launch_spans<2>, launch_spans<3>, launch_spans<4>,
                                                               launch_spans<5>, launch_spans<6>, launch_spans<7>, launch_spans<8>};
        hipError_t e = spans[np - 1](d_periods, su.order, n, d_nua, d_nub, nfreq, d_key_a, d_key_e, d_pos, stream);
        ++rep.launches;
        for (int list = 0; list < 2 && e == hipSuccess; ++list) {
            int32_t* cnt = list ? d_cnt_e : d_cnt_a;
            e = rocprim::radix_sort_pairs(d_temp, temp_bytes, list ? d_key_e : d_key_a, d_key_s, d_pos, list ? d_pos_e : d_pos_a,
                                          (unsigned int)m, 0, key_bits, stream);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(count_kernel, dim3(blocks_for(nfreq, kThreads)), dim3(kThreads), 0, stream, d_key_s, m, (int)nfreq, cnt);
            if ((e = hipGetLastError()) != hipSuccess) break;
            hipLaunchKernelGGL(tile_kernel, dim3(blocks_for(ntiles + 1, kThreads)), dim3(kThreads), 0, stream, cnt, (int)nfreq, ntiles,
                               list ? d_first_e : d_first_a);
            e = hipGetLastError();
            rep.launches += 3;
        }
        return e;
    }));
    MRG_TRY(rep.free_now(d_periods));
    MRG_TRY(rep.free_now(d_key_a));
    MRG_TRY(rep.free_now(d_key_e));
    MRG_TRY(rep.free_now(d_key_s));
    MRG_TRY(rep.free_now(d_pos));
    MRG_TRY(rep.free_now(d_temp));
    MRG_OK(rep.run_blocks(nullptr, [&](long long s0, long long sb, double* d_w, hipStream_t) -> hipError_t {
        hipLaunchKernelGGL(exp_sum_kernel, dim3((unsigned)sb), dim3(kThreads), 0, stream, d_w, (long long)n, (int)s0, d_psum);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(coverage_kernel, dim3((unsigned)(2 * sb)), dim3(kThreads), 0, stream, d_w, (long long)n, d_pos_a, d_pos_e,
                           d_cnt_a, d_cnt_e, d_first_a, d_first_e, (int)nfreq, d_a, d_e);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(tip_kernel, dim3(blocks_for(sb * nfreq, kThreads)), dim3(kThreads), 0, stream, d_a, d_e, d_psum, d_cnt_a,
                           d_cnt_e, (int)nfreq, (int)s0, sb * (long long)nfreq);
        rep.launches += 3;
        return hipGetLastError();
    }, [&](long long s0, long long sb, double*, hipStream_t) {
        return hipMemcpyAsync(tip + s0 * (long long)nfreq, d_a, fbytes * (size_t)sb, hipMemcpyDeviceToHost, stream);
    }));
    MRG_OK(rep.finish(logz, info));
    rep.report(timing);
    if (timing) {
        timing->events = 2 * m;
        timing->threads = kThreads;
        timing->key_bits = key_bits;
    }
    return RVLL_OK;
}

}  // namespace

extern "C" int rvll_fip_replicates(int32_t device, const double* logl, const double* birth, int64_t n_rows, const int64_t* run_start,
                                   int32_t n_runs, const double* periods, int32_t n_planets, const double* nua, const double* nub,
                                   int32_t nfreq, int32_t nsamples, int32_t mode, int32_t bootstrap, uint64_t seed, double* logz,
                                   double* info, double* tip, int64_t block_bytes, rvll_fip_merged_timing* timing)
{
    MRG_OK(check_common(logl, birth, n_rows, run_start, n_runs));
    MRG_OK(check_replicate_args(nsamples, mode, bootstrap, n_runs, block_bytes));
    if (n_planets < 1 || n_planets > kMaxPlanets)
        return rvll::report_error(RVLL_E_INVALID, "n_planets must be in [1, %d]", kMaxPlanets);
    if (nfreq < 1 || nfreq > kMaxFreq) return rvll::report_error(RVLL_E_INVALID, "nfreq must be in [1, %d]", kMaxFreq);
    if (n_rows * (int64_t)n_planets > (int64_t)INT32_MAX)
        return rvll::report_error(RVLL_E_INVALID, "n_rows * n_planets must stay below 2^31");
    if (!periods || !nua || !nub || !logz || !info || !tip) return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (std::isnan(nua[0]) || std::isnan(nub[0])) return rvll::report_error(RVLL_E_INVALID, "nua / nub hold NaN");
    for (int32_t b = 1; b < nfreq; ++b)
        if (!(nua[b] >= nua[b - 1]) || !(nub[b] >= nub[b - 1]))
            return rvll::report_error(RVLL_E_INVALID, "nua and nub must be non-decreasing (bin %d)", (int)b);
    for (int64_t i = 0; i < n_rows * (int64_t)n_planets; ++i)
        if (!std::isfinite(periods[i]) || !(periods[i] > 0.0))
            return rvll::report_error(RVLL_E_INVALID, "row %lld, planet %lld: the period is not finite and positive",
                                      (long long)(i / n_planets), (long long)(i % n_planets));
    if (timing) *timing = rvll_fip_merged_timing{0., 0., 0., 0., 0., n_rows, 0, 0, 0, kThreads, 0, 0};
    return run_fip(device, logl, birth, n_rows, run_start, n_runs, periods, n_planets, nua, nub, nfreq, nsamples,
                   mode == RVLL_SHRINK_EXPECTED ? 1 : 0, bootstrap, seed, logz, info, tip, block_bytes, timing);
}
