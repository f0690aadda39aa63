// Posterior summaries of the replicates of a merged run on gfx950: per replicate and per column of `values` the weighted mean,
// the weighted standard deviation about that mean and weighted quantiles (the inverted weighted CDF), reduced on the device
// from the weights that the replicate kernel of rvll_merge_setup.hip writes.  No weight leaves the device.
// evidence_amd/posterior.py holds the numpy definition; DESIGN §4k.
//
// Once per call:
//     setup     the merge's own (rvll_merge_setup.hip: keys, two sorts, place) -> the merged order and the event stream
//     permute   values [N, C] in input row order -> column-major [C, N] in merged order
//     columns   per column one rocPRIM radix sort of key_of(x) carrying the merged position -> perm_c, the column's rows by
//               value (stable: ties keep the merged order; the quantile does not depend on it)
// Per block of replicates (as many as fit the block bound next to the tables):
//     weights   replicate_kernel writes logw - lnZ into the replicate's slot; exp_kernel turns the block into p = exp(logwt)
//               in place (0 for rows without weight)
//     summary   one 256-thread workgroup per (replicate, column), three passes over the replicate's slot:
//               A  P = sum p and sum p (x - a), a = the column's midrange (fixed per call): mean = a + sum / P
//               B  sum p (x - mean)^2: the spread about the replicate's own mean, std = sqrt(sum / P)
//               C  walks perm_c in tiles of 1024 (lane t holds positions 4t .. 4t + 3), gathers p[perm_c[j]] and runs the
//                  inclusive scan of the replicate kernel's logX (64-lane shuffle scan, wave totals through LDS, compensated
//                  two-sum carry between tiles); level k is x at the first j whose running sum reaches q_k * P.  A tile is
//                  searched only when the running sum after it has reached a level not yet found (a uniform test), so all
//                  levels come out of the one pass, which ends when the last is found.  Should rounding leave a level above
//                  the last running sum (q within an ulp or two of 1), it takes the last row with weight.
// A and B give every lane four accumulators over the rows lane + 256 (4 m + k) in rising m, folded in the order k = 0 .. 3,
// then a 64-lane butterfly and the four waves in order: a fixed tree, no floating-point atomics.
//
// A (replicate, column) workgroup reads its replicate's slot and the per-call tables only, so its results depend on the input,
// the seed and the replicate's index: the same bits alone, in any batch, from call to call.
// The call itself (device, stream, buffers, blocks of replicates, timing) is rvll_merge_setup.h's Replicates.
#include "rvll_merge_setup.h"
#include <climits>

using namespace rvll::merge;

namespace {

constexpr int kMaxCols = 64;
constexpr int kMaxQ = 16;
constexpr int kAcc = 4;                                   // accumulators a lane keeps in passes A and B

__global__ __launch_bounds__(kThreads)
void permute_kernel(const double* __restrict__ vin, const int32_t* __restrict__ order, long long n, int ncols,
                    double* __restrict__ vals)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double* row = vin + (long long)order[i] * ncols;
        for (int c = 0; c < ncols; ++c) vals[(long long)c * n + i] = row[c];
    }
}

__global__ __launch_bounds__(kThreads)
void colkeys_kernel(const double* __restrict__ col, long long n, u64* __restrict__ keys)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
        keys[i] = rvll::key_of(col[i]);
}

__global__ __launch_bounds__(kThreads)
void exp_kernel(double* __restrict__ w, long long total)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads)
        w[i] = exp(w[i]);
}

template <bool kMin>
__device__ long long block_minmax(long long v, long long* sh)
{
    for (int off = 1; off < kWave; off <<= 1) {
        const long long o = __shfl_xor(v, off, kWave);
        v = kMin ? (o < v ? o : v) : (o > v ? o : v);
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    long long r = sh[0];
    for (int w = 1; w < kWaves; ++w) r = kMin ? (sh[w] < r ? sh[w] : r) : (sh[w] > r ? sh[w] : r);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kThreads) void summary_kernel(
    const double* __restrict__ pblock, const double* __restrict__ vals, const int32_t* __restrict__ perms, long long n, int ncols,
    const double* __restrict__ q, int nq, int s0, double* __restrict__ mean_out, double* __restrict__ std_out,
    double* __restrict__ quant_out)
{
    __shared__ double sh_d[kWaves];
    __shared__ long long sh_l[kWaves];
    __shared__ double sh_x[2][kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int sl = (int)(blockIdx.x / (unsigned)ncols), c = (int)(blockIdx.x % (unsigned)ncols);
    const long long s = (long long)s0 + sl;
    const double* __restrict__ p = pblock + (long long)sl * n;
    const double* __restrict__ x = vals + (long long)c * n;
    const int32_t* __restrict__ perm = perms + (long long)c * n;

    const double a = 0.5 * x[perm[0]] + 0.5 * x[perm[n - 1]];
    // pass A
    double ap[kAcc], ax[kAcc];
#pragma unroll
    for (int k = 0; k < kAcc; ++k) ap[k] = ax[k] = 0.0;
    for (long long i0 = tid; i0 < n; i0 += (long long)kThreads * kAcc) {
#pragma unroll
        for (int k = 0; k < kAcc; ++k) {
            const long long i = i0 + (long long)k * kThreads;
            if (i < n) {
                const double pi = p[i];
                ap[k] += pi;
                ax[k] += pi * (x[i] - a);
            }
        }
    }
    double tp = ap[0], tx = ax[0];
#pragma unroll
    for (int k = 1; k < kAcc; ++k) { tp += ap[k]; tx += ax[k]; }
    const double P = block_sum(tp, sh_d);
    const double mean = a + block_sum(tx, sh_d) / P;
    // pass B
#pragma unroll
    for (int k = 0; k < kAcc; ++k) ax[k] = 0.0;
    for (long long i0 = tid; i0 < n; i0 += (long long)kThreads * kAcc) {
#pragma unroll
        for (int k = 0; k < kAcc; ++k) {
            const long long i = i0 + (long long)k * kThreads;
            if (i < n) {
                const double d = x[i] - mean;
                ax[k] += p[i] * (d * d);
            }
        }
    }
    tx = ax[0];
#pragma unroll
    for (int k = 1; k < kAcc; ++k) tx += ax[k];
    const double var = block_sum(tx, sh_d) / P;
    if (tid == 0) {
        mean_out[s * ncols + c] = mean;
        std_out[s * ncols + c] = sqrt(var);
    }

    // pass C
    unsigned done = 0;
    const unsigned all = nq >= 32 ? 0xffffffffu : (1u << nq) - 1u;
    double carry_hi = 0.0, carry_lo = 0.0;
    long long lastpos = -1;
    int parity = 0;
    for (long long t0 = 0; t0 < n && done != all; t0 += kTile, parity ^= 1) {
        const long long j0 = t0 + (long long)tid * kPer;
        double pv[kPer], S[kPer];
        double xs = 0.0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const long long j = j0 + k;
            pv[k] = j < n ? p[perm[j]] : 0.0;
            if (pv[k] > 0.0) lastpos = j;
            xs += pv[k];
        }
        const double in_x = wave_scan(xs, lane);
        if (lane == kWave - 1) sh_x[parity][wave] = in_x;
        __syncthreads();
        double bx = 0.0, tot = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const double v = sh_x[parity][w];
            if (w < wave) bx += v;
            tot += v;
        }
        double loc = bx + (in_x - xs);
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            loc += pv[k];
            S[k] = carry_hi + (carry_lo + loc);
        }
        // two-sum of carry_hi + tot
        const double sum = carry_hi + tot, bv = sum - carry_hi;
        carry_lo += (carry_hi - (sum - bv)) + (tot - bv);
        carry_hi = sum;
        const double after = carry_hi + carry_lo;
        const bool last = t0 + kTile >= n;
        for (int k = 0; k < nq; ++k) {                    // uniform: `after`, `done` and q are the same in every thread
            if ((done >> k) & 1u) continue;
            const double t = q[k] * P;
            if (!(after >= t) && !last) continue;
            long long cand = LLONG_MAX;
#pragma unroll
            for (int e = kPer - 1; e >= 0; --e)
                if (j0 + e < n && S[e] >= t) cand = j0 + e;
            cand = block_minmax<true>(cand, sh_l);
            if (cand != LLONG_MAX) {
                done |= 1u << k;
                if (tid == 0) quant_out[(s * nq + k) * ncols + c] = x[perm[cand]];
            }
        }
    }
    if (done != all) {                                    // uniform
        const long long lp = block_minmax<false>(lastpos, sh_l);
        if (tid == 0)
            for (int k = 0; k < nq; ++k)
                if (!((done >> k) & 1u)) quant_out[(s * nq + k) * ncols + c] = lp >= 0 ? x[perm[lp]] : NAN;
    }
}

int run_posterior(int32_t device, const double* logl, const double* birth, int64_t n, const int64_t* run_start, int32_t n_runs,
                  const double* values, int32_t ncols, const double* quantiles, int32_t nq, int32_t nsamples, int expected,
                  int bootstrap, uint64_t seed, double* logz, double* info, double* mean, double* sd, double* quant,
                  int64_t block_bytes, rvll_posterior_timing* timing)
{
    const long long per_rep = n * (long long)sizeof(double);
    const long long tables = n * (long long)ncols * (long long)(sizeof(double) + sizeof(int32_t));
    char what[64];
    snprintf(what, sizeof what, "the tables of %d columns", (int)ncols);
    Replicates rep(device, logl, birth, n, run_start, n_runs, nsamples, expected, bootstrap, seed);
    MRG_OK(rep.plan_blocks(block_bytes, tables + kDefaultWeightBytes, tables, per_rep, kMaxGroups, what, "the weights"));
    double *d_vin = nullptr, *d_vals = nullptr, *d_q = nullptr, *d_mean = nullptr, *d_sd = nullptr, *d_quant = nullptr;
    int32_t* d_perm = nullptr;
    const size_t nc = (size_t)n * (size_t)ncols;
    const size_t sc = (size_t)nsamples * (size_t)ncols;

    MRG_OK(rep.begin());
    MergeSetup& su = rep.su;
    const hipStream_t stream = rep.stream;
    MRG_TRY(rep.alloc(d_mean, sc));
    MRG_TRY(rep.alloc(d_sd, sc));
    MRG_TRY(rep.alloc(d_quant, sc * nq));
    MRG_TRY(rep.alloc(d_q, (size_t)nq));
    MRG_TRY(rep.alloc(d_vals, nc));
    MRG_TRY(rep.alloc(d_perm, nc));
    MRG_TRY(rep.alloc(d_vin, nc));                         // the input's copy: freed once it is permuted
    MRG_TRY(hipMemcpyAsync(d_vin, values, sizeof(double) * nc, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_q, quantiles, sizeof(double) * (size_t)nq, hipMemcpyHostToDevice, stream));

    MRG_OK(rep.setup([&]() -> hipError_t {
        hipLaunchKernelGGL(permute_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, d_vin, su.order, (long long)n,
                           (int)ncols, d_vals);
        hipError_t e = hipGetLastError();
        ++rep.launches;
        for (int c = 0; c < ncols && e == hipSuccess; ++c) {   // su.kl / su.kb are free after the setup; su.idx holds 0 .. n - 1
            hipLaunchKernelGGL(colkeys_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, d_vals + (size_t)c * n,
                               (long long)n, su.kl);
            if ((e = hipGetLastError()) != hipSuccess) break;
            e = su.sort(su.kl, su.kb, su.idx, d_perm + (size_t)c * n, n, stream);
            rep.launches += 2;
        }
        return e;
    }));
    MRG_TRY(rep.free_now(d_vin));
    MRG_OK(rep.run_blocks(nullptr, [&](long long s0, long long sb, double* d_w, hipStream_t) -> hipError_t {
        hipLaunchKernelGGL(exp_kernel, dim3(blocks_for(sb * n, kThreads)), dim3(kThreads), 0, stream, d_w, sb * (long long)n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(summary_kernel, dim3((unsigned)(sb * ncols)), dim3(kThreads), 0, stream, d_w, d_vals, d_perm,
                           (long long)n, (int)ncols, d_q, (int)nq, (int)s0, d_mean, d_sd, d_quant);
        rep.launches += 2;
        return hipGetLastError();
    }, nullptr));
    MRG_TRY(hipMemcpyAsync(mean, d_mean, sizeof(double) * sc, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(sd, d_sd, sizeof(double) * sc, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(quant, d_quant, sizeof(double) * sc * nq, hipMemcpyDeviceToHost, stream));
    MRG_OK(rep.finish(logz, info));
    rep.report(timing);
    if (timing) {
        timing->threads = kThreads;
        timing->reserved = 0;
    }
    return RVLL_OK;
}

}  // namespace

extern "C" int rvll_posterior_replicates(int32_t device, const double* logl, const double* birth, int64_t n_rows,
                                         const int64_t* run_start, int32_t n_runs, const double* values, int32_t n_cols,
                                         const double* quantiles, int32_t n_q, int32_t nsamples, int32_t mode, int32_t bootstrap,
                                         uint64_t seed, double* logz, double* info, double* mean, double* sd, double* quant,
                                         int64_t block_bytes, rvll_posterior_timing* timing)
{
    MRG_OK(check_common(logl, birth, n_rows, run_start, n_runs));
    MRG_OK(check_replicate_args(nsamples, mode, bootstrap, n_runs, block_bytes));
    if (n_cols < 1 || n_cols > kMaxCols) return rvll::report_error(RVLL_E_INVALID, "n_cols must be in [1, %d]", kMaxCols);
    if (n_q < 1 || n_q > kMaxQ) return rvll::report_error(RVLL_E_INVALID, "n_q must be in [1, %d]", kMaxQ);
    if (!values || !quantiles || !logz || !info || !mean || !sd || !quant)
        return rvll::report_error(RVLL_E_INVALID, "null argument");
    for (int32_t k = 0; k < n_q; ++k)
        if (!(quantiles[k] > 0.0 && quantiles[k] < 1.0))
            return rvll::report_error(RVLL_E_INVALID, "quantile level %d is outside (0, 1)", (int)k);
    MRG_OK(check_finite_values(values, n_rows, n_cols));
    if (timing) *timing = rvll_posterior_timing{0., 0., 0., 0., 0., n_rows, 0, 0, kThreads, 0, 0};
    return run_posterior(device, logl, birth, n_rows, run_start, n_runs, values, n_cols, quantiles, n_q, nsamples,
                         mode == RVLL_SHRINK_EXPECTED ? 1 : 0, bootstrap, seed, logz, info, mean, sd, quant, block_bytes, timing);
}
