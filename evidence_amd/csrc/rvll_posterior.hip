// Posterior summaries of the replicates of a merged run on gfx950: per replicate and per column of `values` the weighted mean,
// the weighted standard deviation about that mean and weighted quantiles (the inverted weighted CDF), reduced on the device
// from the weights that the replicate kernel of rvll_merge_setup.h writes.  No weight leaves the device.
// evidence_amd/posterior.py holds the numpy definition; DESIGN §4k.
//
// Once per call:
//     setup     the merge's own (rvll_merge_setup.h: keys, two sorts, place) -> the merged order and the event stream
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
#include "rvll_merge_setup.h"
#include <climits>

namespace {

constexpr int kMaxCols = 64;
constexpr int kMaxQ = 16;
// The default block of weights.  A block holds bound / (8 N) replicates and the replicate kernel runs one workgroup a replicate, so a
// small block leaves most of the device idle: at 2.6e6 rows, 512 MiB (24 replicates) took 2.8 s for the weights of 1000 replicates
// and 8 GiB 0.24 s (profiles/posterior_probe.txt).  Only min(nsamples, bound / (8 N)) replicates are allocated.
constexpr long long kDefaultWeightBytes = 8ll << 30;
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

// the sum of v over the workgroup, in every thread: butterfly inside a wave, then the waves in order
__device__ double block_sum(double v, double* sh)
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
    const auto t_start = std::chrono::steady_clock::now();
    const long long per_rep = n * (long long)sizeof(double);
    const long long tables = n * (long long)ncols * (long long)(sizeof(double) + sizeof(int32_t));
    const long long bound = block_bytes > 0 ? block_bytes : tables + kDefaultWeightBytes;
    if (tables + per_rep > bound)
        return rvll::report_error(RVLL_E_NOMEM, "the tables of %d columns (%lld bytes) and one replicate of the weights (%lld "
                                  "bytes) are above the device block bound of %lld", (int)ncols, tables, per_rep, bound);
    const long long s_blk = std::min<long long>(std::min<long long>(nsamples, kMaxGroups), (bound - tables) / per_rep);
    int status = RVLL_OK;
    int prev_device = -1;
    double *d_logz = nullptr, *d_info = nullptr, *d_w = nullptr, *d_vin = nullptr, *d_vals = nullptr, *d_q = nullptr;
    double *d_mean = nullptr, *d_sd = nullptr, *d_quant = nullptr;
    int32_t* d_perm = nullptr;
    MergeSetup su;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double setup_ms = 0., weights_ms = 0., reduce_ms = 0.;
    int launches = 0, blocks = 0;
    const size_t shmem = bootstrap ? sizeof(int32_t) * (size_t)n_runs : 0;
    const size_t nc = (size_t)n * (size_t)ncols;

    MRG_TRY(su.query(n));
    MRG_TRY(hipGetDevice(&prev_device));
    if (device >= 0) MRG_TRY(hipSetDevice(device));
    MRG_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) MRG_TRY(hipEventCreate(&e));
    // every device block before the first launch: running out of memory fails the call before any work
    MRG_TRY(su.alloc(n, n_runs));
    MRG_TRY(hipMalloc(&d_logz, sizeof(double) * (size_t)nsamples));
    MRG_TRY(hipMalloc(&d_info, sizeof(double) * (size_t)nsamples));
    MRG_TRY(hipMalloc(&d_mean, sizeof(double) * (size_t)nsamples * ncols));
    MRG_TRY(hipMalloc(&d_sd, sizeof(double) * (size_t)nsamples * ncols));
    MRG_TRY(hipMalloc(&d_quant, sizeof(double) * (size_t)nsamples * ncols * nq));
    MRG_TRY(hipMalloc(&d_q, sizeof(double) * (size_t)nq));
    MRG_TRY(hipMalloc(&d_vals, sizeof(double) * nc));
    MRG_TRY(hipMalloc(&d_perm, sizeof(int32_t) * nc));
    MRG_TRY(hipMalloc(&d_w, sizeof(double) * (size_t)(s_blk * n)));
    MRG_TRY(hipMalloc(&d_vin, sizeof(double) * nc));       // the input's copy: freed once it is permuted
    MRG_TRY(su.upload(logl, birth, run_start, n, n_runs, stream));
    MRG_TRY(hipMemcpyAsync(d_vin, values, sizeof(double) * nc, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_q, quantiles, sizeof(double) * (size_t)nq, hipMemcpyHostToDevice, stream));

    MRG_TRY(hipEventRecord(ev[0], stream));
    MRG_TRY(su.launch(n, n_runs, stream));
    hipLaunchKernelGGL(permute_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, d_vin, su.order, (long long)n,
                       (int)ncols, d_vals);
    MRG_TRY(hipGetLastError());
    launches += 5;
    for (int c = 0; c < ncols; ++c) {                     // su.kl / su.kb are free after the setup; su.idx holds 0 .. n - 1
        hipLaunchKernelGGL(colkeys_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, d_vals + (size_t)c * n,
                           (long long)n, su.kl);
        MRG_TRY(hipGetLastError());
        MRG_TRY(rocprim::radix_sort_pairs(su.temp, su.temp_bytes, su.kl, su.kb, su.idx, d_perm + (size_t)c * n, (unsigned int)n, 0,
                                          64, stream));
        launches += 2;
    }
    MRG_TRY(hipEventRecord(ev[1], stream));
    MRG_TRY(hipEventSynchronize(ev[1]));
    {
        float ms = 0.f;
        MRG_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        setup_ms += ms;
    }
    MRG_TRY(hipFree(d_vin));
    d_vin = nullptr;
    for (long long s0 = 0; s0 < nsamples; s0 += s_blk) {
        const long long sb = std::min<long long>(s_blk, nsamples - s0);
        MRG_TRY(hipEventRecord(ev[0], stream));
        hipLaunchKernelGGL(replicate_kernel, dim3((unsigned)sb), dim3(kThreads), shmem, stream, su.ev, su.L, su.rho, (long long)n,
                           (int)n_runs, (int)s0, (u64)seed, expected, bootstrap, d_logz, d_info, d_w);
        MRG_TRY(hipGetLastError());
        MRG_TRY(hipEventRecord(ev[1], stream));
        hipLaunchKernelGGL(exp_kernel, dim3(blocks_for(sb * n, kThreads)), dim3(kThreads), 0, stream, d_w, sb * (long long)n);
        MRG_TRY(hipGetLastError());
        hipLaunchKernelGGL(summary_kernel, dim3((unsigned)(sb * ncols)), dim3(kThreads), 0, stream, d_w, d_vals, d_perm,
                           (long long)n, (int)ncols, d_q, (int)nq, (int)s0, d_mean, d_sd, d_quant);
        MRG_TRY(hipGetLastError());
        MRG_TRY(hipEventRecord(ev[2], stream));
        launches += 3;
        ++blocks;
        MRG_TRY(hipEventSynchronize(ev[2]));
        float ms = 0.f;
        MRG_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        weights_ms += ms;
        MRG_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
        reduce_ms += ms;
    }
    MRG_TRY(hipMemcpyAsync(logz, d_logz, sizeof(double) * (size_t)nsamples, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(info, d_info, sizeof(double) * (size_t)nsamples, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(mean, d_mean, sizeof(double) * (size_t)nsamples * ncols, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(sd, d_sd, sizeof(double) * (size_t)nsamples * ncols, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(quant, d_quant, sizeof(double) * (size_t)nsamples * ncols * nq, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipStreamSynchronize(stream));
    if (timing) {
        timing->kernel_ms = setup_ms + weights_ms + reduce_ms;
        timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        timing->setup_ms = setup_ms;
        timing->weights_ms = weights_ms;
        timing->reduce_ms = reduce_ms;
        timing->rows = n;
        timing->elements = n * (long long)nsamples;
        timing->launches = launches;
        timing->threads = kThreads;
        timing->blocks = blocks;
        timing->reserved = 0;
    }

done:
    su.release();
    for (void* p : {(void*)d_logz, (void*)d_info, (void*)d_w, (void*)d_vin, (void*)d_vals, (void*)d_q, (void*)d_mean, (void*)d_sd,
                    (void*)d_quant, (void*)d_perm})
        if (p) (void)hipFree(p);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (prev_device >= 0 && device >= 0) (void)hipSetDevice(prev_device);
    return status;
}

}  // namespace

extern "C" int rvll_posterior_replicates(int32_t device, const double* logl, const double* birth, int64_t n_rows,
                                         const int64_t* run_start, int32_t n_runs, const double* values, int32_t n_cols,
                                         const double* quantiles, int32_t n_q, int32_t nsamples, int32_t mode, int32_t bootstrap,
                                         uint64_t seed, double* logz, double* info, double* mean, double* sd, double* quant,
                                         int64_t block_bytes, rvll_posterior_timing* timing)
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
    if (n_cols < 1 || n_cols > kMaxCols) return rvll::report_error(RVLL_E_INVALID, "n_cols must be in [1, %d]", kMaxCols);
    if (n_q < 1 || n_q > kMaxQ) return rvll::report_error(RVLL_E_INVALID, "n_q must be in [1, %d]", kMaxQ);
    if (!values || !quantiles || !logz || !info || !mean || !sd || !quant)
        return rvll::report_error(RVLL_E_INVALID, "null argument");
    for (int32_t k = 0; k < n_q; ++k)
        if (!(quantiles[k] > 0.0 && quantiles[k] < 1.0))
            return rvll::report_error(RVLL_E_INVALID, "quantile level %d is outside (0, 1)", (int)k);
    for (int64_t i = 0; i < n_rows * (int64_t)n_cols; ++i)
        if (!std::isfinite(values[i]))
            return rvll::report_error(RVLL_E_INVALID, "row %lld, column %lld: value is not finite", (long long)(i / n_cols),
                                      (long long)(i % n_cols));
    if (timing) *timing = rvll_posterior_timing{0., 0., 0., 0., 0., n_rows, 0, 0, kThreads, 0, 0};
    return run_posterior(device, logl, birth, n_rows, run_start, n_runs, values, n_cols, quantiles, n_q, nsamples,
                         mode == RVLL_SHRINK_EXPECTED ? 1 : 0, bootstrap, seed, logz, info, mean, sd, quant, block_bytes, timing);
}
