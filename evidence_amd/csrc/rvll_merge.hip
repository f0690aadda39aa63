// Merging finished nested-sampling runs by their birth contours on gfx950, and replicates of the merged run (simulated
// shrinkage, optionally on top of a bootstrap of the runs).  evidence_amd/merge.py holds the numpy definition; DESIGN §4j.
// The kernels, the setup and the argument checks described here are in rvll_merge_setup.h, which rvll_posterior.hip shares.
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
#include "rvll_merge_setup.h"

namespace {

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
    double *d_logz = nullptr, *d_info = nullptr, *d_w = nullptr;
    MergeSetup su;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double kernel_ms = 0.;
    int launches = 0;
    const size_t shmem = bootstrap ? sizeof(int32_t) * (size_t)n_runs : 0;
    std::vector<int32_t> order32;

    MRG_TRY(su.query(n));
    MRG_TRY(hipGetDevice(&prev_device));
    if (device >= 0) MRG_TRY(hipSetDevice(device));
    MRG_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) MRG_TRY(hipEventCreate(&e));
    // every device block before the first launch: running out of memory fails the call before any work
    MRG_TRY(su.alloc(n, n_runs));
    MRG_TRY(hipMalloc(&d_logz, sizeof(double) * (size_t)nsamples));
    MRG_TRY(hipMalloc(&d_info, sizeof(double) * (size_t)nsamples));
    if (logwt) MRG_TRY(hipMalloc(&d_w, sizeof(double) * (size_t)(s_blk * n)));
    MRG_TRY(su.upload(logl, birth, run_start, n, n_runs, stream));

    MRG_TRY(hipEventRecord(ev[0], stream));
    MRG_TRY(su.launch(n, n_runs, stream));
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
        hipLaunchKernelGGL(replicate_kernel, dim3((unsigned)sb), dim3(kThreads), shmem, stream, su.ev, su.L, su.rho, (long long)n,
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
    if (nlive_out) MRG_TRY(hipMemcpyAsync(nlive_out, su.nlive, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, stream));
    if (order_out) {
        order32.resize((size_t)n);
        MRG_TRY(hipMemcpyAsync(order32.data(), su.order, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
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
    su.release();
    for (void* p : {(void*)d_logz, (void*)d_info, (void*)d_w})
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
