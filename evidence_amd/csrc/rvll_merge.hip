// Merging finished nested-sampling runs by their birth contours on gfx950, and replicates of the merged run (simulated
// shrinkage, optionally on top of a bootstrap of the runs).  evidence_amd/merge.py holds the numpy definition; DESIGN §4j.
// The kernels, the setup and the argument checks described here are in rvll_merge_setup.hip, with the driver of a call
// (Replicates, declared in rvll_merge_setup.h) that the reducers of a merged run share: rvll_posterior.hip, rvll_fip_merged.hip
// and rvll_marginal.hip.
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

using namespace rvll::merge;

namespace {

// the whole call: checks done by the caller; nsamples replicates, or (merge != 0) the merged run with its order and counts
int run_merge(int32_t device, const double* logl, const double* birth, int64_t n, const int64_t* run_start, int32_t n_runs,
              int32_t nsamples, int expected, int bootstrap, uint64_t seed, double* logz, double* info, double* logwt,
              int64_t block_bytes, int64_t* order_out, int64_t* nlive_out, rvll_merge_timing* timing)
{
    Replicates rep(device, logl, birth, n, run_start, n_runs, nsamples, expected, bootstrap, seed);
    MRG_OK(rep.plan_blocks(block_bytes, kDefaultBlockBytes, 0, n * (long long)sizeof(double), kMaxGroups, nullptr, "the weights",
                           logwt != nullptr));
    std::vector<int32_t> order32;
    MRG_OK(rep.begin());
    MRG_OK(rep.setup(nullptr));
    Replicates::Step download;
    if (logwt)
        download = [&](long long s0, long long sb, double* d_w, hipStream_t stream) {
            return hipMemcpyAsync(logwt + s0 * n, d_w, sizeof(double) * (size_t)(sb * n), hipMemcpyDeviceToHost, stream);
        };
    MRG_OK(rep.run_blocks(nullptr, nullptr, download));
    if (nlive_out)
        MRG_TRY(hipMemcpyAsync(nlive_out, rep.su.nlive, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, rep.stream));
    if (order_out) {
        order32.resize((size_t)n);
        MRG_TRY(hipMemcpyAsync(order32.data(), rep.su.order, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, rep.stream));
    }
    MRG_OK(rep.finish(logz, info));
    if (order_out) std::copy(order32.begin(), order32.end(), order_out);
    if (timing) {
        timing->kernel_ms = rep.setup_ms + rep.weights_ms;
        timing->total_ms = rep.elapsed_ms();
        timing->rows = n;
        timing->elements = n * (long long)nsamples;
        timing->launches = rep.launches;
        timing->threads = kThreads;
    }
    return RVLL_OK;
}

}  // namespace

extern "C" int rvll_merge_runs(int32_t device, const double* logl, const double* birth, int64_t n_rows, const int64_t* run_start,
                               int32_t n_runs, int64_t* order_out, int64_t* nlive_out, double* logz, double* info,
                               double* logwt_out, int64_t* n_off_contour, rvll_merge_timing* timing)
{
    MRG_OK(check_common(logl, birth, n_rows, run_start, n_runs));
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
    MRG_OK(check_common(logl, birth, n_rows, run_start, n_runs));
    MRG_OK(check_replicate_args(nsamples, mode, bootstrap, n_runs, block_bytes));
    if (!logz || !info) return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (timing) *timing = rvll_merge_timing{0., 0., n_rows, 0, 0, kThreads};
    return run_merge(device, logl, birth, n_rows, run_start, n_runs, nsamples, mode == RVLL_SHRINK_EXPECTED ? 1 : 0, bootstrap,
                     seed, logz, info, logwt, block_bytes, nullptr, nullptr, timing);
}
