// Marginal posterior histograms of the replicates of a merged run on gfx950: per replicate the posterior mass of every bin of a
// list of 1-D and 2-D panels, and per bin the mean, standard deviation, minimum and maximum of that mass over the replicates,
// reduced on the device from the weights that the replicate kernel of rvll_merge_setup.hip writes.  No weight leaves the device.
// evidence_amd/marginals.py holds the numpy definition; DESIGN §4m.
//
// Once per call:
//     setup     the merge's own (rvll_merge_setup.hip: keys, two sorts, place) -> the merged order
//     bin       one thread per (merged row, axis): the binary search of the axis's edges by numpy's histogram convention
//               (searchsorted(edges, x, "right") - 1, the last edge belongs to the last bin) -> a uint16 bin index, 0xFFFF for a
//               row outside, in an axis-major table in merged order (2 N n_axes bytes).  The bin of a row does not depend on the
//               replicate, so nothing below gathers: weights and bin indices are both streamed in merged order.
//     count     hist_kernel with the weight 1 -> counts and outside_count
// Per block of replicates (as many as fit the block bound next to the table):
//     weights   replicate_kernel writes logw - lnZ into the replicate's slot
//     fixed     every slot entry becomes m = rint(exp(logwt) 2^62) as int64 in place (0 for a row without weight); M = sum m
//               per replicate by integer adds (shuffles, LDS, one 64-bit integer atomic a workgroup): launch_fixed of
//               rvll_merge_setup.hip, which rvll_draws.hip shares
//     hist      one 512-thread workgroup per (replicate, panel group, row chunk): an int64 histogram of the group's panels in
//               LDS (a panel's bins and one entry for its outside rows; panels are packed into a group while 8192 entries, 64
//               KiB, allow), accumulated with 64-bit integer LDS atomics and flushed with 64-bit integer global atomics into
//               the replicate's h, zero entries skipped.  A lane loads four rows at a time; rows with m = 0 are skipped.
//               RVLL_MARGINAL_WAVE_REDUCE=1 in the environment selects a variant in which a wave whose weighted rows all land
//               in one entry adds them by shuffles and issues one atomic; on 51 Peg it was slower, so it is off.
//     stats     one thread per bin: mass = (double)h / (double)M (NaN where M = 0), stored if asked for, and the Welford update
//               of (n, mean, m2, min, max) replicate by replicate in order; the state lives in global memory across blocks.
// Every sum over rows is an integer sum and the sum over replicates is sequential, so the bits do not depend on the grouping of
// panels, the chunking of rows, the block bound, the other panels or the other replicates of the call.  No floating-point
// atomics.
// The call itself (device, stream, buffers, blocks of replicates, timing) is rvll_merge_setup.h's Replicates.
#include "rvll_merge_setup.h"
#include <cstdlib>

using namespace rvll::merge;

namespace {

constexpr int kMaxCols = 64;
constexpr int kMaxAxes = 128;
constexpr int kMaxPanels = 256;
constexpr int kMaxAxisBins = 4096;
constexpr int kMaxPanelBins = 4096;
constexpr int kHistThreads = 512;
constexpr int kHistRows = 4;                              // rows a lane loads before it bins them
constexpr int kGroupEntries = 8192;                       // int64 entries of LDS a workgroup may hold: 64 KiB
constexpr unsigned kOutsideBin = 0xFFFFu;
constexpr long long kMinChunkRows = 1024;                 // chunks shrink to this only while the launch is short of workgroups
constexpr long long kTargetGroups = 4096;                 // workgroups a hist launch aims at
constexpr long long kMaxBlockReps = 32768;                // grid y

struct Panel {
    int32_t a, b;            // axes; b = -1: one-dimensional
    int32_t nb_b;            // bins of axis b (1 for a 1-D panel)
    int32_t nbins;
    int32_t lds_off;         // first entry inside the group's LDS image; entry lds_off + nbins counts the outside rows
    int32_t start;           // first bin in the flat bin array
    int32_t index;           // the panel's own index: its outside entry is n_bins_total + index
    int32_t pad;
};

__global__ __launch_bounds__(kThreads)
void bin_kernel(const double* __restrict__ vin, const int32_t* __restrict__ order, long long n, int ncols, int naxes,
                const double* __restrict__ edges, const int32_t* __restrict__ axis_col, const long long* __restrict__ axis_start,
                uint16_t* __restrict__ bins)
{
    const long long total = n * (long long)naxes;
    for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long long)gridDim.x * kThreads) {
        const int a = (int)(t / n);
        const long long i = t - (long long)a * n;
        const double x = vin[(long long)order[i] * ncols + axis_col[a]];
        const double* __restrict__ e = edges + axis_start[a];
        const int ne = (int)(axis_start[a + 1] - axis_start[a]);
        int lo = 0, hi = ne;                              // the number of edges <= x
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (e[mid] <= x) lo = mid + 1; else hi = mid;
        }
        unsigned j = kOutsideBin;
        if (lo >= 1 && x <= e[ne - 1]) j = (unsigned)(lo == ne ? ne - 2 : lo - 1);
        bins[t] = (uint16_t)j;
    }
}

// kUnit: every row weighs 1 (the counts); kWaveReduce: one atomic a wave where its weighted rows share the entry
template <bool kUnit, bool kWaveReduce>
__global__ __launch_bounds__(kHistThreads)
void hist_kernel(const long long* __restrict__ slots, const uint16_t* __restrict__ bins, long long n,
                 const Panel* __restrict__ panels, const int32_t* __restrict__ group_first, int ngroups, long long chunk_rows,
                 long long nbins_total, long long nentries, unsigned long long* __restrict__ h)
{
    extern __shared__ unsigned long long sh_h[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int g = (int)(blockIdx.x % (unsigned)ngroups);
    const long long chunk = blockIdx.x / (unsigned)ngroups;
    const int p0 = group_first[g], p1 = group_first[g + 1];
    const int entries = panels[p1 - 1].lds_off + panels[p1 - 1].nbins + 1;
    for (int e = tid; e < entries; e += kHistThreads) sh_h[e] = 0ull;
    __syncthreads();
    const long long r0 = chunk * chunk_rows, r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
    const long long* __restrict__ m = kUnit ? nullptr : slots + (long long)blockIdx.y * n;
    for (long long i0 = r0; i0 < r1; i0 += (long long)kHistThreads * kHistRows) {   // uniform bounds: no lane leaves the loop early
        long long mk[kHistRows];
#pragma unroll
        for (int k = 0; k < kHistRows; ++k) {                            // the loads of kHistRows rows a lane are in flight together
            const long long i = i0 + (long long)k * kHistThreads + tid;
            mk[k] = i < r1 ? (kUnit ? 1ll : m[i]) : 0ll;
        }
#pragma unroll
        for (int k = 0; k < kHistRows; ++k) {
            const long long i = i0 + (long long)k * kHistThreads + tid;
            const long long mi = mk[k];
            const unsigned long long has = __ballot(mi != 0);
            if (has == 0ull) continue;
            const int lead = __ffsll((unsigned long long)has) - 1;
            long long wsum = 0;
            if (kWaveReduce) wsum = wave_sum(mi);
            for (int p = p0; p < p1; ++p) {
                const Panel d = panels[p];
                int e = -1;
                if (mi != 0) {
                    e = d.lds_off + d.nbins;
                    const unsigned ja = bins[(long long)d.a * n + i];
                    if (ja != kOutsideBin) {
                        if (d.b < 0) {
                            e = d.lds_off + (int)ja;
                        } else {
                            const unsigned jb = bins[(long long)d.b * n + i];
                            if (jb != kOutsideBin) e = d.lds_off + (int)ja * d.nb_b + (int)jb;
                        }
                    }
                }
                if (kWaveReduce) {
                    const int e_ref = __shfl(e, lead, kWave);
                    if (__all(e < 0 || e == e_ref)) {
                        if (lane == lead) atomicAdd(&sh_h[e_ref], (unsigned long long)wsum);
                        continue;
                    }
                }
                if (e >= 0) atomicAdd(&sh_h[e], (unsigned long long)mi);
            }
        }
    }
    __syncthreads();
    unsigned long long* __restrict__ out = h + (long long)blockIdx.y * nentries;
    for (int p = p0; p < p1; ++p) {
        const Panel d = panels[p];
        for (int e = tid; e <= d.nbins; e += kHistThreads) {
            const unsigned long long v = sh_h[d.lds_off + e];
            if (v != 0ull) atomicAdd(&out[e < d.nbins ? (long long)d.start + e : nbins_total + d.index], v);
        }
    }
}

// state: n, mean, m2, min, max, each [nbins]
__global__ __launch_bounds__(kThreads)
void stats_kernel(const unsigned long long* __restrict__ h, const unsigned long long* __restrict__ msum, long long nbins,
                  long long nentries, int sb, double* __restrict__ state, double* __restrict__ mass, double* __restrict__ outside)
{
    const long long b = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (b >= nentries) return;
    const bool bin = b < nbins;
    double cnt = 0., mean = 0., m2 = 0., mn = 0., mx = 0.;
    if (bin) {
        cnt = state[b];
        mean = state[nbins + b];
        m2 = state[2 * nbins + b];
        mn = state[3 * nbins + b];
        mx = state[4 * nbins + b];
    }
    for (int sl = 0; sl < sb; ++sl) {
        const long long M = (long long)msum[sl];
        const double x = M == 0 ? NAN : (double)(long long)h[(long long)sl * nentries + b] / (double)M;
        if (bin) {
            if (mass) mass[(long long)sl * nbins + b] = x;
            if (M != 0) {
                cnt += 1.0;
                const double d = x - mean;
                mean += d / cnt;
                m2 += d * (x - mean);
                mn = x < mn ? x : mn;
                mx = x > mx ? x : mx;
            }
        } else if (outside) {
            outside[(long long)sl * (nentries - nbins) + (b - nbins)] = x;
        }
    }
    if (bin) {
        state[b] = cnt;
        state[nbins + b] = mean;
        state[2 * nbins + b] = m2;
        state[3 * nbins + b] = mn;
        state[4 * nbins + b] = mx;
    }
}

struct Plan {
    std::vector<Panel> panels;
    std::vector<int32_t> group_first;
    std::vector<long long> axis_start;
    long long nbins = 0;
    int max_entries = 0;
};

template <bool kUnit>
hipError_t launch_hist(bool wave_reduce, dim3 grid, size_t lds, hipStream_t stream, const long long* slots, const uint16_t* bins,
                       long long n, const Panel* panels, const int32_t* group_first, int ngroups, long long chunk_rows,
                       long long nbins, long long nentries, unsigned long long* h)
{
    if (wave_reduce)
        hipLaunchKernelGGL((hist_kernel<kUnit, true>), grid, dim3(kHistThreads), lds, stream, slots, bins, n, panels, group_first,
                           ngroups, chunk_rows, nbins, nentries, h);
    else
        hipLaunchKernelGGL((hist_kernel<kUnit, false>), grid, dim3(kHistThreads), lds, stream, slots, bins, n, panels, group_first,
                           ngroups, chunk_rows, nbins, nentries, h);
    return hipGetLastError();
}

// rows a workgroup walks: enough workgroups to fill the device, chunks long enough to pay for zeroing and flushing the image
long long chunk_rows_for(long long n, long long groups, long long reps)
{
    long long chunks = (kTargetGroups + groups * reps - 1) / (groups * reps);
    const long long most = (n + kMinChunkRows - 1) / kMinChunkRows;
    chunks = std::max<long long>(1, std::min(chunks, most));
    const long long rows = (n + chunks - 1) / chunks;
    return (rows + kHistThreads - 1) / kHistThreads * kHistThreads;
}

int run_marginal(int32_t device, const double* logl, const double* birth, int64_t n, const int64_t* run_start, int32_t n_runs,
                 const double* values, int32_t ncols, const double* edges, const int32_t* axis_col, int32_t n_axes,
                 const Plan& plan, int32_t n_panels, int32_t nsamples, int expected, int bootstrap, uint64_t seed, double* logz,
                 double* info, int64_t* counts, int64_t* outside_count, double* stats, double* mass, double* outside,
                 int64_t block_bytes, rvll_marginal_timing* timing)
{
    const long long nbins = plan.nbins, nentries = nbins + n_panels;
    const long long per_rep = (n + nentries) * (long long)sizeof(double);
    const long long tables = n * (long long)n_axes * (long long)sizeof(uint16_t);
    char what[64];
    snprintf(what, sizeof what, "the bin table of %d axes", (int)n_axes);
    Replicates rep(device, logl, birth, n, run_start, n_runs, nsamples, expected, bootstrap, seed);
    MRG_OK(rep.plan_blocks(block_bytes, tables + kDefaultWeightBytes, tables, per_rep, kMaxBlockReps, what,
                           "the weights and its histograms"));
    const long long s_blk = rep.s_blk;
    const char* env = std::getenv("RVLL_MARGINAL_WAVE_REDUCE");
    const bool wave_reduce = env && env[0] == '1';        // off: it lost 12 - 14 % on 51 Peg (profiles/marginals_probe.txt)
    const int ngroups = (int)plan.group_first.size() - 1;
    const size_t lds = sizeof(unsigned long long) * (size_t)plan.max_entries;
    const size_t n_edges = (size_t)plan.axis_start[n_axes];
    double *d_vin = nullptr, *d_edges = nullptr, *d_state = nullptr, *d_mass = nullptr, *d_outside = nullptr;
    unsigned long long *d_h = nullptr, *d_msum = nullptr, *d_counts = nullptr;
    uint16_t* d_bins = nullptr;
    int32_t *d_axis_col = nullptr, *d_group_first = nullptr;
    long long* d_axis_start = nullptr;
    Panel* d_panels = nullptr;
    const size_t nc = (size_t)n * (size_t)ncols;
    std::vector<double> state((size_t)(5 * nbins), 0.0);
    std::vector<long long> cnt((size_t)nentries);
    for (long long b = 0; b < nbins; ++b) {
        state[(size_t)(3 * nbins + b)] = INFINITY;
        state[(size_t)(4 * nbins + b)] = -INFINITY;
    }

    MRG_OK(rep.begin());
    MergeSetup& su = rep.su;
    const hipStream_t stream = rep.stream;
    MRG_TRY(rep.alloc(d_edges, n_edges));
    MRG_TRY(rep.alloc(d_axis_col, (size_t)n_axes));
    MRG_TRY(rep.alloc(d_axis_start, (size_t)(n_axes + 1)));
    MRG_TRY(rep.alloc(d_panels, (size_t)n_panels));
    MRG_TRY(rep.alloc(d_group_first, (size_t)(ngroups + 1)));
    MRG_TRY(rep.alloc(d_state, state.size()));
    MRG_TRY(rep.alloc(d_counts, (size_t)nentries));
    MRG_TRY(rep.alloc(d_msum, (size_t)s_blk));
    MRG_TRY(rep.alloc(d_h, (size_t)(s_blk * nentries)));
    if (mass) MRG_TRY(rep.alloc(d_mass, (size_t)(s_blk * nbins)));
    if (outside) MRG_TRY(rep.alloc(d_outside, (size_t)(s_blk * n_panels)));
    MRG_TRY(rep.alloc(d_bins, (size_t)n * (size_t)n_axes));
    MRG_TRY(rep.alloc(d_vin, nc));                         // the input's copy: freed once it is binned
    MRG_TRY(hipMemcpyAsync(d_vin, values, sizeof(double) * nc, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_edges, edges, sizeof(double) * n_edges, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_axis_col, axis_col, sizeof(int32_t) * (size_t)n_axes, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_axis_start, plan.axis_start.data(), sizeof(long long) * (size_t)(n_axes + 1), hipMemcpyHostToDevice,
                           stream));
    MRG_TRY(hipMemcpyAsync(d_panels, plan.panels.data(), sizeof(Panel) * (size_t)n_panels, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_group_first, plan.group_first.data(), sizeof(int32_t) * (size_t)(ngroups + 1), hipMemcpyHostToDevice,
                           stream));
    MRG_TRY(hipMemcpyAsync(d_state, state.data(), sizeof(double) * state.size(), hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * (size_t)nentries, stream));

    MRG_OK(rep.setup([&]() -> hipError_t {
        hipLaunchKernelGGL(bin_kernel, dim3(blocks_for(n * (long long)n_axes, kThreads)), dim3(kThreads), 0, stream, d_vin, su.order,
                           (long long)n, (int)ncols, (int)n_axes, d_edges, d_axis_col, d_axis_start, d_bins);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const long long chunk = chunk_rows_for(n, ngroups, 1);
        const long long chunks = (n + chunk - 1) / chunk;
        rep.launches += 2;
        return launch_hist<true>(wave_reduce, dim3((unsigned)(chunks * ngroups), 1), lds, stream, nullptr, d_bins, (long long)n,
                                 d_panels, d_group_first, ngroups, chunk, nbins, nentries, d_counts);
    }));
    // the counts come down behind the setup's clock; the first block's synchronise covers them
    MRG_TRY(hipMemcpyAsync(cnt.data(), d_counts, sizeof(long long) * (size_t)nentries, hipMemcpyDeviceToHost, stream));
    MRG_TRY(rep.free_now(d_vin));
    MRG_OK(rep.run_blocks([&](long long, long long sb, double*, hipStream_t) -> hipError_t {
        const hipError_t e = hipMemsetAsync(d_msum, 0, sizeof(unsigned long long) * (size_t)sb, stream);
        if (e != hipSuccess) return e;
        return hipMemsetAsync(d_h, 0, sizeof(unsigned long long) * (size_t)(sb * nentries), stream);
    }, [&](long long, long long sb, double* d_w, hipStream_t) -> hipError_t {
        const long long chunk = chunk_rows_for(n, ngroups, sb);
        const long long chunks = (n + chunk - 1) / chunk;
        hipError_t e = launch_fixed(d_w, (long long)n, sb, d_msum, stream);
        if (e != hipSuccess) return e;
        e = launch_hist<false>(wave_reduce, dim3((unsigned)(chunks * ngroups), (unsigned)sb), lds, stream,
                               reinterpret_cast<const long long*>(d_w), d_bins, (long long)n, d_panels, d_group_first, ngroups,
                               chunk, nbins, nentries, d_h);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(stats_kernel, dim3(blocks_for(nentries, kThreads)), dim3(kThreads), 0, stream, d_h, d_msum, nbins,
                           nentries, (int)sb, d_state, d_mass, d_outside);
        rep.launches += 3;
        return hipGetLastError();
    }, [&](long long s0, long long sb, double*, hipStream_t) -> hipError_t {
        hipError_t e = hipSuccess;
        if (mass)
            e = hipMemcpyAsync(mass + s0 * nbins, d_mass, sizeof(double) * (size_t)(sb * nbins), hipMemcpyDeviceToHost, stream);
        if (outside && e == hipSuccess)
            e = hipMemcpyAsync(outside + s0 * n_panels, d_outside, sizeof(double) * (size_t)(sb * n_panels), hipMemcpyDeviceToHost,
                               stream);
        return e;
    }));
    MRG_TRY(hipMemcpyAsync(state.data(), d_state, sizeof(double) * state.size(), hipMemcpyDeviceToHost, stream));
    MRG_OK(rep.finish(logz, info));
    for (long long b = 0; b < nbins; ++b) {
        const double c = state[(size_t)b];
        const bool any = c > 0.0;
        stats[b] = any ? state[(size_t)(nbins + b)] : NAN;
        stats[nbins + b] = any ? std::sqrt(state[(size_t)(2 * nbins + b)] / c) : NAN;
        stats[2 * nbins + b] = any ? state[(size_t)(3 * nbins + b)] : NAN;
        stats[3 * nbins + b] = any ? state[(size_t)(4 * nbins + b)] : NAN;
        counts[b] = cnt[(size_t)b];
    }
    for (int t = 0; t < n_panels; ++t) outside_count[t] = cnt[(size_t)(nbins + t)];
    rep.report(timing);
    if (timing) {
        timing->bins = nbins;
        timing->threads = kHistThreads;
        timing->groups = ngroups;
    }
    return RVLL_OK;
}

}  // namespace

extern "C" int rvll_marginal_replicates(int32_t device, const double* logl, const double* birth, int64_t n_rows,
                                        const int64_t* run_start, int32_t n_runs, const double* values, int32_t n_cols,
                                        const double* edges, const int32_t* axis_col, const int64_t* axis_edge_start,
                                        int32_t n_axes, const int32_t* panel_axes, int32_t n_panels, int32_t nsamples,
                                        int32_t mode, int32_t bootstrap, uint64_t seed, double* logz, double* info,
                                        int64_t* counts, int64_t* outside_count, double* stats, double* mass, double* outside,
                                        int64_t block_bytes, rvll_marginal_timing* timing)
{
    MRG_OK(check_common(logl, birth, n_rows, run_start, n_runs));
    MRG_OK(check_replicate_args(nsamples, mode, bootstrap, n_runs, block_bytes));
    if (n_cols < 1 || n_cols > kMaxCols) return rvll::report_error(RVLL_E_INVALID, "n_cols must be in [1, %d]", kMaxCols);
    if (n_axes < 1 || n_axes > kMaxAxes) return rvll::report_error(RVLL_E_INVALID, "n_axes must be in [1, %d]", kMaxAxes);
    if (n_panels < 1 || n_panels > kMaxPanels)
        return rvll::report_error(RVLL_E_INVALID, "n_panels must be in [1, %d]", kMaxPanels);
    if (!values || !edges || !axis_col || !axis_edge_start || !panel_axes || !logz || !info || !counts || !outside_count || !stats)
        return rvll::report_error(RVLL_E_INVALID, "null argument");
    Plan plan;
    plan.axis_start.resize((size_t)n_axes + 1);
    if (axis_edge_start[0] != 0) return rvll::report_error(RVLL_E_INVALID, "axis_edge_start must begin at 0");
    plan.axis_start[0] = 0;
    for (int32_t a = 0; a < n_axes; ++a) {
        const int64_t ne = axis_edge_start[a + 1] - axis_edge_start[a];
        if (ne < 2 || ne > kMaxAxisBins + 1)
            return rvll::report_error(RVLL_E_INVALID, "axis %d has %lld edges: need 2 to %d", (int)a, (long long)ne, kMaxAxisBins + 1);
        if (axis_col[a] < 0 || axis_col[a] >= n_cols)
            return rvll::report_error(RVLL_E_INVALID, "axis %d names column %d of %d", (int)a, (int)axis_col[a], (int)n_cols);
        const double* e = edges + axis_edge_start[a];
        for (int64_t j = 0; j < ne; ++j)
            if (!std::isfinite(e[j]) || (j > 0 && !(e[j] > e[j - 1])))
                return rvll::report_error(RVLL_E_INVALID, "axis %d: edges must be finite and strictly increasing (edge %lld)",
                                          (int)a, (long long)j);
        plan.axis_start[(size_t)a + 1] = axis_edge_start[a + 1];
    }
    plan.panels.resize((size_t)n_panels);
    plan.group_first.push_back(0);
    int used = 0;
    for (int32_t t = 0; t < n_panels; ++t) {
        const int32_t a = panel_axes[2 * t], b = panel_axes[2 * t + 1];
        if (a < 0 || a >= n_axes || b < -1 || b >= n_axes)
            return rvll::report_error(RVLL_E_INVALID, "panel %d names the axes (%d, %d) of %d", (int)t, (int)a, (int)b, (int)n_axes);
        const long long na = plan.axis_start[(size_t)a + 1] - plan.axis_start[(size_t)a] - 1;
        const long long nb = b < 0 ? 1 : plan.axis_start[(size_t)b + 1] - plan.axis_start[(size_t)b] - 1;
        if (na * nb > kMaxPanelBins)
            return rvll::report_error(RVLL_E_INVALID, "panel %d has %lld bins: at most %d", (int)t, na * nb, kMaxPanelBins);
        const int need = (int)(na * nb) + 1;
        if (used + need > kGroupEntries) {
            plan.group_first.push_back(t);
            used = 0;
        }
        plan.panels[(size_t)t] = Panel{a, b, (int32_t)nb, (int32_t)(na * nb), used, (int32_t)plan.nbins, t, 0};
        used += need;
        plan.max_entries = std::max(plan.max_entries, used);
        plan.nbins += na * nb;
    }
    plan.group_first.push_back(n_panels);
    MRG_OK(check_finite_values(values, n_rows, n_cols));
    if (timing) *timing = rvll_marginal_timing{0., 0., 0., 0., 0., n_rows, 0, plan.nbins, 0, kHistThreads, 0, 0};
    return run_marginal(device, logl, birth, n_rows, run_start, n_runs, values, n_cols, edges, axis_col, n_axes, plan, n_panels,
                        nsamples, mode == RVLL_SHRINK_EXPECTED ? 1 : 0, bootstrap, seed, logz, info, counts, outside_count, stats,
                        mass, outside, block_bytes, timing);
}
