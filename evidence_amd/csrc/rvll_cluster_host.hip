// rvll_cluster_host.hip — host side of the clustering of live points (rvll_cluster_runs; include/rvll.h): argument
// checks, the workgroup table, grow-only device blocks, one upload and one download per call, around a core on device pointers
// that the clustered step of the resident ensemble (rvll_live_runs_step_clustered) also calls.  The kernels are in
// rvll_cluster.hip.
#include "rvll_host.h"

using rvll::report_error;
using namespace rvll::host;

namespace {

constexpr size_t kClusterMaxBytes = (size_t)4 << 30;     // the three device blocks together; beyond: RVLL_E_NOMEM, nothing allocated

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// grow-only device block of at least `bytes` (freed first: a failed allocation leaves no block and a zero capacity)
int reserve(rvll_handle* h, void** p, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return RVLL_OK;
    HIP_TRY(hipStreamSynchronize(h->compute));
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    *cap = 0;
    HIP_TRY(hipMalloc(p, bytes));
    *cap = bytes;
    return RVLL_OK;
}

}  // namespace

namespace rvll {
namespace host {

std::vector<int32_t> cluster_blocks(const int64_t* run_start, int64_t R)
{
    std::vector<int32_t> blocks;
    for (int64_t r = 0; r < R; ++r)
        for (int64_t i = run_start[r]; i < run_start[r + 1]; i += 64) { blocks.push_back((int32_t)r); blocks.push_back((int32_t)i); }
    return blocks;
}

// packed inputs: cube, scale, run_start, seeds, block table; work: forest, per-run maxima; packed outputs: radius2, nclusters, labels
ClusterLayout cluster_layout(int64_t N, int64_t R, int D, size_t block_ints)
{
    ClusterLayout L{};
    L.o_cube = 0;
    L.o_scale = up16(L.o_cube + sizeof(double) * (size_t)N * D);
    L.o_start = up16(L.o_scale + sizeof(double) * (size_t)R * D);
    L.o_seed = up16(L.o_start + sizeof(int64_t) * (size_t)(R + 1));
    L.o_blk = up16(L.o_seed + sizeof(uint64_t) * (size_t)R);
    L.in_bytes = up16(L.o_blk + sizeof(int32_t) * block_ints);
    L.w_slots = up16(sizeof(int32_t) * (size_t)N);
    L.work_bytes = L.w_slots + sizeof(unsigned long long) * rvll::kClusterSlots * (size_t)R;
    L.p_ncl = up16(sizeof(double) * (size_t)R);
    L.p_lab = up16(L.p_ncl + sizeof(int32_t) * (size_t)R);
    L.out_bytes = up16(L.p_lab + sizeof(int32_t) * (size_t)N);
    L.N = N; L.R = R; L.nblocks = (long long)(block_ints / 2);
    return L;
}

int cluster_reserve(rvll_handle* h, const ClusterLayout& L, const char* who)
{
    if (L.in_bytes + L.work_bytes + L.out_bytes > kClusterMaxBytes)
        return report_error(RVLL_E_NOMEM, "%s: %zu bytes of device memory exceed the clustering's budget", who,
                            L.in_bytes + L.work_bytes + L.out_bytes);
    int rc = reserve(h, &h->d_cl_in, &h->cl_in_cap, L.in_bytes);
    if (!rc) rc = reserve(h, &h->d_cl_work, &h->cl_work_cap, L.work_bytes);
    if (!rc) rc = reserve(h, &h->d_cl_out, &h->cl_out_cap, L.out_bytes);
    return rc;
}

rvll::ClusterArgs cluster_args(rvll_handle* h, const ClusterLayout& L, int D, int nboot, const int32_t* wrapped)
{
    unsigned long long wmask = 0;
    if (wrapped)
        for (int d = 0; d < D; ++d) if (wrapped[d]) wmask |= 1ull << d;
    char* din = static_cast<char*>(h->d_cl_in);
    char* dwork = static_cast<char*>(h->d_cl_work);
    char* dout = static_cast<char*>(h->d_cl_out);
    rvll::ClusterArgs a{};
    a.cube = reinterpret_cast<const double*>(din + L.o_cube);
    a.scale = reinterpret_cast<const double*>(din + L.o_scale);
    a.run_start = reinterpret_cast<const long long*>(din + L.o_start);
    a.seeds = reinterpret_cast<const unsigned long long*>(din + L.o_seed);
    a.blocks = reinterpret_cast<const int32_t*>(din + L.o_blk);
    a.nblocks = L.nblocks;
    a.R = (int)L.R; a.D = D; a.nboot = nboot; a.tile_rows = rvll::cluster_tile_rows(D);
    a.wrapped = wmask;
    a.parent = reinterpret_cast<int32_t*>(dwork);
    a.slots = reinterpret_cast<unsigned long long*>(dwork + L.w_slots);
    a.radius2 = reinterpret_cast<double*>(dout);
    a.nclusters = reinterpret_cast<int32_t*>(dout + L.p_ncl);
    a.labels = reinterpret_cast<int32_t*>(dout + L.p_lab);
    return a;
}

// the clustering itself, on inputs already in the device blocks: the per-run maxima zeroed, the three kernels; asynchronous
int cluster_core(rvll_handle* h, const rvll::ClusterArgs& a)
{
    HIP_TRY(hipMemsetAsync(a.slots, 0, sizeof(unsigned long long) * rvll::kClusterSlots * (size_t)a.R, h->compute));
    HIP_TRY(rvll::launch_cluster(a, h->compute));
    return RVLL_OK;
}

}  // namespace host
}  // namespace rvll

extern "C" {

int rvll_cluster_runs(rvll_handle* h, const double* cube, const int64_t* run_start, int64_t R, const double* scale,
                      const int32_t* wrapped, int nboot, const uint64_t* seeds, int32_t* labels, int32_t* nclusters,
                      double* radius2)
{
    if (!h) return report_error(RVLL_E_INVALID, "rvll_cluster_runs: null handle");
    int rc = use_device(h);
    if (rc) return rc;
    if (R < 0 || !run_start) return report_error(RVLL_E_INVALID, "rvll_cluster_runs: bad run table");
    if (nboot < 0 || nboot > rvll::kClusterMaxBoot)
        return report_error(RVLL_E_INVALID, "rvll_cluster_runs: nboot = %d is outside [0, %d]", nboot, rvll::kClusterMaxBoot);
    if (run_start[0] != 0) return report_error(RVLL_E_INVALID, "rvll_cluster_runs: run_start[0] must be 0");
    for (int64_t r = 0; r < R; ++r)
        if (run_start[r + 1] < run_start[r])
            return report_error(RVLL_E_INVALID, "rvll_cluster_runs: run_start decreases at run %lld", (long long)r);
    const int64_t N = run_start[R];
    if (N >= (1LL << 31) || R >= (1LL << 31)) return report_error(RVLL_E_INVALID, "rvll_cluster_runs: too many rows or runs");
    if (R == 0) return RVLL_OK;
    if (!scale || !seeds || !nclusters || !radius2 || (N > 0 && (!cube || !labels)))
        return report_error(RVLL_E_INVALID, "rvll_cluster_runs: null buffer");
    const int D = h->L.ndim;
    if (D < 1 || D > rvll::kClusterMaxDims)
        return report_error(RVLL_E_UNSUPPORTED, "rvll_cluster_runs: %d parameters (the clustering takes 1 .. %d)", D, rvll::kClusterMaxDims);
    for (int64_t k = 0; k < R * D; ++k)
        if (!(std::isfinite(scale[k]) && scale[k] > 0.0))
            return report_error(RVLL_E_INVALID, "rvll_cluster_runs: scale[%lld] is not finite and positive", (long long)k);
    // workgroups of the row kernels: 64 rows of one run each
    const std::vector<int32_t> blocks = cluster_blocks(run_start, R);
    const ClusterLayout L = cluster_layout(N, R, D, blocks.size());
    rc = cluster_reserve(h, L, "rvll_cluster_runs");
    if (rc) return rc;

    std::vector<char> in(L.in_bytes), out(L.out_bytes);
    if (N > 0) memcpy(in.data() + L.o_cube, cube, sizeof(double) * (size_t)N * D);
    memcpy(in.data() + L.o_scale, scale, sizeof(double) * (size_t)R * D);
    memcpy(in.data() + L.o_start, run_start, sizeof(int64_t) * (size_t)(R + 1));
    memcpy(in.data() + L.o_seed, seeds, sizeof(uint64_t) * (size_t)R);
    if (!blocks.empty()) memcpy(in.data() + L.o_blk, blocks.data(), sizeof(int32_t) * blocks.size());

    hipStream_t st = h->compute;
    const rvll::ClusterArgs a = cluster_args(h, L, D, nboot, wrapped);
    HIP_TRY(hipMemcpyAsync(h->d_cl_in, in.data(), L.in_bytes, hipMemcpyHostToDevice, st));
    rc = cluster_core(h, a);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out.data(), h->d_cl_out, L.out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(radius2, out.data(), sizeof(double) * (size_t)R);
    memcpy(nclusters, out.data() + L.p_ncl, sizeof(int32_t) * (size_t)R);
    if (N > 0) memcpy(labels, out.data() + L.p_lab, sizeof(int32_t) * (size_t)N);
    return RVLL_OK;
}

}  // extern "C"
