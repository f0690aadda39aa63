// Prior log densities of many parameter rows under many sets of priors on gfx950 (rvll_prior_logpdf_batch): the ratio table of
// the prior-sensitivity scan (evidence_amd/sensitivity.py).  The formulas are rvll_prior_density.h's, host+device;
// evidence_amd/priors.py (log_density) holds the numpy definition.
//
// Kernel.  A workgroup is one wave and takes kRows = 64 consecutive rows; a lane is a row.
//     stage    the rows' theta, one contiguous piece of [rows, ndim], comes in with coalesced loads and is laid out in LDS with
//              an odd row stride, so that the lanes' reads of one column fall on different banks
//     sets     the loop over (set, dim) reads the descriptors at addresses that do not depend on the lane: scalar loads, and
//              the switch on the kind is a uniform branch.  A SKIP descriptor costs its load.
//     store    kSetChunk sets at a time go through an LDS tile (odd stride again) and leave as pieces of [rows, n_sets] that
//              are contiguous over the sets of a row
// A row's sum is added in rising dim by its own lane from its own theta: the same bits in any batching.  No atomics.
//
// Host.  The descriptors are checked and put into the kernel's form once per call (a sorted member gets the bounds of its
// group's last member, the dim of the member before it and, at the last member, the group's size and ln n!).  The rows go in
// chunks whose theta and out stay within kChunkBytes.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>
#include <algorithm>

#pragma GCC visibility push(default)
#include "rvll.h"
#pragma GCC visibility pop
#include "rvll_prior_density.h"

namespace rvll {
int report_error(int code, const char* fmt, ...);
}

namespace {

constexpr int kRows = 64;                                  // rows of a workgroup = its threads: one wave
constexpr int kSetChunk = 16;                              // sets of one pass through the output tile
constexpr int kOutStride = kSetChunk + 1;
constexpr int kMaxDim = 64, kMaxSets = 4096;
constexpr long long kMaxRows = 1ll << 30;
constexpr long long kChunkBytes = 256ll << 20;

// a descriptor as the kernel reads it
struct Desc {
    int32_t kind;
    int32_t prev;              // sorted kinds: the dim of the group's member before this one, -1 at the first
    int32_t n;                 // sorted kinds: the group's size at its last member, 0 at the others
    int32_t reserved;
    double lognfact;           // ln n! at the last member
    double args[RVLL_DENSITY_NARGS];
};

#define DEN_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            status = rvll::report_error(e_ == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, \
                                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                        __FILE__, __LINE__);                                   \
            goto done;                                                                         \
        }                                                                                      \
    } while (0)

__global__ __launch_bounds__(kRows)
void prior_logpdf_kernel(const Desc* __restrict__ descs, int n_sets, int ndim, const double* __restrict__ theta, long long rows,
                         double* __restrict__ out)
{
    extern __shared__ double lds[];
    const int stride = ndim | 1;
    double* __restrict__ th = lds;                          // [kRows][stride]
    double* __restrict__ res = lds + kRows * stride;        // [kRows][kOutStride]
    const long long row0 = (long long)blockIdx.x * kRows;
    const int nr = (int)(rows - row0 < kRows ? rows - row0 : kRows);
    const int t = threadIdx.x;

    const double* __restrict__ src = theta + row0 * ndim;
    for (int i = t; i < nr * ndim; i += kRows) {
        const int r = i / ndim;
        th[r * stride + (i - r * ndim)] = src[i];
    }
    __syncthreads();

    const double* __restrict__ mine = th + t * stride;
    for (int a0 = 0; a0 < n_sets; a0 += kSetChunk) {
        const int sc = n_sets - a0 < kSetChunk ? n_sets - a0 : kSetChunk;
        if (t < nr) {
            for (int j = 0; j < sc; ++j) {
                const Desc* __restrict__ set = descs + (long long)(a0 + j) * ndim;
                double sum = 0.;
                for (int d = 0; d < ndim; ++d) {
                    const Desc& ds = set[d];
                    const int kind = ds.kind;
                    if (kind == RVLL_DENSITY_SKIP) continue;
                    const double x = mine[d];
                    if (kind == RVLL_DENSITY_SORTED_UNIFORM || kind == RVLL_DENSITY_SORTED_LOGUNIFORM) {
                        const bool first = ds.prev < 0;
                        sum += rvll::sorted_logpdf(kind, ds.args[0], ds.args[1], ds.n, ds.lognfact, first, mine[first ? d : ds.prev], x);
                    } else {
                        sum += rvll::prior_logpdf(kind, ds.args, x);
                    }
                }
                res[t * kOutStride + j] = sum;
            }
        }
        __syncthreads();
        for (int i = t; i < nr * sc; i += kRows) {
            const int r = i / sc, j = i - r * sc;
            out[(row0 + r) * n_sets + a0 + j] = res[r * kOutStride + j];
        }
        __syncthreads();
    }
}

// The descriptors of the call in the kernel's form, or RVLL_E_INVALID.
int compile_sets(const rvll_prior_density* sets, int32_t n_sets, int32_t ndim, std::vector<Desc>& descs)
{
    descs.assign((size_t)n_sets * ndim, Desc{});
    for (int32_t a = 0; a < n_sets; ++a) {
        const rvll_prior_density* set = sets + (size_t)a * ndim;
        Desc* out = descs.data() + (size_t)a * ndim;
        for (int32_t d = 0; d < ndim; ++d) {
            const int kind = set[d].kind;
            if (kind < 0 || kind >= RVLL_DENSITY__COUNT)
                return rvll::report_error(RVLL_E_INVALID, "set %d, parameter %d: unknown density kind %d", (int)a, (int)d, kind);
            if (!rvll::density_args_ok(kind, set[d].args))
                return rvll::report_error(RVLL_E_INVALID, "set %d, parameter %d: invalid arguments for density kind %d", (int)a, (int)d,
                                          kind);
            out[d].kind = kind;
            out[d].prev = -1;
            for (int k = 0; k < RVLL_DENSITY_NARGS; ++k) out[d].args[k] = set[d].args[k];
        }
        for (int32_t d = 0; d < ndim; ++d) {
            const int kind = set[d].kind;
            if (kind != RVLL_DENSITY_SORTED_UNIFORM && kind != RVLL_DENSITY_SORTED_LOGUNIFORM) continue;
            if (set[d].group < 0)
                return rvll::report_error(RVLL_E_INVALID, "set %d, parameter %d: a sorted density needs a group >= 0", (int)a, (int)d);
            int32_t last = d, n = 0, prev = -1;
            for (int32_t k = 0; k < ndim; ++k) {
                const bool sorted = set[k].kind == RVLL_DENSITY_SORTED_UNIFORM || set[k].kind == RVLL_DENSITY_SORTED_LOGUNIFORM;
                if (!sorted || set[k].group != set[d].group) continue;
                if (set[k].kind != kind)
                    return rvll::report_error(RVLL_E_INVALID, "set %d: sorted group %d mixes kinds", (int)a, (int)set[d].group);
                if (k < d) prev = k;
                last = k;
                ++n;
            }
            out[d].prev = prev;
            out[d].args[0] = set[last].args[0];
            out[d].args[1] = set[last].args[1];
            if (d == last) {
                out[d].n = n;
                out[d].lognfact = std::lgamma((double)n + 1.0);
            }
        }
    }
    return RVLL_OK;
}

}  // namespace

extern "C" int rvll_prior_logpdf_batch(int32_t device, const rvll_prior_density* sets, int32_t n_sets, int32_t ndim,
                                       const double* theta, int64_t B, double* out, rvll_density_timing* timing)
{
    const auto t_start = std::chrono::steady_clock::now();
    if (!sets || !theta || !out) return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (B < 1 || B >= kMaxRows) return rvll::report_error(RVLL_E_INVALID, "B must be in [1, 2^30)");
    if (ndim < 1 || ndim > kMaxDim) return rvll::report_error(RVLL_E_INVALID, "ndim must be in [1, %d]", kMaxDim);
    if (n_sets < 1 || n_sets > kMaxSets) return rvll::report_error(RVLL_E_INVALID, "n_sets must be in [1, %d]", kMaxSets);
    std::vector<Desc> descs;
    {
        const int rc = compile_sets(sets, n_sets, ndim, descs);
        if (rc) return rc;
    }
    if (timing) *timing = rvll_density_timing{0., 0., B, (int64_t)B * n_sets * ndim, 0, kRows};

    // whole workgroups of rows per chunk
    const long long row_bytes = (long long)sizeof(double) * ((long long)ndim + n_sets);
    const long long chunk_rows = std::min<long long>(B, std::max<long long>(kChunkBytes / row_bytes / kRows, 1) * kRows);
    const size_t lds_bytes = sizeof(double) * (size_t)kRows * (size_t)((ndim | 1) + kOutStride);

    int status = RVLL_OK;
    int prev_device = -1;
    Desc* d_descs = nullptr;
    double *d_theta = nullptr, *d_out = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double kernel_ms = 0.;
    int launches = 0;

    DEN_TRY(hipGetDevice(&prev_device));
    if (device >= 0) DEN_TRY(hipSetDevice(device));
    DEN_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) DEN_TRY(hipEventCreate(&e));
    DEN_TRY(hipMalloc(&d_descs, sizeof(Desc) * descs.size()));
    DEN_TRY(hipMalloc(&d_theta, sizeof(double) * (size_t)chunk_rows * (size_t)ndim));
    DEN_TRY(hipMalloc(&d_out, sizeof(double) * (size_t)chunk_rows * (size_t)n_sets));
    DEN_TRY(hipMemcpyAsync(d_descs, descs.data(), sizeof(Desc) * descs.size(), hipMemcpyHostToDevice, stream));
    for (long long r0 = 0; r0 < B; r0 += chunk_rows) {
        const long long rows = std::min<long long>(chunk_rows, B - r0);
        DEN_TRY(hipMemcpyAsync(d_theta, theta + r0 * ndim, sizeof(double) * (size_t)rows * (size_t)ndim, hipMemcpyHostToDevice, stream));
        DEN_TRY(hipEventRecord(ev[0], stream));
        hipLaunchKernelGGL(prior_logpdf_kernel, dim3((unsigned)((rows + kRows - 1) / kRows)), dim3(kRows), lds_bytes, stream, d_descs,
                           (int)n_sets, (int)ndim, d_theta, rows, d_out);
        DEN_TRY(hipGetLastError());
        DEN_TRY(hipEventRecord(ev[1], stream));
        ++launches;
        DEN_TRY(hipMemcpyAsync(out + r0 * n_sets, d_out, sizeof(double) * (size_t)rows * (size_t)n_sets, hipMemcpyDeviceToHost, stream));
        DEN_TRY(hipStreamSynchronize(stream));
        float ms = 0.f;
        DEN_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        kernel_ms += ms;
    }
    if (timing) {
        timing->kernel_ms = kernel_ms;
        timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        timing->launches = launches;
    }

done:
    for (void* p : {(void*)d_descs, (void*)d_theta, (void*)d_out})
        if (p) (void)hipFree(p);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (prev_device >= 0 && device >= 0) (void)hipSetDevice(prev_device);
    return status;
}
