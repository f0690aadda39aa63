// The distances of the slice walk's step-count adaptation on gfx950 (rvll_walk_distances_runs).  evidence_amd/adapt.py
// holds the numpy definition:
//     dist_g(a, b) = sqrt(sum_k z_k z_k),  z_k = (delta_k - sum_{j<k} L_kj z_j) / L_kk,  delta = b - a (minimum image on wrapped
//     dimensions: x - floor(x + 0.5)), every operation rounded on its own (-ffp-contract=off; IEEE division and square root)
//     pair_g       = mean of dist_g over the unordered pairs of the group's rows (NaN below two rows)
//     move_k       = dist_g(start_k, end_k)
//
// Device work per call:
//     pairs     one 256-thread workgroup per (group, tile of kTileRows rows i): the group's factor and the tile's rows staged in
//               LDS (ndim <= 64: 32 KB + 16 KB), thread t takes the rows j = i0 + 1 + t, + 256, ... of the group, each once,
//               and forms dist(i, j) for the tile's rows i < j, z in registers (the substitution unrolled to a compile-time
//               bound on ndim).  A thread sums its distances in a fixed order, the workgroup by a fixed tree: one partial per
//               tile, no atomics.
//     finish    one thread per group adds its tiles' partials in tile order and divides by the number of pairs: a group's
//               result depends on its own rows alone, whatever else the call holds.
//     moves     one thread per walker, its group's factor read from global memory.
#include "rvll_host.h"

using rvll::report_error;
using namespace rvll::host;

namespace {

constexpr int kAdaptThreads = 256;
constexpr int kTileRows = 32;
constexpr int kAdaptMaxDims = 64;

// dist between rows a and b under the lower-triangular factor L [D, D] (row-major), DM >= D a compile-time bound so that z
// stays in registers
template <int DM>
__device__ __forceinline__ double fsub_dist(const double* a, const double* b, const double* L, unsigned long long wmask, int D)
{
    double z[DM];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DM; ++k) {
        if (k < D) {
            double d = b[k] - a[k];
            if ((wmask >> k) & 1ull) d = d - floor(d + 0.5);
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < k; ++j) s = s + L[k * D + j] * z[j];
            z[k] = (d - s) / L[k * D + k];
            acc = acc + z[k] * z[k];
        }
    }
    return sqrt(acc);
}

struct PairArgs {
    const double* rows;          // [*, D]
    const int32_t* idx;          // or null: member i of group g is row idx[gofs[g] + i] (else row gofs[g] + i)
    const int64_t* gofs;         // [G]
    const int64_t* gcnt;         // [G] members
    const double* factors;       // [G, D, D]
    const int32_t* tiles;        // [T][2]: (group, first row i0 inside the group)
    double* partial;             // [T]
    unsigned long long wmask;
    int D;
};

template <int DM>
__global__ __launch_bounds__(kAdaptThreads)
void pair_tiles_kernel(const PairArgs p)
{
    __shared__ double Ls[kAdaptMaxDims * kAdaptMaxDims];
    __shared__ double As[kTileRows * kAdaptMaxDims];
    __shared__ double red[kAdaptThreads];
    const int D = p.D, tid = threadIdx.x;
    const int g = p.tiles[2 * blockIdx.x], i0 = p.tiles[2 * blockIdx.x + 1];
    const long long base = p.gofs[g];
    const int n = (int)p.gcnt[g];
    const int ni = min(kTileRows, n - i0);
    auto row = [&](int i) -> const double* { return p.rows + (long long)(p.idx ? p.idx[base + i] : base + i) * D; };
    for (int e = tid; e < D * D; e += kAdaptThreads) Ls[e] = p.factors[(long long)g * D * D + e];
    for (int e = tid; e < ni * D; e += kAdaptThreads) As[e] = row(i0 + e / D)[e % D];
    __syncthreads();
    double sum = 0.0;
    for (int j = i0 + 1 + tid; j < n; j += kAdaptThreads) {
        const double* bj = row(j);
        const int iend = min(ni, j - i0);
        for (int i = 0; i < iend; ++i) sum = sum + fsub_dist<DM>(As + i * D, bj, Ls, p.wmask, D);
    }
    red[tid] = sum;
    __syncthreads();
    for (int w = kAdaptThreads / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    if (tid == 0) p.partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kAdaptThreads)
void pair_finish_kernel(const int64_t* gcnt, const int32_t* tile_start, const double* partial, int G, double* pair_out)
{
    const int g = blockIdx.x * kAdaptThreads + threadIdx.x;
    if (g >= G) return;
    const long long n = gcnt[g];
    if (n < 2) { pair_out[g] = __builtin_nan(""); return; }
    double s = 0.0;
    for (int t = tile_start[g]; t < tile_start[g + 1]; ++t) s = s + partial[t];
    pair_out[g] = s / (double)(n * (n - 1) / 2);
}

template <int DM>
__global__ __launch_bounds__(kAdaptThreads)
void move_kernel(const double* starts, const double* ends, const int32_t* walker_group, const double* factors, long long K,
                 unsigned long long wmask, int D, double* move_out)
{
    const long long k = (long long)blockIdx.x * kAdaptThreads + threadIdx.x;
    if (k >= K) return;
    move_out[k] = fsub_dist<DM>(starts + k * D, ends + k * D, factors + (long long)walker_group[k] * D * D, wmask, D);
}

template <int DM>
hipError_t launch_all(const PairArgs& p, int T, const int32_t* tile_start, int G, double* pair_out, const double* starts,
                      const double* ends, const int32_t* walker_group, long long K, double* move_out, hipStream_t st)
{
    if (T > 0) hipLaunchKernelGGL(pair_tiles_kernel<DM>, dim3((unsigned)T), dim3(kAdaptThreads), 0, st, p);
    if (G > 0) hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)((G + kAdaptThreads - 1) / kAdaptThreads)), dim3(kAdaptThreads), 0, st,
                                  p.gcnt, tile_start, p.partial, G, pair_out);
    if (K > 0) hipLaunchKernelGGL(move_kernel<DM>, dim3((unsigned)((K + kAdaptThreads - 1) / kAdaptThreads)), dim3(kAdaptThreads), 0, st,
                                  starts, ends, walker_group, p.factors, K, p.wmask, p.D, move_out);
    return hipGetLastError();
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

namespace rvll {
namespace host {

int walk_distances_core(rvll_handle* h, const double* d_rows, const int32_t* d_idx, const std::vector<int64_t>& gofs,
                        const std::vector<int64_t>& gcnt, const double* d_factors, unsigned long long wmask, const double* d_starts,
                        const double* d_ends, const int32_t* d_walker_group, int64_t K, double** d_pair, double** d_move,
                        std::vector<int32_t>& tables)
{
    const int D = h->L.ndim;
    const int32_t G = (int32_t)gofs.size();
    // (group, i0) for every kTileRows members of a group with a pair, then tile_start [G + 1], in one host table
    tables.clear();
    std::vector<int32_t> ts((size_t)G + 1, 0);
    for (int32_t g = 0; g < G; ++g) {
        if (gcnt[(size_t)g] >= 2)
            for (int64_t i0 = 0; i0 + 1 < gcnt[(size_t)g]; i0 += kTileRows) { tables.push_back(g); tables.push_back((int32_t)i0); }
        ts[(size_t)g + 1] = (int32_t)(tables.size() / 2);
    }
    const int T = (int)(tables.size() / 2);
    tables.insert(tables.end(), ts.begin(), ts.end());
    const size_t o_g = 0, o_c = up16(8 * (size_t)G), o_tab = up16(o_c + 8 * (size_t)G), o_part = up16(o_tab + 4 * tables.size());
    const size_t o_pair = up16(o_part + 8 * (size_t)T), o_move = up16(o_pair + 8 * (size_t)G), total = up16(o_move + 8 * (size_t)K);
    if (total > h->adapt_cap) {
        HIP_TRY(hipStreamSynchronize(h->compute));
        dev_free(h->d_adapt);
        h->adapt_cap = 0;
        if (hipMalloc(&h->d_adapt, total) != hipSuccess) { h->d_adapt = nullptr; return report_error(RVLL_E_NOMEM, "walk distances: %zu bytes", total); }
        h->adapt_cap = total;
    }
    char* b = static_cast<char*>(h->d_adapt);
    hipStream_t st = h->compute;
    if (G > 0) {
        HIP_TRY(hipMemcpyAsync(b + o_g, gofs.data(), 8 * (size_t)G, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b + o_c, gcnt.data(), 8 * (size_t)G, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(b + o_tab, tables.data(), 4 * tables.size(), hipMemcpyHostToDevice, st));
    const int32_t* d_tiles = reinterpret_cast<const int32_t*>(b + o_tab);
    PairArgs p{d_rows, d_idx, reinterpret_cast<const int64_t*>(b + o_g), reinterpret_cast<const int64_t*>(b + o_c), d_factors,
               d_tiles, reinterpret_cast<double*>(b + o_part), wmask, D};
    const int32_t* d_ts = d_tiles + 2 * (size_t)T;
    *d_pair = reinterpret_cast<double*>(b + o_pair);
    *d_move = reinterpret_cast<double*>(b + o_move);
    hipError_t e;
    if (D <= 8)       e = launch_all<8>(p, T, d_ts, G, *d_pair, d_starts, d_ends, d_walker_group, K, *d_move, st);
    else if (D <= 16) e = launch_all<16>(p, T, d_ts, G, *d_pair, d_starts, d_ends, d_walker_group, K, *d_move, st);
    else if (D <= 32) e = launch_all<32>(p, T, d_ts, G, *d_pair, d_starts, d_ends, d_walker_group, K, *d_move, st);
    else              e = launch_all<64>(p, T, d_ts, G, *d_pair, d_starts, d_ends, d_walker_group, K, *d_move, st);
    if (e != hipSuccess) return report_error(RVLL_E_HIP, "walk distances: launch failed: %s", hipGetErrorString(e));
    return RVLL_OK;
}

int adapt_in_reserve(rvll_handle* h, size_t bytes)
{
    if (bytes <= h->adapt_in_cap) return RVLL_OK;
    HIP_TRY(hipStreamSynchronize(h->compute));
    dev_free(h->d_adapt_in);
    h->adapt_in_cap = 0;
    if (hipMalloc(&h->d_adapt_in, bytes) != hipSuccess) { h->d_adapt_in = nullptr; return report_error(RVLL_E_NOMEM, "walk distances: %zu bytes", bytes); }
    h->adapt_in_cap = bytes;
    return RVLL_OK;
}

}  // namespace host
}  // namespace rvll

extern "C" {

int rvll_walk_distances_runs(rvll_handle* h, const double* survivors, const int64_t* group_start, int32_t G, const double* factors,
                             const int32_t* wrapped, const double* starts, const double* ends, const int32_t* walker_group, int64_t K,
                             double* pair_out, double* move_out)
{
    const char* who = "rvll_walk_distances_runs";
    if (!h) return report_error(RVLL_E_INVALID, "%s: null handle", who);
    int rc = use_device(h);
    if (rc) return rc;
    if (G < 0 || K < 0 || !group_start) return report_error(RVLL_E_INVALID, "%s: bad group table", who);
    if (group_start[0] != 0) return report_error(RVLL_E_INVALID, "%s: group_start[0] must be 0", who);
    for (int32_t g = 0; g < G; ++g)
        if (group_start[g + 1] < group_start[g]) return report_error(RVLL_E_INVALID, "%s: group_start decreases at group %d", who, (int)g);
    const int64_t N = group_start[G];
    if (N >= (1LL << 31) || K >= (1LL << 31)) return report_error(RVLL_E_INVALID, "%s: too many rows or walkers", who);
    if ((G > 0 && (!factors || !pair_out)) || (N > 0 && !survivors) || (K > 0 && (!starts || !ends || !walker_group || !move_out)))
        return report_error(RVLL_E_INVALID, "%s: null buffer", who);
    for (int64_t k = 0; k < K; ++k)
        if (walker_group[k] < 0 || walker_group[k] >= G)
            return report_error(RVLL_E_INVALID, "%s: walker_group[%lld] = %d is outside [0, %d)", who, (long long)k, (int)walker_group[k], (int)G);
    const int D = h->L.ndim;
    if (D < 1 || D > kAdaptMaxDims) return report_error(RVLL_E_UNSUPPORTED, "%s: %d parameters (the distances take 1 .. %d)", who, D, kAdaptMaxDims);
    if (G == 0 && K == 0) return RVLL_OK;
    // the inputs in one block: rows | factors | starts | ends | walker groups
    const size_t Dz = (size_t)D;
    const size_t o_fac = up16(8 * (size_t)N * Dz), o_s = up16(o_fac + 8 * (size_t)G * Dz * Dz), o_e = up16(o_s + 8 * (size_t)K * Dz);
    const size_t o_wg = up16(o_e + 8 * (size_t)K * Dz), total = up16(o_wg + 4 * (size_t)K);
    rc = adapt_in_reserve(h, total);
    if (rc) return rc;
    char* b = static_cast<char*>(h->d_adapt_in);
    hipStream_t st = h->compute;
    if (N > 0) HIP_TRY(hipMemcpyAsync(b, survivors, 8 * (size_t)N * Dz, hipMemcpyHostToDevice, st));
    if (G > 0) HIP_TRY(hipMemcpyAsync(b + o_fac, factors, 8 * (size_t)G * Dz * Dz, hipMemcpyHostToDevice, st));
    if (K > 0) {
        HIP_TRY(hipMemcpyAsync(b + o_s, starts, 8 * (size_t)K * Dz, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b + o_e, ends, 8 * (size_t)K * Dz, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b + o_wg, walker_group, 4 * (size_t)K, hipMemcpyHostToDevice, st));
    }
    std::vector<int64_t> gofs((size_t)G), gcnt((size_t)G);
    for (int32_t g = 0; g < G; ++g) { gofs[(size_t)g] = group_start[g]; gcnt[(size_t)g] = group_start[g + 1] - group_start[g]; }
    std::vector<int32_t> tables;
    double *d_pair = nullptr, *d_move = nullptr;
    rc = walk_distances_core(h, reinterpret_cast<const double*>(b), nullptr, gofs, gcnt, reinterpret_cast<const double*>(b + o_fac),
                             wrapped_mask(wrapped, D), reinterpret_cast<const double*>(b + o_s), reinterpret_cast<const double*>(b + o_e),
                             reinterpret_cast<const int32_t*>(b + o_wg), K, &d_pair, &d_move, tables);
    if (rc) return rc;
    if (G > 0) HIP_TRY(hipMemcpyAsync(pair_out, d_pair, 8 * (size_t)G, hipMemcpyDeviceToHost, st));
    if (K > 0) HIP_TRY(hipMemcpyAsync(move_out, d_move, 8 * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

}  // extern "C"
