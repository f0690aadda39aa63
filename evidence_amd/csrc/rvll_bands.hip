// Order statistics of groups of Keplerian curves on gfx950 (rvll_kep_rv_bands): G groups of n curves at T times, as
// keprv_kernel writes them ([G n, T], row-major), become per (group, time) the number of values that are not NaN, Q quantiles by
// the inverted CDF of equal weights and the mean.  evidence_amd/predictive.py holds the numpy definition.
//
// One workgroup handles one (group, tile of times).  The tile's columns sit side by side in LDS, each padded to P, the power of
// two at or above n, with +inf; a NaN (an invalid orbit) is replaced by +inf as it is loaded and counted, so the valid values are
// the first n_valid of the sorted column.  One bitonic network sorts all columns of the tile at once, a compare-exchange a thread
// and step.  Then one thread a (column, level) picks sorted[max(0, ceil(level n_valid) - 1)], the product taken in double, and
// one thread a column adds the sorted valid values from left to right: numpy's cumsum order, so the mean has numpy's bits.
// The tile is as many times as 64 KiB of the CU's 160 KiB hold next to the 32 NaN counts, at most 32: 31 at P = 256, 1 at P = 4096.
#include "rvll_kernels.h"

namespace rvll {

namespace {

constexpr int kBandThreads = 256;
constexpr int kBandLdsBytes = 65536;                      // a workgroup's columns and their NaN counts
constexpr int kBandMaxTile = 32;

__global__ __launch_bounds__(kBandThreads)
void band_kernel(const double* __restrict__ vals, int n, int P, int T, int tile, const double* __restrict__ levels, int nq,
                 double* __restrict__ q, double* __restrict__ mean, int32_t* __restrict__ n_valid)
{
    extern __shared__ double sh_col[];                    // [tile][P], then the NaN count of every column
    int* sh_nan = reinterpret_cast<int*>(sh_col + (size_t)tile * P);
    const int tid = threadIdx.x;
    const long long g = blockIdx.y;
    const int j0 = (int)blockIdx.x * tile;
    const int tt = T - j0 < tile ? T - j0 : tile;         // the columns of this workgroup
    if (tid < kBandMaxTile) sh_nan[tid] = 0;
    __syncthreads();
    const double* __restrict__ src = vals + g * (long long)n * T + j0;
    for (int e = tid; e < tt * P; e += kBandThreads) {    // consecutive threads take consecutive times of one row
        const int i = e / tt, c = e - i * tt;
        double v = INFINITY;
        if (i < n) {
            v = src[(long long)i * T + c];
            if (v != v) {
                v = INFINITY;
                atomicAdd(&sh_nan[c], 1);
            }
        }
        sh_col[c * P + i] = v;
    }
    __syncthreads();
    const int half = P >> 1, pairs = tt * half;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < pairs; p += kBandThreads) {
                const int c = p / half, r = p - c * half;
                const int i = ((r & ~(j - 1)) << 1) | (r & (j - 1)), l = i | j;
                double* col = sh_col + c * P;
                const double a = col[i], b = col[l];
                if ((a > b) == ((i & k) == 0)) {
                    col[i] = b;
                    col[l] = a;
                }
            }
            __syncthreads();
        }
    for (int e = tid; e < tt * nq; e += kBandThreads) {
        const int c = e / nq, k = e - c * nq;
        const int nv = n - sh_nan[c];
        double out = NAN;
        if (nv > 0) {
            int idx = (int)ceil(levels[k] * (double)nv) - 1;
            idx = idx < 0 ? 0 : idx > nv - 1 ? nv - 1 : idx;
            out = sh_col[c * P + idx];
        }
        q[(g * nq + k) * T + j0 + c] = out;
    }
    if (tid < tt) {
        const int nv = n - sh_nan[tid];
        const double* col = sh_col + tid * P;
        double sum = NAN;
        if (nv > 0) {
            sum = col[0];
            for (int i = 1; i < nv; ++i) sum += col[i];
            sum /= (double)nv;
        }
        mean[g * T + j0 + tid] = sum;
        n_valid[g * T + j0 + tid] = nv;
    }
}

}  // namespace

hipError_t launch_bands(const double* vals, long long groups, int n, int Nt, const double* levels, int nq, double* q,
                        double* mean, int32_t* n_valid, hipStream_t stream)
{
    if (groups <= 0 || Nt <= 0) return hipSuccess;
    int P = 1;
    while (P < n) P <<= 1;
    int tile = (kBandLdsBytes - (int)sizeof(int) * kBandMaxTile) / ((int)sizeof(double) * P);
    tile = tile > kBandMaxTile ? kBandMaxTile : tile;
    tile = tile > Nt ? Nt : tile;
    const size_t lds = sizeof(double) * (size_t)tile * (size_t)P + sizeof(int) * kBandMaxTile;
    for (long long g0 = 0; g0 < groups; g0 += 65535) {    // grid y
        const long long gb = groups - g0 < 65535 ? groups - g0 : 65535;
        hipLaunchKernelGGL(band_kernel, dim3((unsigned)((Nt + tile - 1) / tile), (unsigned)gb), dim3(kBandThreads), lds, stream,
                           vals + g0 * (long long)n * Nt, n, P, Nt, tile, levels, nq, q + g0 * (long long)nq * Nt,
                           mean + g0 * (long long)Nt, n_valid + g0 * (long long)Nt);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rvll
