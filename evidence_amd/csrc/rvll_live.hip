// rvll_live.hip — small data-movement kernels of the device-resident live set (rvll_live_*; include/rvll.h): row gather /
// scatter by index, and the mean and covariance of a subset of rows in a fixed summation order.
//
// The reference leaves nested sampling to UltraNest (evidence/ultranest/__init__.py:159-185), whose region slice sampler
// whitens its directions with the live points' covariance; evidence_amd/nested.py does the same.  With the walk on the
// device (rvll_walk.hip) what was left on the host per iteration was index copies of the live points and of the walker rows
// through PCIe (a fifth of the end-to-end time): these kernels keep all of it in HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include "rvll_kernels.h"

namespace rvll {

namespace {

constexpr int kMomBlocks = 128;       // partial sums: a fixed number of blocks, so the summation order is fixed

// dst[i][:] = src[idx[i]][:]   (rows of `width` doubles)
__global__ __launch_bounds__(kThreads)
void gather_rows_kernel(const double* src, const int32_t* idx, long long n, int width, double* dst)
{
    const long long total = n * width;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
        const long long i = e / width;
        dst[e] = src[(long long)idx[i] * width + (e - i * width)];
    }
}

// dst[idx[i]][:] = src[i][:]   (idx holds distinct rows)
__global__ __launch_bounds__(kThreads)
void scatter_rows_kernel(const double* src, const int32_t* idx, long long n, int width, double* dst)
{
    const long long total = n * width;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
        const long long i = e / width;
        dst[(long long)idx[i] * width + (e - i * width)] = src[e];
    }
}

// partial column sums of the rows idx[0..n): block b takes rows b, b + kMomBlocks, ...; its threads are kThreads / D groups
// of D, group g summing every (kThreads / D)-th of the block's rows, and the groups' sums are added in group order — a
// fixed order for a given (n, D).  (One thread per column, as first written, left 237 of 256 threads idle: 63 us per call.)
// kSeg: set blockIdx.y is segment y0 + blockIdx.y of a table of (offset, rows) pairs (launch_moments_segs) instead of a stride.
template <bool kSeg>
__global__ __launch_bounds__(kThreads)
void moments_sum_kernel(const double* u, const int32_t* idx, long long n, int D, double* part /*[kMomBlocks][D]*/,
                        long long idx_stride, long long part_stride, const long long* seg, long long y0)
{
    if (kSeg) {
        idx += seg[2 * (y0 + blockIdx.y)];
        n = seg[2 * (y0 + blockIdx.y) + 1];
    } else {
        idx += blockIdx.y * idx_stride;                      // run blockIdx.y of a batch (launch_moments_runs); 0 for one run
    }
    part += blockIdx.y * part_stride;
    __shared__ double acc[kThreads];
    const int groups = D <= kThreads ? kThreads / D : 1;
    const int g = threadIdx.x / D, d = threadIdx.x - g * D;
    if (D <= kThreads) {
        double s = 0.;
        if (g < groups)
            for (long long i = blockIdx.x + (long long)kMomBlocks * g; i < n; i += (long long)kMomBlocks * groups)
                s += u[(long long)idx[i] * D + d];
        acc[threadIdx.x] = s;
        __syncthreads();
        if (g == 0) {
            double t = 0.;
            for (int k = 0; k < groups; ++k) t += acc[k * D + d];
            part[(long long)blockIdx.x * D + d] = t;
        }
    } else {
        for (int dd = threadIdx.x; dd < D; dd += kThreads) {
            double s = 0.;
            for (long long i = blockIdx.x; i < n; i += kMomBlocks) s += u[(long long)idx[i] * D + dd];
            part[(long long)blockIdx.x * D + dd] = s;
        }
    }
}

// out[d] = (sum over blocks) * scale: four threads a column, each a quarter of the blocks in block order, the quarters added in
// order — a fixed order for a given width.  (One thread a column walked 128 dependent loads: 9.5 us a call, two calls a step.)
// kSeg: the scale is segment (y0 + blockIdx.y)'s, sc[2 (y0 + blockIdx.y)].
constexpr int kFoldCols = kThreads / 4;
template <bool kSeg>
__global__ __launch_bounds__(kThreads)
void moments_fold_kernel(const double* part, int width, double scale, double* out, long long part_stride, long long out_stride,
                         const double* sc, long long y0)
{
    if (kSeg) scale = sc[2 * (y0 + blockIdx.y)];
    part += blockIdx.y * part_stride;
    out += blockIdx.y * out_stride;
    __shared__ double q[4][kFoldCols];
    const int c = threadIdx.x % kFoldCols, k = threadIdx.x / kFoldCols;
    const int d = blockIdx.x * kFoldCols + c;
    double s = 0.;
    if (d < width)
        for (int b = k * (kMomBlocks / 4); b < (k + 1) * (kMomBlocks / 4); ++b) s += part[(long long)b * width + d];
    q[k][c] = s;
    __syncthreads();
    if (k == 0 && d < width) out[d] = ((q[0][c] + q[1][c]) + (q[2][c] + q[3][c])) * scale;
}

// partial sums of the centred products (u_j - m_j)(u_l - m_l): thread p one (j, l) pair, rows as above — staged through LDS
// kCovRows at a time (read from HBM row by row, every (j, l) pair waited ~2 us for each of its block's rows: 51 us a call at
// 16384 rows; the sums are the same terms in the same order)
constexpr int kCovRows = 32;
template <bool kSeg>
__global__ __launch_bounds__(kThreads)
void moments_cov_kernel(const double* u, const int32_t* idx, long long n, int D, const double* mean,
                        double* part /*[kMomBlocks][D*D]*/, long long idx_stride, long long part_stride, const long long* seg,
                        long long y0)
{
    if (kSeg) {
        idx += seg[2 * (y0 + blockIdx.y)];
        n = seg[2 * (y0 + blockIdx.y) + 1];
    } else {
        idx += blockIdx.y * idx_stride;
    }
    mean += (long long)blockIdx.y * D;
    part += blockIdx.y * part_stride;
    extern __shared__ double rows[];                         // [kCovRows][D], centred
    double* ms = rows + (size_t)kCovRows * D;                // [D]
    for (int d = threadIdx.x; d < D; d += kThreads) ms[d] = mean[d];
    constexpr int kPairs = 8;                                // (j, l) pairs a thread may hold: D * D <= kPairs * kThreads
    double s[kPairs];
#pragma unroll
    for (int q = 0; q < kPairs; ++q) s[q] = 0.;
    const bool in_regs = (long long)D * D <= (long long)kPairs * kThreads;
    if (!in_regs) for (int p = threadIdx.x; p < D * D; p += kThreads) part[(long long)blockIdx.x * D * D + p] = 0.;
    __syncthreads();
    for (long long i0 = blockIdx.x; i0 < n; i0 += (long long)kMomBlocks * kCovRows) {
        // this block's next kCovRows rows: i0, i0 + kMomBlocks, ...
        int nr = 0;
        for (long long i = i0; i < n && nr < kCovRows; i += kMomBlocks) ++nr;
        for (int e = threadIdx.x; e < nr * D; e += kThreads) {
            const int r = e / D, d = e - r * D;
            rows[e] = u[(long long)idx[i0 + (long long)r * kMomBlocks] * D + d] - ms[d];
        }
        __syncthreads();
        if (in_regs) {
#pragma unroll
            for (int q = 0; q < kPairs; ++q) {
                const int p = threadIdx.x + q * kThreads;
                if (p < D * D) {
                    const int j = p / D, l = p - j * D;
                    double acc = s[q];
                    for (int r = 0; r < nr; ++r) acc += rows[r * D + j] * rows[r * D + l];
                    s[q] = acc;
                }
            }
        } else {
            for (int p = threadIdx.x; p < D * D; p += kThreads) {
                const int j = p / D, l = p - j * D;
                double acc = part[(long long)blockIdx.x * D * D + p];
                for (int r = 0; r < nr; ++r) acc += rows[r * D + j] * rows[r * D + l];
                part[(long long)blockIdx.x * D * D + p] = acc;
            }
        }
        __syncthreads();
    }
    if (in_regs) {
#pragma unroll
        for (int q = 0; q < kPairs; ++q) {
            const int p = threadIdx.x + q * kThreads;
            if (p < D * D) part[(long long)blockIdx.x * D * D + p] = s[q];
        }
    }
}

// ---- the live points' order, on the device (rvll_live_sort) ----------------------------------------------------------------
// log-L -> a key whose unsigned order is the doubles' order (the sign bit flipped for positives, every bit for negatives)
__global__ __launch_bounds__(kThreads)
void sort_keys_kernel(const double* logl, long long n, unsigned long long* keys, int32_t* rows)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(logl[i]);
        keys[i] = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
        rows[i] = (int32_t)i;
    }
}

// out[i] = order[offset + rank[i]]
__global__ __launch_bounds__(kThreads)
void compose_index_kernel(const int32_t* order, long long offset, const int32_t* rank, long long n, int32_t* out)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads)
        out[i] = order[offset + rank[i]];
}

// ---- the resident ensemble (rvll_live_runs_*): R live sets of n rows, run r = rows r n .. r n + n - 1 ----------------------
// keys of the A listed runs, packed: element a n + i is row runs[a] n + i (its global row goes with it); segment a of the
// segmented sort is [a n, a n + n), its offsets in seg[0 .. A]
__global__ __launch_bounds__(kThreads)
void runs_sort_keys_kernel(const double* logl, const int32_t* runs, int A, long long n, unsigned long long* keys, int32_t* rows,
                           int32_t* seg)
{
    const long long total = (long long)A * n;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total || e <= A; e += (long long)gridDim.x * kThreads) {
        if (e <= A) seg[e] = (int32_t)(e * n);
        if (e >= total) continue;
        const long long a = e / n, g = (long long)runs[a] * n + (e - a * n);
        const unsigned long long b = (unsigned long long)__double_as_longlong(logl[g]);
        keys[e] = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
        rows[e] = (int32_t)g;
    }
}

// out[a (kdead + 1) + j] = log-L of run a's rank j (j < kdead), then of its highest (order: [A][n] global rows)
__global__ __launch_bounds__(kThreads)
void runs_sorted_logl_kernel(const double* logl, const int32_t* order, int A, long long n, long long kdead, double* out)
{
    const long long w = kdead + 1, total = (long long)A * w;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
        const long long a = e / w, j = e - a * w;
        out[e] = logl[order[a * n + (j < kdead ? j : n - 1)]];
    }
}

// walker e = a kdead + i of run a: the row that dies, dying[e] = order[a n + i], the row it starts from, start[e] =
// order[a n + kdead + rank[e]], and its place in the run-mode walk (run[e] = a, wid[e] = i)
__global__ __launch_bounds__(kThreads)
void runs_compose_kernel(const int32_t* order, int A, long long n, long long kdead, const int32_t* rank, int32_t* dying,
                         int32_t* start, int32_t* run, int32_t* wid)
{
    const long long total = (long long)A * kdead;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
        const long long a = e / kdead, i = e - a * kdead;
        dying[e] = order[a * n + i];
        start[e] = order[a * n + kdead + rank[e]];
        run[e] = (int32_t)a;
        wid[e] = (int32_t)i;
    }
}

// the clustered step (rvll_live_runs_step_clustered): listed run a's survivors, ranks kdead .. n - 1, packed in rank order as rows
// a m .. a m + m - 1 (m = n - kdead) of the clustering's row buffer; slot[e] = e (the values of the (label, rank) sort) and
// seg[a] = a m, a <= A (its segments)
__global__ __launch_bounds__(kThreads)
void runs_survivors_kernel(const double* u, const int32_t* order, int A, long long n, long long kdead, int D, double* dst,
                           int32_t* slot, int32_t* seg)
{
    const long long m = n - kdead, total = (long long)A * m * D;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total || e <= A; e += (long long)gridDim.x * kThreads) {
        if (e <= A) seg[e] = (int32_t)(e * m);
        if (e >= total) continue;
        const long long r = e / D, d = e - r * D, a = r / m;
        dst[e] = u[(long long)order[a * n + kdead + (r - a * m)] * D + d];
        if (d == 0) slot[r] = (int32_t)r;
    }
}

__global__ __launch_bounds__(kThreads)
void fill_kernel(double* p, long long n, double v)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) p[i] = v;
}

// a step's births: walker e's dying row hands its birth to the dead store (slot e, where its theta and log-L went) and takes its
// run's lstar.  One thread reads and then writes its own row: the rows are distinct, so nothing races.
__global__ __launch_bounds__(kThreads)
void births_step_kernel(const int32_t* dying, long long K, long long kdead, const double* lstar_at, double lstar, double* live_birth,
                        double* dead_birth)
{
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < K; e += (long long)gridDim.x * kThreads) {
        const int32_t r = dying[e];
        dead_birth[e] = live_birth[r];
        live_birth[r] = lstar_at ? lstar_at[(e / kdead) * kdead] : lstar;
    }
}

int blocks_for(long long total)
{
    long long b = (total + kThreads - 1) / kThreads;
    return (int)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

}  // namespace

hipError_t launch_gather_rows(const double* src, const int32_t* idx, long long n, int width, double* dst, hipStream_t st)
{
    if (n <= 0 || width <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks_for(n * width)), dim3(kThreads), 0, st, src, idx, n, width, dst);
    return hipGetLastError();
}

hipError_t launch_scatter_rows(const double* src, const int32_t* idx, long long n, int width, double* dst, hipStream_t st)
{
    if (n <= 0 || width <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(blocks_for(n * width)), dim3(kThreads), 0, st, src, idx, n, width, dst);
    return hipGetLastError();
}

size_t moments_scratch_doubles(int D) { return (size_t)kMomBlocks * D * D + (size_t)D; }

// mean[D] and cov[D*D] (divided by n - 1, as numpy's d.T @ d / (n - 1)) of the rows idx[0..n) of u; scratch:
// moments_scratch_doubles(D) doubles.  Two passes, every sum in a fixed order: the same bits for the same rows.
hipError_t launch_moments(const double* u, const int32_t* idx, long long n, int D, double* scratch, double* mean, double* cov,
                          hipStream_t st)
{
    return launch_moments_runs(u, idx, 0, 1, n, D, scratch, mean, cov, st);
}

size_t moments_runs_scratch_doubles(int D) { return (size_t)kMomBlocks * D * D; }

// The moments of A row sets in one set of four launches: set a is the rows idx[a idx_stride .. a idx_stride + n) of u, with
// scratch [A][moments_runs_scratch_doubles(D)], mean [A][D], cov [A][D*D].  Block (b, a) does what block b of launch_moments
// does for set a alone — same partition of the same rows, same order of every sum — so each set's mean and covariance are
// those of its own launch_moments, bit for bit.  (More than 65535 sets: several grids, one after the other.)
hipError_t launch_moments_runs(const double* u, const int32_t* idx, long long idx_stride, int A, long long n, int D, double* scratch,
                               double* mean, double* cov, hipStream_t st)
{
    if (n <= 0 || D <= 0 || A <= 0) return hipErrorInvalidValue;
    const long long ps = (long long)moments_runs_scratch_doubles(D);
    for (int a0 = 0; a0 < A; a0 += 65535) {
        const int na = std::min(A - a0, 65535);
        const int32_t* ix = idx + (long long)a0 * idx_stride;
        double* part = scratch + (long long)a0 * ps;
        double* m = mean + (long long)a0 * D;
        double* c = cov + (long long)a0 * D * D;
        hipLaunchKernelGGL(moments_sum_kernel<false>, dim3(kMomBlocks, na), dim3(kThreads), 0, st, u, ix, n, D, part, idx_stride, ps,
                           nullptr, 0LL);
        hipLaunchKernelGGL(moments_fold_kernel<false>, dim3((D + kFoldCols - 1) / kFoldCols, na), dim3(kThreads), 0, st, part, D,
                           1.0 / (double)n, m, ps, (long long)D, nullptr, 0LL);
        hipLaunchKernelGGL(moments_cov_kernel<false>, dim3(kMomBlocks, na), dim3(kThreads), sizeof(double) * ((size_t)kCovRows * D + D), st,
                           u, ix, n, D, m, part, idx_stride, ps, nullptr, 0LL);
        hipLaunchKernelGGL(moments_fold_kernel<false>, dim3((D * D + kFoldCols - 1) / kFoldCols, na), dim3(kThreads), 0, st, part, D * D,
                           1.0 / (double)(n > 1 ? n - 1 : 1), c, ps, (long long)D * D, nullptr, 0LL);
    }
    return hipGetLastError();
}

// Stable ascending order of logl[0..n) (ties by row, as numpy's stable argsort): keys / rows are scratch of n each (in and out),
// temp of sort_temp_bytes(n) bytes; order_out[n] receives the rows, sorted_out[n] (or null) the sorted keys' log-L is not
// returned — the caller gathers what it needs by index.
size_t sort_temp_bytes(long long n)
{
    size_t bytes = 0;
    unsigned long long* k = nullptr;
    int32_t* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)n, 0, 64, (hipStream_t) nullptr);
    return bytes;
}

hipError_t launch_sort_logl(const double* logl, long long n, unsigned long long* keys_in, unsigned long long* keys_out, int32_t* rows_in,
                            int32_t* order_out, void* temp, size_t temp_bytes, hipStream_t st)
{
    if (n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sort_keys_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, logl, n, keys_in, rows_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, rows_in, order_out, (size_t)n, 0, 64, st);
}

hipError_t launch_compose_index(const int32_t* order, long long offset, const int32_t* rank, long long n, int32_t* out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(compose_index_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, order, offset, rank, n, out);
    return hipGetLastError();
}

// ---- the resident ensemble ----------------------------------------------------------------------------------------------------
// Every listed run's own stable ascending order of its log-L, as global rows, in one segmented radix sort over the A n packed
// keys: order_out[a n + i] = the row of rank i in run runs[a] — what launch_sort_logl gives that run alone (a stable order by
// (key, row) is unique).  keys / rows: A n scratch each (keys twice that), seg: A + 1 ints, runs: A ints on the device.
size_t runs_sort_temp_bytes(int A, long long n)
{
    size_t bytes = 0;
    unsigned long long* k = nullptr;
    int32_t* v = nullptr;
    (void)rocprim::segmented_radix_sort_pairs(nullptr, bytes, k, k, v, v, (unsigned int)(A * n), (unsigned int)A, v, v + 1, 0, 64,
                                              (hipStream_t) nullptr);
    return bytes;
}

hipError_t launch_runs_sort(const double* logl, const int32_t* runs, int A, long long n, unsigned long long* keys_in,
                            unsigned long long* keys_out, int32_t* rows_in, int32_t* seg, int32_t* order_out, void* temp,
                            size_t temp_bytes, hipStream_t st)
{
    if (A <= 0 || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(runs_sort_keys_kernel, dim3(blocks_for((long long)A * n + 1)), dim3(kThreads), 0, st, logl, runs, A, n, keys_in,
                       rows_in, seg);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rocprim::segmented_radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, rows_in, order_out, (unsigned int)(A * n),
                                               (unsigned int)A, seg, seg + 1, 0, 64, st);
}

hipError_t launch_runs_sorted_logl(const double* logl, const int32_t* order, int A, long long n, long long kdead, double* out, hipStream_t st)
{
    hipLaunchKernelGGL(runs_sorted_logl_kernel, dim3(blocks_for((long long)A * (kdead + 1))), dim3(kThreads), 0, st, logl, order, A, n,
                       kdead, out);
    return hipGetLastError();
}

hipError_t launch_runs_compose(const int32_t* order, int A, long long n, long long kdead, const int32_t* rank, int32_t* dying,
                               int32_t* start, int32_t* run, int32_t* wid, hipStream_t st)
{
    hipLaunchKernelGGL(runs_compose_kernel, dim3(blocks_for((long long)A * kdead)), dim3(kThreads), 0, st, order, A, n, kdead, rank,
                       dying, start, run, wid);
    return hipGetLastError();
}

// ---- the clustered step of the resident ensemble ------------------------------------------------------------------------------
hipError_t launch_runs_survivors(const double* u, const int32_t* order, int A, long long n, long long kdead, int D, double* dst,
                                 int32_t* slot, int32_t* seg, hipStream_t st)
{
    if (A <= 0 || kdead >= n || D <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(runs_survivors_kernel, dim3(blocks_for((long long)A * (n - kdead) * D + 1)), dim3(kThreads), 0, st, u, order, A,
                       n, kdead, D, dst, slot, seg);
    return hipGetLastError();
}

// Every run's stable order by cluster label: one segmented radix sort of the A m labels (values: slots a m + j in rank order, so ties
// keep rank order), segment a = [seg[a], seg[a + 1]).  The labels are below 2^31.
size_t label_sort_temp_bytes(int A, long long total)
{
    size_t bytes = 0;
    unsigned int* k = nullptr;
    int32_t* v = nullptr;
    (void)rocprim::segmented_radix_sort_pairs(nullptr, bytes, k, k, v, v, (unsigned int)total, (unsigned int)A, v, v + 1, 0, 32,
                                              (hipStream_t) nullptr);
    return bytes;
}

hipError_t launch_label_sort(const int32_t* labels, int32_t* labels_out, const int32_t* slot_in, int32_t* slot_out, int A, long long total,
                             const int32_t* seg, void* temp, size_t temp_bytes, hipStream_t st)
{
    if (A <= 0 || total <= 0) return hipErrorInvalidValue;
    return rocprim::segmented_radix_sort_pairs(temp, temp_bytes, reinterpret_cast<const unsigned int*>(labels),
                                               reinterpret_cast<unsigned int*>(labels_out), slot_in, slot_out, (unsigned int)total,
                                               (unsigned int)A, seg, seg + 1, 0, 32, st);
}

// The moments of S ragged segments in one set of four launches per chunk of up to `chunk` segments: segment s is the rows
// idx[seg[2 s] .. seg[2 s] + seg[2 s + 1]) of u, sc[2 s] = 1 / rows and sc[2 s + 1] = 1 / (rows - 1) (rows > 1) its fold scales as
// launch_moments forms them.  Block (b, s) does what block b of launch_moments does for segment s alone, so each segment's mean
// [S][D] and covariance [S][D, D] are those of its own launch_moments, bit for bit.  seg, sc on the device; scratch: chunk x
// moments_runs_scratch_doubles(D) doubles (the chunks reuse it, in stream order).
hipError_t launch_moments_segs(const double* u, const int32_t* idx, const long long* seg, const double* sc, int S, int D, double* scratch,
                               int chunk, double* mean, double* cov, hipStream_t st)
{
    if (S <= 0 || D <= 0 || chunk <= 0) return hipErrorInvalidValue;
    const long long ps = (long long)moments_runs_scratch_doubles(D);
    chunk = std::min(chunk, 65535);
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int ns = std::min(S - s0, chunk);
        double* m = mean + (long long)s0 * D;
        double* c = cov + (long long)s0 * D * D;
        hipLaunchKernelGGL(moments_sum_kernel<true>, dim3(kMomBlocks, ns), dim3(kThreads), 0, st, u, idx, 0LL, D, scratch, 0LL, ps, seg,
                           (long long)s0);
        hipLaunchKernelGGL(moments_fold_kernel<true>, dim3((D + kFoldCols - 1) / kFoldCols, ns), dim3(kThreads), 0, st, scratch, D, 0.0,
                           m, ps, (long long)D, sc, (long long)s0);
        hipLaunchKernelGGL(moments_cov_kernel<true>, dim3(kMomBlocks, ns), dim3(kThreads), sizeof(double) * ((size_t)kCovRows * D + D), st,
                           u, idx, 0LL, D, m, scratch, 0LL, ps, seg, (long long)s0);
        hipLaunchKernelGGL(moments_fold_kernel<true>, dim3((D * D + kFoldCols - 1) / kFoldCols, ns), dim3(kThreads), 0, st, scratch,
                           D * D, 0.0, c, ps, (long long)D * D, sc + 1, (long long)s0);
    }
    return hipGetLastError();
}

// ---- birth contours (rvll_live_births, rvll_live_runs_births) -----------------------------------------------------------------
hipError_t launch_fill(double* p, long long n, double v, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, p, n, v);
    return hipGetLastError();
}

hipError_t launch_births_step(const int32_t* dying, long long K, long long kdead, const double* lstar_at, double lstar, double* live_birth,
                              double* dead_birth, hipStream_t st)
{
    if (K <= 0 || kdead <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(births_step_kernel, dim3(blocks_for(K)), dim3(kThreads), 0, st, dying, K, kdead, lstar_at, lstar, live_birth,
                       dead_birth);
    return hipGetLastError();
}

}  // namespace rvll
