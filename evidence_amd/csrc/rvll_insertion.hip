// Insertion indexes of finished nested-sampling runs on gfx950 (Fowlie, Handley & Su 2020): for every row born on a contour b,
// its rank among the live points right after it was inserted, and how many there were.  evidence_amd/insertion.py holds the numpy
// definition; DESIGN §4g.
//
// For row j of run r with birth b > -inf:
//     live(j)  = { k in r : birth_k <= b < logl_k }
//     n_at[j]  = |live(j)|            = #{birth <= b} - #{logl <= b} + #{k : logl_k <= b < birth_k}
//     index[j] = #{k in live(j) : logl_k < logl_j}
//              = #{k : birth_k <= b} over the band b < logl_k < logl_j of the run's rows sorted by log-L
// The last term of n_at only counts off-contour rows (logl_k <= birth_k; the exact redo of a wandering solve can lower an
// accepted end point to lstar or below), which are rare: the host lists them per run and every row scans its run's list.
//
// Device work, per chunk of whole runs (a chunk holds below 2^31 rows):
//     keys      the doubles in place as uint64 keys whose order is theirs (-0.0 canonicalised to +0.0, so key comparisons are
//               double comparisons)
//     sorts     one rocPRIM segmented radix sort of the log-L keys carrying the birth keys (SL, BL), one of the birth keys (SB)
//     counts    one wave64 per row: three binary searches in SL / SB, the band [upper_bound(SL, b), lower_bound(SL, logl_j))
//               of BL read 64 keys per coalesced load and counted by __ballot / __popcll, the off-contour list likewise.
//               No LDS, no atomics: a row's outputs depend on its own run alone, the same in any batch and from call to call.
// The band is O(nlive) long for a sampler that inserts above its lowest live point, so the pass is O(rows nlive).
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>

#pragma GCC visibility push(default)
#include "rvll.h"
#pragma GCC visibility pop
#include "rvll_keys.h"

namespace rvll {
int report_error(int code, const char* fmt, ...);
}

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWavesPerBlock = kThreads / kWave;
constexpr int kMaxBlocks = 8192;
constexpr long long kChunkRows = (1ll << 31) - 1;         // rows of one chunk: rocPRIM's sizes and our offsets are 32-bit
constexpr unsigned long long kKeyNegInf = 0x000FFFFFFFFFFFFFull;   // key(-inf)

typedef unsigned long long u64;

#define INS_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            status = rvll::report_error(e_ == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, \
                                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                        __FILE__, __LINE__);                                   \
            goto done;                                                                         \
        }                                                                                      \
    } while (0)

using rvll::key_of;                                          // -0.0 and +0.0 compare equal: one key

// the two double columns, in place, as keys
__global__ __launch_bounds__(kThreads)
void keys_kernel(u64* a, u64* b, long long n)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        a[i] = key_of(__longlong_as_double((long long)a[i]));
        b[i] = key_of(__longlong_as_double((long long)b[i]));
    }
}

// first position in s[0 .. n) whose key is > v (upper) or >= v (lower); every lane searches alike (uniform addresses)
__device__ inline int upper_bound(const u64* s, int n, u64 v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline int lower_bound(const u64* s, int n, u64 v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wave per row j of the chunk (rows 0 .. n), runs seg[0 .. nruns]; off_l / off_b [off_seg[r] .. off_seg[r + 1]): run r's
// off-contour rows
__global__ __launch_bounds__(kThreads)
void counts_kernel(const u64* kl, const u64* kb, const u64* sl, const u64* bl, const u64* sb, const int32_t* seg, int nruns,
                   const u64* off_l, const u64* off_b, const int32_t* off_seg, long long n, int32_t* index, int32_t* n_at)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long waves = (long long)gridDim.x * kWavesPerBlock;
    for (long long j = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); j < n; j += waves) {
        const u64 b = kb[j];
        if (b == kKeyNegInf) {
            if (lane == 0) { index[j] = -1; n_at[j] = -1; }
            continue;
        }
        // the run of row j: the last r with seg[r] <= j
        int lo = 0, hi = nruns;
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (seg[mid] <= j) lo = mid; else hi = mid;
        }
        const int r = lo, s0 = seg[r], m = seg[r + 1] - s0;
        const int below_l = upper_bound(sl + s0, m, b);      // #{logl <= b}: the band starts here
        const int below_b = upper_bound(sb + s0, m, b);      // #{birth <= b}
        const int band_end = lower_bound(sl + s0, m, kl[j]); // #{logl < logl_j}
        int off = 0;
        for (long long k0 = off_seg[r]; k0 < off_seg[r + 1]; k0 += kWave) {
            const long long k = k0 + lane;
            const bool hit = k < off_seg[r + 1] && off_l[k] <= b && b < off_b[k];
            off += __popcll(__ballot(hit));
        }
        int cnt = 0;
        const long long band_hi = (long long)s0 + band_end;
        for (long long k0 = (long long)s0 + below_l; k0 < band_hi; k0 += kWave) {
            const long long k = k0 + lane;
            cnt += __popcll(__ballot(k < band_hi && bl[k] <= b));
        }
        if (lane == 0) {
            index[j] = cnt;
            n_at[j] = below_b - below_l + off;
        }
    }
}

int blocks_for(long long total, int per_block)
{
    const long long b = (total + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > kMaxBlocks ? kMaxBlocks : b);
}

}  // namespace

extern "C" int rvll_insertion_indexes(int32_t device, const double* logl, const double* birth, int64_t n_rows, const int64_t* run_start,
                                      int32_t n_runs, int32_t* index_out, int32_t* n_at_out, rvll_insertion_timing* timing)
{
    const auto t_start = std::chrono::steady_clock::now();
    if (n_runs < 1) return rvll::report_error(RVLL_E_INVALID, "n_runs must be >= 1");
    if (n_rows < 0) return rvll::report_error(RVLL_E_INVALID, "negative n_rows");
    if (!run_start || (n_rows > 0 && (!logl || !birth || !index_out || !n_at_out)))
        return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (run_start[0] != 0 || run_start[n_runs] != n_rows)
        return rvll::report_error(RVLL_E_INVALID, "run_start must run from 0 to n_rows = %lld", (long long)n_rows);
    for (int32_t r = 0; r < n_runs; ++r) {
        const long long rows = run_start[r + 1] - run_start[r];
        if (rows < 0) return rvll::report_error(RVLL_E_INVALID, "run_start must be non-decreasing (run %d)", (int)r);
        if (rows > kChunkRows) return rvll::report_error(RVLL_E_INVALID, "run %d has %lld rows: at most 2^31 - 1", (int)r, rows);
    }
    for (int64_t i = 0; i < n_rows; ++i)
        if (std::isnan(logl[i]) || std::isnan(birth[i]))
            return rvll::report_error(RVLL_E_INVALID, "row %lld: NaN log-L or birth", (long long)i);
    if (timing) *timing = rvll_insertion_timing{0., 0., n_rows, 0, kThreads};
    if (n_rows == 0) return RVLL_OK;

    // chunks of whole runs below 2^31 rows; the largest sizes the device blocks
    std::vector<int32_t> chunk_first(1, 0);
    for (int32_t r = 0; r < n_runs; ++r)
        if (run_start[r + 1] - run_start[chunk_first.back()] > kChunkRows) chunk_first.push_back(r);
    chunk_first.push_back(n_runs);
    long long max_rows = 0, max_runs = 0, max_off = 0;
    // off-contour rows (a birth above -inf, logl <= birth), per run, as keys
    std::vector<int64_t> off_start((size_t)n_runs + 1, 0);
    std::vector<u64> off_l, off_b;
    for (int32_t r = 0; r < n_runs; ++r) {
        for (int64_t i = run_start[r]; i < run_start[r + 1]; ++i)
            if (birth[i] > -INFINITY && logl[i] <= birth[i]) { off_l.push_back(key_of(logl[i])); off_b.push_back(key_of(birth[i])); }
        off_start[(size_t)r + 1] = (int64_t)off_l.size();
    }
    for (size_t c = 0; c + 1 < chunk_first.size(); ++c) {
        const int32_t r0 = chunk_first[c], r1 = chunk_first[c + 1];
        max_rows = std::max<long long>(max_rows, run_start[r1] - run_start[r0]);
        max_runs = std::max<long long>(max_runs, r1 - r0);
        max_off = std::max<long long>(max_off, off_start[(size_t)r1] - off_start[(size_t)r0]);
    }

    int status = RVLL_OK;
    int prev_device = -1;
    u64 *d_kl = nullptr, *d_kb = nullptr, *d_sl = nullptr, *d_bl = nullptr, *d_sb = nullptr, *d_off = nullptr;
    int32_t *d_seg = nullptr, *d_offseg = nullptr, *d_index = nullptr, *d_nat = nullptr;
    void* d_temp = nullptr;
    size_t temp_bytes = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double kernel_ms = 0.;
    int launches = 0;
    std::vector<int32_t> seg, offseg;

    {
        size_t b1 = 0, b2 = 0;
        u64* k = nullptr;
        int32_t* o = nullptr;
        INS_TRY(rocprim::segmented_radix_sort_pairs(nullptr, b1, k, k, k, k, (unsigned int)max_rows, (unsigned int)max_runs, o, o + 1, 0, 64,
                                                    (hipStream_t) nullptr));
        INS_TRY(rocprim::segmented_radix_sort_keys(nullptr, b2, k, k, (unsigned int)max_rows, (unsigned int)max_runs, o, o + 1, 0, 64,
                                                   (hipStream_t) nullptr));
        temp_bytes = std::max<size_t>(std::max(b1, b2), 1);
    }
    INS_TRY(hipGetDevice(&prev_device));
    if (device >= 0) INS_TRY(hipSetDevice(device));
    INS_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) INS_TRY(hipEventCreate(&e));
    // every device block before the first launch: running out of memory fails the call before any work
    INS_TRY(hipMalloc(&d_kl, sizeof(u64) * (size_t)max_rows));
    INS_TRY(hipMalloc(&d_kb, sizeof(u64) * (size_t)max_rows));
    INS_TRY(hipMalloc(&d_sl, sizeof(u64) * (size_t)max_rows));
    INS_TRY(hipMalloc(&d_bl, sizeof(u64) * (size_t)max_rows));
    INS_TRY(hipMalloc(&d_sb, sizeof(u64) * (size_t)max_rows));
    INS_TRY(hipMalloc(&d_off, sizeof(u64) * (size_t)std::max<long long>(2 * max_off, 1)));
    INS_TRY(hipMalloc(&d_seg, sizeof(int32_t) * (size_t)(max_runs + 1)));
    INS_TRY(hipMalloc(&d_offseg, sizeof(int32_t) * (size_t)(max_runs + 1)));
    INS_TRY(hipMalloc(&d_index, sizeof(int32_t) * (size_t)max_rows));
    INS_TRY(hipMalloc(&d_nat, sizeof(int32_t) * (size_t)max_rows));
    INS_TRY(hipMalloc(&d_temp, temp_bytes));
    for (size_t c = 0; c + 1 < chunk_first.size(); ++c) {
        const int32_t r0 = chunk_first[c], r1 = chunk_first[c + 1], nr = r1 - r0;
        const long long row0 = run_start[r0], rows = run_start[r1] - row0;
        const long long o0 = off_start[(size_t)r0], noff = off_start[(size_t)r1] - o0;
        if (rows == 0) continue;
        seg.resize((size_t)nr + 1);
        offseg.resize((size_t)nr + 1);
        for (int32_t r = 0; r <= nr; ++r) {
            seg[(size_t)r] = (int32_t)(run_start[r0 + r] - row0);
            offseg[(size_t)r] = (int32_t)(off_start[(size_t)(r0 + r)] - o0);
        }
        INS_TRY(hipMemcpyAsync(d_kl, logl + row0, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice, stream));
        INS_TRY(hipMemcpyAsync(d_kb, birth + row0, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice, stream));
        INS_TRY(hipMemcpyAsync(d_seg, seg.data(), sizeof(int32_t) * seg.size(), hipMemcpyHostToDevice, stream));
        INS_TRY(hipMemcpyAsync(d_offseg, offseg.data(), sizeof(int32_t) * offseg.size(), hipMemcpyHostToDevice, stream));
        if (noff > 0) {
            INS_TRY(hipMemcpyAsync(d_off, off_l.data() + o0, sizeof(u64) * (size_t)noff, hipMemcpyHostToDevice, stream));
            INS_TRY(hipMemcpyAsync(d_off + noff, off_b.data() + o0, sizeof(u64) * (size_t)noff, hipMemcpyHostToDevice, stream));
        }
        INS_TRY(hipEventRecord(ev[0], stream));
        hipLaunchKernelGGL(keys_kernel, dim3(blocks_for(rows, kThreads)), dim3(kThreads), 0, stream, d_kl, d_kb, rows);
        INS_TRY(hipGetLastError());
        INS_TRY(rocprim::segmented_radix_sort_pairs(d_temp, temp_bytes, d_kl, d_sl, d_kb, d_bl, (unsigned int)rows, (unsigned int)nr,
                                                    d_seg, d_seg + 1, 0, 64, stream));
        INS_TRY(rocprim::segmented_radix_sort_keys(d_temp, temp_bytes, d_kb, d_sb, (unsigned int)rows, (unsigned int)nr, d_seg, d_seg + 1,
                                                   0, 64, stream));
        hipLaunchKernelGGL(counts_kernel, dim3(blocks_for(rows, kWavesPerBlock)), dim3(kThreads), 0, stream, d_kl, d_kb, d_sl, d_bl, d_sb,
                           d_seg, (int)nr, d_off, d_off + noff, d_offseg, rows, d_index, d_nat);
        INS_TRY(hipGetLastError());
        INS_TRY(hipEventRecord(ev[1], stream));
        launches += 4;
        INS_TRY(hipMemcpyAsync(index_out + row0, d_index, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToHost, stream));
        INS_TRY(hipMemcpyAsync(n_at_out + row0, d_nat, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToHost, stream));
        INS_TRY(hipStreamSynchronize(stream));
        float ms = 0.f;
        INS_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        kernel_ms += ms;
    }
    if (timing) {
        timing->kernel_ms = kernel_ms;
        timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        timing->rows = n_rows;
        timing->launches = launches;
        timing->threads = kThreads;
    }

done:
    for (void* p : {(void*)d_kl, (void*)d_kb, (void*)d_sl, (void*)d_bl, (void*)d_sb, (void*)d_off, (void*)d_seg, (void*)d_offseg,
                    (void*)d_index, (void*)d_nat, d_temp})
        if (p) (void)hipFree(p);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (prev_device >= 0 && device >= 0) (void)hipSetDevice(prev_device);
    return status;
}
