// rvll_batch_route.h — which transport a host-buffer batch call takes (rvll_batch.hip), and where its bytes lie: the measurement
// switches, the route of each entry point, the layouts of the pinned result block and of a streamed staging block, the two chunk
// partitions.  Integer arithmetic without a HIP call or a handle, so tests/test_batch_route_host.py builds it with a host compiler
// and holds it against the same rules stated in numpy.
#pragma once
#include <unistd.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

constexpr size_t kPinBytes = 1u << 20;          // each of the two mapped pinned blocks of a handle (pin_in, pin_out)
// rvll_loglike_batch: host batches from kSplitMinPoints on go up in overlapped chunks of about kSplitChunkPoints
constexpr long long kSplitMinPoints = 16384, kSplitChunkPoints = 16384, kSplitMaxChunks = 8;   // profiles/r02_split_probe.txt
constexpr long long kFusedSplitMaxPoints = 131072;   // rvll_prior_loglike_batch: two halves from kSplitMinPoints up to here
constexpr size_t kStreamMinBytes = 24u << 20;   // cube -> theta -> log-L host batches whose rows take this much are streamed (stream_host_batch)
constexpr long long kStreamChunkRows = 16384;   // ... in chunks of this many rows
constexpr size_t kPriorZeroCopyBytes = 384 * 1024;   // rvll_prior_batch: cubes up to here are read from, and theta written to, the pinned blocks

namespace rvll {
namespace host {

constexpr size_t kDownloadStagedMin = 32u << 20;   // rvll_dev_download: theta of this size and more comes down through the staging blocks

// ---- the measurement switches: read on every call (tests and scripts/*_probe.py change them on a live handle) ----
struct BatchSwitches {
    size_t zero_copy_in = kPinBytes;   // RVLL_ZERO_COPY_IN_KB: theta rows up to here go through the pinned block (bytes)
    bool stream_loglike = false;       // RVLL_STREAM_LOGLIKE: rvll_loglike_batch may take the streamed route
    long long stream_min = 0;          // RVLL_STREAM_MIN: rows from which a batch is streamed (0: from kStreamMinBytes of rows)
    int split = 0;                     // RVLL_SPLIT: chunks of the two-lane route (0: the route's own rule)
    bool no_pinned_out = false;        // RVLL_NO_PINNED_OUT: no results through the pinned block
    long long stream_chunk = kStreamChunkRows;   // RVLL_STREAM_CHUNK: rows of a streamed chunk
    int stream_lag = 2;                // RVLL_STREAM_LAG: chunks the calling thread runs ahead of the results it waits for
    bool stream_timing = false;        // RVLL_STREAM_TIMING: report where the calling thread waited
    int copy_threads = 0;              // RVLL_COPY_THREADS: workers of a copy pool made by this call (0: by the machine)
};

// One pass over the environment that looks no further than an entry's first letters unless they are RVLL_: it costs less than
// one getenv.  The calls of a few rows take 20 us; a getenv per switch would add most of a microsecond to each, and even a
// strncmp per entry measured 0.1 - 0.3 us on them.
inline BatchSwitches read_batch_switches()
{
    BatchSwitches s;
    for (char** e = environ; e && *e; ++e) {
        const char* p = *e;
        if (p[0] != 'R' || p[1] != 'V' || p[2] != 'L' || p[3] != 'L' || p[4] != '_') continue;
        const char* name = p + 5;
        const char* eq = strchr(name, '=');
        if (!eq) continue;
        auto is = [&](const char* key) { return strlen(key) == (size_t)(eq - name) && strncmp(name, key, (size_t)(eq - name)) == 0; };
        if (is("ZERO_COPY_IN_KB")) s.zero_copy_in = std::min((size_t)std::max(0, atoi(eq + 1)) * 1024, kPinBytes);
        else if (is("STREAM_LOGLIKE")) s.stream_loglike = true;
        else if (is("STREAM_MIN")) s.stream_min = std::max(1ll, atoll(eq + 1));
        else if (is("SPLIT")) s.split = std::max(1, std::min(64, atoi(eq + 1)));
        else if (is("NO_PINNED_OUT")) s.no_pinned_out = true;
        else if (is("STREAM_CHUNK")) s.stream_chunk = std::max(256, atoi(eq + 1));
        else if (is("STREAM_LAG")) s.stream_lag = std::max(1, std::min(2, atoi(eq + 1)));
        else if (is("STREAM_TIMING")) s.stream_timing = true;
        else if (is("COPY_THREADS")) s.copy_threads = std::max(1, std::min(32, atoi(eq + 1)));
    }
    return s;
}

// ---- the routes ----
//   kZeroCopy   rows by memcpy into pin_in, the kernels read and write the mapped blocks: no copy command either way
//   kPinnedOut  one upload, one launch whose results are stores into the mapped result block
//   kSplit      nsplit chunks alternating between lanes 0 and 1
//   kStreamed   chunks of chunk_rows rows through pinned staging blocks, the host's copies on worker threads
//   kResident   rvll_dev_upload_*, the resident launches, rvll_dev_download
enum class Transport { kZeroCopy, kPinnedOut, kSplit, kStreamed, kResident };

struct BatchRoute {
    Transport transport;
    int nsplit;               // kSplit
    bool out_pinned;          // log-L and flags (kZeroCopy of the fused call: theta too) leave through the pinned result block
    long long chunk_rows;     // kStreamed
    int lag;                  // kStreamed
};

inline size_t row_bytes(long long B, int ndim) { return sizeof(double) * (size_t)B * (size_t)ndim; }
inline size_t result_bytes(long long B) { return (sizeof(double) + sizeof(int32_t)) * (size_t)B; }

// Streamed from 24 MB of rows on (165565 points at 19 parameters).  Below, the two-chunk route copies straight from and to the
// caller's arrays and is level or ahead (131072 rows: 1.04 - 1.08 ms against 1.0 - 1.2 ms); above, the caller's arrays are
// fresh mappings every call (glibc's 32 MB mmap threshold), the runtime's cache of pinned ranges misses, and that route
// collapses (262144 rows: 3.5 - 4.1 ms against 1.9 - 2.2 ms; profiles/r03_stream_probe.txt).
inline long long stream_min_points(int ndim, const BatchSwitches& sw)
{
    return sw.stream_min ? sw.stream_min : (long long)((kStreamMinBytes + row_bytes(1, ndim) - 1) / row_bytes(1, ndim));
}

inline BatchRoute streamed_route(const BatchSwitches& sw) { return {Transport::kStreamed, 1, false, sw.stream_chunk, sw.stream_lag}; }

inline BatchRoute loglike_route(long long B, int ndim, const BatchSwitches& sw)
{
    const size_t nin = row_bytes(B, ndim), nout = result_bytes(B);
    // results that fit the pinned block (87381 points) leave the kernels as stores into mapped host memory: no download commands
    // behind the last kernel, one memcpy on the host
    const bool out_pinned = nout <= kPinBytes && !sw.no_pinned_out;
    // theta rows that fit the pinned block (6898 points at 19 parameters) go there by memcpy and are read by the kernel
    // over PCIe: 10 us less than an upload command at 512 .. 4096 points
    if (nin <= sw.zero_copy_in && nout <= kPinBytes) return {Transport::kZeroCopy, 1, true, 0, 0};
    // (theta -> log-L has no large download: the runtime's own staged upload from pageable memory is as fast as ours and the
    //  chunked route below wins at every size, fresh arrays or kept ones — profiles/r03_stream_probe.txt; streamed only by switch)
    if (sw.stream_loglike && B >= stream_min_points(ndim, sw)) return streamed_route(sw);
    int nsplit = B >= kSplitMinPoints ? (int)std::min<long long>(kSplitMaxChunks, std::max<long long>(2, B / kSplitChunkPoints)) : 1;
    if (sw.split) nsplit = sw.split;
    if (nsplit > 1 && B >= 2 * nsplit) return {Transport::kSplit, nsplit, out_pinned, 0, 0};
    return {out_pinned ? Transport::kPinnedOut : Transport::kResident, 1, out_pinned, 0, 0};
}

inline BatchRoute prior_route(long long B, int ndim, const BatchSwitches& sw)
{
    // a vectorized prior callback of up to 2586 points (19 parameters; beyond, the two host memcpys cost more than they save)
    if (row_bytes(B, ndim) <= kPriorZeroCopyBytes && !sw.no_pinned_out) return {Transport::kZeroCopy, 1, true, 0, 0};
    return {Transport::kResident, 1, false, 0, 0};
}

inline BatchRoute prior_loglike_route(long long B, int ndim, bool all_direct, const BatchSwitches& sw)
{
    // a sampler's proposal round (up to 6393 points at 19 parameters): cube, theta, log-L and flags all fit the pinned blocks.
    // One launch needs every Beta / Gamma prior to have a verified table (all_direct).
    if (row_bytes(B, ndim) + result_bytes(B) + 16 <= kPinBytes && all_direct && !sw.no_pinned_out)
        return {Transport::kZeroCopy, 1, true, 0, 0};
    if (B >= stream_min_points(ndim, sw)) return streamed_route(sw);
    // measured (profiles/r01_split_probe.txt): two halves help from 16384 points (+15 %) to 65536 (+35 %); more chunks
    // lose to the per-copy fixed costs, and at 262144 points the large pageable downloads on two streams collapse
    int nsplit = (B >= kSplitMinPoints && B <= kFusedSplitMaxPoints) ? 2 : 1;
    if (sw.split) nsplit = sw.split;
    if (nsplit > 1 && B >= 2 * nsplit) return {Transport::kSplit, nsplit, false, 0, 0};
    return {Transport::kResident, 1, false, 0, 0};
}

// rvll_dev_download of B rows (theta, log-L, flags as asked for)
//   kPinned       small: one pinned landing zone, one sync
//   kDirect       copy commands straight into the caller's arrays
//   kStagedTheta  ... but theta, from kDownloadStagedMin on, through the pinned staging blocks (download_rows)
enum class Download { kPinned, kDirect, kStagedTheta };

inline Download download_route(long long B, int ndim, bool theta, bool logL, bool flags)
{
    const size_t nt = theta ? row_bytes(B, ndim) : 0;
    const size_t nl = logL ? sizeof(double) * (size_t)B : 0, nf = flags ? sizeof(int32_t) * (size_t)B : 0;
    if (nt + nl + nf <= kPinBytes) return Download::kPinned;
    return nt >= kDownloadStagedMin ? Download::kStagedTheta : Download::kDirect;
}

// ---- layouts (byte offsets) ----
// The pinned result block of B rows: log-L, flags (they end on a multiple of 4 bytes), and for the fused call theta on the next
// multiple of 16.  theta <= 12 B + 15, and the fused zero-copy route is taken only when 8 B D + 12 B + 16 <= kPinBytes, so
// theta's 8 B D bytes always end inside the block (the check that they do, "pinned block too small", could never fire).
struct PinnedResult { size_t logL, flags, theta; };

inline PinnedResult pinned_result(long long B) { return {0, sizeof(double) * (size_t)B, (result_bytes(B) + 15) & ~(size_t)15}; }

// A staging block of a streamed batch in chunks of `rows` rows: the rows on the way up; theta, log-L, flags on the way down
struct StageBlock { size_t in_bytes, theta, logL, flags, out_bytes; };

inline StageBlock stage_block(long long rows, int ndim)
{
    return {row_bytes(rows, ndim), 0, row_bytes(rows, ndim), row_bytes(rows, ndim + 1), row_bytes(rows, ndim + 1) + sizeof(int32_t) * (size_t)rows};
}

// ---- chunk partitions: rows [lo, hi) of chunk c ----
struct Rows { long long lo, hi; };

inline Rows split_chunk(long long B, int nsplit, int c) { return {B * c / nsplit, B * (c + 1) / nsplit}; }

inline int stream_chunks(long long B, long long rows) { return (int)((B + rows - 1) / rows); }
inline Rows stream_chunk(long long B, long long rows, int c) { return {(long long)c * rows, std::min<long long>(B, (long long)(c + 1) * rows)}; }

}  // namespace host
}  // namespace rvll
