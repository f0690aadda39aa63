// rvll_batch.hip — the calls that take and return host arrays: rvll_loglike_batch, rvll_prior_batch, rvll_prior_loglike_batch (what
// every sampler callback goes through), and the uploads and the download of the device-resident forms.  Each entry point checks its
// arguments, asks rvll_batch_route.h which transport the size of the call takes, and runs that transport; the transports are
// built from one set of steps.  Whatever the route, the same kernels run on the same rows: the same bits
// (tests/test_gpu_boundary.py runs every size class).
#include <chrono>
#include <exception>
#include <thread>

#include "rvll_host.h"

using rvll::report_error;
using namespace rvll::host;

namespace {

// ---- the steps the transports share ---------------------------------------------------------------------------------------------

// Runs a route's `settle` on every way out of it, so that plain HIP_TRY and RVLL_TRY work inside the route: no call returns while
// a copy into or out of the caller's arrays, or a worker's copy, is still in flight, and the copy pool is left not busy.
template <typename F>
struct Settled {
    F settle;
    bool armed = true;                      // (set false once everything the route started has been waited for)
    explicit Settled(F f) : settle(f) {}
    ~Settled() { run(); }
    void run() { if (armed) { armed = false; settle(); } }
};

// log-L, flags and theta of B rows in the mapped result block (rvll_batch_route.h, pinned_result): at `base` = pin_out_dev as the
// kernels address them, at pin_out as the host reads them
struct ResultBlock { double* logL; int32_t* flags; double* theta; };

ResultBlock result_block(void* base, int64_t B)
{
    const PinnedResult p = pinned_result(B);
    char* out = static_cast<char*>(base);
    return {reinterpret_cast<double*>(out + p.logL), reinterpret_cast<int32_t*>(out + p.flags), reinterpret_cast<double*>(out + p.theta)};
}

// ... and out of it into the caller's arrays, once the stream that wrote it has been waited for
void pinned_copy_out(const rvll_handle* h, int64_t B, double* theta_out, double* logL, int32_t* flags)
{
    const ResultBlock out = result_block(h->pin_out, B);
    memcpy(logL, out.logL, sizeof(double) * (size_t)B);
    if (flags) memcpy(flags, out.flags, sizeof(int32_t) * (size_t)B);
    if (theta_out) memcpy(theta_out, out.theta, row_bytes(B, h->L.ndim));
}

// The chunk step: rows [lo, lo + m) of the resident input — unit-cube rows if in_is_cube, which the prior kernels turn into theta
// rows first — to log-L and flags at out_l + lo and out_f + lo, on `st`.
int chunk_step(rvll_handle* h, bool in_is_cube, long long lo, long long m, double* out_l, int32_t* out_f, hipStream_t st)
{
    const long long D = h->L.ndim;
    if (in_is_cube) {
        rvll::PriorArgs pa{h->d_cube + lo * D, h->d_theta + lo * D, m, h->L.ndim, h->d_priors, h->d_heavy, h->n_heavy};
        HIP_TRY(rvll::launch_prior(pa, st));
    }
    rvll::LoglikeArgs a;
    int cu = 0;
    RVLL_TRY(build_args(h, h->d_theta + lo * D, out_l + lo, out_f + lo, m, &a, &cu));
    HIP_TRY(launch_form(a, cu, st));
    return RVLL_OK;
}

// rvll_dev_upload_theta / rvll_dev_upload_cube
int upload_rows(rvll_handle* h, const double* rows, int64_t B, bool cube)
{
    RVLL_TRY(rvll_dev_reserve(h, B));
    if (B == 0) return RVLL_OK;
    if (!rows) return report_error(RVLL_E_INVALID, "%s is null", cube ? "cube" : "theta");
    const size_t nbytes = row_bytes(B, h->L.ndim);
    double* dst = cube ? h->d_cube : h->d_theta;
    if (!cube) RVLL_TRY(sync_other_lanes(h));                       // other lanes may still be reading the old theta
    // small: stage through pinned memory (a true asynchronous DMA; the caller's buffer is free at once,
    // and every host-buffer call ends in a stream sync before the staging buffer is written again)
    const bool staged = nbytes <= kPinBytes;
    if (staged) {
        HIP_TRY(hipStreamSynchronize(h->compute));
        memcpy(h->pin_in, rows, nbytes);
    }
    HIP_TRY(hipMemcpyAsync(dst, staged ? h->pin_in : rows, nbytes, hipMemcpyHostToDevice, h->compute));
    if (!staged) HIP_TRY(hipStreamSynchronize(h->compute));
    else if (!cube) h->theta_async = true;
    return RVLL_OK;
}

// ---- the device-resident fallback: upload, the resident launches, download ------------------------------------------------------
// what a host-buffer call computes: log-L of theta rows, theta of cube rows, both in one go, or (a one-launch batch whose slim
// prior stage deferred an element) both with the prior kernels that carry the full solvers
enum class Work { kLogLike, kPrior, kPriorLogLike, kPriorThenLogLike };

int resident_host_batch(rvll_handle* h, const double* in, Work work, int64_t B, double* theta_out, double* logL, int32_t* flags)
{
    RVLL_TRY(upload_rows(h, in, B, work != Work::kLogLike));
    if (work == Work::kPrior || work == Work::kPriorThenLogLike) RVLL_TRY(rvll_dev_prior(h, B));
    // measured (profiles/r01_fused_probe.txt): one launch saves ~1 us up to a few thousand points; beyond that
    // the separate prior kernels win by ~5 % because their work spreads over the whole chip instead of
    // running as a short serial prologue of every log-L workgroup
    if (work == Work::kPriorLogLike) RVLL_TRY(rvll_dev_prior_loglike(h, B));
    if (work == Work::kPriorThenLogLike) h->logl_cur = 0;          // (its results live on lane 0, as the one-launch form's do)
    if (work == Work::kLogLike || work == Work::kPriorThenLogLike) RVLL_TRY(rvll_dev_loglike(h, B));
    return rvll_dev_download(h, B, theta_out, logL, flags);
}

// ---- zero-copy through the mapped pinned blocks, and the single upload with pinned-out stores -----------------------------------
// Zero-copy (the scalar / small-batch callback, a vectorized prior callback, a sampler's proposal round): the rows go into the
// mapped input block by memcpy, once lane 0's stream — whose last call may still read the block — has drained; the kernels read
// them over PCIe and store their results into the mapped result block: no copy commands, one launch, one sync.
int zero_copy_batch(rvll_handle* h, const double* in, Work work, int64_t B, double* theta_out, double* logL, int32_t* flags)
{
    const bool fused = work == Work::kPriorLogLike;
    RVLL_TRY(fused ? rvll_dev_reserve(h, B) : use_device(h));
    HIP_TRY(hipStreamSynchronize(h->compute));
    memcpy(h->pin_in, in, row_bytes(B, h->L.ndim));
    if (fused) RVLL_TRY(sync_other_lanes(h));
    const double* rows = static_cast<const double*>(h->pin_in_dev);
    const ResultBlock out = result_block(h->pin_out_dev, B);
    if (work == Work::kPrior) {                     // theta alone: at the start of the result block
        rvll::PriorArgs a{rows, static_cast<double*>(h->pin_out_dev), (long long)B, h->L.ndim, h->d_priors, h->d_heavy, h->n_heavy};
        HIP_TRY(rvll::launch_prior(a, h->compute));
    } else {
        rvll::LoglikeArgs a;
        int cu = 0;
        RVLL_TRY(build_args(h, fused ? h->d_theta : rows, out.logL, out.flags, B, &a, fused ? nullptr : &cu));
        if (fused) make_fused(h, rows, out.theta, &a);
        if (fused) *h->pin_defer = 0;
        HIP_TRY(fused ? rvll::launch_prior_loglike(a, h->compute) : launch_form(a, cu, h->compute));
    }
    HIP_TRY(hipStreamSynchronize(h->compute));
    if (fused && __atomic_load_n(h->pin_defer, __ATOMIC_ACQUIRE) != 0) {
        // an element fell outside the slim stage's tables (rvll_tile.h): the full prior kernels take the batch
        *h->pin_defer = 0;
        return resident_host_batch(h, in, Work::kPriorThenLogLike, B, theta_out, logL, flags);
    }
    if (work == Work::kPrior) memcpy(theta_out, h->pin_out, row_bytes(B, h->L.ndim));
    else pinned_copy_out(h, B, theta_out, logL, flags);
    return RVLL_OK;
}

// one upload, one launch whose results are stores into mapped pinned host memory, one synchronisation
int loglike_pinned_out(rvll_handle* h, const double* theta, int64_t B, double* logL, int32_t* flags)
{
    RVLL_TRY(rvll_dev_reserve(h, B));
    RVLL_TRY(sync_other_lanes(h));
    HIP_TRY(hipStreamSynchronize(h->compute));     // the pinned block may still be read by an earlier call's copy
    Settled guard([&] { (void)hipStreamSynchronize(h->compute); });
    HIP_TRY(hipMemcpyAsync(h->d_theta, theta, row_bytes(B, h->L.ndim), hipMemcpyHostToDevice, h->compute));
    const ResultBlock out = result_block(h->pin_out_dev, B);
    RVLL_TRY(chunk_step(h, false, 0, B, out.logL, out.flags, h->compute));
    HIP_TRY(hipStreamSynchronize(h->compute));
    guard.armed = false;
    h->theta_async = false;
    pinned_copy_out(h, B, nullptr, logL, flags);
    return RVLL_OK;
}

// ---- two-lane overlapped chunks -------------------------------------------------------------------------------------------------
// Large host batch: nsplit chunks alternate between lanes 0 and 1.  A copy from or to pageable memory occupies the calling thread
// while the runtime stages it, so the upload of chunk c + 1 overlaps the kernels of chunk c.  Where the results go:
//   kPinned    stores into the mapped result block: no download commands behind the last kernel, one memcpy on the host
//   kDownload  all chunks write the lane-0 result buffers, which come back with one download
//   kPerChunk  software-pipelined by one chunk: the download of chunk c - 1 is staged while the GPU runs chunk c
enum class SplitOut { kPinned, kDownload, kPerChunk };

int split_host_batch(rvll_handle* h, const double* in, bool in_is_cube, int64_t B, double* theta_out, double* logL, int32_t* flags,
                     int nsplit, SplitOut mode)
{
    RVLL_TRY(rvll_dev_reserve(h, B));
    RVLL_TRY(sync_other_lanes(h));
    HIP_TRY(hipStreamSynchronize(h->compute));
    const long long D = h->L.ndim;
    // an error in the middle leaves copies from / to the caller's arrays in flight on either stream: wait for both first
    Settled guard([&] { (void)hipStreamSynchronize(h->lanes[0]); (void)hipStreamSynchronize(h->lanes[1]); });
    const ResultBlock out = mode == SplitOut::kPinned ? result_block(h->pin_out_dev, B) : ResultBlock{h->d_logL2[0], h->d_flags2[0], h->d_theta};
    double* dev_in = in_is_cube ? h->d_cube : h->d_theta;
    auto fetch = [&](int c) -> int {
        const Rows r = split_chunk(B, nsplit, c);
        const size_t m = (size_t)(r.hi - r.lo);
        hipStream_t st = h->lanes[c & 1];
        if (theta_out) HIP_TRY(hipMemcpyAsync(theta_out + r.lo * D, h->d_theta + r.lo * D, sizeof(double) * m * (size_t)D, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(logL + r.lo, out.logL + r.lo, sizeof(double) * m, hipMemcpyDeviceToHost, st));
        if (flags) HIP_TRY(hipMemcpyAsync(flags + r.lo, out.flags + r.lo, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
        return RVLL_OK;
    };
    for (int c = 0; c < nsplit; ++c) {
        const Rows r = split_chunk(B, nsplit, c);
        hipStream_t st = h->lanes[c & 1];
        HIP_TRY(hipMemcpyAsync(dev_in + r.lo * D, in + r.lo * D, row_bytes(r.hi - r.lo, h->L.ndim), hipMemcpyHostToDevice, st));
        RVLL_TRY(chunk_step(h, in_is_cube, r.lo, r.hi - r.lo, out.logL, out.flags, st));
        if (mode == SplitOut::kPerChunk && c > 0) RVLL_TRY(fetch(c - 1));
    }
    if (mode == SplitOut::kPerChunk) {
        RVLL_TRY(fetch(nsplit - 1));
        HIP_TRY(hipStreamSynchronize(h->lanes[0]));
    }
    HIP_TRY(hipStreamSynchronize(h->lanes[1]));
    h->theta_async = false;
    h->logl_last = 0;
    if (mode == SplitOut::kDownload) RVLL_TRY(rvll_dev_download(h, B, nullptr, logL, flags));
    if (mode == SplitOut::kPinned) {
        HIP_TRY(hipStreamSynchronize(h->lanes[0]));
        pinned_copy_out(h, B, nullptr, logL, flags);
    }
    guard.armed = false;                            // both lanes have been waited for
    return RVLL_OK;
}

// ---- large host batches: a pipeline of chunks, the host's copies on worker threads (round 3) --------------------------
// A 262144-point cube -> theta -> log-L call moves 80 MB between the caller's pageable arrays and the device.  Through copy
// commands on pageable memory that is ONE host thread at ~12 GB/s (the runtime's staging copy on the way up, ours — into a
// freshly mapped result array, page faults included — on the way down): 6.5 ms around 1.2 ms of kernels (the
// "cliff").  Here the batch goes in chunks of 16384 rows through pinned staging blocks: worker threads copy chunk c + 2 in
// and chunk c - 1 out while the DMA engines and the kernels work on chunk c (uploads, kernels and downloads each on a stream of
// their own, chained by events: the link carries both directions at once).

void free_stage_blocks(rvll_handle* h)
{
    for (int s = 0; s < kStageSlots; ++s) {
        if (h->stage_in[s]) (void)hipHostFree(h->stage_in[s]);
        if (h->stage_out[s]) (void)hipHostFree(h->stage_out[s]);
        h->stage_in[s] = h->stage_out[s] = nullptr;
    }
    h->stage_in_bytes = h->stage_out_bytes = 0;
}

// workers, events and staging blocks for chunks of `rows` rows (grown on demand, kept with the handle)
int stream_reserve(rvll_handle* h, long long rows, int copy_threads)
{
    const StageBlock need = stage_block(rows, h->L.ndim);
    if (!h->pool) {
        // (2, 4 and 8 workers measure the same within the run-to-run spread — the GPU side of the pipeline is the longer one)
        const int n = copy_threads ? copy_threads : (int)std::min(4u, std::max(2u, std::thread::hardware_concurrency() / 2));
        try {
            h->pool = new CopyPool(n);
        } catch (const std::exception& e) {             // (no memory, or the system refuses more threads)
            h->pool = nullptr;
            return report_error(RVLL_E_NOMEM, "cannot start %d copy workers: %s", n, e.what());
        }
    }
    for (int s = 0; s < kStageSlots; ++s)
        for (hipEvent_t* e : {&h->stage_ev[s], &h->stage_up[s], &h->stage_done[s]})
            if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    if (!h->stream_up) {
        // The runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4; this handle alone has seven
        // streams), and a copy's completion marker holds up whatever else shares its queue.  When one of the two copy streams
        // lands on the kernels' queue, every chunk's kernels wait for the previous chunk's download: 3.3 against 2.0 ms at
        // 262144 rows — and which stream lands where depends on what the process has done before (inside bench.py streams made
        // here collided and the handle's spare lanes did not; in the standalone probe it was the other way round; stream
        // priorities changed nothing).  The queue count is the caller's choice (include/rvll.h, rvll_runtime_info); results
        // are the same either way.
        HIP_TRY(hipStreamCreateWithFlags(&h->stream_up, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&h->stream_down, hipStreamNonBlocking));
    }
    if (need.in_bytes > h->stage_in_bytes || need.out_bytes > h->stage_out_bytes) {
        free_stage_blocks(h);
        for (int s = 0; s < kStageSlots; ++s) {
            HIP_TRY(hipHostMalloc(&h->stage_in[s], need.in_bytes, hipHostMallocDefault));
            HIP_TRY(hipHostMalloc(&h->stage_out[s], need.out_bytes, hipHostMallocDefault));
        }
        h->stage_in_bytes = need.in_bytes;
        h->stage_out_bytes = need.out_bytes;
    }
    return RVLL_OK;
}

// RVLL_STREAM_TIMING: the microseconds the calling thread spent up to each of its waits, summed per kind of wait
struct Laps {
    bool on;
    double start = 0., t0 = 0., waited[4] = {0., 0., 0., 0.};
    static double now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    explicit Laps(bool on_) : on(on_) { if (on) start = now(); }
    void begin() { if (on) t0 = now(); }
    void lap(int kind) { if (on) { const double t1 = now(); waited[kind] += t1 - t0; t0 = t1; } }
};

// rows of `in` (unit-cube rows if in_is_cube, else theta rows) -> [theta_out], logL, [flags], all host arrays of B rows
int stream_host_batch(rvll_handle* h, const double* in, bool in_is_cube, int64_t B, double* theta_out, double* logL, int32_t* flags,
                      const BatchRoute& route, const BatchSwitches& sw)
{
    // the calling thread runs `lag` chunks ahead of the results it waits for (1: the next chunk's commands were issued only when
    // the last-but-one's results had landed, and the kernels waited for that: 2.3 -> 1.8 ms at 262144 rows)
    const long long rows = route.chunk_rows, lag = route.lag;
    RVLL_TRY(rvll_dev_reserve(h, B));
    RVLL_TRY(sync_other_lanes(h));
    HIP_TRY(hipStreamSynchronize(h->compute));
    RVLL_TRY(stream_reserve(h, rows, sw.copy_threads));
    const long long D = h->L.ndim;
    const int n = stream_chunks(B, rows);
    const StageBlock blk = stage_block(rows, h->L.ndim);
    CopyPool& pool = *h->pool;
    CopyPool::Ticket tin[kStageSlots], tout[kStageSlots];
    auto copy_in = [&](int c) {
        const Rows r = stream_chunk(B, rows, c);
        if (c < n) pool.copy(h->stage_in[c % kStageSlots], in + r.lo * D, row_bytes(r.hi - r.lo, h->L.ndim), &tin[c % kStageSlots]);
    };
    auto copy_out = [&](int c) {
        const Rows r = stream_chunk(B, rows, c);
        const size_t m = (size_t)(r.hi - r.lo);
        const char* so = static_cast<const char*>(h->stage_out[c % kStageSlots]);
        CopyPool::Ticket* t = &tout[c % kStageSlots];
        if (theta_out) pool.copy(theta_out + r.lo * D, so + blk.theta, sizeof(double) * m * (size_t)D, t);
        pool.copy(logL + r.lo, so + blk.logL, sizeof(double) * m, t);
        if (flags) pool.copy(flags + r.lo, so + blk.flags, sizeof(int32_t) * m, t);
    };
    // whatever happens, leave with no copy in flight into or out of the caller's arrays and the workers asleep
    Settled guard([&] {
        for (int s = 0; s < kStageSlots; ++s) { CopyPool::wait(&tin[s]); CopyPool::wait(&tout[s]); }
        (void)hipStreamSynchronize(h->stream_up);
        (void)hipStreamSynchronize(h->compute);
        (void)hipStreamSynchronize(h->stream_down);
        pool.busy(false);
    });
    Laps laps(sw.stream_timing);
    pool.busy(true);
    copy_in(0);
    copy_in(1);
    double* dev_in = in_is_cube ? h->d_cube : h->d_theta;
    for (int c = 0; c < n; ++c) {
        const int s = c % kStageSlots;
        const Rows r = stream_chunk(B, rows, c);
        const size_t m = (size_t)(r.hi - r.lo);
        laps.begin();
        CopyPool::wait(&tin[s]);                            // the chunk's rows are in their pinned block ...
        laps.lap(0);
        CopyPool::wait(&tout[s]);                           // ... and the results of the chunk that used the block before are out of theirs
        laps.lap(1);
        // up | kernels | down on three streams, so that chunk c + 1 comes up and chunk c - 1 goes down (the link is full duplex)
        // under the kernels of chunk c
        HIP_TRY(hipMemcpyAsync(dev_in + r.lo * D, h->stage_in[s], sizeof(double) * m * (size_t)D, hipMemcpyHostToDevice, h->stream_up));
        HIP_TRY(hipEventRecord(h->stage_up[s], h->stream_up));
        HIP_TRY(hipStreamWaitEvent(h->compute, h->stage_up[s], 0));
        RVLL_TRY(chunk_step(h, in_is_cube, r.lo, r.hi - r.lo, h->d_logL2[0], h->d_flags2[0], h->compute));
        HIP_TRY(hipEventRecord(h->stage_done[s], h->compute));
        HIP_TRY(hipStreamWaitEvent(h->stream_down, h->stage_done[s], 0));
        char* so = static_cast<char*>(h->stage_out[s]);
        if (theta_out) HIP_TRY(hipMemcpyAsync(so + blk.theta, h->d_theta + r.lo * D, sizeof(double) * m * (size_t)D, hipMemcpyDeviceToHost, h->stream_down));
        HIP_TRY(hipMemcpyAsync(so + blk.logL, h->d_logL2[0] + r.lo, sizeof(double) * m, hipMemcpyDeviceToHost, h->stream_down));
        if (flags) HIP_TRY(hipMemcpyAsync(so + blk.flags, h->d_flags2[0] + r.lo, sizeof(int32_t) * m, hipMemcpyDeviceToHost, h->stream_down));
        HIP_TRY(hipEventRecord(h->stage_ev[s], h->stream_down));
        laps.lap(2);
        if (c >= lag) {
            HIP_TRY(hipEventSynchronize(h->stage_ev[(c - lag) % kStageSlots]));
            laps.lap(3);
            copy_out(c - lag);
        }
        copy_in(c + 2);     // (its block was last read by the upload of chunk c - 2, whose event has been waited for)
    }
    for (int c = (int)std::max(0ll, n - lag); c < n; ++c) {
        HIP_TRY(hipEventSynchronize(h->stage_ev[c % kStageSlots]));
        copy_out(c);
    }
    h->theta_async = false;
    h->logl_last = 0;
    if (laps.on) {
        const double t1 = Laps::now();
        guard.run();
        fprintf(stderr, "stream %lld rows, %d chunks, %d workers: %.0f us to the last event, %.0f us in all; waited for rows in %.0f, results out %.0f, "
                "issue %.0f, events %.0f us\n", (long long)B, n, pool.size(), t1 - laps.start, Laps::now() - laps.start, laps.waited[0],
                laps.waited[1], laps.waited[2], laps.waited[3]);
    }
    return RVLL_OK;
}

// ---- a host-buffer call: the argument checks, the route, the transport ----------------------------------------------------------
// One order of checks gives each of the three calls the code it has always given.  A single point goes to the scalar-call server
// when it is on (the pair prior(cube) + loglike(theta) as ONE request) — decided before any measurement switch is read.
int host_batch(rvll_handle* h, Work work, const double* in, int64_t B, double* theta_out, double* logL, int32_t* flags)
{
    static const char* const kArrays[] = {"theta/logL", "cube/theta", "cube/logL"};
    static const unsigned kServerOp[] = {rvll::kServerLogLike, rvll::kServerPrior, rvll::kServerPriorLogLike};
    const bool cube = work != Work::kLogLike;
    if (!h) return report_error(RVLL_E_INVALID, "null handle");
    if (B < 0) return report_error(RVLL_E_INVALID, "B < 0");
    if (cube && !h->have_priors) return report_error(RVLL_E_NOPRIORS, "rvll_set_priors has not been called");
    if (B == 0) return use_device(h);
    if (!in || !(work == Work::kPrior ? theta_out : logL)) return report_error(RVLL_E_INVALID, "%s is null", kArrays[(int)work]);
    if (B == 1 && h->srv_enabled) {
        const bool noop = work == Work::kLogLike && getenv("RVLL_SERVER_NOOP");
        return scalar_call(h, noop ? rvll::kServerNoop : kServerOp[(int)work], in, logL, flags, theta_out);
    }
    const BatchSwitches sw = read_batch_switches();
    const BatchRoute route = work == Work::kLogLike ? loglike_route(B, h->L.ndim, sw) : work == Work::kPrior ? prior_route(B, h->L.ndim, sw)
                                                    : prior_loglike_route(B, h->L.ndim, h->all_direct, sw);
    switch (route.transport) {
    case Transport::kZeroCopy: return zero_copy_batch(h, in, work, B, theta_out, logL, flags);
    case Transport::kPinnedOut: return loglike_pinned_out(h, in, B, logL, flags);
    case Transport::kSplit:
        return split_host_batch(h, in, cube, B, theta_out, logL, flags, route.nsplit,
                                cube ? SplitOut::kPerChunk : route.out_pinned ? SplitOut::kPinned : SplitOut::kDownload);
    case Transport::kStreamed: return stream_host_batch(h, in, cube, B, theta_out, logL, flags, route, sw);
    case Transport::kResident: break;
    }
    return resident_host_batch(h, in, work, B, theta_out, logL, flags);
}

}  // namespace

namespace rvll {
namespace host {

void stream_free(rvll_handle* h)
{
    delete h->pool;
    h->pool = nullptr;
    free_stage_blocks(h);
    for (int s = 0; s < kStageSlots; ++s)
        for (hipEvent_t* e : {&h->stage_ev[s], &h->stage_up[s], &h->stage_done[s]}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    if (h->stream_up) (void)hipStreamDestroy(h->stream_up);
    if (h->stream_down) (void)hipStreamDestroy(h->stream_down);
    h->stream_up = h->stream_down = nullptr;
}

// A large device array into the caller's pageable memory: chunks through the pinned staging blocks on the download stream, up to
// three in flight, each copied on to its place by the workers as it lands (a copy command straight into pageable memory runs
// at 50 GB/s into a range the runtime has pinned and cached, at 1.5 - 7 GB/s into one it has never seen — and a result array
// usually is one; round 2 staged through two 1 MiB blocks on the calling thread: 6 ms for 38 MB).  Work queued on lane 0's
// stream before the call is waited for first.  From here on every device -> pageable host copy of size goes this way: arrays the
// caller makes per call (above glibc's mmap threshold every array is a fresh mapping), and the dead points' one download per run.
int download_rows(rvll_handle* h, void* dst, const void* src_dev, size_t bytes)
{
    if (!bytes) return RVLL_OK;
    RVLL_TRY(stream_reserve(h, kStreamChunkRows, h->pool ? 0 : read_batch_switches().copy_threads));
    HIP_TRY(hipStreamSynchronize(h->compute));
    const size_t chunk = h->stage_out_bytes & ~(size_t)4095;
    const int n = (int)((bytes + chunk - 1) / chunk);
    CopyPool& pool = *h->pool;
    CopyPool::Ticket tout[kStageSlots];
    char* to = static_cast<char*>(dst);
    const char* from = static_cast<const char*>(src_dev);
    Settled guard([&] {
        for (int s = 0; s < kStageSlots; ++s) CopyPool::wait(&tout[s]);
        (void)hipStreamSynchronize(h->stream_down);
        pool.busy(false);
    });
    auto fetch = [&](int c) -> hipError_t {
        const int s = c % kStageSlots;
        const size_t off = (size_t)c * chunk;
        hipError_t e = hipMemcpyAsync(h->stage_out[s], from + off, std::min(chunk, bytes - off), hipMemcpyDeviceToHost, h->stream_down);
        return e != hipSuccess ? e : hipEventRecord(h->stage_ev[s], h->stream_down);
    };
    pool.busy(true);
    for (int c = 0; c < std::min(n, kStageSlots - 1); ++c) HIP_TRY(fetch(c));
    for (int c = 0; c < n; ++c) {
        const int s = c % kStageSlots;
        const size_t off = (size_t)c * chunk;
        HIP_TRY(hipEventSynchronize(h->stage_ev[s]));
        pool.copy(to + off, h->stage_out[s], std::min(chunk, bytes - off), &tout[s]);
        const int next = c + kStageSlots - 1;               // its block held chunk c - 1: wait until the workers have emptied it
        if (next < n) {
            CopyPool::wait(&tout[next % kStageSlots]);
            HIP_TRY(fetch(next));
        }
    }
    return RVLL_OK;
}

}  // namespace host
}  // namespace rvll

extern "C" {

int rvll_dev_upload_theta(rvll_handle* h, const double* theta, int64_t B) { return upload_rows(h, theta, B, false); }

int rvll_dev_upload_cube(rvll_handle* h, const double* cube, int64_t B) { return upload_rows(h, cube, B, true); }

int rvll_dev_download(rvll_handle* h, int64_t B, double* theta, double* logL, int32_t* flags)
{
    RVLL_TRY(use_device(h));
    RVLL_TRY(check_capacity(h, B));
    if (h->logl_last != 0) HIP_TRY(hipStreamSynchronize(h->lanes[h->logl_last]));   // read through lane 0's stream
    const size_t nt = theta ? row_bytes(B, h->L.ndim) : 0;                          // (B == 0: nothing to copy)
    const size_t nl = logL ? sizeof(double) * (size_t)B : 0, nf = flags ? sizeof(int32_t) * (size_t)B : 0;
    const Download how = download_route(B, h->L.ndim, theta != nullptr, logL != nullptr, flags != nullptr);
    // small: one pinned landing zone (theta, log-L, flags back to back), one sync; else straight into the caller's arrays
    char* const zone = how == Download::kPinned ? static_cast<char*>(h->pin_out) : nullptr;
    // A device-to-host copy into pageable memory runs at 50 GB/s once the runtime has pinned the destination
    // range and cached that — which it cannot for a range it has never seen: 38 MB of theta into a fresh numpy
    // array take 20-28 ms (1.5 GB/s), and numpy arrays above 32 MB are fresh mappings every time (glibc's mmap
    // threshold stops growing there; below it the heap hands the same block out again and the copy is fast:
    // profiles/r02_d2h_probe.txt).  Large downloads therefore go through pinned staging blocks, the workers
    // copying chunk c to its place while chunks c + 1 .. c + 3 land (download_rows; round 2: two 1 MiB blocks on
    // the calling thread, 6 ms for those 38 MB).
    if (how == Download::kStagedTheta) RVLL_TRY(download_rows(h, theta, h->d_theta, nt));
    else if (nt) HIP_TRY(hipMemcpyAsync(zone ? (void*)zone : theta, h->d_theta, nt, hipMemcpyDeviceToHost, h->compute));
    if (nl) HIP_TRY(hipMemcpyAsync(zone ? (void*)(zone + nt) : logL, h->d_logL2[h->logl_last], nl, hipMemcpyDeviceToHost, h->compute));
    if (nf) HIP_TRY(hipMemcpyAsync(zone ? (void*)(zone + nt + nl) : flags, h->d_flags2[h->logl_last], nf, hipMemcpyDeviceToHost, h->compute));
    HIP_TRY(hipStreamSynchronize(h->compute));
    if (zone && nt) memcpy(theta, zone, nt);
    if (zone && nl) memcpy(logL, zone + nt, nl);
    if (zone && nf) memcpy(flags, zone + nt + nl, nf);
    return RVLL_OK;
}

// ---- host-buffer hot calls -------------------------------------------------------
int rvll_loglike_batch(rvll_handle* h, const double* theta, int64_t B, double* logL, int32_t* flags) { return host_batch(h, Work::kLogLike, theta, B, nullptr, logL, flags); }

int rvll_prior_batch(rvll_handle* h, const double* cube, int64_t B, double* theta) { return host_batch(h, Work::kPrior, cube, B, theta, nullptr, nullptr); }

int rvll_prior_loglike_batch(rvll_handle* h, const double* cube, int64_t B, double* theta_out, double* logL, int32_t* flags)
{
    return host_batch(h, Work::kPriorLogLike, cube, B, theta_out, logL, flags);
}

}  // extern "C"
