// The route choice and the layouts of the host-buffer batch calls (evidence_amd/csrc/rvll_batch_route.h) behind C functions, for
// tests/test_batch_route_host.py: host code only, the header alone.  The measurement switches are read from the environment, as
// the library reads them.
#include "rvll_batch_route.h"

using namespace rvll::host;

extern "C" {

// entry 0: rvll_loglike_batch, 1: rvll_prior_batch, 2: rvll_prior_loglike_batch.  out = {transport, nsplit, out_pinned, chunk rows, lag}
void br_route(int entry, int64_t B, int ndim, int all_direct, int64_t* out)
{
    const BatchSwitches sw = read_batch_switches();
    const BatchRoute r = entry == 0 ? loglike_route(B, ndim, sw) : entry == 1 ? prior_route(B, ndim, sw)
                                                                              : prior_loglike_route(B, ndim, all_direct != 0, sw);
    out[0] = (int64_t)r.transport; out[1] = r.nsplit; out[2] = r.out_pinned; out[3] = r.chunk_rows; out[4] = r.lag;
}

// out = the nine switches in the order of the struct
void br_switches(int64_t* out)
{
    const BatchSwitches s = read_batch_switches();
    const int64_t v[9] = {(int64_t)s.zero_copy_in, s.stream_loglike, s.stream_min, s.split, s.no_pinned_out, s.stream_chunk, s.stream_lag,
                          s.stream_timing, s.copy_threads};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
}

int br_download(int64_t B, int ndim, int theta, int logL, int flags) { return (int)download_route(B, ndim, theta != 0, logL != 0, flags != 0); }

// out [Bmax, 3]: where log-L, flags and theta begin in the pinned result block of B = 1 .. Bmax rows
void br_pinned_results(int64_t Bmax, int64_t* out)
{
    for (int64_t B = 1; B <= Bmax; ++B) {
        const PinnedResult p = pinned_result(B);
        int64_t* o = out + 3 * (B - 1);
        o[0] = (int64_t)p.logL; o[1] = (int64_t)p.flags; o[2] = (int64_t)p.theta;
    }
}

// out = {in_bytes, theta, logL, flags, out_bytes}
void br_stage_block(int64_t rows, int ndim, int64_t* out)
{
    const StageBlock b = stage_block(rows, ndim);
    out[0] = (int64_t)b.in_bytes; out[1] = (int64_t)b.theta; out[2] = (int64_t)b.logL; out[3] = (int64_t)b.flags; out[4] = (int64_t)b.out_bytes;
}

// out [nsplit, 2]: the chunks of the two-lane route
void br_split_chunks(int64_t B, int nsplit, int64_t* out)
{
    for (int c = 0; c < nsplit; ++c) { const Rows r = split_chunk(B, nsplit, c); out[2 * c] = r.lo; out[2 * c + 1] = r.hi; }
}

// the chunks of the streamed route: returns their number n, out [n, 2] (up to `room` chunks are written)
int br_stream_chunks(int64_t B, int64_t rows, int room, int64_t* out)
{
    const int n = stream_chunks(B, rows);
    for (int c = 0; c < n && c < room; ++c) { const Rows r = stream_chunk(B, rows, c); out[2 * c] = r.lo; out[2 * c + 1] = r.hi; }
    return n;
}

}  // extern "C"
