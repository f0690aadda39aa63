// GP prediction under correlated noise on gfx950 (rvll_celerite_predict_batch): alpha = Sigma^-1 r, the mean and
// variance of the latent GP at the data epochs and at query times.  evidence_amd/correlated.py holds the numpy definitions;
// rvll_celerite_predict.h the sweeps these kernels run.
//
//   residuals   launch_residuals (rvll_gls.hip) with every planet subtracted, as in the log-L call
//   factor      celerite_kernel<J, double*, long long> (rvll_celerite.hip): the log-L sweep, which also leaves W, D, z, r and var of every epoch in
//               the workspace ws [epoch in time order][J + kCelWsExtra fields][rp rows], rp the chunk's rows rounded up to a wave:
//               the 64 lanes of a wave read and write 512 consecutive bytes a field in every sweep
//   backward    cel_backward_kernel<J>: g and the upper triangle of M from the last epoch to the first; alpha goes where z was,
//               the variance and the mean at the epoch where var was and into a field of their own; every query in
//               [t_(n-1), t_n) takes the later epochs' share of its mean from G_n.  U and P are recomputed from the columns (one
//               exponential a distinct c, one sincos a complex term, as in the factor): storing them would add 2 J fields to J + 5
//   forward     cel_forward_kernel<J>, only with queries: F, and the earlier epochs' share of every query in [t_n, t_(n+1))
//   variance    cel_gridvar_kernel<J>, only on request: one forward substitution per (row, query).  The lanes are rows, a
//               workgroup takes kCelVarQueries queries: W and D are read coalesced, once for those queries, and the queries'
//               times at wave-uniform addresses
//   transpose   cel_transpose_kernel: [epoch or query][row] to the caller's [row][epoch in table order] or [row][query as
//               given] through a 64 x 65 LDS tile, both sides coalesced (the scatter through `order` wherever it runs in
//               table order), NaN into every row with a flag.  A kernel of its own, not a tile inside the sweeps: those keep
//               their registers for the state, and the epoch outputs exist only after the last step of the backward sweep
// All sweeps: one row a lane, a workgroup of one wave, the state in registers.  The queries arrive sorted with the host's table of
// their times from the first epoch, the time since the epoch before and until the epoch after, and per epoch n the range
// qstart[n] .. qstart[n + 1] of the queries in [t_(n-1), t_n); every lane reads them at the same address.
// A row's outputs read nothing of other rows: their bits depend on the row, the epoch table and the query times alone.  No
// atomics, no inline assembly.
#include <cmath>
#include <numeric>
#include "rvll_host.h"
#include "rvll_celerite_predict.h"

namespace rvll {

namespace {

constexpr int kCelVarQueries = 4;                         // queries a workgroup of the variance kernel carries
constexpr int kCelTile = 64;                              // the transpose's tile

template <int J>
__global__ __launch_bounds__(kCelRows)
void cel_backward_kernel(const double* __restrict__ theta, int D, long long R, int Ne, const double* __restrict__ ts,
                         const double* __restrict__ dts, const CelPlan plan, double* __restrict__ ws, long long rp,
                         const int32_t* __restrict__ qstart, const double* __restrict__ qx, const double* __restrict__ qdtb,
                         double* __restrict__ wq)
{
    const long long row = (long long)blockIdx.x * kCelRows + threadIdx.x;
    const bool live = row < R;
    const long long rc = live ? row : R - 1;                          // a lane past the end works on the last row and stores nothing
    CelColumn col[J];
    double suma;
    bool pair;
    cel_plan_columns<J>(plan, theta + rc * D, col, suma, pair);
    CelBack<J> bk;
    cel_back_init(bk);
    for (int q = qstart[Ne]; q < qstart[Ne + 1]; ++q)                 // at or after the last epoch: no later epochs
        if (live) wq[(long long)q * rp + row] = 0.0;
    for (int n = Ne - 1; n >= 0; --n) {
        double* w = ws + (long long)n * (J + kCelWsExtra) * rp + rc;
        double W[J], U[J], V[J], G[J], alpha, znn;
#pragma unroll
        for (int j = 0; j < J; ++j) W[j] = w[j * rp];
        const double Dn = w[(J + kCelWsD) * rp], z = w[(J + kCelWsZ) * rp], r = w[(J + kCelWsR) * rp], v = w[(J + kCelWsVar) * rp];
        CelGap<J> P;
        cel_gap<J>(col, ts[n], dts[n], P, U, V);
        cel_back_step<J>(bk, P, U, W, Dn, z, alpha, znn, G);
        if (live) {
            w[(J + kCelWsZ) * rp] = alpha;
            w[(J + kCelWsVar) * rp] = v - v * v * znn;
            w[(J + kCelWsMean) * rp] = r - v * alpha;
        }
        for (int q = qstart[n]; q < qstart[n + 1]; ++q) {
            const double m = cel_query_back<J>(col, qx[q], qdtb[q], G);
            if (live) wq[(long long)q * rp + row] = m;
        }
    }
}

template <int J>
__global__ __launch_bounds__(kCelRows)
void cel_forward_kernel(const double* __restrict__ theta, int D, long long R, int Ne, const double* __restrict__ ts,
                        const double* __restrict__ dts, const CelPlan plan, const double* __restrict__ ws, long long rp,
                        const int32_t* __restrict__ qstart, const double* __restrict__ qx, const double* __restrict__ qdtf,
                        double* __restrict__ wq)
{
    const long long row = (long long)blockIdx.x * kCelRows + threadIdx.x;
    const bool live = row < R;
    const long long rc = live ? row : R - 1;
    CelColumn col[J];
    double suma;
    bool pair;
    cel_plan_columns<J>(plan, theta + rc * D, col, suma, pair);
    double F[J];
#pragma unroll
    for (int j = 0; j < J; ++j) F[j] = 0.0;
    for (int n = 0; n < Ne; ++n) {
        const double alpha = ws[((long long)n * (J + kCelWsExtra) + J + kCelWsZ) * rp + rc];
        CelGap<J> P;
        double U[J], V[J];
        cel_gap<J>(col, ts[n], dts[n], P, U, V);
        cel_fwd_step<J>(F, P, V, alpha);
        for (int q = qstart[n + 1]; q < qstart[n + 2]; ++q) {
            const double m = cel_query_fwd<J>(col, qx[q], qdtf[q], F);
            if (live) wq[(long long)q * rp + row] += m;
        }
    }
}

template <int J>
__global__ __launch_bounds__(kCelRows)
void cel_gridvar_kernel(const double* __restrict__ theta, int D, long long R, int Ne, const double* __restrict__ ts,
                        const double* __restrict__ dts, const CelPlan plan, const double* __restrict__ ws, long long rp,
                        const double* __restrict__ qx, int M, double* __restrict__ wv)
{
    const long long row = (long long)blockIdx.x * kCelRows + threadIdx.x;
    const bool live = row < R;
    const long long rc = live ? row : R - 1;
    const int q0 = blockIdx.y * kCelVarQueries;
    CelColumn col[J];
    double suma;
    bool pair;
    cel_plan_columns<J>(plan, theta + rc * D, col, suma, pair);
    CelVar<J> st[kCelVarQueries];
    double x[kCelVarQueries], Wp[J];
#pragma unroll
    for (int i = 0; i < kCelVarQueries; ++i) {
        cel_var_init(st[i]);
        x[i] = qx[q0 + i < M ? q0 + i : M - 1];                       // a slot past the end works on the last query and stores nothing
    }
#pragma unroll
    for (int j = 0; j < J; ++j) Wp[j] = 0.0;
    for (int n = 0; n < Ne; ++n) {
        const double* w = ws + (long long)n * (J + kCelWsExtra) * rp + rc;
        const double Dn = w[(J + kCelWsD) * rp], tn = ts[n];
        CelGap<J> P;
        double U[J], V[J];
        cel_gap<J>(col, tn, dts[n], P, U, V);
#pragma unroll
        for (int i = 0; i < kCelVarQueries; ++i) cel_var_step<J>(st[i], P, U, Wp, Dn, cel_kernel_value<J>(col, fabs(x[i] - tn)));
#pragma unroll
        for (int j = 0; j < J; ++j) Wp[j] = w[j * rp];
    }
#pragma unroll
    for (int i = 0; i < kCelVarQueries; ++i)
        if (live && q0 + i < M) wv[(long long)(q0 + i) * rp + row] = suma - st[i].acc;
}

// dst[row][col_of[n]] = src[n * nstride + row] for n < N and row < R (col_of NULL: n), NaN where flags[row] is set
__global__ __launch_bounds__(kCelTile * 4)
void cel_transpose_kernel(const double* __restrict__ src, long long nstride, int N, long long R, const int32_t* __restrict__ col_of,
                          const int32_t* __restrict__ flags, double* __restrict__ dst, int ncols)
{
    __shared__ double tile[kCelTile][kCelTile + 1];
    const int x = threadIdx.x, y = threadIdx.y;
    const long long row0 = (long long)blockIdx.x * kCelTile;
    const int n0 = blockIdx.y * kCelTile;
    for (int nn = y; nn < kCelTile; nn += 4)
        if (n0 + nn < N && row0 + x < R) tile[nn][x] = src[(long long)(n0 + nn) * nstride + row0 + x];
    __syncthreads();
    if (n0 + x < N) {
        const int c = col_of ? col_of[n0 + x] : n0 + x;
        for (int rr = y; rr < kCelTile; rr += 4)
            if (row0 + rr < R) dst[(row0 + rr) * ncols + c] = flags[row0 + rr] ? (double)NAN : tile[x][rr];
    }
}

template <int J>
hipError_t launch_sweeps(const double* theta, int D, long long R, int Ne, const double* ts, const double* dts, const CelPlan& plan,
                         double* ws, long long rp, const int32_t* qstart, const double* qtab, int M, double* wq, double* wv,
                         hipStream_t stream, hipEvent_t after_mean)
{
    const dim3 blocks((unsigned)((R + kCelRows - 1) / kCelRows)), wave(kCelRows);
    hipLaunchKernelGGL(cel_backward_kernel<J>, blocks, wave, 0, stream, theta, D, R, Ne, ts, dts, plan, ws, rp, qstart, qtab,
                       qtab + 2 * (long long)M, wq);
    if (M > 0)
        hipLaunchKernelGGL(cel_forward_kernel<J>, blocks, wave, 0, stream, theta, D, R, Ne, ts, dts, plan, ws, rp, qstart, qtab,
                           qtab + M, wq);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && after_mean) e = hipEventRecord(after_mean, stream);
    if (e == hipSuccess && wv && M > 0) {
        const dim3 grid(blocks.x, (unsigned)((M + kCelVarQueries - 1) / kCelVarQueries));
        hipLaunchKernelGGL(cel_gridvar_kernel<J>, grid, wave, 0, stream, theta, D, R, Ne, ts, dts, plan, ws, rp, qtab, M, wv);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_transpose(const double* src, long long nstride, int N, long long R, const int32_t* col_of, const int32_t* flags,
                            double* dst, int ncols, hipStream_t stream)
{
    if (N < 1 || R < 1) return hipSuccess;
    const dim3 grid((unsigned)((R + kCelTile - 1) / kCelTile), (unsigned)((N + kCelTile - 1) / kCelTile));
    hipLaunchKernelGGL(cel_transpose_kernel, grid, dim3(kCelTile, 4), 0, stream, src, nstride, N, R, col_of, flags, dst, ncols);
    return hipGetLastError();
}

}  // namespace

}  // namespace rvll

extern "C" {

int rvll_celerite_predict_batch(rvll_handle* h, const double* theta, int64_t B, const rvll_noise_term* terms, int32_t n_terms,
                                const int32_t* order, const double* times, int64_t M, int32_t want_var, double* residual,
                                double* mean_data, double* var_data, double* mean, double* var, double* logl, int32_t* flags,
                                double* phase_ms)
{
    using rvll::report_error;
    int rc = rvll::host::use_device(h);
    if (rc) return rc;
    if (B < 0 || M < 0) return report_error(RVLL_E_INVALID, "negative size");
    if (M > INT32_MAX / 4) return report_error(RVLL_E_INVALID, "more than %d query times", INT32_MAX / 4);
    rvll::CelPlan plan;
    int J = 0;
    rc = rvll::cel_make_plan(h, terms, n_terms, plan, J);
    if (rc) return rc;
    if (var && !want_var) return report_error(RVLL_E_INVALID, "var is given without want_var");
    if (M > 0 && (!times || !mean || (want_var && !var))) return report_error(RVLL_E_INVALID, "null buffer");
    for (int64_t i = 0; i < M; ++i)
        if (!std::isfinite(times[i])) return report_error(RVLL_E_INVALID, "times[%lld] is not finite", (long long)i);
    const int Ne = h->Ne, m = (int)M;
    const bool with_var = want_var && m > 0;
    if (phase_ms) phase_ms[0] = phase_ms[1] = phase_ms[2] = phase_ms[3] = 0.0;
    std::vector<int32_t> ord;
    std::vector<double> tab;                                          // times, then gaps
    rc = rvll::cel_time_tables(h, order, ord, tab);
    if (rc) return rc;
    if (B == 0) return RVLL_OK;
    if (!theta || !mean_data || !logl || !flags) return report_error(RVLL_E_INVALID, "null buffer");

    // the queries in time order (stable): their times from the first epoch, since the epoch before and until the epoch after;
    // where each goes in the caller's order; per epoch n the first query at or after t_(n-1) and before t_n
    std::vector<int32_t> qperm((size_t)m), qstart((size_t)Ne + 2);
    std::vector<double> qtab(3 * (size_t)m);
    {
        const double t0 = h->cel_times[(size_t)ord[0]];
        std::vector<double> xs((size_t)m);
        for (int i = 0; i < m; ++i) xs[(size_t)i] = times[i] - t0;
        std::iota(qperm.begin(), qperm.end(), 0);
        std::stable_sort(qperm.begin(), qperm.end(), [&](int32_t a, int32_t b) { return xs[(size_t)a] < xs[(size_t)b]; });
        int q = 0;
        for (int k = 0; k <= Ne; ++k) {                               // bucket k: the queries with exactly k epochs at or before them
            qstart[(size_t)k] = q;
            while (q < m && (k == Ne || xs[(size_t)qperm[(size_t)q]] < tab[(size_t)k])) {
                const double x = xs[(size_t)qperm[(size_t)q]];
                qtab[(size_t)q] = x;
                qtab[(size_t)m + (size_t)q] = k > 0 ? x - tab[(size_t)k - 1] : 0.0;
                qtab[2 * (size_t)m + (size_t)q] = k < Ne ? tab[(size_t)k] - x : 0.0;
                ++q;
            }
        }
        qstart[(size_t)Ne + 1] = m;
    }

    // rows a chunk: res, var, the workspace, the queries' sums and the transposed outputs of them take at most kCelChunkBytes,
    // in whole waves (RVLL_CELERITE_CHUNK_ROWS: a row count for tests of the chunk boundary)
    const int F = J + rvll::kCelWsExtra, nq = with_var ? 2 : 1;
    const long long row_bytes = (long long)sizeof(double) * ((long long)Ne * (2 + F + 3) + (long long)m * 2 * nq);
    long long rows = std::max<long long>(rvll::kCelRows, rvll::kCelChunkBytes / row_bytes / rvll::kCelRows * rvll::kCelRows);
    if (const char* env = getenv("RVLL_CELERITE_CHUNK_ROWS")) {
        const long long v = atoll(env);
        if (v >= 1) rows = std::min(rows, v);
    }
    rows = std::min<long long>(rows, B);
    const long long rp = (rows + rvll::kCelRows - 1) / rvll::kCelRows * rvll::kCelRows;
    const size_t d8 = sizeof(double), rne = (size_t)rows * (size_t)Ne, rm = (size_t)rows * (size_t)m;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off += rvll::cel_up8(bytes); return o; };
    const size_t o_ord = take(sizeof(int32_t) * (size_t)Ne), o_tab = take(d8 * 2 * (size_t)Ne), o_qstart = take(sizeof(int32_t) * ((size_t)Ne + 2)),
                 o_qperm = take(sizeof(int32_t) * (size_t)m), o_qtab = take(d8 * 3 * (size_t)m), o_res = take(d8 * rne), o_var = take(d8 * rne),
                 o_logl = take(d8 * (size_t)rows), o_flag = take(sizeof(int32_t) * (size_t)rows),
                 o_ws = take(d8 * (size_t)Ne * (size_t)F * (size_t)rp), o_wq = take(d8 * (size_t)nq * (size_t)m * (size_t)rp),
                 o_oute = take(d8 * 3 * rne), o_outq = take(d8 * (size_t)nq * rm);
    rc = rvll::cel_reserve(h, off);
    if (rc) return rc;
    char* base = static_cast<char*>(h->d_cel);
    int32_t* d_ord = reinterpret_cast<int32_t*>(base + o_ord);
    double* d_tab = reinterpret_cast<double*>(base + o_tab);
    int32_t *d_qstart = reinterpret_cast<int32_t*>(base + o_qstart), *d_qperm = reinterpret_cast<int32_t*>(base + o_qperm);
    double* d_qtab = reinterpret_cast<double*>(base + o_qtab);
    double *d_res = reinterpret_cast<double*>(base + o_res), *d_var = reinterpret_cast<double*>(base + o_var);
    double* d_logl = reinterpret_cast<double*>(base + o_logl);
    int32_t* d_flag = reinterpret_cast<int32_t*>(base + o_flag);
    double *d_ws = reinterpret_cast<double*>(base + o_ws), *d_wq = reinterpret_cast<double*>(base + o_wq);
    double* d_wv = with_var ? d_wq + (size_t)m * (size_t)rp : nullptr;
    double *d_oute = reinterpret_cast<double*>(base + o_oute), *d_outq = reinterpret_cast<double*>(base + o_outq);
    HIP_TRY(hipMemcpyAsync(d_ord, ord.data(), sizeof(int32_t) * (size_t)Ne, hipMemcpyHostToDevice, h->compute));
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), d8 * 2 * (size_t)Ne, hipMemcpyHostToDevice, h->compute));
    HIP_TRY(hipMemcpyAsync(d_qstart, qstart.data(), sizeof(int32_t) * ((size_t)Ne + 2), hipMemcpyHostToDevice, h->compute));
    if (m > 0) {
        HIP_TRY(hipMemcpyAsync(d_qperm, qperm.data(), sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, h->compute));
        HIP_TRY(hipMemcpyAsync(d_qtab, qtab.data(), d8 * 3 * (size_t)m, hipMemcpyHostToDevice, h->compute));
    }

    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    if (phase_ms)
        for (auto& k : ev)
            if (e == hipSuccess) e = hipEventCreate(&k);
    const rvll::DriftSlots ds = rvll::drift_slots(h);
    const long long fstride = rp, estride = (long long)F * rp;        // between the fields of an epoch, between the epochs
    int status = RVLL_OK;
    for (long long r0 = 0; r0 < B && status == RVLL_OK && e == hipSuccess; r0 += rows) {
        const long long R = std::min<long long>(rows, B - r0);
        status = rvll_dev_upload_theta(h, theta + r0 * (long long)h->L.ndim, R);
        if (status != RVLL_OK) break;
        rvll::LoglikeArgs a;
        status = rvll::host::build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], R, &a);
        if (status != RVLL_OK) break;
        if (phase_ms) e = hipEventRecord(ev[0], h->compute);
        if (e == hipSuccess) e = rvll::launch_residuals(a, ds, ~0u, d_res, d_var, h->compute);
        if (e == hipSuccess && phase_ms) e = hipEventRecord(ev[1], h->compute);
        if (e == hipSuccess)
            e = rvll::launch_celerite_factor(J, h->d_theta, h->L.ndim, R, d_res, d_var, Ne, d_ord, d_tab, d_tab + Ne, plan, h->cte, d_logl,
                                             d_flag, d_ws, rp, h->compute);
        if (e == hipSuccess && phase_ms) e = hipEventRecord(ev[2], h->compute);
        if (e == hipSuccess) {
            switch (J) {
#define RVLL_CEL_SWEEPS(N) \
    case N: e = rvll::launch_sweeps<N>(h->d_theta, h->L.ndim, R, Ne, d_tab, d_tab + Ne, plan, d_ws, rp, d_qstart, d_qtab, m, d_wq, d_wv, \
                                       h->compute, ev[3]); break
                RVLL_CEL_SWEEPS(1);
                RVLL_CEL_SWEEPS(2);
                RVLL_CEL_SWEEPS(3);
                RVLL_CEL_SWEEPS(4);
#undef RVLL_CEL_SWEEPS
            }
        }
        if (e == hipSuccess && phase_ms) e = hipEventRecord(ev[4], h->compute);
        // into the caller's layouts: the epochs through `order` into table order, the queries into the order they were given
        const int fields[3] = {J + rvll::kCelWsR, J + rvll::kCelWsMean, J + rvll::kCelWsVar};
        double* const host_e[3] = {residual, mean_data, var_data};
        for (int k = 0; k < 3; ++k) {
            if (!host_e[k]) continue;
            if (e == hipSuccess)
                e = rvll::launch_transpose(d_ws + fields[k] * fstride, estride, Ne, R, d_ord, d_flag, d_oute + (size_t)k * rne, Ne, h->compute);
            if (e == hipSuccess)
                e = hipMemcpyAsync(host_e[k] + r0 * Ne, d_oute + (size_t)k * rne, d8 * (size_t)R * (size_t)Ne, hipMemcpyDeviceToHost, h->compute);
        }
        double* const host_q[2] = {mean, with_var ? var : nullptr};
        for (int k = 0; k < nq && m > 0; ++k) {
            if (e == hipSuccess)
                e = rvll::launch_transpose(d_wq + (size_t)k * (size_t)m * (size_t)rp, rp, m, R, d_qperm, d_flag, d_outq + (size_t)k * rm, m, h->compute);
            if (e == hipSuccess)
                e = hipMemcpyAsync(host_q[k] + r0 * m, d_outq + (size_t)k * rm, d8 * (size_t)R * (size_t)m, hipMemcpyDeviceToHost, h->compute);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(logl + r0, d_logl, d8 * (size_t)R, hipMemcpyDeviceToHost, h->compute);
        if (e == hipSuccess) e = hipMemcpyAsync(flags + r0, d_flag, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, h->compute);
        if (e == hipSuccess) e = hipStreamSynchronize(h->compute);
        float ms = 0.f;
        for (int k = 0; k < 4; ++k)
            if (e == hipSuccess && phase_ms && (e = hipEventElapsedTime(&ms, ev[k], ev[k + 1])) == hipSuccess) phase_ms[k] += ms;
    }
    if (status == RVLL_OK && e != hipSuccess)
        status = report_error(e == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, "celerite_predict_batch: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->compute);
    for (auto& k : ev)
        if (k) (void)hipEventDestroy(k);
    return status;
}

}  // extern "C"
