// Log-likelihood under correlated noise on gfx950: celerite kernels, solved per row (rvll_celerite_loglike_batch).
// evidence_amd/correlated.py holds the numpy definitions; rvll_celerite.h the recursion this kernel runs.
//
//   stage 1   launch_residuals (rvll_gls.hip) with every planet subtracted: res and var [rows, Ne] in HBM.
//   stage 2   celerite_kernel<J>, J = 1 .. 4 the number of columns (celerite_kernel<J, double*, long long> is the same sweep with
//             stores for the prediction, whose other sweeps are in rvll_celerite_predict.hip).  A row's factorisation is a serial chain in the epoch, the rows
//             are the parallel axis: one lane a row, a workgroup is one wave of kCelRows rows, and a row's state (the upper
//             triangle of S, f, W, D, z, two sums) and its columns stay in registers.  The columns (a, b, c, d) and sum a are
//             computed once a row from theta, before the epoch loop.
//             A lane reading its own row of res would stride by Ne doubles across the wave.  Instead the workgroup stages
//             kCelRows rows x kCelEpochs epochs of res and var in LDS: half a wave reads kCelEpochs consecutive epochs of one
//             row, gathered through `order` (consecutive addresses wherever the table is in time order), and the epoch loop
//             reads one epoch a step at a row stride of kCelStride = kCelEpochs + 1 doubles.  ds_read_b64 serves 32 lanes a
//             cycle over 64 dword banks: lane l of a half reads dword 2 (l kCelStride + e), and an odd stride sends the 32 lanes
//             to 32 different bank pairs.
//             The times from the first epoch and the gaps are read from per-epoch tables the host builds in time order (the same
//             address for every lane: scalar loads), so an epoch costs one sincos per complex term and one exponential per
//             distinct c, both unavoidable while c and d are free parameters.
// A row's result reads nothing of other rows and adds its epochs in time order: its bits depend on the row and the epoch table
// alone, not on the batch, the chunk or the lane.  No atomics, no inline assembly.
#include "rvll_host.h"
#include "rvll_celerite.h"

namespace rvll {

namespace {

constexpr int kCelEpochs = 32;                            // epochs of a tile
constexpr int kCelStride = kCelEpochs + 1;                // doubles between the rows of a tile: odd
static_assert(kCelRows == kWave && kCelEpochs * 2 == kCelRows, "the tile load gives half a wave to a row");
static_assert(kCelStride % 2 == 1, "an even stride folds the lanes of a read onto fewer banks");

// What the prediction's factor sweep leaves of an epoch (rvll_celerite_predict.hip): W, D, z, r and var in
// ws [epoch][J + kCelWsExtra fields][rp rows] (rvll_celerite.h); the 64 lanes of the wave write 512 consecutive bytes a field.
template <int J>
__device__ __forceinline__ void cel_store(const CelState<J>& st, double r, double v, int epoch, long long row, double* __restrict__ ws,
                                          long long rp)
{
    double* w = ws + (long long)epoch * (J + kCelWsExtra) * rp + row;
#pragma unroll
    for (int j = 0; j < J; ++j) w[j * rp] = st.W[j];
    w[(J + kCelWsD) * rp] = st.D;
    w[(J + kCelWsZ) * rp] = st.z;
    w[(J + kCelWsR) * rp] = r;
    w[(J + kCelWsVar) * rp] = v;
}

// Ws: nothing for the log-L call, whose kernel then has the arguments and, instruction for instruction, the code it had before
// there was a prediction; (double* ws, long long rp) for the prediction, whose sweep also stores every epoch (cel_store).
template <int J, typename... Ws>
__global__ __launch_bounds__(kCelRows)
void celerite_kernel(const double* __restrict__ theta, int D, long long B, const double* __restrict__ res,
                     const double* __restrict__ var, int Ne, const int32_t* __restrict__ order, const double* __restrict__ ts,
                     const double* __restrict__ dts, const CelPlan plan, double cte, double* __restrict__ logl,
                     int32_t* __restrict__ flags, Ws... ws)
{
    __shared__ double sh_r[kCelRows * kCelStride], sh_v[kCelRows * kCelStride];
    const int lane = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * kCelRows, row = row0 + lane;
    const double* th = theta + (row < B ? row : B - 1) * D;           // a lane past the end works on the last row and stores nothing
    CelColumn col[J];
    bool valid = true;
    double suma = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double p[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const rvll_slot s = plan.par[j][q];
            p[q] = s.idx >= 0 ? th[s.idx] : s.val;
        }
        valid &= cel_column(plan.kind[j], plan.sub[j], p, col[j]);
        if (col[j].form != kCelColSin) suma += col[j].a;             // a complex term's a counts once
    }
    const bool pair = cel_prepare<J>(col);                            // a near-degenerate SHO pair changes basis (rvll_celerite.h)
    CelState<J> st;
    cel_init(st);
    const int le = lane & (kCelEpochs - 1), lr = lane >> 5;           // the tile load: this lane's epoch, and which row of a pair
    for (int e0 = 0; e0 < Ne; e0 += kCelEpochs) {
        const int ec = Ne - e0 < kCelEpochs ? Ne - e0 : kCelEpochs;
        __syncthreads();                                              // the previous tile has been read
        if (le < ec) {
            const int src = order[e0 + le];
#pragma unroll 8                                                      // 16 loads in flight (3 % of the solve at J = 1: the chain, not the load, is its time)
            for (int rr = lr; rr < kCelRows; rr += 2) {
                const long long g = row0 + rr < B ? row0 + rr : B - 1;
                sh_r[rr * kCelStride + le] = res[g * Ne + src];
                sh_v[rr * kCelStride + le] = var[g * Ne + src];
            }
        }
        __syncthreads();
        for (int e = 0; e < ec; ++e) {
            cel_step<J>(col, suma, pair, st, ts[e0 + e], dts[e0 + e], sh_r[lane * kCelStride + e], sh_v[lane * kCelStride + e]);
            if constexpr (sizeof...(Ws) > 0)
                if (row < B) cel_store<J>(st, sh_r[lane * kCelStride + e], sh_v[lane * kCelStride + e], e0 + e, row, ws...);
        }
    }
    if (row < B) {
        double l;
        int32_t f;
        cel_result<J>(st, valid, cte, l, f);
        logl[row] = l;
        flags[row] = f;
    }
}

using CelKernel = void (*)(const double*, int, long long, const double*, const double*, int, const int32_t*, const double*,
                           const double*, const CelPlan, double, double*, int32_t*);
using CelStoreKernel = void (*)(const double*, int, long long, const double*, const double*, int, const int32_t*, const double*,
                                const double*, const CelPlan, double, double*, int32_t*, double*, long long);

CelKernel cel_kernel_of(int J)
{
    switch (J) {
    case 1: return celerite_kernel<1>;
    case 2: return celerite_kernel<2>;
    case 3: return celerite_kernel<3>;
    default: return celerite_kernel<4>;
    }
}

CelStoreKernel cel_store_kernel_of(int J)
{
    switch (J) {
    case 1: return celerite_kernel<1, double*, long long>;
    case 2: return celerite_kernel<2, double*, long long>;
    case 3: return celerite_kernel<3, double*, long long>;
    default: return celerite_kernel<4, double*, long long>;
    }
}

int cel_term_columns(int kind) { return kind == RVLL_NOISE_REAL ? 1 : kind == RVLL_NOISE_SHO ? 2 : kind == RVLL_NOISE_ROTATION ? 4 : -1; }

}  // namespace

size_t cel_up8(size_t n) { return (n + 7) & ~(size_t)7; }

// The factor sweep of R rows on a stream; ws (with its row stride rp) NULL: log-L and flags alone.
hipError_t launch_celerite_factor(int J, const double* theta, int D, long long R, const double* res, const double* var, int Ne,
                                  const int32_t* ord, const double* ts, const double* dts, const CelPlan& plan, double cte,
                                  double* logl, int32_t* flags, double* ws, long long rp, hipStream_t stream)
{
    const unsigned blocks = (unsigned)((R + kCelRows - 1) / kCelRows);
    if (ws)
        hipLaunchKernelGGL(cel_store_kernel_of(J), dim3(blocks), dim3(kCelRows), 0, stream, theta, D, R, res, var, Ne, ord, ts, dts,
                           plan, cte, logl, flags, ws, rp);
    else
        hipLaunchKernelGGL(cel_kernel_of(J), dim3(blocks), dim3(kCelRows), 0, stream, theta, D, R, res, var, Ne, ord, ts, dts, plan,
                           cte, logl, flags);
    return hipGetLastError();
}

// The checks on the handle and the terms that every correlated-noise call makes, and the terms as a plan of J columns.
int cel_make_plan(rvll_handle* h, const rvll_noise_term* terms, int32_t n_terms, CelPlan& plan, int& J)
{
    if (h->L.precision != RVLL_PREC_FP64) return report_error(RVLL_E_UNSUPPORTED, "the correlated-noise likelihood exists for fp64 only");
    if (!terms) return report_error(RVLL_E_INVALID, "null buffer");
    if (n_terms < 1 || n_terms > RVLL_NOISE_MAX_TERMS)
        return report_error(RVLL_E_INVALID, "n_terms must be in [1, %d]", RVLL_NOISE_MAX_TERMS);
    plan = CelPlan{};
    J = 0;
    for (int32_t k = 0; k < n_terms; ++k) {
        const int nc = cel_term_columns(terms[k].kind);
        if (nc < 0) return report_error(RVLL_E_INVALID, "term %d: unknown kind %d", (int)k, (int)terms[k].kind);
        if (J + nc > RVLL_NOISE_MAX_RANK) return report_error(RVLL_E_INVALID, "more than %d columns", RVLL_NOISE_MAX_RANK);
        for (int q = 0; q < 5; ++q)
            if (terms[k].par[q].idx >= h->L.ndim)
                return report_error(RVLL_E_INVALID, "term %d: slot index %d outside [0, %d)", (int)k, (int)terms[k].par[q].idx, h->L.ndim);
        for (int s = 0; s < nc; ++s, ++J) {
            plan.kind[J] = terms[k].kind;
            plan.sub[J] = s;
            for (int q = 0; q < 5; ++q) plan.par[J][q] = terms[k].par[q];
        }
    }
    if (h->Ne < 1) return report_error(RVLL_E_INVALID, "the epoch table is empty");
    return RVLL_OK;
}

// The epochs in time order: the order itself, and tab = the times from the first of them [Ne], then the gaps [Ne].
int cel_time_tables(rvll_handle* h, const int32_t* order, std::vector<int32_t>& ord, std::vector<double>& tab)
{
    const int Ne = h->Ne;
    if (h->cel_times.size() != (size_t)Ne) {
        std::vector<double> t((size_t)Ne);
        HIP_TRY(hipMemcpy(t.data(), h->d_t, sizeof(double) * (size_t)Ne, hipMemcpyDeviceToHost));
        h->cel_times.swap(t);
    }
    ord.assign((size_t)Ne, 0);
    tab.assign(2 * (size_t)Ne, 0.0);
    std::vector<char> seen((size_t)Ne, 0);
    for (int n = 0; n < Ne; ++n) {
        const int32_t e = order ? order[n] : n;
        if (e < 0 || e >= Ne || seen[(size_t)e]) return report_error(RVLL_E_INVALID, "order is not a permutation of the epochs");
        seen[(size_t)e] = 1;
        ord[(size_t)n] = e;
    }
    const double t0 = h->cel_times[(size_t)ord[0]];
    for (int n = 0; n < Ne; ++n) {
        const double tn = h->cel_times[(size_t)ord[(size_t)n]];
        const double tp = n > 0 ? h->cel_times[(size_t)ord[(size_t)n - 1]] : tn;
        if (!(tn >= tp)) return report_error(RVLL_E_INVALID, "the times decrease along order at position %d", n);
        tab[(size_t)n] = tn - t0;
        tab[(size_t)Ne + (size_t)n] = tn - tp;
    }
    return RVLL_OK;
}

// d_cel grown to at least `total` bytes.
int cel_reserve(rvll_handle* h, size_t total)
{
    if (total <= h->cel_cap) return RVLL_OK;
    HIP_TRY(hipStreamSynchronize(h->compute));
    host::dev_free(h->d_cel);
    h->cel_cap = 0;
    if (hipMalloc(&h->d_cel, total) != hipSuccess) {
        h->d_cel = nullptr;
        return report_error(RVLL_E_NOMEM, "celerite: %zu bytes", total);
    }
    h->cel_cap = total;
    return RVLL_OK;
}

}  // namespace rvll

extern "C" {

int rvll_celerite_loglike_batch(rvll_handle* h, const double* x, int64_t B, int32_t from_cube, const rvll_noise_term* terms,
                                int32_t n_terms, const int32_t* order, double* theta_out, double* logl, int32_t* flags,
                                double* phase_ms)
{
    using rvll::report_error;
    int rc = rvll::host::use_device(h);
    if (rc) return rc;
    if (B < 0) return report_error(RVLL_E_INVALID, "negative size");
    rvll::CelPlan plan;
    int J = 0;
    rc = rvll::cel_make_plan(h, terms, n_terms, plan, J);
    if (rc) return rc;
    const int Ne = h->Ne;
    if (from_cube && !h->have_priors) return report_error(RVLL_E_NOPRIORS, "rvll_set_priors has not been called");
    if (phase_ms) phase_ms[0] = phase_ms[1] = 0.0;

    // the epochs in time order: the order itself, the times from the first of them, the gaps
    std::vector<int32_t> ord;
    std::vector<double> tab;                                          // times, then gaps
    rc = rvll::cel_time_tables(h, order, ord, tab);
    if (rc) return rc;
    if (B == 0) return RVLL_OK;
    if (!x || !logl || !flags) return report_error(RVLL_E_INVALID, "null buffer");

    // rows a chunk: res and var of them take at most kCelChunkBytes (RVLL_CELERITE_CHUNK_ROWS: a row count for tests of the
    // chunk boundary)
    long long rows = std::max<long long>(1, rvll::kCelChunkBytes / (2ll * (long long)sizeof(double) * Ne));
    if (const char* env = getenv("RVLL_CELERITE_CHUNK_ROWS")) {
        const long long v = atoll(env);
        if (v >= 1) rows = std::min(rows, v);
    }
    rows = std::min<long long>(rows, B);
    const size_t o_ord = 0, o_tab = rvll::cel_up8(sizeof(int32_t) * (size_t)Ne), o_res = o_tab + sizeof(double) * 2 * (size_t)Ne,
                 o_var = o_res + sizeof(double) * (size_t)rows * (size_t)Ne, o_logl = o_var + sizeof(double) * (size_t)rows * (size_t)Ne,
                 o_flag = o_logl + sizeof(double) * (size_t)rows, total = o_flag + rvll::cel_up8(sizeof(int32_t) * (size_t)rows);
    rc = rvll::cel_reserve(h, total);
    if (rc) return rc;
    char* base = static_cast<char*>(h->d_cel);
    int32_t* d_ord = reinterpret_cast<int32_t*>(base + o_ord);
    double* d_tab = reinterpret_cast<double*>(base + o_tab);
    double *d_res = reinterpret_cast<double*>(base + o_res), *d_var = reinterpret_cast<double*>(base + o_var);
    double* d_logl = reinterpret_cast<double*>(base + o_logl);
    int32_t* d_flag = reinterpret_cast<int32_t*>(base + o_flag);
    HIP_TRY(hipMemcpyAsync(d_ord, ord.data(), sizeof(int32_t) * (size_t)Ne, hipMemcpyHostToDevice, h->compute));
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(double) * 2 * (size_t)Ne, hipMemcpyHostToDevice, h->compute));
    HIP_TRY(hipStreamSynchronize(h->compute));                        // ord and tab leave scope with this call

    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    if (phase_ms)
        for (auto& m : ev)
            if (e == hipSuccess) e = hipEventCreate(&m);
    const rvll::DriftSlots ds = rvll::drift_slots(h);
    const size_t row_bytes = sizeof(double) * (size_t)h->L.ndim;
    int status = RVLL_OK;
    for (long long r0 = 0; r0 < B && status == RVLL_OK && e == hipSuccess; r0 += rows) {
        const long long R = std::min<long long>(rows, B - r0);
        const double* xr = x + r0 * (long long)h->L.ndim;
        if (from_cube) {
            status = rvll_dev_upload_cube(h, xr, R);
            if (status == RVLL_OK) status = rvll_dev_prior(h, R);
        } else {
            status = rvll_dev_upload_theta(h, xr, R);
        }
        if (status != RVLL_OK) break;
        rvll::LoglikeArgs a;
        status = rvll::host::build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], R, &a);
        if (status != RVLL_OK) break;
        if (phase_ms) e = hipEventRecord(ev[0], h->compute);
        if (e == hipSuccess) e = rvll::launch_residuals(a, ds, ~0u, d_res, d_var, h->compute);
        if (e == hipSuccess && phase_ms) e = hipEventRecord(ev[1], h->compute);
        if (e == hipSuccess)
            e = rvll::launch_celerite_factor(J, h->d_theta, h->L.ndim, R, d_res, d_var, Ne, d_ord, d_tab, d_tab + Ne, plan, h->cte, d_logl,
                                             d_flag, nullptr, 0, h->compute);
        if (e == hipSuccess && phase_ms) e = hipEventRecord(ev[2], h->compute);
        if (e == hipSuccess) e = hipMemcpyAsync(logl + r0, d_logl, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost, h->compute);
        if (e == hipSuccess) e = hipMemcpyAsync(flags + r0, d_flag, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, h->compute);
        if (e == hipSuccess && from_cube && theta_out)
            e = hipMemcpyAsync(theta_out + r0 * (long long)h->L.ndim, h->d_theta, row_bytes * (size_t)R, hipMemcpyDeviceToHost, h->compute);
        if (e == hipSuccess) e = hipStreamSynchronize(h->compute);
        float ms = 0.f;
        for (int k = 0; k < 2; ++k)
            if (e == hipSuccess && phase_ms && (e = hipEventElapsedTime(&ms, ev[k], ev[k + 1])) == hipSuccess) phase_ms[k] += ms;
    }
    if (status == RVLL_OK && e != hipSuccess)
        status = report_error(e == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, "celerite_loglike_batch: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->compute);
    for (auto& m : ev)
        if (m) (void)hipEventDestroy(m);
    return status;
}

}  // extern "C"
