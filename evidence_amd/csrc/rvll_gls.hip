// Residuals of the likelihood's own model and their generalised Lomb-Scargle periodograms on gfx950 (rvll_residuals_batch,
// rvll_gls_bands).  evidence_amd/periodogram.py holds the numpy definitions.
//
//   residual_kernel   one thread a (row, epoch): res = y - (offset + Keplerian sum + drift + linear terms), the additions in the
//                     order of RVModel.log_likelihood (rvmodel:180-215), and var = svrad^2 + jitter^2 of the epoch's instrument.
//                     The Keplerian sum is what keprv_kernel wrote for the epoch table's times: an invalid orbit's NaN row stays one.
//   weights_kernel    one wave a row: w_i = (1 / var_i) / sum(1 / var) over var, w_i r_i over res (both in place), W = sum w,
//                     Y = sum w r and YY = sum w r^2 - Y^2.  A lane adds epochs lane, lane + 64, ... in order, a fixed xor tree
//                     adds the lanes.
//   gls_kernel        a workgroup owns kGlsFreqs consecutive frequencies x kGlsDraws consecutive rows.  sin and cos of an (epoch,
//                     frequency) pair do not depend on the row: a thread takes ONE sincos an epoch at its first frequency
//                     k0 = kGlsFpt * (its index among all threads of the frequency axis), rotates by the epoch's (cos, sin) of
//                     2 pi df tau to reach k0 + 1 .. k0 + kGlsFpt - 1, and feeds the kGlsDraws rows, whose w and w r of the epoch
//                     every lane reads from the same LDS address (a broadcast).  Six weighted sums of every (row, frequency)
//                     stay in registers — of cos, sin, cos^2 - sin^2, cos sin with w and of cos, sin with w r: one fused
//                     multiply-add each a term, the two products of cos and sin shared by the rows; sum w cos^2 and sum w sin^2
//                     are (W +- sum w (cos^2 - sin^2)) / 2.  Epochs pass through LDS kGlsEpochs at a time, in order, so the epoch
//                     count is not bounded by LDS; the terms of kGlsBlock consecutive epochs (blocks start at multiples of it in
//                     the epoch table) are added up first and the blocks' sums then, which keeps the rounding of a sum over
//                     thousands of epochs near that of numpy's pairwise sums.  Frequency k is always the
//                     (k mod kGlsFpt)-th rotation from an exact sincos at k - k mod kGlsFpt, and a row's sums read nothing of other
//                     rows: the bits of a power depend on its row and its frequency alone, not on the tile, the group or the chunk.
//   peak_kernel       one wave a row: the first index of the largest power (a NaN power counts as the largest, as numpy.argmax
//                     has it) and the power there; -1 and NaN for a row that is NaN throughout (an invalid orbit).
// No floating-point atomics, no inline assembly.  The order statistics over a group's rows are launch_bands' (rvll_bands.hip).
//
// What holds the powers (tests/test_gpu_gls_windows.py): windows of 512 absolute frequency indices, each within 8 delta
// of its own row and window of the long-double definition, on the default grid f0 = df = 1 / (8 span) up to k = 2^18 + 2 (so
// df * (double)k0 at k0 = 262144 and phases of 1e5 rad), on tables of 4 to 513 epochs in and out of time order.  A frequency at
// which every epoch has the same sine or cosine in exact arithmetic (an alias of f = 0 or of the half sampling rate on an evenly
// spaced table) is not guarded beyond den > 0: CC, SS and D are rounding residue there, the power is a NaN or a number without
// meaning, as the definition's is, and where the NaNs fall depends on the order of the sums.
#include "rvll_host.h"
#include "rvll_math.h"

namespace rvll {

namespace {

constexpr double kGlsTwoPi = 6.283185307179586476925286766559;   // fl(2 pi), as 2 * np.pi
constexpr int kGlsThreads = 256;
constexpr int kGlsFpt = 2;                                // consecutive frequencies a thread
constexpr int kGlsFreqs = kGlsThreads * kGlsFpt;          // ... a workgroup
constexpr int kGlsDraws = 4;                              // rows a workgroup
constexpr int kGlsEpochs = 256;                           // epochs in LDS at a time: (3 + 2 kGlsDraws) x 2 KiB = 22 KiB
constexpr int kGlsBlock = 64;                             // epochs whose terms are added up before they join the running sums
constexpr int kGlsSums = 6;
static_assert(kGlsEpochs % kGlsBlock == 0, "the blocks of a sum must start at multiples of kGlsBlock in the epoch table");

__device__ __forceinline__ double gls_slot(const rvll_slot s, const double* th) { return s.idx >= 0 ? th[s.idx] : s.val; }

__global__ __launch_bounds__(kGlsThreads)
void residual_kernel(const LoglikeArgs a, const DriftSlots ds, double* __restrict__ res /* in: the Keplerian sums */,
                     double* __restrict__ var)
{
    const long long n = a.B * (long long)a.Ne;
    for (long long i = (long long)blockIdx.x * kGlsThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kGlsThreads) {
        const long long b = i / a.Ne;
        const int j = (int)(i - b * a.Ne);
        const double* th = a.theta + b * a.D;
        const rvll_inst in = a.insts[a.inst[j]];
        const double t = a.t[j];
        double rvm = gls_slot(in.offset, th);                                   // rvmodel:187
        double v = a.s2[j];
        if (a.has_jitter) { const double jit = gls_slot(in.jitter, th); v = v + jit * jit; }   // rvmodel:190
        rvm += res[i];                                                          // rvmodel:199
        if (a.has_drift) {                                                      // rvmodel:242-271
            const double tref = a.tref_from_data ? a.t[0] : gls_slot(ds.s[4], th);
            const double tt = (t - tref) / 365.25;
            const double t2 = tt * tt;
            rvm += gls_slot(ds.s[0], th) * tt + gls_slot(ds.s[1], th) * t2 + gls_slot(ds.s[2], th) * (t2 * tt)
                   + gls_slot(ds.s[3], th) * (t2 * t2);
        }
        for (int k = 0; k < a.nlin; ++k)                                        // rvmodel:210-212
            rvm += gls_slot(a.linslots[k], th) * a.linpar[(size_t)k * a.Ne + j];
        res[i] = a.y[j] - rvm;                                                  // rvmodel:215
        var[i] = v;
    }
}

__device__ __forceinline__ double gls_wave_sum(double v)      // every lane gets the sum; the tree is the same for every row
{
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

__global__ __launch_bounds__(kGlsThreads)
void weights_kernel(double* __restrict__ wr /* in: res */, double* __restrict__ w /* in: var */, long long R, int Ne,
                    double* __restrict__ W, double* __restrict__ Y, double* __restrict__ YY)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * (kGlsThreads / kWave) + (threadIdx.x >> 6);
    if (row >= R) return;                                  // (a whole wave leaves: no barrier below)
    double* __restrict__ pr = wr + row * Ne;
    double* __restrict__ pv = w + row * Ne;
    double sum = 0.;
    for (int i = lane; i < Ne; i += kWave) sum += 1.0 / pv[i];
    sum = gls_wave_sum(sum);
    double y = 0., yy = 0., ws = 0.;
    for (int i = lane; i < Ne; i += kWave) {
        const double wi = (1.0 / pv[i]) / sum, r = pr[i], wri = wi * r;
        pv[i] = wi;
        pr[i] = wri;
        ws += wi;
        y += wri;
        yy = __builtin_fma(wri, r, yy);
    }
    y = gls_wave_sum(y);
    yy = gls_wave_sum(yy);
    ws = gls_wave_sum(ws);
    if (lane == 0) {
        W[row] = ws;
        Y[row] = y;
        YY[row] = yy - y * y;
    }
}

__global__ __launch_bounds__(kGlsThreads)
void gls_kernel(const double* __restrict__ w, const double* __restrict__ wr, const double* __restrict__ W,
                const double* __restrict__ Y, const double* __restrict__ YY, const double* __restrict__ t, double tmin, int Ne,
                long long R, double f0, double df, int F, int nft, double* __restrict__ P)
{
    __shared__ double sh_tau[kGlsEpochs], sh_cd[kGlsEpochs], sh_sd[kGlsEpochs];
    __shared__ double sh_w[kGlsEpochs * kGlsDraws], sh_wr[kGlsEpochs * kGlsDraws];        // [epoch][draw]
    const int tid = threadIdx.x;
    const int ft = (int)(blockIdx.x % (unsigned)nft);
    const long long r0 = (long long)(blockIdx.x / (unsigned)nft) * kGlsDraws;
    const long long k0 = ((long long)ft * kGlsThreads + tid) * kGlsFpt;     // an absolute frequency index: a multiple of kGlsFpt
    const bool active = k0 < F;
    const double om = kGlsTwoPi * (f0 + df * (double)k0), dom = kGlsTwoPi * df;
    // per (draw, frequency): sum w c, w s, w (c c - s s), w c s, w r c, w r s — of the current block of kGlsBlock epochs, and of
    // the blocks before it
    double acc[kGlsDraws][kGlsFpt][kGlsSums], tot[kGlsDraws][kGlsFpt][kGlsSums];
#pragma unroll
    for (int d = 0; d < kGlsDraws; ++d)
#pragma unroll
        for (int j = 0; j < kGlsFpt; ++j)
#pragma unroll
            for (int q = 0; q < kGlsSums; ++q) acc[d][j][q] = tot[d][j][q] = 0.;
    for (int e0 = 0; e0 < Ne; e0 += kGlsEpochs) {
        const int ec = Ne - e0 < kGlsEpochs ? Ne - e0 : kGlsEpochs;
        __syncthreads();                                   // the previous chunk has been read
        for (int i = tid; i < ec; i += kGlsThreads) {
            const double tau = t[e0 + i] - tmin;
            double s, c;
            sincos_f64(dom * tau, s, c);
            sh_tau[i] = tau;
            sh_cd[i] = c;
            sh_sd[i] = s;
        }
        for (int e = tid; e < ec * kGlsDraws; e += kGlsThreads) {              // consecutive threads: consecutive epochs of a row
            const int d = e / ec, i = e - d * ec;
            const long long row = r0 + d;
            double a = 0., b = 0.;
            if (row < R) {
                a = w[row * Ne + e0 + i];
                b = wr[row * Ne + e0 + i];
            }
            sh_w[i * kGlsDraws + d] = a;
            sh_wr[i * kGlsDraws + d] = b;
        }
        __syncthreads();
        if (active)
            for (int i0 = 0; i0 < ec; i0 += kGlsBlock) {                       // (kGlsEpochs is a multiple of kGlsBlock: the blocks
                const int i1 = i0 + kGlsBlock < ec ? i0 + kGlsBlock : ec;      // start at multiples of it in the epoch table)
                for (int i = i0; i < i1; ++i) {
                    double s, c;
                    sincos_f64(om * sh_tau[i], s, c);
                    const double cd = sh_cd[i], sd = sh_sd[i];
#pragma unroll
                    for (int j = 0; j < kGlsFpt; ++j) {
                        if (j > 0) {                                           // one frequency step on
                            const double cn = __builtin_fma(c, cd, -(s * sd)), sn = __builtin_fma(s, cd, c * sd);
                            c = cn;
                            s = sn;
                        }
                        const double c2 = __builtin_fma(c, c, -(s * s)), cs = c * s;
#pragma unroll
                        for (int d = 0; d < kGlsDraws; ++d) {
                            const double wv = sh_w[i * kGlsDraws + d], wrv = sh_wr[i * kGlsDraws + d];
                            acc[d][j][0] = __builtin_fma(wv, c, acc[d][j][0]);
                            acc[d][j][1] = __builtin_fma(wv, s, acc[d][j][1]);
                            acc[d][j][2] = __builtin_fma(wv, c2, acc[d][j][2]);
                            acc[d][j][3] = __builtin_fma(wv, cs, acc[d][j][3]);
                            acc[d][j][4] = __builtin_fma(wrv, c, acc[d][j][4]);
                            acc[d][j][5] = __builtin_fma(wrv, s, acc[d][j][5]);
                        }
                    }
                }
#pragma unroll
                for (int d = 0; d < kGlsDraws; ++d)
#pragma unroll
                    for (int j = 0; j < kGlsFpt; ++j)
#pragma unroll
                        for (int q = 0; q < kGlsSums; ++q) {
                            tot[d][j][q] += acc[d][j][q];
                            acc[d][j][q] = 0.;
                        }
            }
    }
    if (!active) return;
#pragma unroll
    for (int d = 0; d < kGlsDraws; ++d) {
        const long long row = r0 + d;
        if (row >= R) break;
        const double y = Y[row], yy = YY[row], hw = 0.5 * W[row];
#pragma unroll
        for (int j = 0; j < kGlsFpt; ++j) {
            if (k0 + j >= F) break;
            // sum w c c = (sum w + sum w (c c - s s)) / 2 and sum w s s = (sum w - ...) / 2
            const double C = tot[d][j][0], S = tot[d][j][1], A = 0.5 * tot[d][j][2];
            const double CC = (hw + A) - C * C, SS = (hw - A) - S * S, CS = tot[d][j][3] - C * S;
            const double YC = tot[d][j][4] - y * C, YS = tot[d][j][5] - y * S;
            const double D = CC * SS - CS * CS;
            const double num = SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS;
            const double den = yy * D;
            P[row * F + k0 + j] = den > 0. ? num / den : NAN;
        }
    }
}

__global__ __launch_bounds__(kGlsThreads)
void peak_kernel(const double* __restrict__ P, long long R, int F, int32_t* __restrict__ idx,
                 double* __restrict__ pow)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * (kGlsThreads / kWave) + (threadIdx.x >> 6);
    if (row >= R) return;
    const double* __restrict__ p = P + row * F;
    // the order numpy.argmax keeps: a NaN beats every number, otherwise the larger value, and among equals the lower index
    double best = -INFINITY;
    int at = 0x7fffffff;
    bool bnan = false, hasnum = false;
    for (int k = lane; k < F; k += kWave) {
        const double v = p[k];
        const bool vnan = v != v;
        hasnum |= !vnan;
        if (at == 0x7fffffff || (!bnan && (vnan || v > best))) {
            best = v;
            at = k;
            bnan = vnan;
        }
    }
    const bool dead = __ballot(hasnum) == 0ull;            // not one number in the row
    for (int m = 32; m > 0; m >>= 1) {
        const double ov = __shfl_xor(best, m, kWave);
        const int oat = __shfl_xor(at, m, kWave);
        const bool onan = ov != ov;
        const bool take = oat != 0x7fffffff && (at == 0x7fffffff || (onan && (!bnan || oat < at)) ||
                                                (!onan && !bnan && (ov > best || (ov == best && oat < at))));
        if (take) {
            best = ov;
            at = oat;
            bnan = onan;
        }
    }
    if (lane == 0) {
        idx[row] = dead ? -1 : at;
        pow[row] = dead ? NAN : best;
    }
}

}  // namespace

hipError_t launch_residuals(const LoglikeArgs& a, const DriftSlots& ds, unsigned include_mask, double* res, double* var,
                            hipStream_t stream)
{
    const long long n = a.B * (long long)a.Ne;
    if (n <= 0) return hipSuccess;
    hipError_t e = launch_keprv(a, a.t, a.Ne, include_mask, res, stream);
    if (e != hipSuccess) return e;
    long long blocks = (n + kGlsThreads - 1) / kGlsThreads;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(residual_kernel, dim3((unsigned)blocks), dim3(kGlsThreads), 0, stream, a, ds, res, var);
    return hipGetLastError();
}

DriftSlots drift_slots(const rvll_handle* h)
{
    DriftSlots ds;
    for (int k = 0; k < 4; ++k) ds.s[k] = h->L.drift[k];
    ds.s[4] = h->L.tref;
    return ds;
}

namespace {

constexpr long long kGlsMaxBlocks = 1ll << 30;

}  // namespace

}  // namespace rvll

using rvll::host::dev_free;

extern "C" {

int rvll_residuals_batch(rvll_handle* h, const double* theta, int64_t B, uint32_t include_mask, double* res, double* var)
{
    int rc = rvll::host::use_device(h);
    if (rc) return rc;
    if (B < 0) return rvll::report_error(RVLL_E_INVALID, "negative size");
    if (B == 0 || h->Ne == 0) return RVLL_OK;
    if (!theta || !res || !var) return rvll::report_error(RVLL_E_INVALID, "null buffer");
    rc = rvll_dev_upload_theta(h, theta, B);
    if (rc) return rc;
    const size_t bytes = sizeof(double) * (size_t)B * (size_t)h->Ne;
    double *d_res = nullptr, *d_var = nullptr;
    int status = RVLL_OK;
    hipError_t e = hipMalloc(&d_res, bytes);
    if (e == hipSuccess) e = hipMalloc(&d_var, bytes);
    if (e == hipSuccess) {
        rvll::LoglikeArgs a;
        status = rvll::host::build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], B, &a);
        if (status == RVLL_OK) e = rvll::launch_residuals(a, rvll::drift_slots(h), include_mask, d_res, d_var, h->compute);
    }
    if (status == RVLL_OK && e == hipSuccess) e = hipMemcpyAsync(res, d_res, bytes, hipMemcpyDeviceToHost, h->compute);
    if (status == RVLL_OK && e == hipSuccess) e = hipMemcpyAsync(var, d_var, bytes, hipMemcpyDeviceToHost, h->compute);
    if (status == RVLL_OK && e == hipSuccess) e = hipStreamSynchronize(h->compute);
    if (status == RVLL_OK && e != hipSuccess)
        status = rvll::report_error(e == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, "residuals_batch: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->compute);
    dev_free(d_res); dev_free(d_var);
    return status;
}

int rvll_gls_bands(rvll_handle* h, const double* theta, int64_t n_groups, int32_t n, uint32_t include_mask, double f0, double df,
                   int32_t n_freq, const double* levels, int32_t n_q, double* q, double* mean, int32_t* n_valid,
                   int32_t* peak_index, double* peak_power, double* power_out, int64_t chunk_bytes, double* phase_ms)
{
    using rvll::report_error;
    int rc = rvll::host::use_device(h);
    if (rc) return rc;
    if (n_groups < 0 || chunk_bytes < 0) return report_error(RVLL_E_INVALID, "negative size");
    if (n < 1 || n > 4096) return report_error(RVLL_E_INVALID, "n must be in [1, 4096]");
    if (n_q < 1 || n_q > 16) return report_error(RVLL_E_INVALID, "n_q must be in [1, 16]");
    if (!(f0 > 0.0) || !(df > 0.0) || !(f0 < INFINITY) || !(df < INFINITY))
        return report_error(RVLL_E_INVALID, "f0 and df must be positive and finite");
    if (n_freq < 1 || n_freq > (1 << 24)) return report_error(RVLL_E_INVALID, "n_freq must be in [1, 2^24]");
    if (h->Ne < 4) return report_error(RVLL_E_INVALID, "a periodogram needs at least 4 epochs");
    if (!levels) return report_error(RVLL_E_INVALID, "null buffer");
    for (int32_t k = 0; k < n_q; ++k)
        if (!(levels[k] > 0.0 && levels[k] < 1.0)) return report_error(RVLL_E_INVALID, "level %d is outside (0, 1)", (int)k);
    if (phase_ms) phase_ms[0] = phase_ms[1] = phase_ms[2] = 0.0;
    if (n_groups == 0) return RVLL_OK;
    if (!theta || !q || !mean || !n_valid || !peak_index || !peak_power) return report_error(RVLL_E_INVALID, "null buffer");
    const int Ne = h->Ne, F = n_freq;
    const int nft = (F + rvll::kGlsFreqs - 1) / rvll::kGlsFreqs;
    const long long group_bytes = (long long)sizeof(double) * n * ((long long)F + 2ll * Ne);     // powers, w, w r
    const long long bound = chunk_bytes > 0 ? chunk_bytes : 256ll << 20;
    long long gc = std::min<long long>(n_groups, std::max<long long>(1, bound / group_bytes));    // whole groups a chunk
    const long long tiles_group = ((long long)n + rvll::kGlsDraws - 1) / rvll::kGlsDraws * nft;   // an upper bound a group
    gc = std::max<long long>(1, std::min<long long>(gc, rvll::kGlsMaxBlocks / tiles_group));
    const long long rc_rows = gc * n;
    double *d_levels = nullptr, *d_wr = nullptr, *d_w = nullptr, *d_W = nullptr, *d_Y = nullptr, *d_YY = nullptr, *d_P = nullptr, *d_q = nullptr,
           *d_mean = nullptr, *d_pp = nullptr;
    int32_t *d_nv = nullptr, *d_pi = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int status = RVLL_OK;
    hipError_t e = hipMalloc(&d_levels, sizeof(double) * (size_t)n_q);
    if (e == hipSuccess) e = hipMalloc(&d_wr, sizeof(double) * (size_t)(rc_rows * Ne));
    if (e == hipSuccess) e = hipMalloc(&d_w, sizeof(double) * (size_t)(rc_rows * Ne));
    if (e == hipSuccess) e = hipMalloc(&d_W, sizeof(double) * (size_t)rc_rows);
    if (e == hipSuccess) e = hipMalloc(&d_Y, sizeof(double) * (size_t)rc_rows);
    if (e == hipSuccess) e = hipMalloc(&d_YY, sizeof(double) * (size_t)rc_rows);
    if (e == hipSuccess) e = hipMalloc(&d_P, sizeof(double) * (size_t)(rc_rows * F));
    if (e == hipSuccess) e = hipMalloc(&d_q, sizeof(double) * (size_t)(gc * n_q * F));
    if (e == hipSuccess) e = hipMalloc(&d_mean, sizeof(double) * (size_t)(gc * F));
    if (e == hipSuccess) e = hipMalloc(&d_nv, sizeof(int32_t) * (size_t)(gc * F));
    if (e == hipSuccess) e = hipMalloc(&d_pi, sizeof(int32_t) * (size_t)rc_rows);
    if (e == hipSuccess) e = hipMalloc(&d_pp, sizeof(double) * (size_t)rc_rows);
    for (auto& x : ev)
        if (e == hipSuccess) e = hipEventCreate(&x);
    if (e == hipSuccess) e = hipMemcpyAsync(d_levels, levels, sizeof(double) * (size_t)n_q, hipMemcpyHostToDevice, h->compute);
    const rvll::DriftSlots ds = rvll::drift_slots(h);
    for (long long g0 = 0; g0 < n_groups && status == RVLL_OK && e == hipSuccess; g0 += gc) {
        const long long gb = std::min<long long>(gc, n_groups - g0), R = gb * n;
        status = rvll_dev_upload_theta(h, theta + g0 * n * (long long)h->L.ndim, R);
        if (status != RVLL_OK) break;
        rvll::LoglikeArgs a;
        status = rvll::host::build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], R, &a);
        if (status != RVLL_OK) break;
        const unsigned row_blocks = (unsigned)((R + rvll::kGlsThreads / rvll::kWave - 1) / (rvll::kGlsThreads / rvll::kWave));
        e = hipEventRecord(ev[0], h->compute);
        if (e == hipSuccess) e = rvll::launch_residuals(a, ds, include_mask, d_wr, d_w, h->compute);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(rvll::weights_kernel, dim3(row_blocks), dim3(rvll::kGlsThreads), 0, h->compute, d_wr, d_w, R, Ne, d_W, d_Y, d_YY);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev[1], h->compute);
        if (e == hipSuccess) {
            const long long blocks = (R + rvll::kGlsDraws - 1) / rvll::kGlsDraws * nft;
            hipLaunchKernelGGL(rvll::gls_kernel, dim3((unsigned)blocks), dim3(rvll::kGlsThreads), 0, h->compute, d_w, d_wr, d_W, d_Y, d_YY,
                               h->d_t, h->tmin, Ne, R, f0, df, F, nft, d_P);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev[2], h->compute);
        if (e == hipSuccess) e = rvll::launch_bands(d_P, gb, n, F, d_levels, n_q, d_q, d_mean, d_nv, h->compute);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(rvll::peak_kernel, dim3(row_blocks), dim3(rvll::kGlsThreads), 0, h->compute, d_P, R, F, d_pi, d_pp);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev[3], h->compute);
        auto down = [&](void* dst, const void* src, size_t bytes) {
            if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->compute);
        };
        down(q + g0 * n_q * F, d_q, sizeof(double) * (size_t)(gb * n_q * F));
        down(mean + g0 * F, d_mean, sizeof(double) * (size_t)(gb * F));
        down(n_valid + g0 * F, d_nv, sizeof(int32_t) * (size_t)(gb * F));
        down(peak_index + g0 * n, d_pi, sizeof(int32_t) * (size_t)R);
        down(peak_power + g0 * n, d_pp, sizeof(double) * (size_t)R);
        if (power_out) down(power_out + g0 * n * F, d_P, sizeof(double) * (size_t)(R * F));
        if (e == hipSuccess) e = hipStreamSynchronize(h->compute);
        float ms = 0.f;
        for (int k = 0; k < 3; ++k)
            if (e == hipSuccess && phase_ms && (e = hipEventElapsedTime(&ms, ev[k], ev[k + 1])) == hipSuccess) phase_ms[k] += ms;
    }
    if (status == RVLL_OK && e != hipSuccess)
        status = report_error(e == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, "gls_bands: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->compute);
    for (auto& x : ev)
        if (x) (void)hipEventDestroy(x);
    dev_free(d_levels); dev_free(d_wr); dev_free(d_w); dev_free(d_W); dev_free(d_Y); dev_free(d_YY); dev_free(d_P); dev_free(d_q); dev_free(d_mean);
    dev_free(d_nv); dev_free(d_pi); dev_free(d_pp);
    return status;
}

}  // extern "C"
