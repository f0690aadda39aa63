// rvll_celerite.h — the log-likelihood of one row of residuals under a celerite covariance, host+device.
//
// Sigma = diag(var) + K, K[n][m] = sum over columns of exp(-c x)(a cos d x + b sin d x) at x = |t_n - t_m| (Foreman-Mackey et
// al. 2017).  evidence_amd/correlated.py holds the numpy definition (log_likelihood_dense) and the same recursion in numpy
// (log_likelihood_recursive); the kernel of rvll_celerite.hip runs this source on the GPU, one row a lane.
//
//   cel_column    one column (a, b, c, d) of a term from its parameters, and how it enters the recursion: a real column
//                 (U = a, V = 1), or the cosine or sine half of a complex term (U = (a cos dt + b sin dt, a sin dt - b cos dt),
//                 V = (cos dt, sin dt)).  An SHO with q >= 1/2 is one complex term, below 1/2 two real columns; |q - 1/2| is
//                 taken as at least kCelQClamp on the side q lies on.
//   CelState<J>   what a row carries from epoch to epoch: the upper triangle of S, f, W, D, z and the two sums.  J is a template
//                 argument and every loop over columns has constant bounds, so the state stays in registers.
//   cel_step      one epoch: S <- P P^T o (S + D W W^T), f <- P o (f + W z) with P = exp(-c dt) of the gap to the previous epoch,
//                 D = A - U S U^T, W = (V - S U) / D, z = r - U f, and the sums of z^2 / D and ln D.  Before the first epoch S,
//                 f, W, D and z are 0 and its gap is 0, so the first epoch takes the same code.
//   cel_result    log-L = -1/2 sum z^2 / D - 1/2 sum ln D - Ne / 2 ln(2 pi), or -1e30 and a flag.
// The times are measured from the first epoch in time order, and both they and the gaps come from a per-epoch table the host
// builds (rvll_celerite.hip): the kernel takes one sincos per epoch and complex term and one exponential per epoch and distinct c.
// -ffp-contract=off holds: every fused multiply-add is an explicit __builtin_fma.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "rvll.h"
#include "rvll_math.h"

namespace rvll {

constexpr double kCelTwoPi = 6.283185307179586476925286766559;    // fl(2 pi), as 2 * np.pi
constexpr double kCelQClamp = 1.0e-6;
constexpr double kCelInvalid = -1.0e30;                            // the reference's sentinel (rvmodel:203)
enum { kCelColReal = 0, kCelColCos = 1, kCelColSin = 2 };

struct CelColumn { double a, b, c, d; int form; };                // form: kCelCol*

// Column `sub` of an SHO at w0 with quality q and variance amp = S0 w0 q (its k(0)).  q >= 1/2: the two halves of one complex
// term; q < 1/2: two real columns (sub 0 the slowly, sub 1 the fast decaying one).
RVLL_HD CelColumn cel_sho_column(double amp, double w0, double q, int sub)
{
    CelColumn k;
    if (q >= 0.5) {
        const double qc = q - 0.5 < kCelQClamp ? 0.5 + kCelQClamp : q;
        const double f = sqrt((2.0 * qc - 1.0) * (2.0 * qc + 1.0));          // sqrt(4 q^2 - 1) without the cancellation
        k.a = amp;
        k.b = k.a / f;
        k.c = w0 / (2.0 * qc);
        k.d = k.c * f;
        k.form = sub == 0 ? kCelColCos : kCelColSin;
    } else {
        const double qc = 0.5 - q < kCelQClamp ? 0.5 - kCelQClamp : q;
        const double f = sqrt((1.0 - 2.0 * qc) * (1.0 + 2.0 * qc));          // sqrt(1 - 4 q^2)
        const double h = 0.5 * amp, g = w0 / (2.0 * qc);
        k.a = sub == 0 ? h * (1.0 + 1.0 / f) : h * (1.0 - 1.0 / f);
        k.c = sub == 0 ? g * (1.0 - f) : g * (1.0 + f);
        k.b = 0.0;
        k.d = 0.0;
        k.form = kCelColReal;
    }
    return k;
}

// Column `sub` of a term of `kind` with parameters p (include/rvll.h lists them).  false: the parameters are not valid.
RVLL_HD bool cel_column(int kind, int sub, const double* p, CelColumn& k)
{
    k.a = k.b = k.c = k.d = 0.0;
    k.form = kCelColReal;
    if (kind == RVLL_NOISE_REAL) {
        const double sigma = p[0], tau = p[1];
        if (!(sigma >= 0.0 && sigma < INFINITY && tau > 0.0 && tau < INFINITY)) return false;
        k.a = sigma * sigma;
        k.c = 1.0 / tau;
        return true;
    }
    if (kind == RVLL_NOISE_SHO) {
        const double sigma = p[0], rho = p[1], q = p[2];
        if (!(sigma >= 0.0 && sigma < INFINITY && rho > 0.0 && rho < INFINITY && q > 0.0 && q < INFINITY)) return false;
        const double w0 = kCelTwoPi / rho;
        k = cel_sho_column(sigma * sigma, w0, q, sub);             // S0 w0 q = sigma^2
        return true;
    }
    // RVLL_NOISE_ROTATION: columns 0, 1 the oscillator at prot, columns 2, 3 the one at prot / 2
    const double sigma = p[0], prot = p[1], q0 = p[2], dq = p[3], mix = p[4];
    if (!(sigma >= 0.0 && sigma < INFINITY && prot > 0.0 && prot < INFINITY && q0 + 0.5 > 0.0 && q0 < INFINITY && dq > 0.0 &&
          dq < INFINITY && mix >= 0.0 && mix < INFINITY))
        return false;
    const double amp = sigma * sigma / (1.0 + mix);
    const bool second = sub >= 2;
    const double q = second ? 0.5 + q0 : 0.5 + q0 + dq;
    const double root = sqrt((2.0 * q - 1.0) * (2.0 * q + 1.0));             // NaN below 1/2: the pivots then refuse the row
    const double w = (second ? 2.0 : 1.0) * (2.0 * kCelTwoPi) * q / (prot * root);
    k = cel_sho_column(second ? mix * amp : amp, w, q, sub & 1);            // S w q of either oscillator
    return true;
}

template <int J>
struct CelState {
    double S[J * (J + 1) / 2];            // upper triangle, row by row
    double f[J], W[J];
    double D, z, chi, lndet;
    int bad;                               // 1: a residual was NaN (an invalid orbit); 2: a pivot was not > 0
};

template <int J>
RVLL_HD constexpr int cel_tri(int j, int k) { return j * J - j * (j - 1) / 2 + (k - j); }      // j <= k

template <int J>
RVLL_HD void cel_init(CelState<J>& st)
{
#pragma unroll
    for (int i = 0; i < J * (J + 1) / 2; ++i) st.S[i] = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) st.f[j] = st.W[j] = 0.0;
    st.D = st.z = st.chi = st.lndet = 0.0;
    st.bad = 0;
}

// One epoch at time t (from the first epoch), dt after the previous one (0 at the first), with residual r and variance var;
// A = var + sum of the columns' a.
template <int J>
RVLL_HD void cel_step(const CelColumn (&col)[J], double suma, CelState<J>& st, double t, double dt, double r, double var)
{
    double P[J], U[J], V[J];
    double sn = 0.0, cs = 1.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        if (col[j].form == kCelColSin) {                 // the sine half shares the cosine half's c and d
            P[j] = j > 0 ? P[j - 1] : 1.0;
            U[j] = __builtin_fma(col[j].a, sn, -(col[j].b * cs));
            V[j] = sn;
        } else {
            P[j] = exp(-(col[j].c * dt));
            if (col[j].form == kCelColCos) {
                sincos_f64(col[j].d * t, sn, cs);
                U[j] = __builtin_fma(col[j].a, cs, col[j].b * sn);
                V[j] = cs;
            } else {
                U[j] = col[j].a;
                V[j] = 1.0;
            }
        }
    }
    // S <- P P^T o (S + D W W^T), f <- P o (f + W z)
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const double dw = st.D * st.W[j];
#pragma unroll
        for (int k = j; k < J; ++k)
            st.S[cel_tri<J>(j, k)] = (P[j] * P[k]) * __builtin_fma(dw, st.W[k], st.S[cel_tri<J>(j, k)]);
        st.f[j] = P[j] * __builtin_fma(st.W[j], st.z, st.f[j]);
    }
    // D = A - U S U^T, W = (V - S U) / D, z = r - U f
    double SU[J];
    double usu = 0.0, uf = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < J; ++k) s = __builtin_fma(st.S[j <= k ? cel_tri<J>(j, k) : cel_tri<J>(k, j)], U[k], s);
        SU[j] = s;
        usu = __builtin_fma(U[j], s, usu);
        uf = __builtin_fma(U[j], st.f[j], uf);
    }
    const double D = (var + suma) - usu;
    const double z = r - uf;
#pragma unroll
    for (int j = 0; j < J; ++j) st.W[j] = (V[j] - SU[j]) / D;
    st.D = D;
    st.z = z;
    st.chi += z * z / D;
    st.lndet += log(D);
    if (r != r) st.bad |= 1;
    if (!(D > 0.0)) st.bad |= 2;
}

// cte = -Ne / 2 ln(2 pi).  valid: every column's parameters were.
template <int J>
RVLL_HD void cel_result(const CelState<J>& st, bool valid, double cte, double& logl, int32_t& flag)
{
    if (st.bad & 1) {
        logl = kCelInvalid;
        flag = RVLL_FLAG_INVALID_ORBIT;
    } else if (!valid || (st.bad & 2)) {
        logl = kCelInvalid;
        flag = RVLL_FLAG_NOISE_INVALID;
    } else {
        logl = (-0.5 * st.chi - 0.5 * st.lndet) + cte;
        flag = 0;
    }
}

}  // namespace rvll
