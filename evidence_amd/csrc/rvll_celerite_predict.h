// rvll_celerite_predict.h — the conditional mean and variance of a celerite GP given one row of residuals, host+device
// (DESIGN §4t).  The factor of Sigma = L D L^T is rvll_celerite.h's: L[m][n] = U_m^T P_m .. P_(n+1) W_n for m > n, with P_n the
// propagator over the gap before epoch n, in the basis cel_prepare left the row in.  evidence_amd/correlated.py holds the numpy
// definition (predict_dense) and these sweeps in numpy (predict_recursive); rvll_celerite_predict.hip runs this source on the
// GPU, one row a lane.
//
//   cel_gap         U and V of a time and P over a gap as three diagonals (al, up, dn): the first loop of cel_advance_pair, which
//                   on a row without a prepared pair gives cel_advance's values (up = dn = 0)
//   cel_back_step   one epoch of the backward sweep, from the last epoch to the first, g = 0 and M = 0 at the start:
//                   alpha_n = z_n / D_n - W_n . g (alpha = Sigma^-1 r), m = M W_n, Z_nn = 1 / D_n + W_n . m (the diagonal of
//                   Sigma^-1), G_n = g + U_n alpha_n, g <- P_n^T G_n, M <- P_n^T (M + Z_nn U U^T - U m^T - m U^T) P_n
//   cel_query_back  a query x in [t_(n-1), t_n): the later epochs' share of the mean, V(x) . P(t_n - x)^T G_n
//   cel_fwd_step    F_n = P_n F_(n-1) + V_n alpha_n
//   cel_query_fwd   a query x in [t_n, t_(n+1)): the earlier epochs' share of the mean, U(x) . P(x - t_n) F_n
//   cel_var_step    one epoch of w = L^-1 k(x), the forward substitution cel_step does for z, with k(x)_n = cel_kernel_value at
//                   |x - t_n| in the row's basis (a prepared pair's plain columns cancel); var(x) = sum a - sum w_n² / D_n
// At the data epochs mean_n = r_n - var_n alpha_n and var_n - var_n² Z_nn.  -ffp-contract=off holds: every fused multiply-add
// is an explicit __builtin_fma.
#pragma once
#include "rvll_celerite.h"

namespace rvll {

template <int J>
struct CelGap { double al[J], up[J], dn[J]; };          // row j of P X = al_j X_j + up_j X_(j+1) + dn_j X_(j-1)

// A copy of the first loop of cel_advance_pair, not a call: a shared helper would change the code of the log-L kernel, whose
// results and time this header must leave alone.  Whatever changes U, V or P there changes here.
template <int J>
RVLL_HD void cel_gap(const CelColumn (&col)[J], double t, double dt, CelGap<J>& P, double (&U)[J], double (&V)[J])
{
    double sn = 0.0, cs = 1.0, m21 = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int form = col[j].form;
        P.up[j] = P.dn[j] = 0.0;
        if (form == kCelColSin) {
            P.al[j] = j > 0 ? P.al[j - 1] : 1.0;
            U[j] = __builtin_fma(col[j].a, sn, -(col[j].b * cs));
            V[j] = sn;
        } else if (form == kCelColPairB) {
            P.al[j] = j > 0 ? P.al[j - 1] : 1.0;
            P.dn[j] = m21;
            U[j] = col[j].a;
            V[j] = 0.0;
        } else if (form == kCelColPairA) {
            cel_pair_propagator(col[j], dt, P.al[j], m21);
            P.up[j] = col[j].b * m21;
            U[j] = col[j].a;
            V[j] = 1.0;
        } else {
            P.al[j] = exp(-(col[j].c * dt));
            if (form == kCelColCos) {
                sincos_f64(col[j].d * t, sn, cs);
                U[j] = __builtin_fma(col[j].a, cs, col[j].b * sn);
                V[j] = cs;
            } else {
                U[j] = col[j].a;
                V[j] = 1.0;
            }
        }
    }
}

// y = P x and y = P^T x (y is not x)
template <int J>
RVLL_HD void cel_apply(const CelGap<J>& P, const double (&x)[J], double (&y)[J])
{
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double s = P.al[j] * x[j];
        if (j + 1 < J) s = __builtin_fma(P.up[j], x[j + 1], s);
        if (j > 0) s = __builtin_fma(P.dn[j], x[j - 1], s);
        y[j] = s;
    }
}

template <int J>
RVLL_HD void cel_apply_t(const CelGap<J>& P, const double (&x)[J], double (&y)[J])
{
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double s = P.al[j] * x[j];
        if (j > 0) s = __builtin_fma(P.up[j - 1], x[j - 1], s);
        if (j + 1 < J) s = __builtin_fma(P.dn[j + 1], x[j + 1], s);
        y[j] = s;
    }
}

template <int J>
struct CelBack {
    double g[J];
    double M[J * (J + 1) / 2];             // upper triangle, row by row
};

template <int J>
RVLL_HD void cel_back_init(CelBack<J>& st)
{
#pragma unroll
    for (int j = 0; j < J; ++j) st.g[j] = 0.0;
#pragma unroll
    for (int i = 0; i < J * (J + 1) / 2; ++i) st.M[i] = 0.0;
}

// Epoch n with its W, D, z from the factor and its U and P (over the gap before it): alpha_n, Z_nn and G_n, and the state carried
// to epoch n - 1.
template <int J>
RVLL_HD void cel_back_step(CelBack<J>& st, const CelGap<J>& P, const double (&U)[J], const double (&W)[J], double D, double z,
                           double& alpha, double& znn, double (&G)[J])
{
    double m[J];
    double wg = 0.0, wm = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < J; ++k) s = __builtin_fma(st.M[j <= k ? cel_tri<J>(j, k) : cel_tri<J>(k, j)], W[k], s);
        m[j] = s;
        wg = __builtin_fma(W[j], st.g[j], wg);
    }
#pragma unroll
    for (int j = 0; j < J; ++j) wm = __builtin_fma(W[j], m[j], wm);
    alpha = z / D - wg;
    znn = 1.0 / D + wm;
#pragma unroll
    for (int j = 0; j < J; ++j) G[j] = __builtin_fma(U[j], alpha, st.g[j]);
    cel_apply_t<J>(P, G, st.g);
    double X[J * (J + 1) / 2], R[J][J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const double zu = znn * U[j];
#pragma unroll
        for (int k = j; k < J; ++k)
            X[cel_tri<J>(j, k)] = st.M[cel_tri<J>(j, k)] + ((__builtin_fma(zu, U[k], -(U[j] * m[k]))) - m[j] * U[k]);
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {                                    // R = P^T X
#pragma unroll
        for (int k = 0; k < J; ++k) {
            double x = P.al[j] * X[j <= k ? cel_tri<J>(j, k) : cel_tri<J>(k, j)];
            if (j > 0) x = __builtin_fma(P.up[j - 1], X[j - 1 <= k ? cel_tri<J>(j - 1, k) : cel_tri<J>(k, j - 1)], x);
            if (j + 1 < J) x = __builtin_fma(P.dn[j + 1], X[j + 1 <= k ? cel_tri<J>(j + 1, k) : cel_tri<J>(k, j + 1)], x);
            R[j][k] = x;
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {                                    // M = R P
#pragma unroll
        for (int k = j; k < J; ++k) {
            double x = R[j][k] * P.al[k];
            if (k > 0) x = __builtin_fma(R[j][k - 1], P.up[k - 1], x);
            if (k + 1 < J) x = __builtin_fma(R[j][k + 1], P.dn[k + 1], x);
            st.M[cel_tri<J>(j, k)] = x;
        }
    }
}

// x (from the first epoch) lies dtb before the epoch whose G this is.
template <int J>
RVLL_HD double cel_query_back(const CelColumn (&col)[J], double x, double dtb, const double (&G)[J])
{
    CelGap<J> P;
    double U[J], V[J], y[J];
    cel_gap<J>(col, x, dtb, P, U, V);
    cel_apply_t<J>(P, G, y);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) s = __builtin_fma(V[j], y[j], s);
    return s;
}

template <int J>
RVLL_HD void cel_fwd_step(double (&F)[J], const CelGap<J>& P, const double (&V)[J], double alpha)
{
    double y[J];
    cel_apply<J>(P, F, y);
#pragma unroll
    for (int j = 0; j < J; ++j) F[j] = __builtin_fma(V[j], alpha, y[j]);
}

// x lies dtf after the epoch whose F this is.
template <int J>
RVLL_HD double cel_query_fwd(const CelColumn (&col)[J], double x, double dtf, const double (&F)[J])
{
    CelGap<J> P;
    double U[J], V[J], y[J];
    cel_gap<J>(col, x, dtf, P, U, V);
    cel_apply<J>(P, F, y);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) s = __builtin_fma(U[j], y[j], s);
    return s;
}

// k(x) at a lag x >= 0 from the columns as cel_prepare left them: u1 phi1(x) + u2 phi2(x) for a prepared pair.
template <int J>
RVLL_HD double cel_kernel_value(const CelColumn (&col)[J], double x)
{
    double k = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int form = col[j].form;
        if (form == kCelColReal) {
            k = __builtin_fma(col[j].a, exp(-(col[j].c * x)), k);
        } else if (form == kCelColCos) {
            double sn, cs;
            sincos_f64(col[j].d * x, sn, cs);
            k = __builtin_fma(exp(-(col[j].c * x)), __builtin_fma(col[j].a, cs, col[j].b * sn), k);
        } else if (form == kCelColPairA) {
            double m11, m21;
            cel_pair_propagator(col[j], x, m11, m21);
            k += __builtin_fma(col[j].a, m11, col[j + 1 < J ? j + 1 : j].a * m21);
        }
    }
    return k;
}

template <int J>
struct CelVar {
    double f[J];                           // f as in CelState
    double w, acc;                         // w of the previous epoch, the sum of w² / D
};

template <int J>
RVLL_HD void cel_var_init(CelVar<J>& st)
{
#pragma unroll
    for (int j = 0; j < J; ++j) st.f[j] = 0.0;
    st.w = st.acc = 0.0;
}

// Epoch n with its U, P and D, the W of epoch n - 1 (0 at the first) and kn = k(|x - t_n|).
template <int J>
RVLL_HD void cel_var_step(CelVar<J>& st, const CelGap<J>& P, const double (&U)[J], const double (&Wprev)[J], double D, double kn)
{
    double y[J];
#pragma unroll
    for (int j = 0; j < J; ++j) y[j] = __builtin_fma(Wprev[j], st.w, st.f[j]);
    cel_apply<J>(P, y, st.f);
    double uf = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) uf = __builtin_fma(U[j], st.f[j], uf);
    st.w = kn - uf;
    st.acc += st.w * st.w / D;
}

}  // namespace rvll
