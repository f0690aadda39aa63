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
//   cel_prepare   a near-degenerate SHO pair (|q - 1/2| < 0.01) is rewritten into a sum / difference basis whose block of P is
//                 2 x 2 and whose U and V are constant; cel_step then carries S and f over the gap with a tridiagonal P
//                 (cel_advance_pair) where the row has such a pair, and with the diagonal P above (cel_advance) where not.
//   CelPlan       where a kernel finds a row's term parameters in theta; cel_plan_columns makes the row's prepared columns from it
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
constexpr double kCelPairF = 0.2;                                   // an SHO pair with f = sqrt|4 q^2 - 1| below this changes basis
enum { kCelColReal = 0, kCelColCos = 1, kCelColSin = 2, kCelColPairA = 3, kCelColPairB = 4 };

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

// The near-degenerate pairs.  Near q = 1/2 the two columns of an SHO hold a = +-amp / (2 f) (below 1/2) or a and b = a / f
// (above), f = sqrt|4 q^2 - 1|, and U S U^T subtracts terms 1 / f^2 times what it leaves: at the clamp float64 loses
// (sigma / svrad)^2 2e-12 of log-L.  A pair with f < kCelPairF is therefore carried in the basis
//     phi1(x) = exp(-g x) cosh w x, phi2(x) = exp(-g x) sinh(w x) / w       (below: g = (c0 + c1) / 2, w = (c1 - c0) / 2)
//     phi1(x) = exp(-g x) cos w x,  phi2(x) = exp(-g x) sin(w x) / w        (above: g = c, w = d)
// in which k(x) = u1 phi1 + u2 phi2 with u1 = a0 + a1 or a and u2 = (a0 - a1) w or b d, both of the order of amp (the two
// differences are exact or harmless: the columns are the definition's, rounding included), U = (u1, u2) and V = (1, 0) are
// constant, and the pair's block of P is [[m11, s w^2 m21], [m21, m11]] with m11 = phi1(dt), m21 = phi2(dt), s = +-1.
// cel_prepare rewrites such a pair in place: a = u1 | u2, b = s w^2, c = g, d = w, form = kCelColPairA | kCelColPairB.  It keys on
// the columns alone: the second column of an SHO below 1/2 is the only real column with a < 0.  true: the row has such a pair.
template <int J>
RVLL_HD bool cel_prepare(CelColumn (&col)[J])
{
    bool any = false;
#pragma unroll
    for (int j = 0; j + 1 < J; ++j) {
        CelColumn &p = col[j], &q = col[j + 1];
        if (p.form == kCelColReal && q.form == kCelColReal && q.a < 0.0 && q.c - p.c < kCelPairF * (q.c + p.c)) {
            const double w = 0.5 * (q.c - p.c), g = 0.5 * (q.c + p.c), u1 = p.a + q.a, u2 = (p.a - q.a) * w;
            p.a = u1;
            q.a = u2;
            p.b = q.b = w * w;
            p.c = q.c = g;
            p.d = q.d = w;
            p.form = kCelColPairA;
            q.form = kCelColPairB;
            any = true;
        } else if (p.form == kCelColCos && q.form == kCelColSin && p.d < kCelPairF * p.c) {
            q.a = p.b * p.d;
            p.b = q.b = -(p.d * p.d);
            p.form = kCelColPairA;
            q.form = kCelColPairB;
            any = true;
        }
    }
    return any;
}

// Per column its term's kind and parameters, and which of the term's columns it is: how a kernel finds a row's columns in theta.
struct CelPlan {
    int32_t kind[RVLL_NOISE_MAX_RANK], sub[RVLL_NOISE_MAX_RANK];
    rvll_slot par[RVLL_NOISE_MAX_RANK][5];
};

// The workspace the prediction's sweeps share (rvll_celerite_predict.hip): [epoch in time order][field][row of the chunk], an
// epoch's fields W_0 .. W_(J-1) and then these.  The factor sweep leaves W, D, z, r and var; the backward sweep puts alpha where z
// was, the variance at the epoch where var was, and the mean at the epoch.
enum { kCelWsD = 0, kCelWsZ = 1, kCelWsR = 2, kCelWsVar = 3, kCelWsMean = 4, kCelWsExtra = 5 };

// A row's columns from its theta, prepared: suma the sum of the columns' a (a complex term's counts once), pair what cel_prepare
// returned.  false: a term's parameters are not valid.
template <int J>
RVLL_HD bool cel_plan_columns(const CelPlan& plan, const double* th, CelColumn (&col)[J], double& suma, bool& pair)
{
    bool valid = true;
    suma = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        double p[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const rvll_slot s = plan.par[j][q];
            p[q] = s.idx >= 0 ? th[s.idx] : s.val;
        }
        valid &= cel_column(plan.kind[j], plan.sub[j], p, col[j]);
        if (col[j].form != kCelColSin) suma += col[j].a;
    }
    pair = cel_prepare<J>(col);
    return valid;
}

// m11 = phi1(dt) and m21 = phi2(dt) of a prepared pair.  sinh y / y comes from its series below y = 1/2, where
// (exp(y) - exp(-y)) / 2 cancels, and from the two exponentials of the columns above it, where exp(-g dt) cosh(y) would be 0 inf.
RVLL_HD void cel_pair_propagator(const CelColumn& k, double dt, double& m11, double& m21)
{
    const double w = k.d, y = w * dt;
    if (k.b < 0.0) {
        const double E = exp(-(k.c * dt));
        double sn, cs;
        sincos_f64(y, sn, cs);
        m11 = E * cs;
        m21 = E * sn / w;
    } else if (y < 0.5) {
        const double E = exp(-(k.c * dt)), y2 = y * y;
        double ch = 1.0 / 87178291200.0, sh = 1.0 / 1307674368000.0;             // 1 / 14!, 1 / 15!: the next terms are < 1e-18
        ch = __builtin_fma(ch, y2, 1.0 / 479001600.0);  sh = __builtin_fma(sh, y2, 1.0 / 6227020800.0);
        ch = __builtin_fma(ch, y2, 1.0 / 3628800.0);    sh = __builtin_fma(sh, y2, 1.0 / 39916800.0);
        ch = __builtin_fma(ch, y2, 1.0 / 40320.0);      sh = __builtin_fma(sh, y2, 1.0 / 362880.0);
        ch = __builtin_fma(ch, y2, 1.0 / 720.0);        sh = __builtin_fma(sh, y2, 1.0 / 5040.0);
        ch = __builtin_fma(ch, y2, 1.0 / 24.0);         sh = __builtin_fma(sh, y2, 1.0 / 120.0);
        ch = __builtin_fma(ch, y2, 0.5);                sh = __builtin_fma(sh, y2, 1.0 / 6.0);
        ch = __builtin_fma(ch, y2, 1.0);                sh = __builtin_fma(sh, y2, 1.0);
        m11 = E * ch;
        m21 = E * (dt * sh);
    } else {
        const double p0 = exp(-((k.c - w) * dt)), p1 = exp(-((k.c + w) * dt));
        m11 = 0.5 * (p0 + p1);
        m21 = 0.5 * (p0 - p1) / w;
    }
}

// U and V of an epoch at time t (from the first epoch), dt after the previous one, and the state carried over the gap:
// S <- P P^T o (S + D W W^T), f <- P o (f + W z).
// cel_gap of rvll_celerite_predict.h computes the same U, V and P for the prediction's sweeps, which run on the W this factor
// leaves: a change to U, V or P here or in cel_advance_pair goes there too (tests/test_predict_host.py holds the two together).
template <int J>
RVLL_HD void cel_advance(const CelColumn (&col)[J], CelState<J>& st, double t, double dt, double (&U)[J], double (&V)[J])
{
    double P[J];
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
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const double dw = st.D * st.W[j];
#pragma unroll
        for (int k = j; k < J; ++k)
            st.S[cel_tri<J>(j, k)] = (P[j] * P[k]) * __builtin_fma(dw, st.W[k], st.S[cel_tri<J>(j, k)]);
        st.f[j] = P[j] * __builtin_fma(st.W[j], st.z, st.f[j]);
    }
}

// The same for a row with a prepared pair: P is tridiagonal, row j of P X = al_j X_j + up_j X_(j+1) + dn_j X_(j-1) with up and dn
// 0 outside a pair's block, so every index is a constant and S <- P (S + D W W^T) P^T, f <- P (f + W z) stay in registers.
// The first loop below is copied in cel_gap of rvll_celerite_predict.h (see cel_advance): keep the two the same.
template <int J>
RVLL_HD void cel_advance_pair(const CelColumn (&col)[J], CelState<J>& st, double t, double dt, double (&U)[J], double (&V)[J])
{
    double al[J], up[J], dn[J];
    double sn = 0.0, cs = 1.0, m21 = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int form = col[j].form;
        up[j] = dn[j] = 0.0;
        if (form == kCelColSin) {
            al[j] = j > 0 ? al[j - 1] : 1.0;
            U[j] = __builtin_fma(col[j].a, sn, -(col[j].b * cs));
            V[j] = sn;
        } else if (form == kCelColPairB) {
            al[j] = j > 0 ? al[j - 1] : 1.0;
            dn[j] = m21;
            U[j] = col[j].a;
            V[j] = 0.0;
        } else if (form == kCelColPairA) {
            cel_pair_propagator(col[j], dt, al[j], m21);
            up[j] = col[j].b * m21;
            U[j] = col[j].a;
            V[j] = 1.0;
        } else {
            al[j] = exp(-(col[j].c * dt));
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
    double T[J * (J + 1) / 2], R[J][J], g[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const double dw = st.D * st.W[j];
#pragma unroll
        for (int k = j; k < J; ++k) T[cel_tri<J>(j, k)] = __builtin_fma(dw, st.W[k], st.S[cel_tri<J>(j, k)]);
        g[j] = __builtin_fma(st.W[j], st.z, st.f[j]);
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int k = 0; k < J; ++k) {
            double x = al[j] * T[j <= k ? cel_tri<J>(j, k) : cel_tri<J>(k, j)];
            if (j + 1 < J) x = __builtin_fma(up[j], T[j + 1 <= k ? cel_tri<J>(j + 1, k) : cel_tri<J>(k, j + 1)], x);
            if (j > 0) x = __builtin_fma(dn[j], T[j - 1 <= k ? cel_tri<J>(j - 1, k) : cel_tri<J>(k, j - 1)], x);
            R[j][k] = x;
        }
        double y = al[j] * g[j];
        if (j + 1 < J) y = __builtin_fma(up[j], g[j + 1], y);
        if (j > 0) y = __builtin_fma(dn[j], g[j - 1], y);
        st.f[j] = y;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int k = j; k < J; ++k) {
            double x = al[k] * R[j][k];
            if (k + 1 < J) x = __builtin_fma(up[k], R[j][k + 1], x);
            if (k > 0) x = __builtin_fma(dn[k], R[j][k - 1], x);
            st.S[cel_tri<J>(j, k)] = x;
        }
    }
}

// One epoch at time t (from the first epoch), dt after the previous one (0 at the first), with residual r and variance var;
// A = var + sum of the columns' a (taken before cel_prepare); pair: what cel_prepare returned for the row.
template <int J>
RVLL_HD void cel_step(const CelColumn (&col)[J], double suma, bool pair, CelState<J>& st, double t, double dt, double r, double var)
{
    double U[J], V[J];
    if (J >= 2 && pair)
        cel_advance_pair<J>(col, st, t, dt, U, V);
    else
        cel_advance<J>(col, st, t, dt, U, V);
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

// The same for columns as cel_column left them, without cel_prepare: every row on the diagonal path.
template <int J>
RVLL_HD void cel_step(const CelColumn (&col)[J], double suma, CelState<J>& st, double t, double dt, double r, double var)
{
    cel_step<J>(col, suma, false, st, t, dt, r, var);
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
