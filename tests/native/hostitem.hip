// hostitem.hip — the one-division log-L item (rvll_math.h: ItemPool, pool_add, pool_chi2) compiled for the CPU: the pooled
// routine by itself, and a whole log-L through it with the solver as eval_item (rvll_tile.h) runs it.
// Test infrastructure; built on demand by tests/test_item_pool_host.py (needs hipcc, no GPU).
#include "rvll_math.h"
#define HI extern "C" __attribute__((visibility("default")))

// out[i] = pool_chi2 of row i's np quotients num[i, p] / den[i, p] joined in planet order; ND[2 i], ND[2 i + 1] = the pool (N, D)
HI void hi_pool(const double* num, const double* den, long n, int np, const double* R, const double* var, double* out, double* ND) {
    for (long i = 0; i < n; ++i) {
        rvll::ItemPool p{0., 1.};
        for (int k = 0; k < np; ++k) rvll::pool_add(p, k == 0, num[i * np + k], den[i * np + k]);
        out[i] = rvll::pool_chi2(p, R[i], var[i]);
        ND[2 * i] = p.N;
        ND[2 * i + 1] = p.D;
    } }
// the arithmetic before the pool: the separately corrected quotients, their sum in planet order from 0, the residual, one more
HI void hi_separate(const double* num, const double* den, long n, int np, const double* R, const double* var, double* out) {
    for (long i = 0; i < n; ++i) {
        double ksum = 0.;
        for (int k = 0; k < np; ++k) ksum += rvll::div_fast(num[i * np + k], den[i * np + k]);
        const double res = np > 0 ? R[i] - ksum : R[i];
        out[i] = rvll::div_fast(res * res, 2 * var[i]);
    } }

// log-L of n points of a model of np planets in the plain parametrisation (K, period, e, omega, mean anomaly at `epoch`) and ni
// instruments (offset, jitter^2), no drift, no linear terms; planet parameters [n, np], instrument parameters [n, ni], the epoch
// table t, y, s2 = sigma^2, inst [ne].  The decode step, the solver (start E = M, newton_next_sincos below kSafeSteps, the long
// reduction from there on, stop |dE| <= tol, a planet that reaches itmax keeps nu = 0 from that epoch on) and the item as the
// kernels have them; the normalisation as a plain sum of logarithms and the contributions added in epoch order (the kernels' own
// orders differ from these by a few 2^-53 of the sums).
HI void hi_loglike(const double* K, const double* Pd, const double* ecc, const double* omega, const double* ma0, const double* epoch,
                   const double* offset, const double* jit2, long n, int np, int ni, const double* t, const double* y,
                   const double* s2, const int* inst, int ne, double tol, int itmax, double cte, double* logl) {
    const rvll::SincosConsts kc = rvll::sincos_consts();
    const double two_pi = 6.283185307179586476925286766559;
    double* pp = new double[(size_t)(np > 0 ? np : 1) * 8];
    int* jfail = new int[np > 0 ? np : 1];
    for (long i = 0; i < n; ++i) {
        double sumc0 = 0.;
        for (int k = 0; k < np; ++k) {
            const long q_ = i * np + k;
            const double e = ecc[q_], ec = e > 0.99 ? 0.99 : e;
            double so, co;
            rvll::sincos_any(omega[q_], so, co);
            const double q = __builtin_sqrt((1. - ec) * (1. + ec));
            double* P = pp + k * 8;
            P[0] = two_pi / Pd[q_];  P[1] = epoch[q_];  P[2] = ma0[q_];  P[3] = ec;
            P[4] = K[q_] * co;       P[5] = K[q_] * q * so;
            P[6] = K[q_] * (e * co);
            sumc0 = k == 0 ? P[6] : sumc0 + P[6];
            jfail[k] = 0x7fffffff;
        }
        double acc = 0., logdet = 0.;
        for (int j = 0; j < ne; ++j) {
            const double var = s2[j] + jit2[i * ni + inst[j]];
            double cterm = 0. + offset[i * ni + inst[j]];
            if (np > 0) cterm = cterm + sumc0;
            rvll::ItemPool pool{0., 1.};
            for (int k = 0; k < np; ++k) {
                const double* P = pp + k * 8;
                const double ec = P[3];
                double num = P[4], den = 1.0;                       // nu = 0
                if (j < jfail[k]) {
                    const double M = P[0] * (t[j] - P[1]) + P[2];
                    double E = M, s, c, dE = __builtin_inf();
                    int steps = 0;
                    do {
                        if (steps < rvll::kSafeSteps) rvll::newton_next_sincos<true>(E, dE, steps, s, c, kc);
                        else                          rvll::sincos_any(E, s, c, kc);
                        const double f  = E - ec * s - M;
                        const double fp = 1 - ec * c;
                        const double En = E - rvll::div_exact(f, fp);
                        dE = En - E;
                        E = En;
                        ++steps;
                    } while (__builtin_fabs(dE) > tol && steps < itmax);
                    if (steps >= itmax) {
                        jfail[k] = j;
                    } else {
                        if (tol <= 1e-3) rvll::rotate_small(dE, s, c);
                        else             rvll::sincos_any(E, s, c, kc);
                        den = __builtin_fma(-ec, c, 1.0);
                        num = __builtin_fma(P[4], c - ec, -(P[5] * s));
                    }
                }
                rvll::pool_add(pool, k == 0, num, den);
            }
            acc += rvll::pool_chi2(pool, y[j] - cterm, var);
            logdet += 0.5 * __builtin_log(var);
        }
        logl[i] = cte - (logdet + acc);
    }
    delete[] pp;
    delete[] jfail;
}
