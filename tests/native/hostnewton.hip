// hostnewton.hip — the Newton step's residuals (rvll_math.h: newton_residuals) and the solve built on them, compiled for the CPU.
// Test infrastructure; built on demand by tests/newton_cases.py (needs hipcc, no GPU).
#include <cmath>
#include "rvll_math.h"
#define HN extern "C" __attribute__((visibility("default")))
// the pair the solver holds at E: sincos_f64
HN void hn_pair(const double* E, long n, double* s, double* c) {
    for (long i = 0; i < n; ++i) rvll::sincos_f64(E[i], s[i], c[i]);
}
// form 1: newton_residuals; form 0: the reference's separately rounded operations (trueanomaly.c:25-26)
HN void hn_residuals(const double* E, const double* s, const double* c, const double* ecc, const double* M, long n, int form,
                     double* f, double* fp) {
    for (long i = 0; i < n; ++i) {
        if (form) rvll::newton_residuals(E[i], s[i], c[i], ecc[i], M[i], f[i], fp[i]);
        else {
            f[i]  = E[i] - ecc[i] * s[i] - M[i];
            fp[i] = 1 - ecc[i] * c[i];
        }
    } }
// One Newton solve per element by the rule of eval_item's first pass (start E = M, stop |dE| <= tol, at least one step, at most
// itmax; newton_next_sincos below kSafeSteps, the full pair from there on; div_exact), with the residuals in the given form, and
// (cos nu, sin nu) at the root as trueanomaly.c:36 forms them.
HN void hn_solve(const double* M, const double* ecc, long n, int form, double tol, int itmax, int* steps, double* Eout,
                 double* cosnu, double* sinnu) {
    const rvll::SincosConsts kc = rvll::sincos_consts();
    for (long i = 0; i < n; ++i) {
        const double ec = ecc[i];
        double E = M[i], s, c, dE = __builtin_inf();
        int k = 0;
        do {
            if (k < rvll::kSafeSteps) rvll::newton_next_sincos<true>(E, dE, k, s, c, kc);
            else                      rvll::sincos_any(E, s, c, kc);
            double f, fp;
            if (form) rvll::newton_residuals(E, s, c, ec, M[i], f, fp);
            else {
                f  = E - ec * s - M[i];
                fp = 1 - ec * c;
            }
            const double En = E - rvll::div_exact(f, fp);
            dE = En - E;
            E = En;
            ++k;
        } while (__builtin_fabs(dE) > tol && k < itmax);
        steps[i] = k;
        Eout[i] = E;
        rvll::sincos_any(E, s, c, kc);
        const double den = 1 - ec * c;
        cosnu[i] = (c - ec) / den;
        sinnu[i] = std::sqrt(1 - ec * ec) * s / den;
    } }
