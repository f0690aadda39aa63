// hostrotate.hip — the rotation between Newton steps (rvll_math.h: rotate_mid, newton_next_sincos) compiled for the CPU.
// Test infrastructure; built on demand by tests/test_rotate_host.py (needs hipcc, no GPU).
#include "rvll_math.h"
#define HR extern "C" __attribute__((visibility("default")))
// (s, c) = sincos_f64(E[i]) rotated nrot times, by h[i * nrot + r]
HR void hr_rotate_mid(const double* E, const double* h, long n, int nrot, double* s, double* c) {
    for (long i = 0; i < n; ++i) {
        rvll::sincos_f64(E[i], s[i], c[i]);
        for (int r = 0; r < nrot; ++r) rvll::rotate_mid(h[i * nrot + r], s[i], c[i]);
    } }
// One Newton solve per element as eval_item runs it (start E = M, stop |dE| <= tol, at least one step, at most itmax).
// rule 0: the full pair at every step; rule 1: newton_next_sincos below kSafeSteps, the full pair from there on
HR void hr_solve(const double* M, const double* ecc, long n, int rule, double tol, int itmax, int* steps, double* Eout) {
    const rvll::SincosConsts kc = rvll::sincos_consts();
    for (long i = 0; i < n; ++i) {
        const double ec = ecc[i];
        double E = M[i], s, c, dE = __builtin_inf();
        int k = 0;
        do {
            if (rule && k < rvll::kSafeSteps) rvll::newton_next_sincos<true>(E, dE, k, s, c, kc);
            else                              rvll::sincos_any(E, s, c, kc);
            const double f  = E - ec * s - M[i];
            const double fp = 1 - ec * c;
            const double En = E - rvll::div_exact(f, fp);
            dE = En - E;
            E = En;
            ++k;
        } while (__builtin_fabs(dE) > tol && k < itmax);
        steps[i] = k;
        Eout[i] = E;
    } }
HR double hr_rotate_mid_max(void) { return rvll::kRotateMidMax; }
