// hostshortcut.hip — the shortcut loop of the fp64 Kepler solve (rvll_math.h: newton_shortcut) compiled for the CPU, and the same
// loop written out with its bookkeeping.  Test infrastructure; built on demand by tests/test_gpu_newton_asm.py (needs hipcc, no GPU).
#include <cmath>
#include "rvll_math.h"
#define HS extern "C" __attribute__((visibility("default")))
// (s, c, dE) as newton_shortcut leaves them from E = M: the host build's compiled loop
HS void hs_shortcut(const double* M, const double* ecc, long n, double tol, double* s, double* c, double* dE) {
    const rvll::SincosConsts kc = rvll::sincos_consts();
    for (long i = 0; i < n; ++i) {
        double E;
        rvll::newton_shortcut<false>(E, dE[i], s[i], c[i], ecc[i], M[i], tol, kc);
    } }
// The same loop step by step: steps taken (<= kSafeSteps), and in `beyond` bit k set where evaluation k (k >= 1) met a step
// beyond pi/4 — where the hand-written trips hand over to the compiled loop.
HS void hs_trace(const double* M, const double* ecc, long n, double tol, int* steps, int* beyond, double* s, double* c, double* dE) {
    const rvll::SincosConsts kc = rvll::sincos_consts();
    for (long i = 0; i < n; ++i) {
        double E = M[i], h = __builtin_inf();
        int k = 0, far = 0;
        do {
            if (k > 0 && !(__builtin_fabs(h) <= rvll::kRotateMidMax)) far |= 1 << k;
            rvll::newton_next_sincos<false>(E, h, k, s[i], c[i], kc);
            double f, fp;
            rvll::newton_residuals(E, s[i], c[i], ecc[i], M[i], f, fp);
            const double En = E - rvll::div_exact(f, fp);
            h = En - E;
            E = En;
            ++k;
        } while (__builtin_fabs(h) > tol && k < rvll::kSafeSteps);
        steps[i] = k;
        beyond[i] = far;
        dE[i] = h;
    } }
