// hostdensity.hip — compiles the prior-density header for the CPU, so that the `-m "not gpu"` tests can compare the very
// same source the kernel of rvll_prior_density.hip uses with the reference's golden values.
// Test infrastructure; built on demand by tests/prior_density_cases.py (needs hipcc, no GPU).
#include "rvll.h"
#include "rvll_prior_density.h"
#define HD extern "C" __attribute__((visibility("default")))
HD void hd_logpdf(int kind, const double* args, const double* x, long n, double* out) {
    for (long i = 0; i < n; ++i) out[i] = rvll::prior_logpdf(kind, args, x[i]); }
HD void hd_sorted(int kind, double a, double b, int n, double lognfact, int first, const double* x_prev, const double* x, long cnt,
                  double* out) {
    for (long i = 0; i < cnt; ++i) out[i] = rvll::sorted_logpdf(kind, a, b, n, lognfact, first != 0, x_prev[i], x[i]); }
HD int hd_args_ok(int kind, const double* args) { return rvll::density_args_ok(kind, args) ? 1 : 0; }
