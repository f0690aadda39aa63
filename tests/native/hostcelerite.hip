// hostcelerite.hip — compiles the celerite recursion header for the CPU, so that the `-m "not gpu"` tests can compare the very
// same source the kernel of rvll_celerite.hip runs with the dense definition of evidence_amd/correlated.py.
// Test infrastructure; built on demand by tests/test_correlated_host.py (needs hipcc, no GPU).
#include "rvll.h"
#include "rvll_celerite.h"
#define HC extern "C" __attribute__((visibility("default")))

// out = a, b, c, d, form; returns 1 where the parameters are valid
HC int hc_column(int kind, int sub, const double* p, double* out) {
    rvll::CelColumn k;
    const bool ok = rvll::cel_column(kind, sub, p, k);
    out[0] = k.a; out[1] = k.b; out[2] = k.c; out[3] = k.d; out[4] = (double)k.form;
    return ok ? 1 : 0; }

namespace {
template <int J>
void run(const int* kind, const int* sub, const double* par, int ne, const double* ts, const double* dts, const double* res,
         const double* var, double cte, double* logl, int* flag) {
    rvll::CelColumn col[J];
    bool valid = true;
    double suma = 0.0;
    for (int j = 0; j < J; ++j) {
        valid &= rvll::cel_column(kind[j], sub[j], par + 5 * j, col[j]);
        if (col[j].form != rvll::kCelColSin) suma += col[j].a;
    }
    const bool pair = rvll::cel_prepare<J>(col);
    rvll::CelState<J> st;
    rvll::cel_init(st);
    for (int n = 0; n < ne; ++n) rvll::cel_step<J>(col, suma, pair, st, ts[n], dts[n], res[n], var[n]);
    int32_t f;
    rvll::cel_result<J>(st, valid, cte, *logl, f);
    *flag = f; }
}  // namespace

// the epochs in time order: ts from the first, dts the gaps (0 at the first); par [J][5] the parameters of every column's term
HC int hc_loglike(int J, const int* kind, const int* sub, const double* par, int ne, const double* ts, const double* dts,
                  const double* res, const double* var, double cte, double* logl, int* flag) {
    switch (J) {
    case 1: run<1>(kind, sub, par, ne, ts, dts, res, var, cte, logl, flag); return 0;
    case 2: run<2>(kind, sub, par, ne, ts, dts, res, var, cte, logl, flag); return 0;
    case 3: run<3>(kind, sub, par, ne, ts, dts, res, var, cte, logl, flag); return 0;
    case 4: run<4>(kind, sub, par, ne, ts, dts, res, var, cte, logl, flag); return 0;
    }
    return -1; }
