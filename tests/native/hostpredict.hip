// hostpredict.hip — compiles the GP-prediction header for the CPU, so that the `-m "not gpu"` tests can compare the very same
// source the kernels of rvll_celerite_predict.hip run with the dense definition of evidence_amd/correlated.py.
// Test infrastructure; built on demand by tests/test_predict_host.py (needs hipcc, no GPU).
#include <vector>
#include "rvll.h"
#include "rvll_celerite_predict.h"
#define HC extern "C" __attribute__((visibility("default")))

namespace {
template <int J>
void run(const int* kind, const int* sub, const double* par, int ne, const double* ts, const double* dts, const double* res,
         const double* var, int m, const int32_t* qstart, const double* xq, const double* dtf, const double* dtb, int want_var,
         double cte, double* alpha, double* mean_data, double* var_data, double* mean, double* vq, double* logl, int* flag) {
    using namespace rvll;
    CelColumn col[J];
    bool valid = true;
    double suma = 0.0;
    for (int j = 0; j < J; ++j) {
        valid &= cel_column(kind[j], sub[j], par + 5 * j, col[j]);
        if (col[j].form != kCelColSin) suma += col[j].a;
    }
    const bool pair = cel_prepare<J>(col);
    // the factor, with what every epoch leaves in the state kept
    CelState<J> st;
    cel_init(st);
    std::vector<double> W((size_t)ne * J), D((size_t)ne), z((size_t)ne);
    for (int n = 0; n < ne; ++n) {
        cel_step<J>(col, suma, pair, st, ts[n], dts[n], res[n], var[n]);
        for (int j = 0; j < J; ++j) W[(size_t)n * J + j] = st.W[j];
        D[(size_t)n] = st.D;
        z[(size_t)n] = st.z;
    }
    int32_t f;
    cel_result<J>(st, valid, cte, *logl, f);
    *flag = f;
    if (f) return;
    // backward: alpha, the data epochs, the later epochs' share of every query
    CelBack<J> bk;
    cel_back_init(bk);
    for (int q = qstart[ne]; q < qstart[ne + 1]; ++q) mean[q] = 0.0;
    for (int n = ne - 1; n >= 0; --n) {
        CelGap<J> P;
        double U[J], V[J], Wn[J], G[J], a, znn;
        for (int j = 0; j < J; ++j) Wn[j] = W[(size_t)n * J + j];
        cel_gap<J>(col, ts[n], dts[n], P, U, V);
        cel_back_step<J>(bk, P, U, Wn, D[(size_t)n], z[(size_t)n], a, znn, G);
        alpha[n] = a;
        mean_data[n] = res[n] - var[n] * a;
        var_data[n] = var[n] - var[n] * var[n] * znn;
        for (int q = qstart[n]; q < qstart[n + 1]; ++q) mean[q] = cel_query_back<J>(col, xq[q], dtb[q], G);
    }
    // forward: the earlier epochs' share
    double F[J];
    for (int j = 0; j < J; ++j) F[j] = 0.0;
    for (int n = 0; n < ne && m > 0; ++n) {
        CelGap<J> P;
        double U[J], V[J];
        cel_gap<J>(col, ts[n], dts[n], P, U, V);
        cel_fwd_step<J>(F, P, V, alpha[n]);
        for (int q = qstart[n + 1]; q < qstart[n + 2]; ++q) mean[q] += cel_query_fwd<J>(col, xq[q], dtf[q], F);
    }
    for (int q = 0; q < m && want_var; ++q) {
        CelVar<J> vs;
        cel_var_init(vs);
        double Wp[J];
        for (int j = 0; j < J; ++j) Wp[j] = 0.0;
        for (int n = 0; n < ne; ++n) {
            CelGap<J> P;
            double U[J], V[J];
            cel_gap<J>(col, ts[n], dts[n], P, U, V);
            cel_var_step<J>(vs, P, U, Wp, D[(size_t)n], cel_kernel_value<J>(col, fabs(xq[q] - ts[n])));
            for (int j = 0; j < J; ++j) Wp[j] = W[(size_t)n * J + j];
        }
        vq[q] = suma - vs.acc;
    }
}
}  // namespace

// One row.  The epochs in time order: ts from the first, dts the gaps (0 at the first); par [J][5] the parameters of every
// column's term.  The m queries in time order: xq from the first epoch, bucket k = qstart[k] .. qstart[k + 1] those in
// [t_(k-1), t_k) (k = 0: before the first epoch, k = ne: at or after the last), dtf the time since the epoch before, dtb until the
// epoch after.  Outputs in time order.
HC int hp_predict(int J, const int* kind, const int* sub, const double* par, int ne, const double* ts, const double* dts,
                  const double* res, const double* var, int m, const int32_t* qstart, const double* xq, const double* dtf,
                  const double* dtb, int want_var, double cte, double* alpha, double* mean_data, double* var_data, double* mean,
                  double* vq, double* logl, int* flag) {
#define HP_RUN(N) run<N>(kind, sub, par, ne, ts, dts, res, var, m, qstart, xq, dtf, dtb, want_var, cte, alpha, mean_data, var_data, mean, vq, logl, flag)
    switch (J) {
    case 1: HP_RUN(1); return 0;
    case 2: HP_RUN(2); return 0;
    case 3: HP_RUN(3); return 0;
    case 4: HP_RUN(4); return 0;
    }
    return -1; }
