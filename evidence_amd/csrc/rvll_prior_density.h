// rvll_prior_density.h — the log density of every prior kind, host+device.
//
// The density is that of the transform the sampler applies (rvll_tile.h: prior_light / prior_heavy / table_ppf): the
// derivative of the inverse of what those compute.  Every function returns the LOG density, -inf outside the support and NaN
// for a NaN argument.  Support ends are closed or open as the reference's `_pdf` conditions have them (include/rvll.h lists
// them with the arguments of every kind); UniformFrequency is cut to [xmin, xmax] and Log10Normal carries its Jacobian, which
// the reference's `.pdf` leave out.  evidence_amd/priors.py (log_density) holds the numpy definition of the same formulas.
//
// The kernel of rvll_prior_density.hip uses these on the GPU and tests/native/hostdensity.hip compiles the very same source
// for the CPU, so that the `-m "not gpu"` suite can compare it with the reference's golden values.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef RVLL_HDF
#define RVLL_HDF __host__ __device__ inline
#endif

namespace rvll {

constexpr double kHalfLog2Pi = 0.91893853320467274178;    // ln sqrt(2 pi)
constexpr double kLog10 = 2.30258509299404568402;          // ln 10
constexpr double kRadPerDeg = 0.017453292519943295;        // pi / 180, the double numpy's pi / 180.0 gives

// scipy.stats.norm.logpdf(x, mu, sigma)
RVLL_HDF double norm_logpdf(double x, double mu, double sigma)
{
    const double z = (x - mu) / sigma;
    return -(z * z) / 2 - kHalfLog2Pi - log(sigma);
}

// ln(exp(a) + exp(b)) without leaving the log domain; -inf where both are
RVLL_HDF double log_add_exp(double a, double b)
{
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (hi == -INFINITY) return -INFINITY;
    return hi + log1p(exp(lo - hi));
}

// One parameter's log density under a kind that stands alone (every kind but SKIP and the two sorted ones).  `a` are the
// arguments in the order include/rvll.h documents; the caller has checked them (density_args_ok).
RVLL_HDF double prior_logpdf(int kind, const double* a, double x)
{
    if (x != x) return NAN;
    switch (kind) {
    case RVLL_DENSITY_UNIFORM:               // xmin, xmax
        return (x >= a[0] && x <= a[1]) ? -log(a[1] - a[0]) : -INFINITY;
    case RVLL_DENSITY_JEFFREYS:              // xmin, xmax
        return (x >= a[0] && x <= a[1]) ? -log(x) - log(log(a[1] / a[0])) : -INFINITY;
    case RVLL_DENSITY_MODJEFFREYS:           // x0, xmax
        return (x >= 0. && x <= a[1]) ? -log(a[0] + x) - log(log(1 + a[1] / a[0])) : -INFINITY;
    case RVLL_DENSITY_UNIFORMFREQUENCY:      // xmin, xmax
        return (x >= a[0] && x <= a[1]) ? log(a[1] * a[0] / (a[1] - a[0])) - 2 * log(x) : -INFINITY;
    case RVLL_DENSITY_NORMAL:                // loc, scale
        return norm_logpdf(x, a[0], a[1]);
    case RVLL_DENSITY_LOGNORMAL: {           // s, loc, scale
        const double y = (x - a[1]) / a[2];
        if (!(y > 0.)) return -INFINITY;
        const double ly = log(y);
        return -(ly * ly) / (2 * (a[0] * a[0])) - log(a[0]) - ly - kHalfLog2Pi - log(a[2]); }
    case RVLL_DENSITY_LOG10NORMAL:           // mu, sigma
        if (!(x > 0.)) return -INFINITY;
        return norm_logpdf(log(x) / kLog10, a[0], a[1]) - log(x * kLog10);
    case RVLL_DENSITY_TRUNCRAYLEIGH: {       // sigma, xmax
        if (!(x >= 0. && x < a[1])) return -INFINITY;
        const double s2 = a[0] * a[0];
        const double A = 1 - exp(-(a[1] * a[1]) / (2 * s2));
        return log(x / s2) - (x * x) / (2 * s2) - log(A); }
    case RVLL_DENSITY_TRUNCUNORMAL:          // mu, sigma, xmin, xmax, ln(Phi((xmax - mu) / sigma) - Phi((xmin - mu) / sigma))
        return (x >= a[2] && x < a[3]) ? norm_logpdf(x, a[0], a[1]) - a[4] : -INFINITY;
    case RVLL_DENSITY_POWERLAW:              // alpha, xmin, xmax, ln A
        if (!(x >= a[1] && x < a[2])) return -INFINITY;
        return a[0] == 0. ? a[3] : a[3] + a[0] * log(x);
    case RVLL_DENSITY_DOUBLEPOWERLAW: {      // alpha, beta, x0, xmin, xmax, ln A
        if (!(x >= a[3] && x < a[4])) return -INFINITY;
        if (x < a[2]) return a[0] == 0. ? a[5] : a[5] + a[0] * log(x);
        const double join = a[5] + (a[0] - a[1]) * log(a[2]);
        return a[1] == 0. ? join : join + a[1] * log(x); }
    case RVLL_DENSITY_SINE:                  // max(xmin, 0), min(xmax, 180), ln(180 / pi (cos lo - cos hi))
        return (x >= a[0] && x <= a[1]) ? log(sin(x * kRadPerDeg)) - a[2] : -INFINITY;
    case RVLL_DENSITY_BINORMAL:              // mu1, sigma1, mu2, sigma2, A
        return log_add_exp(log(0.5 * (1 - a[4])) + norm_logpdf(x, a[0], a[1]),
                           log(0.5 * (1 + a[4])) + norm_logpdf(x, a[2], a[3]));
    case RVLL_DENSITY_ASYMNORMAL: {          // mu, sigma1, sigma2
        const double s = x <= a[0] ? a[1] : a[2];
        return norm_logpdf(x, a[0], s) + log(2 * s / (a[1] + a[2])); }
    case RVLL_DENSITY_ALPHA: {               // a, Phi(a)
        if (!(x > 0.)) return -INFINITY;
        const double z = a[0] - 1 / x;
        return -2 * log(x) - (z * z) / 2 - kHalfLog2Pi - log(a[1]); }
    case RVLL_DENSITY_BETA:                  // a, b, ln B(a, b)
        if (!(x > 0. && x < 1.)) return -INFINITY;
        return (a[0] - 1) * log(x) + (a[1] - 1) * log1p(-x) - a[2];
    case RVLL_DENSITY_GAMMA: {               // alpha, beta, ln Gamma(alpha)
        if (!(x > 0.)) return -INFINITY;
        const double y = x * a[1];
        return (a[0] - 1) * log(y) - y - a[2] + log(a[1]); }
    default:
        return NAN;
    }
}

// One member of a sorted group (a <= x_1 <= ... <= x_n <= b, members in rising parameter order; a, b the bounds of the LAST
// member, as sorted_prior takes them).  The joint density  ln n! - n ln(b - a)  (uniform)  or  ln n! - n ln ln(b / a) - sum
// ln x_i  (log-uniform) is credited at the last member (n > 0 there, 0 at the others; lognfact = ln n!); every member checks
// its own link of the chain, x_prev <= x (the first member: a <= x), the last one x <= b as well, and gives -inf where it is
// broken.
RVLL_HDF double sorted_logpdf(int kind, double a, double b, int n, double lognfact, bool first, double x_prev, double x)
{
    if (x != x || (!first && x_prev != x_prev)) return NAN;
    if (!(x >= (first ? a : x_prev))) return -INFINITY;
    if (n > 0 && !(x <= b)) return -INFINITY;
    const bool logu = kind == RVLL_DENSITY_SORTED_LOGUNIFORM;
    double v = logu ? -log(x) : 0.;
    if (n > 0) v += lognfact - n * (logu ? log(log(b / a)) : log(b - a));
    return v;
}

// The conditions the factories of evidence_amd/priors.py put on the arguments (`_require`), and finite host constants.
inline bool density_args_ok(int kind, const double* a)
{
    auto fin = [](double v) { return v == v && v != INFINITY && v != -INFINITY; };
    switch (kind) {
    case RVLL_DENSITY_SKIP:             return true;
    case RVLL_DENSITY_UNIFORM:          return a[0] < a[1];
    case RVLL_DENSITY_JEFFREYS:         return a[0] > 0. && a[1] > a[0];
    case RVLL_DENSITY_MODJEFFREYS:      return a[1] > a[0] && a[0] > 0.;
    case RVLL_DENSITY_UNIFORMFREQUENCY: return a[1] > a[0] && a[0] > 0.;
    case RVLL_DENSITY_NORMAL:           return fin(a[0]) && a[1] > 0.;
    case RVLL_DENSITY_LOGNORMAL:        return a[0] > 0. && fin(a[1]) && a[2] > 0.;
    case RVLL_DENSITY_LOG10NORMAL:      return fin(a[0]) && a[1] > 0.;
    case RVLL_DENSITY_TRUNCRAYLEIGH:    return a[0] > 0. && a[1] > 0.;
    case RVLL_DENSITY_TRUNCUNORMAL:     return fin(a[0]) && a[1] > 0. && a[2] < a[3] && fin(a[4]);
    case RVLL_DENSITY_POWERLAW:         return a[2] > a[1] && a[1] >= 0. && a[2] > 0. && fin(a[0]) && a[0] != -1. && fin(a[3]);
    case RVLL_DENSITY_DOUBLEPOWERLAW:   return a[4] > a[3] && a[3] >= 0. && a[4] > 0. && fin(a[0]) && a[0] != -1. && fin(a[1])
                                               && a[2] > 0. && fin(a[5]);
    case RVLL_DENSITY_SINE:             return a[0] >= 0. && a[1] <= 180. && a[0] < a[1] && fin(a[2]);
    case RVLL_DENSITY_BINORMAL:         return a[1] > 0. && a[3] > 0. && a[0] <= a[2] && a[4] >= -1. && a[4] <= 1.;
    case RVLL_DENSITY_ASYMNORMAL:       return fin(a[0]) && a[1] > 0. && a[2] > 0.;
    case RVLL_DENSITY_ALPHA:            return a[0] > 0. && a[1] > 0. && a[1] <= 1.;
    case RVLL_DENSITY_BETA:             return a[0] > 0. && a[1] > 0. && fin(a[2]);
    case RVLL_DENSITY_GAMMA:            return a[0] > 0. && a[1] > 0. && fin(a[2]);
    case RVLL_DENSITY_SORTED_UNIFORM:   return a[0] < a[1];
    case RVLL_DENSITY_SORTED_LOGUNIFORM: return a[0] > 0. && a[0] < a[1];
    default:                            return false;
    }
}

}  // namespace rvll
