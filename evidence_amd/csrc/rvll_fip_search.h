// The two binary searches that turn an orbital frequency into its span of frequency bins (evidence/fip_criterion.py:334-335),
// shared by rvll_fip.hip (fip_index_kernel) and rvll_fip_merged.hip (span_kernel): index work, exactly numpy's answer.
#pragma once
#include <hip/hip_runtime.h>

namespace rvll {

// number of a[i] <= v (numpy.searchsorted(a, v, 'right')); a NaN v compares false everywhere -> 0, and the
// matching lower bound is 0 too, i.e. the same empty interval numpy's (n, n) is
__device__ inline int count_le(const double* __restrict__ a, int n, double v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// number of a[i] < v (numpy.searchsorted(a, v, 'left'))
__device__ inline int count_lt(const double* __restrict__ a, int n, double v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace rvll
