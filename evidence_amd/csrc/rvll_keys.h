// Doubles as uint64 radix-sort keys whose unsigned order is the doubles' order (rvll_insertion.hip, rvll_merge.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rvll {

// -0.0 is canonicalised to +0.0, so that equal keys are equal doubles and key comparisons are double comparisons (no NaN)
__host__ __device__ inline unsigned long long key_of(double x)
{
    if (x == 0.0) x = 0.0;
    unsigned long long b;
    __builtin_memcpy(&b, &x, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

}  // namespace rvll
