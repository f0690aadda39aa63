// shrinkuniform.hip — rvll_math.h's uniform01 compiled for the CPU, so that the `-m "not gpu"` tests can hold the numpy
// draws of evidence_amd/shrinkage.py against the very source the shrinkage kernel uses.
// Test infrastructure; built on demand by tests/test_shrinkage_host.py (needs hipcc, no GPU).
#include "rvll_math.h"
#define HM extern "C" __attribute__((visibility("default")))
HM void su_uniform01(unsigned long long seed, long n, double* out) { for (long j = 0; j < n; ++j) out[j] = rvll::uniform01(seed, (uint64_t)j); }
