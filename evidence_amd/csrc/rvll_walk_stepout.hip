// rvll_walk_stepout.hip — the stepout instantiations of the single-kernel walk (rvll_walk_kernel.h), in a
// translation unit of their own: see that header.  Built with the walk's flags (csrc/Makefile).
#define RVLL_LOCAL_CONSTS 1      // (as in rvll_walk.hip)
#ifndef RVLL_WALK_WAVES
#define RVLL_WALK_WAVES 4
#endif
#include "rvll_walk_kernel.h"

namespace rvll {

namespace {
using WalkKernel = void (*)(const LoglikeArgs, const WalkArgsStepout);

WalkKernel stepout_kernel(int precision, bool fat, bool runs)
{
#define RVLL_SO(PREC)                                                                                                \
    return runs ? (fat ? slice_walk_kernel<PREC, true, 0, true, kPropStepout> : slice_walk_kernel<PREC, false, 0, true, kPropStepout>) \
                : (fat ? slice_walk_kernel<PREC, true, 0, false, kPropStepout> : slice_walk_kernel<PREC, false, 0, false, kPropStepout>)
    switch (precision) {
    case RVLL_PREC_MIXED: RVLL_SO(RVLL_PREC_MIXED);
    case RVLL_PREC_FP32:  RVLL_SO(RVLL_PREC_FP32);
    default:              RVLL_SO(RVLL_PREC_FP64);
    }
#undef RVLL_SO
}
}  // namespace

long long slice_walk_stepout_blocks(const LoglikeArgs& a, long long K, bool fat, bool runs, int max_cus)
{
    long long nblocks = (K + a.PB - 1) / a.PB;
    if (max_cus > 0) {
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, stepout_kernel(a.precision, fat, runs), kThreads,
                                                         walk_lds_bytes(a, kPropStepout)) != hipSuccess) return -1;
        nblocks = std::min(nblocks, (long long)std::max(1, occ) * max_cus);
    }
    return nblocks;
}

hipError_t launch_slice_walk_stepout(const LoglikeArgs& a, const WalkArgs& w, const StepoutArgs& so, bool fat, bool runs, int max_cus,
                                     size_t lds, hipStream_t stream)
{
    const long long nb = slice_walk_stepout_blocks(a, w.K, fat, runs, max_cus);
    if (nb < 1 || nb * a.PB > so.basis_slots) return hipErrorInvalidValue;     // every slot has its basis scratch
    WalkArgsStepout ws;
    static_cast<WalkArgs&>(ws) = w;
    ws.so = so;
    hipLaunchKernelGGL(stepout_kernel(a.precision, fat, runs), dim3((unsigned)nb), dim3(kThreads), lds, stream, a, ws);
    return hipGetLastError();
}

}  // namespace rvll
