// rvll_rounds_runs.hip — the rounds form of the walk in RUN MODE (rvll_slice_walk_runs): the step and the directions ahead of
// it with every walker's run indirection (rvll_rounds.h, RUNS = true; RoundsArgs / RoundsDirs run fields).  A translation unit
// of its own so that the one-run kernels of rvll_kernels.hip stay as they are; the tiles of a round are the same in both modes
// (launch_rounds_tiles / launch_rounds_cu: a round's candidates are theta rows, whichever run they belong to).
#include "rvll_tile.h"
#include "rvll_rounds.h"

namespace rvll {

namespace {

__global__ __launch_bounds__(kThreads)
void rounds_dirs_runs_kernel(const RoundsDirs g)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    rounds_dirs_impl<true>(g, smem);
}

// (as rounds_step_kernel: 128 VGPRs at most, a step's wave is to fit a SIMD next to three waves of tiles)
__global__ __launch_bounds__(kThreads, 4) __attribute__((flatten))
void rounds_step_runs_kernel(const RoundsArgs g, const int r)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __builtin_amdgcn_s_setprio(3);
    rounds_step_impl<true>(g, r, (int)blockIdx.x, smem);
}

}  // namespace

hipError_t launch_rounds_dirs_runs(const RoundsDirs& g, int max_blocks, hipStream_t stream)
{
    if (g.K <= 0 || g.nsteps <= 0) return hipSuccess;
    const size_t lds = sizeof(double) * dirs_lds_doubles(g.D);
    if (g.D < 1 || !g.dirs || !g.run || !g.rid || !g.run_seed || !g.run_chol || g.nsteps >= (1 << 18) || lds > 64 * 1024 || max_blocks < 1)
        return hipErrorInvalidValue;
    const long long want = (g.K * g.nsteps + kDirPairs - 1) / kDirPairs;
    hipLaunchKernelGGL(rounds_dirs_runs_kernel, dim3((unsigned)(want < max_blocks ? want : max_blocks)), dim3(kThreads), lds, stream, g);
    return hipGetLastError();
}

hipError_t launch_rounds_step_runs(const RoundsArgs& g, int round, hipStream_t stream)
{
    if (g.K <= 0) return hipSuccess;
    const size_t lds = step_lds_bytes(g.W, g.D, g.spec_max);
    // (the checks of launch_rounds_step, and the run tables)
    if (g.W < 1 || g.W > kWave || g.D < 1 || g.spec_max < 1 || g.C < g.K || g.c_free > g.C || g.c_free < 1 || round < 0 ||
        g.nsteps >= (1 << 18) || g.max_rounds < 1 || g.max_rounds > 4096 || (long long)g.K * g.spec_max >= (1LL << 31) ||
        !g.priors || !g.light_dims || (g.n_heavy > 0 && !g.heavy_dims) || g.n_heavy > g.D || !g.theta_c[0] || !g.theta_c[1] ||
        !g.wdef || !g.wflag || !g.dirs || !g.dirnext || lds > 64 * 1024 ||
        !g.run || !g.rid || !g.run_lstar || !g.run_seed || !g.wcost)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rounds_step_runs_kernel, dim3((unsigned)((g.K + g.W - 1) / g.W)), dim3(kThreads), lds, stream, g, round);
    return hipGetLastError();
}

}  // namespace rvll
