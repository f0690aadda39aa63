// Pointwise predictive checks of the replicates of a merged run on gfx950: per replicate and per unit (an epoch, a night, an
// instrument) the in-sample log predictive density, the importance-sampling leave-one-out value and the posterior mean and
// variance of the unit's log-likelihood (the WAIC correction), reduced on the device from the weights that the replicate
// kernel of rvll_merge_setup.hip writes.  No weight leaves the device.  evidence_amd/pointwise.py holds the numpy definition;
// DESIGN §4q.
//
// All four are ratios of weighted sums over the merged rows, so a block of replicates is one dense product on the matrix units,
//     D [replicates x C] = p [replicates x N] . B [N x C],     C = 4 U + 1,
// with v_mfma_f64_16x16x4_f64.  The columns of B are ones, then per unit u with t the unit's log-likelihood in the merged row and
// the call's shifts c_u, d_u, a_u:  E1 = exp(min(t - c, 0)), E2 = exp(min(d - t, 0)), z = t - a, z^2.  P = sum p is the ones column
// and goes through the same product as every other column: a unit whose t is constant has E1 = E2 = 1, the same column as the
// ones, so its sums equal P bit for bit and lpd = c, loo = d, mean = a, var = 0 exactly.
//
// Once per call:
//     setup     the merge's own (rvll_merge_setup.hip: keys, two sorts, place) -> the merged order
//     operand   B [Np x Cp] row-major in merged order, Np = N rounded up to kChunk rows and Cp = C rounded up to 64 columns; the
//               rows from N on and the columns from C on are zeros, so no tile of the product loads anything it was not given
// Per block of replicates (as many as fit the block bound next to B):
//     weights   replicate_kernel writes logw - lnZ into the replicate's slot; exp_kernel turns the block into p = exp(logwt)
//     product   K (the merged rows) is cut into slabs of kSlabRows rows, a constant.  One 256-thread workgroup per (slab, 64
//               replicates, 64 columns): wave w owns replicates 16 w .. 16 w + 15 of the tile and four 16-column tiles, whose
//               accumulators (4 x 4 doubles a lane) stay in registers.  p is staged through LDS kChunk rows at a time: a wave
//               reads 64 consecutive rows of one replicate's slot (a coalesced 512-byte segment; K is contiguous in a slot), the
//               next chunk's loads are in flight while this one is multiplied, and the LDS rows are kChunk + 2 doubles apart so
//               that the A fragment (lane l: replicate l & 15, row l >> 4 of the k-step) touches every bank once.  Replicates
//               past the block and rows past N are staged as zeros.  B is read row-major from memory, lane l row l >> 4, column
//               l & 15 of its tile: 128-byte segments, kGroup k-steps ahead of the products.  The workgroup writes its 64 x 64
//               partial.
//     finish    one thread per (replicate, unit) adds the slabs' partials in rising slab order and forms the four outputs.
// No floating-point atomics.  An accumulator element sums its replicate's row against its column in rising k, four rows an
// instruction, from the slab's first row: its bits depend on the replicate's weights, the column and the fixed slab cut, not on
// where in a tile, a block or a call the replicate or the column sits.
// The call itself (device, stream, buffers, blocks of replicates, timing) is rvll_merge_setup.h's Replicates.
#include "rvll_merge_setup.h"

using namespace rvll::merge;

namespace {

constexpr int kMaxUnits = 4096;
constexpr double kMaxAbs = 1e30;                          // the largest |t| and |shift|: z^2 stays finite
constexpr int kSlabRows = 16384;                          // rows of one slab of K: it depends on nothing, and so do the bits
constexpr int kChunk = 64;                                // rows staged through LDS at a time
constexpr int kStride = kChunk + 2;                       // doubles between two replicates in LDS
constexpr int kRepTile = 16 * kWaves;                     // replicates of a workgroup
constexpr int kNT = 4;                                    // 16-column tiles of a wave
constexpr int kColTile = 16 * kNT;                        // columns of a workgroup
constexpr int kGroup = 4;                                 // k-steps of B a wave loads ahead of its products
constexpr int kStage = kRepTile * kChunk / kThreads;      // doubles a thread stages per chunk
constexpr long long kMaxReps = 1ll << 20;                 // replicates per block: 2^14 tiles in grid z

static_assert(kSlabRows % kChunk == 0 && kChunk % (4 * kGroup) == 0 && kChunk == kWave, "the staging map needs a chunk of one wave of rows");

typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kThreads)
void exp_kernel(double* __restrict__ w, long long total)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads)
        w[i] = exp(w[i]);
}

// B [np x cp] from the table [n x units] in input row order and the shifts [3 x units] (c, d, a)
__global__ __launch_bounds__(kThreads)
void operand_kernel(const double* __restrict__ table, const double* __restrict__ shifts, const int32_t* __restrict__ order,
                    long long n, long long np, int units, int cp, double* __restrict__ B)
{
    const int ncols = 4 * units + 1;
    const long long total = np * cp;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
        const long long i = e / cp;
        const int c = (int)(e - i * cp);
        double v = 0.0;
        if (i < n && c < ncols) {
            if (c == 0) {
                v = 1.0;
            } else {
                const int u = (c - 1) >> 2, k = (c - 1) & 3;
                const double t = table[(long long)order[i] * units + u];
                if (k == 0) {
                    v = exp(fmin(t - shifts[u], 0.0));
                } else if (k == 1) {
                    v = exp(fmin(shifts[units + u] - t, 0.0));
                } else {
                    const double z = t - shifts[2 * units + u];
                    v = k == 2 ? z : z * z;
                }
            }
        }
        B[e] = v;
    }
}

// part [slab][sbp][cp]: the slab's product of the block's weights p [sb x n] with B [np x cp]; grid (slabs, column tiles, replicate tiles)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3)))
void product_kernel(const double* __restrict__ p, const double* __restrict__ B, long long n, long long np, int cp, int sb, int sbp,
                    double* __restrict__ part)
{
    __shared__ double sh[kRepTile * kStride];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long slab = blockIdx.x;
    const int col0 = (int)blockIdx.y * kColTile, rep0 = (int)blockIdx.z * kRepTile;
    const long long k_begin = slab * kSlabRows;
    const long long k_end = k_begin + kSlabRows < np ? k_begin + kSlabRows : np;
    const int arow = wave * 16 + (lane & 15), kq = lane >> 4;

    double4_t acc[kNT];
#pragma unroll
    for (int t = 0; t < kNT; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};

    // staging: wave w takes replicates w, w + 4, ... of the tile, lane l row l of the chunk.  Every load is in bounds (a
    // replicate past the block reads the block's last, a row past N the last row) and unconditional, so that the sixteen are
    // in flight together; the tails become zeros on the way into LDS.
    double st[kStage];
    auto fetch = [&](long long kb) {
        const long long kc = kb + lane < n ? kb + lane : n - 1;
#pragma unroll
        for (int i = 0; i < kStage; ++i) {
            const int rep = rep0 + i * kWaves + wave;
            st[i] = p[(long long)(rep < sb ? rep : sb - 1) * n + kc];
        }
    };
    auto stash = [&](long long kb) {
        const bool row_ok = kb + lane < n;
#pragma unroll
        for (int i = 0; i < kStage; ++i) {
            asm volatile("" : "+v"(st[i]));                // the load stays unconditional: no branch round it
            sh[(i * kWaves + wave) * kStride + lane] = (rep0 + i * kWaves + wave < sb && row_ok) ? st[i] : 0.0;
        }
    };
    // B: the kGroup k-steps after row `row` (a multiple of 4 kGroup, below np or clamped to the last group: a load that is
    // never used), one group ahead of the products
    auto load_b = [&](double (&b)[kGroup][kNT], long long row) {
        const long long r = row < np ? row : np - 4 * kGroup;
        const double* __restrict__ bp = B + (r + kq) * cp + col0 + (lane & 15);
#pragma unroll
        for (int j = 0; j < kGroup; ++j)
#pragma unroll
            for (int t = 0; t < kNT; ++t) b[j][t] = bp[(long long)(4 * j) * cp + 16 * t];
    };
    double bcur[kGroup][kNT], bnext[kGroup][kNT];
    fetch(k_begin);
    load_b(bcur, k_begin);
    for (long long kb = k_begin; kb < k_end; kb += kChunk) {
        __syncthreads();                                   // the chunk before has been read
        stash(kb);
        __syncthreads();
        if (kb + kChunk < k_end) fetch(kb + kChunk);
#pragma unroll
        for (int g = 0; g < kChunk / (4 * kGroup); ++g) {
            load_b(bnext, kb + (g + 1) * 4 * kGroup);
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                const double a = sh[arow * kStride + (g * kGroup + j) * 4 + kq];
#pragma unroll
                for (int t = 0; t < kNT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bcur[j][t], acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
#pragma unroll
                for (int t = 0; t < kNT; ++t) bcur[j][t] = bnext[j][t];
        }
    }
    // D: column lane & 15, row (lane >> 4) + 4 r in register r
    double* __restrict__ out = part + (slab * sbp + rep0 + wave * 16) * (long long)cp + col0 + (lane & 15);
#pragma unroll
    for (int t = 0; t < kNT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(long long)(kq + 4 * r) * cp + 16 * t] = acc[t][r];
    }
}

__global__ __launch_bounds__(kThreads)
void finish_kernel(const double* __restrict__ part, const double* __restrict__ shifts, long long slabs, int cp, int sb, int sbp,
                   int units, long long s0, double* __restrict__ lpd, double* __restrict__ loo, double* __restrict__ mean,
                   double* __restrict__ var)
{
    const long long total = (long long)sb * units;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
        const int s = (int)(e / units), u = (int)(e - (long long)s * units);
        double P = 0.0, e1 = 0.0, e2 = 0.0, z1 = 0.0, z2 = 0.0;
        for (long long k = 0; k < slabs; ++k) {
            const double* __restrict__ row = part + (k * sbp + s) * (long long)cp;
            P += row[0];
            e1 += row[1 + 4 * u];
            e2 += row[2 + 4 * u];
            z1 += row[3 + 4 * u];
            z2 += row[4 + 4 * u];
        }
        const long long o = (s0 + s) * units + u;
        const double m1 = z1 / P;
        lpd[o] = shifts[u] + log(e1 / P);
        loo[o] = shifts[units + u] - log(e2 / P);
        mean[o] = shifts[2 * units + u] + m1;
        var[o] = z2 / P - m1 * m1;
    }
}

inline long long slabs_of(long long n) { return (n + kSlabRows - 1) / kSlabRows; }
inline long long padded_rows(long long n) { return (n + kChunk - 1) / kChunk * kChunk; }
inline int padded_cols(int units) { return (4 * units + 1 + kColTile - 1) / kColTile * kColTile; }

int run_pointwise(int32_t device, const double* logl, const double* birth, int64_t n, const int64_t* run_start, int32_t n_runs,
                  const double* table, int32_t units, const double* shifts, int32_t nsamples, int expected, int bootstrap,
                  uint64_t seed, double* logz, double* info, double* lpd, double* loo, double* mean, double* var,
                  int64_t block_bytes, rvll_pointwise_timing* timing)
{
    const long long np = padded_rows(n), slabs = slabs_of(n);
    const int cp = padded_cols(units);
    // a block of sb replicates keeps slabs x (sb rounded up to a tile) x cp partials: one tile's worth counts with the tables
    const long long per_rep = (n + slabs * cp) * (long long)sizeof(double);
    const long long tables = (np + (long long)kRepTile * slabs) * cp * (long long)sizeof(double);
    char what[64];
    snprintf(what, sizeof what, "the operand of %d units", (int)units);
    Replicates rep(device, logl, birth, n, run_start, n_runs, nsamples, expected, bootstrap, seed);
    MRG_OK(rep.plan_blocks(block_bytes, tables + kDefaultWeightBytes, tables, per_rep, kMaxReps, what,
                           "the weights and their partial sums"));
    const long long sbp_max = (rep.s_blk + kRepTile - 1) / kRepTile * kRepTile;
    double *d_tin = nullptr, *d_shifts = nullptr, *d_B = nullptr, *d_part = nullptr;
    double *d_lpd = nullptr, *d_loo = nullptr, *d_mean = nullptr, *d_var = nullptr;
    const size_t su_count = (size_t)nsamples * (size_t)units;

    MRG_OK(rep.begin());
    MergeSetup& su = rep.su;
    const hipStream_t stream = rep.stream;
    MRG_TRY(rep.alloc(d_lpd, su_count));
    MRG_TRY(rep.alloc(d_loo, su_count));
    MRG_TRY(rep.alloc(d_mean, su_count));
    MRG_TRY(rep.alloc(d_var, su_count));
    MRG_TRY(rep.alloc(d_shifts, (size_t)3 * units));
    MRG_TRY(rep.alloc(d_B, (size_t)np * cp));
    MRG_TRY(rep.alloc(d_part, (size_t)slabs * sbp_max * cp));
    MRG_TRY(rep.alloc(d_tin, (size_t)n * units));            // the input's copy: freed once B is written
    MRG_TRY(hipMemcpyAsync(d_tin, table, sizeof(double) * (size_t)n * units, hipMemcpyHostToDevice, stream));
    MRG_TRY(hipMemcpyAsync(d_shifts, shifts, sizeof(double) * (size_t)3 * units, hipMemcpyHostToDevice, stream));

    MRG_OK(rep.setup([&]() -> hipError_t {
        hipLaunchKernelGGL(operand_kernel, dim3(blocks_for(np * cp, kThreads)), dim3(kThreads), 0, stream, d_tin, d_shifts, su.order,
                           (long long)n, np, (int)units, cp, d_B);
        ++rep.launches;
        return hipGetLastError();
    }));
    MRG_TRY(rep.free_now(d_tin));
    MRG_OK(rep.run_blocks(nullptr, [&](long long s0, long long sb, double* d_w, hipStream_t) -> hipError_t {
        hipLaunchKernelGGL(exp_kernel, dim3(blocks_for(sb * n, kThreads)), dim3(kThreads), 0, stream, d_w, sb * (long long)n);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const long long tiles = (sb + kRepTile - 1) / kRepTile;
        const int sbp = (int)(tiles * kRepTile);
        hipLaunchKernelGGL(product_kernel, dim3((unsigned)slabs, (unsigned)(cp / kColTile), (unsigned)tiles),
                           dim3(kThreads), 0, stream, d_w, d_B, (long long)n, np, cp, (int)sb, sbp, d_part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(finish_kernel, dim3(blocks_for(sb * units, kThreads)), dim3(kThreads), 0, stream, d_part, d_shifts, slabs,
                           cp, (int)sb, sbp, (int)units, s0, d_lpd, d_loo, d_mean, d_var);
        rep.launches += 3;
        return hipGetLastError();
    }, nullptr));
    MRG_TRY(hipMemcpyAsync(lpd, d_lpd, sizeof(double) * su_count, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(loo, d_loo, sizeof(double) * su_count, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(mean, d_mean, sizeof(double) * su_count, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(var, d_var, sizeof(double) * su_count, hipMemcpyDeviceToHost, stream));
    MRG_OK(rep.finish(logz, info));
    rep.report(timing);
    if (timing) {
        timing->columns = 4ll * units + 1;
        timing->threads = kThreads;
        timing->slabs = (int32_t)slabs;
    }
    return RVLL_OK;
}

int check_bounded(const double* v, int64_t count, const char* what)
{
    for (int64_t i = 0; i < count; ++i)
        if (!(std::fabs(v[i]) <= kMaxAbs))                  // NaN fails the comparison too
            return rvll::report_error(RVLL_E_INVALID, "%s %lld is not finite or is beyond 1e30 in size", what, (long long)i);
    return RVLL_OK;
}

}  // namespace

extern "C" int rvll_pointwise_slab_rows(int32_t* rows)
{
    if (!rows) return rvll::report_error(RVLL_E_INVALID, "null argument");
    *rows = kSlabRows;
    return RVLL_OK;
}

extern "C" int rvll_pointwise_replicates(int32_t device, const double* logl, const double* birth, int64_t n_rows,
                                         const int64_t* run_start, int32_t n_runs, const double* table, int32_t n_units,
                                         const double* shifts, int32_t nsamples, int32_t mode, int32_t bootstrap, uint64_t seed,
                                         double* logz, double* info, double* lpd, double* loo, double* mean, double* var,
                                         int64_t block_bytes, rvll_pointwise_timing* timing)
{
    MRG_OK(check_common(logl, birth, n_rows, run_start, n_runs));
    MRG_OK(check_replicate_args(nsamples, mode, bootstrap, n_runs, block_bytes));
    if (n_units < 1 || n_units > kMaxUnits) return rvll::report_error(RVLL_E_INVALID, "n_units must be in [1, %d]", kMaxUnits);
    if (!table || !shifts || !logz || !info || !lpd || !loo || !mean || !var)
        return rvll::report_error(RVLL_E_INVALID, "null argument");
    MRG_OK(check_bounded(table, n_rows * (int64_t)n_units, "table value"));
    MRG_OK(check_bounded(shifts, 3 * (int64_t)n_units, "shift"));
    if (timing) *timing = rvll_pointwise_timing{0., 0., 0., 0., 0., n_rows, 0, 0, 0, kThreads, 0, 0};
    return run_pointwise(device, logl, birth, n_rows, run_start, n_runs, table, n_units, shifts, nsamples,
                         mode == RVLL_SHRINK_EXPECTED ? 1 : 0, bootstrap, seed, logz, info, lpd, loo, mean, var, block_bytes, timing);
}
