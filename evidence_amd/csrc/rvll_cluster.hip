// rvll_cluster.hip — MLFriends clustering of many independent row sets (rvll_cluster_runs; definition: DESIGN §4e).
//
// Three launches per call, all on rows in HBM:
//   cluster_nn_kernel    per row: the nearest kept row of every bootstrap it is left out of, and the nearest row; their
//                        maxima per run published with a 64-bit atomicMax on the bit pattern (non-negative doubles order as
//                        their bits), so the radius does not depend on scheduling
//   cluster_link_kernel  per pair j > i of a run with d2 <= radius2: union of the two rows in a lock-free union-find (ECL-CC:
//                        the larger root is hooked under the smaller by compare-and-swap), so every root is its component's
//                        smallest row and the partition is unique
//   cluster_label_kernel per run: roots flagged, scanned in row order; a row's label is the scan at its root
//
// Workgroups of the first two own kRowsPerBlock rows of one run (one row per lane, never across a run: the host builds the
// block -> (run, first row) table) and stream the run's rows through LDS in tiles sized from the dimension.  A row's
// coordinates and its bootstrap minima stay in registers: the kernels are instantiated for dimension bounds 8, 16, 32, 64.
// The pair distance is one function for both kernels and separate IEEE operations (the library is built with
// -ffp-contract=off); numpy (evidence_amd/clustering.py) forms the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rvll_kernels.h"
#include "rvll_math.h"

namespace rvll {

namespace {

constexpr int kRowsPerBlock = 64;          // one wave64 per workgroup: its reductions are shuffles
constexpr int kLabelThreads = 256;

// the keep bits of a row: bit b set <=> bit 63 - b of the splitmix64 word uniform01 forms from (seed, index)
__device__ __forceinline__ uint32_t keep_bits(uint64_t seed, uint64_t index, uint32_t bmask)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (index + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return __builtin_bitreverse32((uint32_t)(z >> 32)) & bmask;
}

template <int DM>
__device__ __forceinline__ double pair_d2(const double (&ui)[DM], const double* uj, const double* scale, int D, uint64_t wrapped)
{
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < DM; ++d) {
        if (d < D) {
            double delta = ui[d] - uj[d];
            if ((wrapped >> d) & 1ull) delta = delta - rint(delta);
            const double t = delta * scale[d];
            acc = acc + t * t;
        }
    }
    return acc;
}

// the run's radius2 from its published maxima (slots: kClusterSlots words of the run)
__device__ __forceinline__ double run_radius2(const unsigned long long* slots, long long n, int B)
{
    if (n <= 1) return 0.0;
    const uint32_t bmask = B >= 32 ? 0xFFFFFFFFu : ((1u << B) - 1u);
    const unsigned long long m = slots[33];
    const uint32_t q = (uint32_t)m & (uint32_t)(m >> 32) & bmask;      // bootstraps with a kept row and a left-out row
    if (!q) return __longlong_as_double((long long)slots[32]);
    unsigned long long best = 0;
    for (int b = 0; b < B; ++b)
        if ((q >> b) & 1u) best = slots[b] > best ? slots[b] : best;
    return __longlong_as_double((long long)best);
}

// stage rows j0 .. j0 + cnt of the cube (and optionally their keep bits) in LDS
__device__ __forceinline__ void stage_tile(const double* cube, long long j0, int cnt, int D, double* tile,
                                           uint32_t* kbits, uint64_t seed, long long s, uint32_t bmask)
{
    const double* src = cube + j0 * D;
    for (int e = threadIdx.x; e < cnt * D; e += kRowsPerBlock) tile[e] = src[e];
    if (kbits)
        for (int t = threadIdx.x; t < cnt; t += kRowsPerBlock) kbits[t] = keep_bits(seed, (uint64_t)(j0 + t - s), bmask);
}

template <int DM>
__global__ __launch_bounds__(kRowsPerBlock)
void cluster_nn_kernel(ClusterArgs a)
{
    extern __shared__ double lds[];
    const int D = a.D, TJ = a.tile_rows, B = a.nboot;
    double* s_scale = lds;
    double* tile = lds + D;
    uint32_t* kbits = reinterpret_cast<uint32_t*>(tile + (size_t)TJ * D);
    const int run = a.blocks[2 * blockIdx.x], row0 = a.blocks[2 * blockIdx.x + 1];
    const long long s = a.run_start[run], e = a.run_start[run + 1];
    const uint64_t seed = a.seeds[run];
    const uint32_t bmask = B >= 32 ? 0xFFFFFFFFu : ((1u << B) - 1u);
    const long long i = row0 + threadIdx.x;
    const bool valid = i < e;
    for (int d = threadIdx.x; d < D; d += kRowsPerBlock) s_scale[d] = a.scale[(size_t)run * D + d];
    double ui[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) ui[d] = (valid && d < D) ? a.cube[i * D + d] : 0.0;
    const uint32_t kept = valid ? keep_bits(seed, (uint64_t)(i - s), bmask) : 0u;
    const uint32_t left = valid ? (~kept & bmask) : 0u;
    if (valid) a.parent[i] = (int32_t)i;                  // the union-find of the link launch starts from singletons
    double mins[32];
#pragma unroll
    for (int b = 0; b < 32; ++b) mins[b] = INFINITY;
    double nn = INFINITY, thresh = INFINITY;              // thresh: the largest minimum a pair could still lower
    for (long long j0 = s; j0 < e; j0 += TJ) {
        const int cnt = (int)(e - j0 < TJ ? e - j0 : TJ);
        __syncthreads();
        stage_tile(a.cube, j0, cnt, D, tile, kbits, seed, s, bmask);
        __syncthreads();
        if (!valid) continue;
        for (int t = 0; t < cnt; ++t) {
            const double d2 = pair_d2<DM>(ui, tile + (size_t)t * D, s_scale, D, a.wrapped);
            if (d2 < thresh && j0 + t != i) {
                nn = fmin(nn, d2);
                const uint32_t c = left & kbits[t];
                double th = nn;
#pragma unroll
                for (int b = 0; b < 32; ++b) {
                    if (b < B) {
                        if ((c >> b) & 1u) mins[b] = fmin(mins[b], d2);
                        if ((left >> b) & 1u) th = fmax(th, mins[b]);
                    }
                }
                thresh = th;
            }
        }
    }
    // per run and bootstrap: the largest minimum over the left-out rows (0 where a lane has none: the identity of the max)
    unsigned long long* slots = a.slots + (size_t)run * kClusterSlots;
    const int lane = threadIdx.x;
#pragma unroll
    for (int b = 0; b < 33; ++b) {
        if (b < B || b == 32) {
            double v = 0.0;
            if (b == 32) v = valid ? nn : 0.0;
            else if ((left >> b) & 1u) v = mins[b];
            for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
            if (lane == 0 && v > 0.0) atomicMax(slots + b, (unsigned long long)__double_as_longlong(v));
        }
    }
    uint32_t k_any = kept, l_any = left;
    for (int off = 32; off > 0; off >>= 1) { k_any |= (uint32_t)__shfl_xor((int)k_any, off); l_any |= (uint32_t)__shfl_xor((int)l_any, off); }
    if (lane == 0 && (k_any | l_any)) atomicOr(slots + 33, (unsigned long long)k_any | ((unsigned long long)l_any << 32));
}

// parent words are shared by every workgroup of the link launch: agent-scope atomics, never a plain (L1-cached) access
__device__ __forceinline__ int32_t ld_parent(int32_t* p, long long x)
{
    return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x, halving the path on the way (a non-root's parent only ever moves to one of its ancestors; roots are only
// changed by the compare-and-swap in unite)
__device__ int32_t find_root(int32_t* p, int32_t x)
{
    int32_t cur = ld_parent(p, x);
    if (cur != x) {
        int32_t prev = x, next;
        while (cur > (next = ld_parent(p, cur))) {
            __hip_atomic_store(p + prev, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

__device__ void unite(int32_t* p, int32_t a, int32_t b)
{
    int32_t ra = find_root(p, a), rb = find_root(p, b);
    while (ra != rb) {
        if (ra > rb) { const int32_t t = ra; ra = rb; rb = t; }
        int32_t expected = rb;                           // hook the larger root under the smaller
        if (__hip_atomic_compare_exchange_strong(p + rb, &expected, ra, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        rb = expected;                                   // rb was no root any more: go on from its parent
    }
}

template <int DM>
__global__ __launch_bounds__(kRowsPerBlock)
void cluster_link_kernel(ClusterArgs a)
{
    extern __shared__ double lds[];
    const int D = a.D, TJ = a.tile_rows;
    double* s_scale = lds;
    double* tile = lds + D;
    const int run = a.blocks[2 * blockIdx.x], row0 = a.blocks[2 * blockIdx.x + 1];
    const long long s = a.run_start[run], e = a.run_start[run + 1];
    const double r2 = run_radius2(a.slots + (size_t)run * kClusterSlots, e - s, a.nboot);
    const long long i = row0 + threadIdx.x;
    const bool valid = i < e;
    for (int d = threadIdx.x; d < D; d += kRowsPerBlock) s_scale[d] = a.scale[(size_t)run * D + d];
    double ui[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) ui[d] = (valid && d < D) ? a.cube[i * D + d] : 0.0;
    for (long long j0 = row0; j0 < e; j0 += TJ) {         // pairs j > i only: the tiles from the block's first row on
        const int cnt = (int)(e - j0 < TJ ? e - j0 : TJ);
        __syncthreads();
        stage_tile(a.cube, j0, cnt, D, tile, nullptr, 0, s, 0);
        __syncthreads();
        if (!valid) continue;
        for (int t = 0; t < cnt; ++t) {
            if (j0 + t <= i) continue;
            const double d2 = pair_d2<DM>(ui, tile + (size_t)t * D, s_scale, D, a.wrapped);
            if (d2 <= r2) unite(a.parent, (int32_t)i, (int32_t)(j0 + t));
        }
    }
}

// one workgroup per run: in chunks of rows in order, flag the roots, scan the flags, label the roots, then the others
__global__ __launch_bounds__(kLabelThreads)
void cluster_label_kernel(ClusterArgs a)
{
    __shared__ int wave_count[kLabelThreads / 64];
    const int run = blockIdx.x;
    const long long s = a.run_start[run], e = a.run_start[run + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int base = 0;
    for (long long c0 = s; c0 < e; c0 += kLabelThreads) {
        const long long i = c0 + threadIdx.x;
        const bool valid = i < e;
        int32_t root = -1;
        if (valid) {                                     // the forest is final: plain loads
            root = a.parent[i];
            while (a.parent[root] != root) root = a.parent[root];
        }
        const bool flag = valid && root == (int32_t)i;
        const unsigned long long bal = __ballot(flag);
        if (lane == 0) wave_count[w] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < kLabelThreads / 64; ++k) { before += k < w ? wave_count[k] : 0; total += wave_count[k]; }
        if (flag) a.labels[i] = base + before + __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();                                 // every root's label is written (a root is never after its rows)
        if (valid && !flag) a.labels[i] = a.labels[root];
        base += total;
    }
    if (threadIdx.x == 0) {
        a.nclusters[run] = base;
        a.radius2[run] = run_radius2(a.slots + (size_t)run * kClusterSlots, e - s, a.nboot);
    }
}

template <int DM>
hipError_t launch_dm(const ClusterArgs& a, hipStream_t stream)
{
    const size_t lds = cluster_lds_bytes(a.D, a.tile_rows);
    if (a.nblocks > 0) {
        hipLaunchKernelGGL(cluster_nn_kernel<DM>, dim3((unsigned)a.nblocks), dim3(kRowsPerBlock), lds, stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(cluster_link_kernel<DM>, dim3((unsigned)a.nblocks), dim3(kRowsPerBlock), lds, stream, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cluster_label_kernel, dim3((unsigned)a.R), dim3(kLabelThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

size_t cluster_lds_bytes(int D, int tile_rows)
{
    return sizeof(double) * (size_t)D + (sizeof(double) * (size_t)D + sizeof(uint32_t)) * (size_t)tile_rows;
}

int cluster_tile_rows(int D)
{
    const int t = (int)(kClusterTileBytes / (sizeof(double) * (size_t)(D > 0 ? D : 1)));
    return t < 16 ? 16 : (t > 256 ? 256 : t);
}

hipError_t launch_cluster(const ClusterArgs& a, hipStream_t stream)
{
    if (a.R <= 0) return hipSuccess;
    if (a.D <= 8) return launch_dm<8>(a, stream);
    if (a.D <= 16) return launch_dm<16>(a, stream);
    if (a.D <= 32) return launch_dm<32>(a, stream);
    if (a.D <= kClusterMaxDims) return launch_dm<64>(a, stream);
    return hipErrorInvalidValue;
}

}  // namespace rvll
