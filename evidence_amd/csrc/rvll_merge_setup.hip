// The setup of a merge by birth contours, the replicate kernel, the argument checks and the driver that the merged-run entry
// points share, compiled once for the library (rvll_merge_setup.h declares them).  rvll_merge.hip's header comment describes the
// kernels; DESIGN §4j.
#include "rvll_merge_setup.h"
#include <rocprim/rocprim.hpp>

namespace rvll {
namespace merge {

namespace {

constexpr long long kMaxRows = (1ll << 30) - 1;           // 2N stream positions stay below 2^31
constexpr int kMaxBootRuns = 8192;                        // LDS multiplicities: 32 KiB
constexpr unsigned long long kBootXor = 0x5851F42D4C957F2Dull;
constexpr double kScale = 4611686018427387904.0;          // 2^62

// keys of every row, its index and its run (the last r with run_start[r] <= g)
__global__ __launch_bounds__(kThreads)
void keys_kernel(const double* __restrict__ logl, const double* __restrict__ birth, long long n, const long long* __restrict__ rs,
                 int nruns, u64* __restrict__ kl, u64* __restrict__ kb, int32_t* __restrict__ idx, int32_t* __restrict__ run)
{
    for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < n; g += (long long)gridDim.x * kThreads) {
        const double l = logl[g], b = birth[g];
        kl[g] = rvll::key_of(l);
        kb[g] = rvll::key_of(l <= b ? nextafter(l, -INFINITY) : b);
        idx[g] = (int32_t)g;
        int lo = 0, hi = nruns;
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (rs[mid] <= g) lo = mid; else hi = mid;
        }
        run[g] = lo;
    }
}

// first position in s[0 .. n) whose key is > v (upper) or >= v (lower)
__device__ inline long long upper_bound(const u64* s, long long n, u64 v)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline long long lower_bound(const u64* s, long long n, u64 v)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// per merged row: L, rho, n (unweighted) and its death's place in the stream; per sorted birth: its place
__global__ __launch_bounds__(kThreads)
void place_kernel(const double* __restrict__ logl, const u64* __restrict__ sl, const int32_t* __restrict__ order,
                  const u64* __restrict__ sb, const int32_t* __restrict__ rb, const int32_t* __restrict__ run, long long n,
                  double* __restrict__ L, int32_t* __restrict__ rho, long long* __restrict__ nlive, int32_t* __restrict__ ev)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const int32_t g = order[i];
        L[i] = logl[g];
        rho[i] = run[g];
        const long long cntb = lower_bound(sb, n, sl[i]);     // #{birth < L_i}, >= i + 1
        nlive[i] = cntb - i;
        ev[i + cntb] = (int32_t)i;
        const long long dj = upper_bound(sl, n, sb[i]);       // #{deaths with L <= b_i}: the deaths before birth i
        ev[i + dj] = -1 - rb[i];
    }
}

// (max, sum of exp(w - max), sum of exp(w - max) * L); m = -inf: no row with weight
struct Tri {
    double m, s, a;
};

__device__ __forceinline__ void tri_add(Tri& t, double w, double l)
{
    if (!(w > -INFINITY)) return;
    const double d = w - t.m;
    const double x = exp(-fabs(d));
    const bool up = d > 0.0;
    t.s = up ? t.s * x + 1.0 : t.s + x;
    t.a = up ? t.a * x + l : t.a + x * l;
    t.m = up ? w : t.m;
}

__device__ __forceinline__ Tri tri_join(Tri p, Tri q)
{
    if (!(q.m > -INFINITY)) return p;
    if (!(p.m > -INFINITY)) return q;
    const double mx = fmax(p.m, q.m);
    const double cp = exp(p.m - mx), cq = exp(q.m - mx);
    return Tri{mx, p.s * cp + q.s * cq, p.a * cp + q.a * cq};
}

__device__ Tri tri_reduce(Tri t, Tri* sh)
{
    for (int off = 1; off < kWave; off <<= 1)
        t = tri_join(t, Tri{__shfl_xor(t.m, off, kWave), __shfl_xor(t.s, off, kWave), __shfl_xor(t.a, off, kWave)});
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) sh[wave] = t;
    __syncthreads();
    Tri r = sh[0];
    for (int w = 1; w < kWaves; ++w) r = tri_join(r, sh[w]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kThreads) void replicate_kernel(
    const int32_t* __restrict__ ev, const double* __restrict__ L, const int32_t* __restrict__ rho, long long n, int nruns,
    int s0, u64 seed, int expected, int bootstrap, double* __restrict__ logz, double* __restrict__ info,
    double* __restrict__ logw_out)
{
    extern __shared__ int32_t sh_w[];                     // bootstrap: the multiplicity of every run
    __shared__ long long sh_n[2][kWaves], sh_d[2][kWaves];
    __shared__ double sh_x[2][kWaves];
    __shared__ Tri sh_tri[kWaves];
    __shared__ double sh_lnz;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int s = s0 + (int)blockIdx.x;
    const u64 seed_s = seed + (u64)s * kSeedMul;
    const long long E = 2 * n;
    double* wout = logw_out ? logw_out + (long long)blockIdx.x * n : nullptr;

    if (bootstrap) {
        for (int r = tid; r < nruns; r += kThreads) sh_w[r] = 0;
        __syncthreads();
        const u64 bseed = seed_s ^ kBootXor;
        for (int t = tid; t < nruns; t += kThreads) {
            const int d = (int)fmin(floor(rvll::uniform01(bseed, (u64)t) * (double)nruns), (double)(nruns - 1));
            atomicAdd(&sh_w[d], 1);
        }
        __syncthreads();
    }

    Tri acc{-INFINITY, 0.0, 0.0};
    long long carry_n = 0, carry_d = 0;
    double carry_hi = 0.0, carry_lo = 0.0;               // logX before the tile, as a compensated pair
    int parity = 0;
    for (long long t0 = 0; t0 < E; t0 += kTile, parity ^= 1) {
        const long long e0 = t0 + (long long)tid * kPer;
        int32_t v[kPer];
        int wt[kPer];
        long long sn = 0, sd = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const long long e = e0 + k;
            v[k] = e < E ? ev[e] : INT32_MIN;
            const int r = v[k] >= 0 ? rho[v[k]] : v[k] == INT32_MIN ? -1 : -1 - v[k];
            wt[k] = r < 0 ? 0 : bootstrap ? sh_w[r] : 1;
            if (v[k] >= 0) { sn -= wt[k]; sd += wt[k]; } else sn += wt[k];
        }
        const long long in_n = wave_scan(sn, lane), in_d = wave_scan(sd, lane);
        if (lane == kWave - 1) { sh_n[parity][wave] = in_n; sh_d[parity][wave] = in_d; }
        __syncthreads();
        long long bn = 0, bd = 0, tn = 0, td = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const long long a = sh_n[parity][w], b = sh_d[parity][w];
            if (w < wave) { bn += a; bd += b; }
            tn += a;
            td += b;
        }
        long long nl = carry_n + bn + (in_n - sn), dl = carry_d + bd + (in_d - sd);
        double dt[kPer];
        double xs = 0.0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            dt[k] = 0.0;
            if (v[k] >= 0) {
                for (int q = 0; q < wt[k]; ++q) {
                    const double nn = (double)(nl - q);
                    dt[k] += expected ? -1.0 / nn : log(1.0 - rvll::uniform01(seed_s, (u64)(dl + q))) / nn;
                }
                nl -= wt[k];
                dl += wt[k];
            } else {
                nl += wt[k];
            }
            xs += dt[k];
        }
        carry_n += tn;
        carry_d += td;
        const double in_x = wave_scan(xs, lane);
        if (lane == kWave - 1) sh_x[parity][wave] = in_x;
        __syncthreads();
        double bx = 0.0, tx = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const double a = sh_x[parity][w];
            if (w < wave) bx += a;
            tx += a;
        }
        double loc = bx + (in_x - xs);
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (v[k] >= 0) {
                const double l = L[v[k]];
                const double lx = carry_hi + (carry_lo + loc);
                const double w = wt[k] > 0 ? (l + lx) + log(-expm1(dt[k])) : -INFINITY;
                tri_add(acc, w, l);
                if (wout) wout[v[k]] = w;
            }
            loc += dt[k];
        }
        // two-sum of carry_hi + tx
        const double sum = carry_hi + tx, bv = sum - carry_hi;
        carry_lo += (carry_hi - (sum - bv)) + (tx - bv);
        carry_hi = sum;
    }
    acc = tri_reduce(acc, sh_tri);
    if (tid == 0) {
        const bool any = acc.m > -INFINITY;
        const double lnz = any ? acc.m + log(acc.s) : -INFINITY;
        logz[s] = lnz;
        info[s] = any ? acc.a / acc.s - lnz : 0.0;
        sh_lnz = lnz;
    }
    if (!wout) return;
    __syncthreads();
    const double lnz = sh_lnz;
    for (long long t0 = 0; t0 < E; t0 += kTile)
        for (int k = 0; k < kPer; ++k) {
            const long long e = t0 + (long long)tid * kPer + k;
            if (e < E) {
                const int32_t i = ev[e];
                if (i >= 0) wout[i] -= lnz;
            }
        }
}

// every slot entry becomes m = rint(exp(logwt) 2^62) as int64 in place; msum[replicate] += the sum of its m
__global__ __launch_bounds__(kThreads)
void fixed_kernel(double* __restrict__ w, long long n, unsigned long long* __restrict__ msum)
{
    __shared__ long long sh[kWaves];
    double* slot = w + (long long)blockIdx.y * n;
    long long acc = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double p = exp(slot[i]);
        const long long mi = p > 0.0 ? __double2ll_rn(p * kScale) : 0;    // NaN (a replicate without weight) and 0 give 0
        slot[i] = __longlong_as_double(mi);                               // the integer's bits: the reducers read them as int64
        acc += mi;
    }
    acc = wave_sum(acc);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = sh[0];
        for (int k = 1; k < kWaves; ++k) t += sh[k];
        if (t != 0) atomicAdd(&msum[blockIdx.y], (unsigned long long)t);
    }
}

}  // namespace

hipError_t launch_fixed(double* w, long long n, long long reps, unsigned long long* msum, hipStream_t stream)
{
    hipLaunchKernelGGL(fixed_kernel, dim3((unsigned)std::min<long long>(blocks_for(n, kThreads), 1024), (unsigned)reps),
                       dim3(kThreads), 0, stream, w, n, msum);
    return hipGetLastError();
}

int report_hip(hipError_t e, const char* expr, const char* file, int line)
{
    return rvll::report_error(e == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, "%s failed: %s (%s:%d)", expr,
                              hipGetErrorString(e), file, line);
}

int check_common(const double* logl, const double* birth, int64_t n_rows, const int64_t* run_start, int32_t n_runs)
{
    if (n_runs < 1) return rvll::report_error(RVLL_E_INVALID, "n_runs must be >= 1");
    if (n_rows < 1 || n_rows > kMaxRows) return rvll::report_error(RVLL_E_INVALID, "n_rows must be in [1, %lld]", kMaxRows);
    if (!logl || !birth || !run_start) return rvll::report_error(RVLL_E_INVALID, "null argument");
    if (run_start[0] != 0 || run_start[n_runs] != n_rows)
        return rvll::report_error(RVLL_E_INVALID, "run_start must run from 0 to n_rows = %lld", (long long)n_rows);
    for (int32_t r = 0; r < n_runs; ++r)
        if (run_start[r + 1] < run_start[r])
            return rvll::report_error(RVLL_E_INVALID, "run_start must be non-decreasing (run %d)", (int)r);
    for (int64_t i = 0; i < n_rows; ++i) {
        if (!std::isfinite(logl[i])) return rvll::report_error(RVLL_E_INVALID, "row %lld: log-L is not finite", (long long)i);
        if (std::isnan(birth[i])) return rvll::report_error(RVLL_E_INVALID, "row %lld: NaN birth", (long long)i);
    }
    return RVLL_OK;
}

int check_replicate_args(int32_t nsamples, int32_t mode, int32_t bootstrap, int32_t n_runs, int64_t block_bytes)
{
    if (nsamples < 1) return rvll::report_error(RVLL_E_INVALID, "nsamples must be >= 1");
    if (mode != RVLL_SHRINK_RANDOM && mode != RVLL_SHRINK_EXPECTED)
        return rvll::report_error(RVLL_E_INVALID, "mode %d is neither RVLL_SHRINK_RANDOM nor RVLL_SHRINK_EXPECTED", mode);
    if (bootstrap != 0 && bootstrap != 1) return rvll::report_error(RVLL_E_INVALID, "bootstrap must be 0 or 1");
    if (bootstrap && n_runs > kMaxBootRuns)
        return rvll::report_error(RVLL_E_INVALID, "the run bootstrap takes at most %d runs", kMaxBootRuns);
    if (block_bytes < 0) return rvll::report_error(RVLL_E_INVALID, "negative block_bytes");
    return RVLL_OK;
}

int check_finite_values(const double* values, int64_t n_rows, int32_t n_cols)
{
    for (int64_t i = 0; i < n_rows * (int64_t)n_cols; ++i)
        if (!std::isfinite(values[i]))
            return rvll::report_error(RVLL_E_INVALID, "row %lld, column %lld: value is not finite", (long long)(i / n_cols),
                                      (long long)(i % n_cols));
    return RVLL_OK;
}

hipError_t MergeSetup::query(long long n)
{
    size_t b1 = 0;
    u64* k = nullptr;
    int32_t* o = nullptr;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, b1, k, k, o, o, (unsigned int)n, 0, 64, (hipStream_t) nullptr);
    temp_bytes = std::max<size_t>(b1, 1);
    return e;
}

hipError_t MergeSetup::alloc(Replicates& owner, long long n, int n_runs)
{
    hipError_t e;
#define MRG_SETUP_ALLOC(p, count) if ((e = owner.alloc(p, (size_t)(count))) != hipSuccess) return e
    MRG_SETUP_ALLOC(logl, n);
    MRG_SETUP_ALLOC(birth, n);
    MRG_SETUP_ALLOC(L, n);
    MRG_SETUP_ALLOC(kl, n);
    MRG_SETUP_ALLOC(kb, n);
    MRG_SETUP_ALLOC(sl, n);
    MRG_SETUP_ALLOC(sb, n);
    MRG_SETUP_ALLOC(idx, n);
    MRG_SETUP_ALLOC(order, n);
    MRG_SETUP_ALLOC(run, n);
    MRG_SETUP_ALLOC(rb, n);
    MRG_SETUP_ALLOC(rho, n);
    MRG_SETUP_ALLOC(ev, 2 * n);
    MRG_SETUP_ALLOC(nlive, n);
    MRG_SETUP_ALLOC(rs, n_runs + 1);
    MRG_SETUP_ALLOC(temp, temp_bytes);
#undef MRG_SETUP_ALLOC
    return hipSuccess;
}

hipError_t MergeSetup::upload(const double* h_logl, const double* h_birth, const int64_t* run_start, long long n, int n_runs,
                              hipStream_t stream)
{
    hipError_t e = hipMemcpyAsync(logl, h_logl, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(birth, h_birth, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(rs, run_start, sizeof(long long) * (size_t)(n_runs + 1), hipMemcpyHostToDevice, stream);
}

hipError_t MergeSetup::sort(u64* keys_in, u64* keys_out, int32_t* vals_in, int32_t* vals_out, long long n, hipStream_t stream)
{
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (unsigned int)n, 0, 64, stream);
}

hipError_t MergeSetup::launch(long long n, int n_runs, hipStream_t stream)
{
    hipLaunchKernelGGL(keys_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, logl, birth, n, rs, n_runs, kl, kb,
                       idx, run);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = sort(kl, sl, idx, order, n, stream);
    if (e != hipSuccess) return e;
    e = sort(kb, sb, run, rb, n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(place_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, logl, sl, order, sb, rb, run, n, L,
                       rho, nlive, ev);
    return hipGetLastError();
}

Replicates::Replicates(int32_t device, const double* logl, const double* birth, long long n, const int64_t* run_start, int n_runs,
                       int nsamples, int expected, int bootstrap, uint64_t seed)
    : device(device), logl(logl), birth(birth), n(n), run_start(run_start), n_runs(n_runs), nsamples(nsamples), expected(expected),
      bootstrap(bootstrap), seed(seed), t_start(std::chrono::steady_clock::now())
{
}

Replicates::~Replicates()
{
    for (void* p : owned) (void)hipFree(p);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (prev_device >= 0 && device >= 0) (void)hipSetDevice(prev_device);
}

int Replicates::plan_blocks(int64_t block_bytes, long long default_bound, long long tables, long long per_rep, long long max_reps,
                            const char* tables_name, const char* rep_name, bool with_weights)
{
    weights = with_weights;
    s_blk = std::min<long long>(nsamples, max_reps);
    if (!weights) return RVLL_OK;
    const long long bound = block_bytes > 0 ? block_bytes : default_bound;
    if (tables + per_rep > bound) {
        if (!tables_name)
            return rvll::report_error(RVLL_E_NOMEM, "one replicate of %s needs %lld bytes, above the device block bound of %lld",
                                      rep_name, per_rep, bound);
        return rvll::report_error(RVLL_E_NOMEM, "%s (%lld bytes) and one replicate of %s (%lld bytes) are above the device block "
                                  "bound of %lld", tables_name, tables, rep_name, per_rep, bound);
    }
    s_blk = std::min<long long>(s_blk, (bound - tables) / per_rep);
    return RVLL_OK;
}

int Replicates::begin()
{
    MRG_TRY(su.query(n));
    MRG_TRY(hipGetDevice(&prev_device));
    if (device >= 0) MRG_TRY(hipSetDevice(device));
    MRG_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& e : ev) MRG_TRY(hipEventCreate(&e));
    // every device block before the first launch: running out of memory fails the call before any work
    MRG_TRY(su.alloc(*this, n, n_runs));
    MRG_TRY(alloc(d_logz, (size_t)nsamples));
    MRG_TRY(alloc(d_info, (size_t)nsamples));
    if (weights) MRG_TRY(alloc(d_w, (size_t)(s_blk * n)));
    return RVLL_OK;
}

hipError_t Replicates::alloc_bytes(void** p, size_t bytes)
{
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && *p) owned.push_back(*p);
    return e;
}

hipError_t Replicates::free_bytes(void** p)
{
    owned.erase(std::remove(owned.begin(), owned.end(), *p), owned.end());
    const hipError_t e = hipFree(*p);
    *p = nullptr;
    return e;
}

int Replicates::setup(const std::function<hipError_t()>& own)
{
    MRG_TRY(su.upload(logl, birth, run_start, n, n_runs, stream));
    MRG_TRY(hipEventRecord(ev[0], stream));
    MRG_TRY(su.launch(n, n_runs, stream));
    launches += 4;
    if (own) MRG_TRY(own());
    MRG_TRY(hipEventRecord(ev[1], stream));
    MRG_TRY(hipEventSynchronize(ev[1]));
    float ms = 0.f;
    MRG_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    setup_ms += ms;
    return RVLL_OK;
}

int Replicates::run_blocks(const Step& before, const Step& reduce, const Step& after)
{
    const size_t shmem = bootstrap ? sizeof(int32_t) * (size_t)n_runs : 0;
    for (long long s0 = 0; s0 < nsamples; s0 += s_blk) {
        const long long sb = std::min<long long>(s_blk, nsamples - s0);
        if (before) MRG_TRY(before(s0, sb, d_w, stream));
        MRG_TRY(hipEventRecord(ev[0], stream));
        hipLaunchKernelGGL(replicate_kernel, dim3((unsigned)sb), dim3(kThreads), shmem, stream, su.ev, su.L, su.rho, (long long)n,
                           (int)n_runs, (int)s0, (u64)seed, expected, bootstrap, d_logz, d_info, d_w);
        MRG_TRY(hipGetLastError());
        MRG_TRY(hipEventRecord(ev[1], stream));
        if (reduce) MRG_TRY(reduce(s0, sb, d_w, stream));
        MRG_TRY(hipEventRecord(ev[2], stream));
        if (after) MRG_TRY(after(s0, sb, d_w, stream));
        ++launches;
        ++blocks;
        MRG_TRY(hipStreamSynchronize(stream));
        float ms = 0.f;
        MRG_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        weights_ms += ms;
        MRG_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
        reduce_ms += ms;
    }
    return RVLL_OK;
}

int Replicates::finish(double* logz, double* info)
{
    MRG_TRY(hipMemcpyAsync(logz, d_logz, sizeof(double) * (size_t)nsamples, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipMemcpyAsync(info, d_info, sizeof(double) * (size_t)nsamples, hipMemcpyDeviceToHost, stream));
    MRG_TRY(hipStreamSynchronize(stream));
    return RVLL_OK;
}

double Replicates::elapsed_ms() const
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
}

}  // namespace merge
}  // namespace rvll
