// rvll_api.hip — host side of the C-ABI declared in include/rvll.h.
//
// One handle = one device + its streams (compute = pipeline lane 0, further lanes for the multi-GPU step, one
// for the scalar-call server) + resident epoch table, layout, prior tables and batch buffers.  No PyTorch, no
// other runtime: plain HIP, and RCCL (loaded lazily with dlopen) for the multi-GPU all-gathers.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include <unordered_map>

#include "rvll_host.h"      // the handle, HIP_TRY, what the other host units share

namespace {

thread_local std::string g_last_error;

int vfail(int code, const char* fmt, va_list ap)
{
    char buf[1024];
    vsnprintf(buf, sizeof buf, fmt, ap);
    g_last_error = buf;
    return code;
}

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    code = vfail(code, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace

// error reporting for the other translation units of the library (rvll_fip.hip)
namespace rvll {
int report_error(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    code = vfail(code, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace rvll

using rvll::host::dev_free;

namespace {

hipStream_t lane_stream(const rvll_handle* h, int lane) { return h->lanes[lane]; }

int sync_other_lanes(rvll_handle* h)
{
    for (int l = 1; l < kMaxLanes; ++l)
        if (h->lanes[l]) HIP_TRY(hipStreamSynchronize(h->lanes[l]));
    return RVLL_OK;
}

// A request goes out as the legacy word (models of more than kServerSlotDims parameters: the kernel polls it, then fetches theta) AND
// through the slots (rvll_kernels.h, ServerCtl::in): every value, then beside every value the word keyed with that value — a slot
// read torn or early does not decode to the request, so nothing rests on store order or on how the link splits a read.
void server_post(rvll_handle* h, unsigned long long request, const double* row)
{
    rvll::ServerCtl* c = h->srv;
    const int D = h->L.ndim;
    if (row) memcpy(c->theta, row, sizeof(double) * (size_t)D);
    if (D <= rvll::kServerSlotDims) {
        if (row) for (int i = 0; i < D; ++i) c->in[i].v = row[i];
        __atomic_thread_fence(__ATOMIC_RELEASE);
        for (int i = 0; i < D; ++i) {                                   // the word of a slot is keyed with the slot's value (ServerCtl)
            unsigned long long vb;
            memcpy(&vb, &c->in[i].v, sizeof vb);
            __atomic_store_n(&c->in[i].word, request ^ rvll::ServerCtl::slot_key(vb), __ATOMIC_RELAXED);
        }
    }
    __atomic_store_n(&c->request, request, __ATOMIC_RELEASE);
}

// Ask a running scalar-call server to leave and wait for it.  Every entry point other than the scalar call
// itself goes through use_device(), so the persistent kernel never coexists with allocations, frees or
// collectives of its own handle (hipFree and friends synchronise the whole device).
int server_stop(rvll_handle* h)
{
    if (!h->srv_running || h->srv_dead) return RVLL_OK;
    const unsigned long long request = ((unsigned long long)rvll::kServerQuit << 32) | (unsigned)++h->srv_seq;
    server_post(h, request, nullptr);
    hipError_t e = hipStreamSynchronize(h->srv_stream);
    h->srv_last = request;
    h->srv_running = false;
    if (e != hipSuccess) return fail(RVLL_E_HIP, "scalar server did not stop: %s", hipGetErrorString(e));
    return RVLL_OK;
}

int resolve_fused(rvll_handle* h);

int use_device(rvll_handle* h)
{
    if (!h) return fail(RVLL_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    int rc = server_stop(h);
    if (rc) return rc;
    return h->fused_pending ? resolve_fused(h) : RVLL_OK;
}

bool slot_ok(const rvll_slot& s, int D) { return s.idx < D; }

int validate_layout(const rvll_layout* L)
{
    if (!L) return fail(RVLL_E_INVALID, "layout is null");
    if (L->struct_size != (int32_t)sizeof(rvll_layout))
        return fail(RVLL_E_INVALID, "rvll_layout.struct_size %d != %zu (ABI mismatch)",
                    L->struct_size, sizeof(rvll_layout));
    if (L->ndim < 0 || L->nplanets < 0 || L->ninst < 1 || L->nlinpar < 0)
        return fail(RVLL_E_INVALID, "layout counts out of range (ndim %d, nplanets %d, ninst %d, nlinpar %d)",
                    L->ndim, L->nplanets, L->ninst, L->nlinpar);
    if (L->nplanets > 0 && !L->planets) return fail(RVLL_E_INVALID, "planets pointer is null");
    if (!L->insts) return fail(RVLL_E_INVALID, "insts pointer is null");
    if (L->nlinpar > 0 && !L->linpar) return fail(RVLL_E_INVALID, "linpar pointer is null");
    if (L->precision < RVLL_PREC_FP64 || L->precision > RVLL_PREC_FP32)
        return fail(RVLL_E_INVALID, "unknown precision %d", L->precision);
    if (!(L->tol > 0.) || L->itmax < 1) return fail(RVLL_E_INVALID, "tol/itmax out of range");
    const int D = L->ndim;
    for (int i = 0; i < L->nplanets; ++i) {
        const rvll_planet& p = L->planets[i];
        if (!slot_ok(p.k, D) || !slot_ok(p.p, D) || !slot_ok(p.e1, D) || !slot_ok(p.e2, D) ||
            !slot_ok(p.anom, D) || !slot_ok(p.epoch, D))
            return fail(RVLL_E_INVALID, "planet %d: slot index >= ndim", i + 1);
        if (p.k_kind < 0 || p.k_kind > 1 || p.p_kind < 0 || p.p_kind > 1 || p.ecc_kind < 0 ||
            p.ecc_kind > 2 || p.anom_kind < 0 || p.anom_kind > 1)
            return fail(RVLL_E_INVALID, "planet %d: bad parametrisation enum", i + 1);
    }
    for (int i = 0; i < L->ninst; ++i)
        if (!slot_ok(L->insts[i].offset, D) || (L->has_jitter && !slot_ok(L->insts[i].jitter, D)))
            return fail(RVLL_E_INVALID, "instrument %d: slot index >= ndim", i);
    for (int i = 0; i < 4; ++i)
        if (!slot_ok(L->drift[i], D)) return fail(RVLL_E_INVALID, "drift slot index >= ndim");
    if (!slot_ok(L->tref, D)) return fail(RVLL_E_INVALID, "tref slot index >= ndim");
    for (int i = 0; i < L->nlinpar; ++i)
        if (!slot_ok(L->linpar[i], D)) return fail(RVLL_E_INVALID, "linpar slot index >= ndim");
    return RVLL_OK;
}

// Launch geometry: how many live points one 256-thread workgroup takes.
//
// A workgroup puts one wave on each SIMD of its CU and walks ceil(PB*Ne/256) rounds of
// flattened (point, epoch) items; workgroups are dealt round-robin over the CUs.  The
// fp64 pipes are issue-bound, so a CU's time ~ (workgroups it receives) x (rounds each),
// mildly worse when fewer than ~3 waves per SIMD are resident to hide latency.  Pick the
// PB that minimises that, subject to the LDS carve fitting.
size_t lds_bytes_for(const rvll_handle* h, int pb)
{
    rvll::LoglikeArgs a{};
    a.PB = pb; a.D = h->L.ndim; a.Np = h->L.nplanets; a.Ni = h->L.ninst; a.nlin = h->L.nlinpar;
    a.CH = std::min(h->chunk_items, std::max(rvll::kThreads, pb * h->Ne));
    a.CH = (a.CH + 1) & ~1;
    return rvll::loglike_lds_bytes(a);
}

int choose_points_per_block(rvll_handle* h, long long B)
{
    if (h->pb_override > 0) return std::min(h->pb_override, rvll::kMaxPointsPerBlock);
    { auto it = h->geo.find(B); if (it != h->geo.end()) return it->second; }
    // Cost model fitted to the MI355X sweeps in profiles/r01_sweep_configs.txt.  A workgroup costs its CU
    // W = ceil(PB*Ne/64)/4 wave-rounds per SIMD (a partly filled last round only occupies the waves that
    // have items), plus ~0.6 for staging, decode, barriers and the reduction, plus ~0.5 per extra LDS
    // window when PB*Ne exceeds it.  Workgroups are dealt round-robin and run in residency rounds of
    // up to `occ` per CU; a round with fewer than 4 workgroups per CU hides latency worse; and the
    // kernel ends with a tail of about half of one workgroup's duration (step-count imbalance), which
    // favours more, shorter workgroups.
    const int Ne = h->Ne;
    int best = 1;
    double best_cost = 1e300;
    for (int pb = 1; pb <= rvll::kMaxPointsPerBlock; ++pb) {
        if ((long long)pb > std::max(1LL, B)) break;
        const size_t lds = lds_bytes_for(h, pb);
        if (pb > 1 && lds > 60 * 1024) break;
        const long long items = (long long)pb * Ne;
        // LDS windows hold whole points (or, beyond the window size, slices of one point)
        const double chunks = Ne <= h->chunk_items ? std::ceil((double)pb / (h->chunk_items / Ne))
                                                   : (double)pb * std::ceil((double)Ne / h->chunk_items);
        const double W = (double)((items + rvll::kWave - 1) / rvll::kWave) / 4.0 + 0.6 + 0.5 * (chunks - 1.0);
        const double blocks = std::ceil((double)B / pb);
        int occ;
        { auto it = h->occ_by_lds.find(lds);
          if (it != h->occ_by_lds.end()) occ = it->second;
          else { occ = rvll::loglike_blocks_per_cu(lds); h->occ_by_lds[lds] = occ; } }
        // with two launches in flight (pipeline lanes) the next launch fills the tail, so the tail term drops out
        double remaining = std::ceil(blocks / h->n_cu), cost = h->pipelined ? 0.0 : 0.5 * W;
        while (remaining > 0) {
            const double k = std::min((double)occ, remaining);
            const double pen = k >= 4 ? 1.0 : k >= 3 ? 1.08 : k >= 2 ? 1.25 : 1.6;
            cost += k * W * pen;
            remaining -= k;
        }
        if (cost < best_cost * (1.0 - 1e-9)) { best_cost = cost; best = pb; }
    }
    if (h->geo.size() > 64) h->geo.clear();
    h->geo[B] = best;
    return best;
}

// The CU-wide form (rvll_kernels.hip, loglike_cu_kernel): 1024-thread workgroups, one per CU at a time, each taking
// a tile of PB points whose items all sit in LDS.  Measured against the 256-thread tiles over batch sizes
// (profiles/r02_form_sweep.txt): 7-14 % faster whenever the batch is one to four rounds of tiles over the CUs —
// every CU stays full until its last wave round — down to a few wave rounds per CU; with many rounds per CU the
// tile form wins by 2-7 %, because a CU-filling workgroup's prologue and reduction (~5 us per tile) overlap
// nothing, while four independent workgroups per CU hide each other's.  The tile size is the largest that fits
// the LDS budget, lowered so that the number of tiles is a whole number of rounds over the CUs.
// Returns the grid (0: use the tile form) and sets a->PB / a->CH.
int choose_cu_form(rvll_handle* h, long long B, rvll::LoglikeArgs* a)
{
    if (h->form_override == 1 || h->pb_override > 0) return 0;
    const bool forced = h->form_override == 2;
    // two launches in flight (pipeline lanes): the next launch's tiles backfill every freed slot, which is all the
    // CU-wide form buys, and the 256-thread tiles hide their prologues behind each other (2.71 vs 2.59e8 evals/s)
    if (h->pipelined && !forced) return 0;
    const long long wave_rounds_per_cu = B * h->Ne / rvll::kWave / std::max(1, h->n_cu);
    if (!forced && wave_rounds_per_cu < 8) return 0;
    const long long ncu = std::min<long long>(h->n_cu, B);
    const long long ppc = (B + ncu - 1) / ncu;                      // points per CU
    rvll::LoglikeArgs t = *a;
    auto fits = [&](int pb) {
        t.PB = pb; t.CH = (pb * h->Ne + 1) & ~1;
        return rvll::loglike_lds_bytes(t) <= rvll::kCuLdsBudget;
    };
    int pbmax = (int)std::min<long long>(rvll::kCuMaxPoints, ppc);
    while (pbmax >= 1 && !fits(pbmax)) --pbmax;
    if (pbmax < 1) return 0;
    const long long rounds = (ppc + pbmax - 1) / pbmax;             // tiles per CU
    if (!forced && rounds > 4) return 0;
    const int pb = (int)((B + ncu * rounds - 1) / (ncu * rounds));
    if (!forced && rounds > 1) {
        // several tiles per CU: each one's ~5 us of prologue + reduction is exposed, so the tile has to be long —
        // wave rounds per wave x (0.9 + 1.33 Np) us per round (fitted to the sweep) — for the form to pay
        const double t_tile_us = (double)pb * h->Ne / rvll::kWave / (rvll::kCuThreads / rvll::kWave) * (0.9 + 1.33 * h->L.nplanets);
        if (t_tile_us < 40.0) return 0;
    }
    a->PB = pb;
    a->CH = (pb * h->Ne + 1) & ~1;
    return (int)((B + pb - 1) / pb);
}

int build_args(rvll_handle* h, const double* d_theta, double* d_logL, int32_t* d_flags,
               long long B, rvll::LoglikeArgs* out, int* cu_grid = nullptr)
{
    rvll::LoglikeArgs a{};
    a.layblob = h->d_layblob;
    a.theta = d_theta; a.logL = d_logL; a.flags = d_flags; a.B = B;
    a.t = h->d_t; a.y = h->d_y; a.s2 = h->d_s2; a.inst = h->d_inst; a.linpar = h->d_linpar;
    a.Ne = h->Ne;
    a.planets = h->d_planets; a.insts = h->d_insts; a.linslots = h->d_linslots;
    a.D = h->L.ndim; a.Np = h->L.nplanets; a.Ni = h->L.ninst; a.nlin = h->L.nlinpar;
    a.has_jitter = h->L.has_jitter; a.has_drift = h->L.has_drift;
    a.tref_from_data = h->L.tref_from_data;
    a.tol = h->L.tol; a.itmax = h->L.itmax; a.precision = h->L.precision;
    a.cr_redo = h->wander_exact;
    a.PB = choose_points_per_block(h, B);
    a.CH = std::min(h->chunk_items, std::max(rvll::kThreads, a.PB * h->Ne));
    a.CH = (a.CH + 1) & ~1;
    a.cte = h->cte;
    a.tmin = h->tmin; a.tmax = h->tmax;
    if (cu_grid) {
        *cu_grid = choose_cu_form(h, B, &a);
        if (*cu_grid > 0) { *out = a; return RVLL_OK; }
    }
    // shrink PB until the LDS carve fits the 64 KiB default dynamic limit
    while (a.PB > 1 && rvll::loglike_lds_bytes(a) > 60 * 1024) {
        a.PB -= 1;
        a.CH = std::min(h->chunk_items, std::max(rvll::kThreads, a.PB * h->Ne));
        a.CH = (a.CH + 1) & ~1;
    }
    if (rvll::loglike_lds_bytes(a) > 64 * 1024)
        return fail(RVLL_E_UNSUPPORTED, "per-point state (%d parameters, %d planets) exceeds the LDS budget",
                    a.D, a.Np);
    *out = a;
    return RVLL_OK;
}

hipError_t launch_form(const rvll::LoglikeArgs& a, int cu_grid, hipStream_t stream)
{
    return cu_grid > 0 ? rvll::launch_loglike_cu(a, cu_grid, stream) : rvll::launch_loglike(a, stream);
}

// fused cube -> theta -> log-L launch: the same arguments plus the prior table and the two row buffers
void make_fused(const rvll_handle* h, const double* d_cube, double* d_theta_out, rvll::LoglikeArgs* a)
{
    a->cube = d_cube;
    a->theta_out = d_theta_out;
    a->priors = h->d_priors;
    a->heavy_dims = h->d_heavy;
    a->n_heavy = h->n_heavy;
    a->light_dims = h->d_heavy + h->n_heavy;
    a->defer = h->pin_defer_dev;
    a->slim_umax = h->slim_umax;
}

int ensure_capacity(rvll_handle* h, long long B)
{
    if (B <= h->cap) return RVLL_OK;
    long long cap = std::max<long long>(B, 1024);
    { int rc_ = sync_other_lanes(h); if (rc_) return rc_; }
    if (h->compute) HIP_TRY(hipStreamSynchronize(h->compute));
    dev_free(h->d_theta); dev_free(h->d_cube);
    for (int l = 0; l < kMaxLanes; ++l) { dev_free(h->d_logL2[l]); dev_free(h->d_flags2[l]); }
    h->cap = 0;
    const size_t D = (size_t)std::max(1, h->L.ndim);
    HIP_TRY(hipMalloc(&h->d_theta, sizeof(double) * D * (size_t)cap));
    HIP_TRY(hipMalloc(&h->d_cube,  sizeof(double) * D * (size_t)cap));
    for (int l = 0; l < kMaxLanes; ++l) {
        HIP_TRY(hipMalloc(&h->d_logL2[l], sizeof(double) * (size_t)cap));
        HIP_TRY(hipMalloc(&h->d_flags2[l], sizeof(int32_t) * (size_t)cap));
    }
    h->cap = cap;
    return RVLL_OK;
}

void free_priors(rvll_handle* h)
{
    for (double*& p : h->d_tables) dev_free(p);
    h->d_tables.clear();
    h->table_err.clear();
    h->table_direct.clear();
    dev_free(h->d_priors);
    dev_free(h->d_heavy);
    h->n_heavy = 0;
    h->all_direct = true;
    h->have_priors = false;
}

}  // namespace

extern "C" {

const char* rvll_last_error(void) { return g_last_error.c_str(); }

int rvll_version(int32_t* major, int32_t* minor)
{
    if (major) *major = RVLL_VERSION_MAJOR;
    if (minor) *minor = RVLL_VERSION_MINOR;
    return RVLL_OK;
}

int rvll_device_count(int32_t* count)
{
    if (!count) return fail(RVLL_E_INVALID, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(RVLL_E_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return RVLL_OK;
}

int rvll_device_name(int32_t device, char* buf, int32_t buflen)
{
    if (!buf || buflen < 1) return fail(RVLL_E_INVALID, "bad buffer");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    snprintf(buf, (size_t)buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return RVLL_OK;
}

int rvll_create(const rvll_layout* layout, const double* time, const double* vrad,
                const double* svrad, const int32_t* inst, int32_t n_epochs,
                const double* linpar_series, int32_t device, rvll_handle** out)
{
    if (!out) return fail(RVLL_E_INVALID, "out is null");
    *out = nullptr;
    int rc = validate_layout(layout);
    if (rc) return rc;
    if (!time || !vrad || !svrad || !inst || n_epochs < 1)
        return fail(RVLL_E_INVALID, "epoch table is empty or null");
    if (layout->nlinpar > 0 && !linpar_series)
        return fail(RVLL_E_INVALID, "nlinpar > 0 but linpar_series is null");
    for (int j = 0; j < n_epochs; ++j)
        if (inst[j] < 0 || inst[j] >= layout->ninst)
            return fail(RVLL_E_INVALID, "inst[%d] = %d outside [0, %d)", j, inst[j], layout->ninst);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(RVLL_E_NODEVICE, "no HIP device available (%s); rvll has no CPU path",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return fail(RVLL_E_NODEVICE, "device %d >= device count %d", device, ndev);

    rvll_handle* h = new (std::nothrow) rvll_handle;
    if (!h) return fail(RVLL_E_NOMEM, "out of host memory");
    h->device = device;
    h->L = *layout;
    h->planets.assign(layout->planets, layout->planets + layout->nplanets);
    h->insts.assign(layout->insts, layout->insts + layout->ninst);
    if (layout->nlinpar) h->linslots.assign(layout->linpar, layout->linpar + layout->nlinpar);
    h->L.planets = h->planets.data();
    h->L.insts = h->insts.data();
    h->L.linpar = h->linslots.data();
    h->Ne = n_epochs;
    h->cte = -0.5 * (double)n_epochs * std::log(2 * M_PI);          // rvmodel:77-78
    h->tmin = h->tmax = time[0];
    for (int j = 1; j < n_epochs; ++j) { h->tmin = std::min(h->tmin, time[j]); h->tmax = std::max(h->tmax, time[j]); }

#define CREATE_TRY(expr)                                                             \
    do {                                                                             \
        hipError_t e2_ = (expr);                                                     \
        if (e2_ != hipSuccess) {                                                     \
            int c_ = fail(e2_ == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP,    \
                          "%s failed: %s", #expr, hipGetErrorString(e2_));           \
            rvll_destroy(h);                                                         \
            return c_;                                                               \
        }                                                                            \
    } while (0)

    CREATE_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    CREATE_TRY(hipGetDeviceProperties(&prop, device));
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    CREATE_TRY(hipStreamCreateWithFlags(&h->compute, hipStreamNonBlocking));
    h->lanes[0] = h->compute;
    for (int l = 1; l < kMaxLanes; ++l) CREATE_TRY(hipStreamCreateWithFlags(&h->lanes[l], hipStreamNonBlocking));
    if (const char* e = getenv("RVLL_LANES")) h->nlanes_dev = std::max(1, std::min(kMaxLanes, atoi(e)));
    if (const char* e = getenv("RVLL_WANDER_EXACT")) h->wander_exact = atoi(e) != 0;
    CREATE_TRY(hipHostMalloc(&h->pin_in, rvll_handle::kPinBytes, hipHostMallocMapped));
    CREATE_TRY(hipHostMalloc(&h->pin_out, rvll_handle::kPinBytes, hipHostMallocMapped));
    CREATE_TRY(hipHostGetDevicePointer(&h->pin_in_dev, h->pin_in, 0));
    CREATE_TRY(hipHostGetDevicePointer(&h->pin_out_dev, h->pin_out, 0));
    {
        void *p = nullptr, *pd = nullptr;
        CREATE_TRY(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent));
        CREATE_TRY(hipHostGetDevicePointer(&pd, p, 0));
        h->pin_defer = static_cast<int*>(p);
        h->pin_defer_dev = static_cast<int*>(pd);
        *h->pin_defer = 0;
        h->slim_umax = rvll::prior_table_umax();
    }
    {
        void* p = nullptr;
        CREATE_TRY(hipHostMalloc(&p, sizeof(rvll::ServerCtl), hipHostMallocMapped | hipHostMallocCoherent));
        h->srv = new (p) rvll::ServerCtl();
        void* pd = nullptr;
        CREATE_TRY(hipHostGetDevicePointer(&pd, p, 0));
        h->srv_dev = static_cast<rvll::ServerCtl*>(pd);
        CREATE_TRY(hipStreamCreateWithFlags(&h->srv_stream, hipStreamNonBlocking));
        CREATE_TRY(hipMalloc(&h->d_srv_out, 2 * sizeof(double)));
        // the env switch obeys the same limit as rvll_scalar_server(): the control block holds kServerMaxDim parameters
        if (const char* e = getenv("RVLL_SCALAR_SERVER")) h->srv_enabled = atoi(e) != 0 && layout->ndim <= rvll::kServerMaxDim;
    }

    const size_t nb = sizeof(double) * (size_t)n_epochs;
    std::vector<double> s2((size_t)n_epochs);
    for (int j = 0; j < n_epochs; ++j) s2[j] = svrad[j] * svrad[j];  // rvmodel:190,192
    CREATE_TRY(hipMalloc(&h->d_t, nb));
    CREATE_TRY(hipMalloc(&h->d_y, nb));
    CREATE_TRY(hipMalloc(&h->d_s2, nb));
    CREATE_TRY(hipMalloc(&h->d_inst, sizeof(int32_t) * (size_t)n_epochs));
    CREATE_TRY(hipMemcpy(h->d_t, time, nb, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(h->d_y, vrad, nb, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(h->d_s2, s2.data(), nb, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(h->d_inst, inst, sizeof(int32_t) * (size_t)n_epochs, hipMemcpyHostToDevice));
    if (layout->nlinpar) {
        CREATE_TRY(hipMalloc(&h->d_linpar, nb * (size_t)layout->nlinpar));
        CREATE_TRY(hipMemcpy(h->d_linpar, linpar_series, nb * (size_t)layout->nlinpar, hipMemcpyHostToDevice));
        CREATE_TRY(hipMalloc(&h->d_linslots, sizeof(rvll_slot) * (size_t)layout->nlinpar));
        CREATE_TRY(hipMemcpy(h->d_linslots, h->linslots.data(), sizeof(rvll_slot) * (size_t)layout->nlinpar, hipMemcpyHostToDevice));
    }
    if (layout->nplanets) {
        CREATE_TRY(hipMalloc(&h->d_planets, sizeof(rvll_planet) * (size_t)layout->nplanets));
        CREATE_TRY(hipMemcpy(h->d_planets, h->planets.data(), sizeof(rvll_planet) * (size_t)layout->nplanets, hipMemcpyHostToDevice));
    }
    CREATE_TRY(hipMalloc(&h->d_insts, sizeof(rvll_inst) * (size_t)layout->ninst));
    CREATE_TRY(hipMemcpy(h->d_insts, h->insts.data(), sizeof(rvll_inst) * (size_t)layout->ninst, hipMemcpyHostToDevice));
    {
        std::vector<char> blob;
        auto append = [&](const void* p, size_t n) { const char* c = static_cast<const char*>(p); blob.insert(blob.end(), c, c + n); };
        append(h->planets.data(), sizeof(rvll_planet) * h->planets.size());
        append(h->insts.data(), sizeof(rvll_inst) * h->insts.size());
        append(h->linslots.data(), sizeof(rvll_slot) * h->linslots.size());
        append(h->L.drift, sizeof(rvll_slot) * 4);
        append(&h->L.tref, sizeof(rvll_slot));
        CREATE_TRY(hipMalloc(&h->d_layblob, std::max<size_t>(blob.size(), 8)));
        if (!blob.empty()) CREATE_TRY(hipMemcpy(h->d_layblob, blob.data(), blob.size(), hipMemcpyHostToDevice));
    }
    if (const char* e = getenv("RVLL_FORM")) h->form_override = !strcmp(e, "tile") ? 1 : !strcmp(e, "cu") ? 2 : 0;
#undef CREATE_TRY
    *out = h;
    return RVLL_OK;
}

int rvll_destroy(rvll_handle* h)
{
    if (!h) return RVLL_OK;
    (void)hipSetDevice(h->device);
    if (h->srv) (void)server_stop(h);
    if (h->compute) (void)hipStreamSynchronize(h->compute);
    (void)sync_other_lanes(h);
    rvll::host::comm_release(h);
    free_priors(h);
    dev_free(h->d_theta); dev_free(h->d_cube);
    for (int l = 0; l < kMaxLanes; ++l) { dev_free(h->d_logL2[l]); dev_free(h->d_flags2[l]); dev_free(h->d_gather2[l]); }
    dev_free(h->d_gather_theta); dev_free(h->d_gather_host_in); dev_free(h->d_gather_host_out);
    dev_free(h->d_live_u); dev_free(h->d_live_theta); dev_free(h->d_live_logl); dev_free(h->d_live_birth); dev_free(h->d_live_idx); dev_free(h->d_live_mom);
    dev_free(h->d_sort_keys); dev_free(h->d_sort_rows); dev_free(h->d_sort_temp);
    dev_free(h->d_cl_in); dev_free(h->d_cl_work); dev_free(h->d_cl_out); dev_free(h->d_adapt); dev_free(h->d_adapt_in); dev_free(h->d_region); dev_free(h->d_cel);
    if (h->d_clseg) { (void)hipFree(h->d_clseg); h->d_clseg = nullptr; }
    dev_free(h->d_dead_theta); dev_free(h->d_dead_logl); dev_free(h->d_dead_birth); dev_free(h->d_runs_idx); dev_free(h->d_runs_mom);
    if (h->pin_in) (void)hipHostFree(h->pin_in);
    if (h->pin_out) (void)hipHostFree(h->pin_out);
    if (h->pin_defer) (void)hipHostFree(h->pin_defer);
    rvll::host::stream_free(h);
    dev_free(h->d_walk_steps); dev_free(h->d_walk_wid); dev_free(h->d_walk_start); dev_free(h->d_walk_cost); dev_free(h->d_walk_order); dev_free(h->d_walk_wflag);
    dev_free(h->d_walk_basis);
    dev_free(h->d_rounds); dev_free(h->d_walk_dirs);
    dev_free(h->d_walk_run); dev_free(h->d_run_lstar); dev_free(h->d_run_seed); dev_free(h->d_run_chol); dev_free(h->d_run_nsteps);
    if (h->pin_rounds) (void)hipHostFree(h->pin_rounds);
    if (h->ev_rounds) (void)hipEventDestroy(h->ev_rounds);
    for (auto& s : h->rounds_streams) if (s) (void)hipStreamDestroy(s);
    for (auto& e : h->ev_chain) if (e) (void)hipEventDestroy(e);
    for (auto& e : h->marks) if (e) (void)hipEventDestroy(e);
    if (h->srv_stream) (void)hipStreamDestroy(h->srv_stream);
    if (h->srv) (void)hipHostFree(h->srv);
    dev_free(h->d_srv_out);
    dev_free(h->d_walk_u); dev_free(h->d_walk_theta); dev_free(h->d_walk_logl); dev_free(h->d_walk_chol);
    dev_free(h->d_walk_wrapped); dev_free(h->d_walk_ncalls);
    dev_free(h->d_t); dev_free(h->d_y); dev_free(h->d_s2); dev_free(h->d_inst); dev_free(h->d_linpar);
    dev_free(h->d_planets); dev_free(h->d_insts); dev_free(h->d_linslots); dev_free(h->d_layblob);
    for (int l = 1; l < kMaxLanes; ++l) if (h->lanes[l]) (void)hipStreamDestroy(h->lanes[l]);
    if (h->compute) (void)hipStreamDestroy(h->compute);
    delete h;
    return RVLL_OK;
}

int rvll_set_points_per_block(rvll_handle* h, int32_t points_per_block)
{
    if (!h) return fail(RVLL_E_INVALID, "null handle");
    if (points_per_block > rvll::kMaxPointsPerBlock)
        return fail(RVLL_E_INVALID, "points_per_block > %d", rvll::kMaxPointsPerBlock);
    h->pb_override = points_per_block > 0 ? points_per_block : 0;
    return RVLL_OK;
}

int rvll_set_kernel_form(rvll_handle* h, int32_t form)
{
    if (!h) return fail(RVLL_E_INVALID, "null handle");
    if (form < 0 || form > 2) return fail(RVLL_E_INVALID, "form must be 0 (auto), 1 (tile) or 2 (CU-wide)");
    h->form_override = form;
    return RVLL_OK;
}

// ---- priors -------------------------------------------------------------------
int rvll_set_priors(rvll_handle* h, const rvll_prior* priors, int32_t ndim)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (!priors || ndim != h->L.ndim)
        return fail(RVLL_E_INVALID, "set_priors: ndim %d != layout ndim %d (or priors null)", ndim, h->L.ndim);
    for (int d = 0; d < ndim; ++d) {
        const rvll_prior& p = priors[d];
        switch (p.kind) {
        case RVLL_PRIOR_UNIFORM: case RVLL_PRIOR_JEFFREYS: case RVLL_PRIOR_MODJEFFREYS:
        case RVLL_PRIOR_UNIFORMFREQUENCY: case RVLL_PRIOR_NORMAL: case RVLL_PRIOR_LOGNORMAL:
        case RVLL_PRIOR_TRUNCRAYLEIGH: case RVLL_PRIOR_BETA: case RVLL_PRIOR_GAMMA: case RVLL_PRIOR_ALPHA:
        case RVLL_PRIOR_SORTED_UNIFORM: case RVLL_PRIOR_SORTED_LOGUNIFORM:
            break;
        case RVLL_PRIOR_TABLE:
            if (p.table_n < 2 || !p.table_cdf || !p.table_x)
                return fail(RVLL_E_INVALID, "prior %d: table needs >= 2 knots", d);
            for (int i = 1; i < p.table_n; ++i)
                if (!(p.table_cdf[i] >= p.table_cdf[i - 1]))
                    return fail(RVLL_E_INVALID, "prior %d: table knots not sorted at %d", d, i);
            break;
        default:
            return fail(RVLL_E_UNSUPPORTED, "prior %d: kind %d has no device implementation in this build", d, p.kind);
        }
    }
    free_priors(h);
    std::vector<rvll_prior> dev(priors, priors + ndim);
    h->table_err.assign((size_t)ndim, NAN);
    h->table_direct.assign((size_t)ndim, 0);
    for (int d = 0; d < ndim; ++d) {
        if (dev[d].kind == RVLL_PRIOR_BETA || dev[d].kind == RVLL_PRIOR_GAMMA) {
            // the device tabulates this prior's quantile function once; the kernel starts from it
            // (nodes: value, slope, second derivative) and measures its own quintic interpolant against the
            // full solver; a verified table is evaluated by interpolation alone (table_post = 1)
            const size_t nb = sizeof(double) * (size_t)rvll::prior_table_nodes();
            double *dz0 = nullptr, *dz1 = nullptr, *derr = nullptr;
            HIP_TRY(hipMalloc(&dz0, nb)); h->d_tables.push_back(dz0);
            HIP_TRY(hipMalloc(&dz1, 2 * nb)); h->d_tables.push_back(dz1);
            HIP_TRY(hipMalloc(&derr, sizeof(double))); h->d_tables.push_back(derr);
            HIP_TRY(hipMemsetAsync(derr, 0, sizeof(double), h->compute));
            HIP_TRY(rvll::launch_prior_table(dev[d].kind, priors[d].args, dz0, dz1,
                                             reinterpret_cast<unsigned long long*>(derr), h->compute));
            double err = INFINITY;
            HIP_TRY(hipMemcpyAsync(&err, derr, sizeof(double), hipMemcpyDeviceToHost, h->compute));
            HIP_TRY(hipStreamSynchronize(h->compute));
            dev[d].table_cdf = dz0;
            dev[d].table_x = dz1;
            dev[d].table_n = rvll::prior_table_nodes();
            dev[d].table_post = (err <= rvll::prior_table_direct_tol() && !getenv("RVLL_NO_DIRECT_TABLES")) ? 1 : 0;
            h->table_err[(size_t)d] = err;
            h->table_direct[(size_t)d] = dev[d].table_post;
            continue;
        }
        if (dev[d].kind != RVLL_PRIOR_TABLE) { dev[d].table_cdf = dev[d].table_x = nullptr; continue; }
        const size_t nb = sizeof(double) * (size_t)dev[d].table_n;
        double *dc = nullptr, *dx = nullptr;
        HIP_TRY(hipMalloc(&dc, nb)); h->d_tables.push_back(dc);
        HIP_TRY(hipMalloc(&dx, nb)); h->d_tables.push_back(dx);
        HIP_TRY(hipMemcpy(dc, priors[d].table_cdf, nb, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dx, priors[d].table_x, nb, hipMemcpyHostToDevice));
        dev[d].table_cdf = dc;
        dev[d].table_x = dx;
    }
    HIP_TRY(hipMalloc(&h->d_priors, sizeof(rvll_prior) * (size_t)std::max(1, ndim)));
    if (ndim) HIP_TRY(hipMemcpy(h->d_priors, dev.data(), sizeof(rvll_prior) * (size_t)ndim, hipMemcpyHostToDevice));
    std::vector<int32_t> heavy, light;
    h->priors_rowwise = false;
    for (int d = 0; d < ndim; ++d)
        if (priors[d].kind == RVLL_PRIOR_SORTED_UNIFORM || priors[d].kind == RVLL_PRIOR_SORTED_LOGUNIFORM) h->priors_rowwise = true;
    for (int d = 0; d < ndim; ++d)
        (priors[d].kind == RVLL_PRIOR_BETA || priors[d].kind == RVLL_PRIOR_GAMMA ? heavy : light).push_back(d);
    // the light kinds grouped by what their quantile costs (pow / ndtri / exp + log / table search / a division / nothing),
    // costliest first: in a tile of a few points every wave of the staging step otherwise runs every kind of the model
    auto cost_class = [&](int32_t d) {
        switch (priors[d].kind) {
        case RVLL_PRIOR_JEFFREYS: case RVLL_PRIOR_MODJEFFREYS: case RVLL_PRIOR_SORTED_UNIFORM: case RVLL_PRIOR_SORTED_LOGUNIFORM: return 0;
        case RVLL_PRIOR_NORMAL: case RVLL_PRIOR_LOGNORMAL: case RVLL_PRIOR_ALPHA: return 1;
        case RVLL_PRIOR_TRUNCRAYLEIGH: return 2;
        case RVLL_PRIOR_TABLE: return 3;
        case RVLL_PRIOR_UNIFORMFREQUENCY: return 4;
        default: return 5;
        }
    };
    std::stable_sort(light.begin(), light.end(), [&](int32_t x, int32_t y) {
        return cost_class(x) != cost_class(y) ? cost_class(x) < cost_class(y) : priors[x].kind < priors[y].kind; });
    {
        std::vector<int32_t> both(heavy);
        both.insert(both.end(), light.begin(), light.end());
        HIP_TRY(hipMalloc(&h->d_heavy, sizeof(int32_t) * std::max<size_t>(1, both.size())));
        if (!both.empty()) HIP_TRY(hipMemcpy(h->d_heavy, both.data(), sizeof(int32_t) * both.size(), hipMemcpyHostToDevice));
    }
    h->n_heavy = (int)heavy.size();
    h->all_direct = true;
    for (int32_t d : heavy) if (!h->table_direct[(size_t)d]) h->all_direct = false;
    HIP_TRY(hipStreamSynchronize(h->compute));          // start tables are built
    h->have_priors = true;
    return RVLL_OK;
}

int rvll_prior_table_info(rvll_handle* h, int32_t dim, double* max_err, int32_t* direct)
{
    if (!h) return fail(RVLL_E_INVALID, "null handle");
    if (!h->have_priors) return fail(RVLL_E_NOPRIORS, "rvll_set_priors has not been called");
    if (dim < 0 || dim >= (int32_t)h->table_err.size()) return fail(RVLL_E_INVALID, "dim %d out of range", dim);
    if (max_err) *max_err = h->table_err[(size_t)dim];
    if (direct) *direct = h->table_direct[(size_t)dim];
    return RVLL_OK;
}

// ---- device-resident forms ----------------------------------------------------
int rvll_dev_reserve(rvll_handle* h, int64_t B)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (B < 0) return fail(RVLL_E_INVALID, "B < 0");
    return ensure_capacity(h, B);
}

int rvll_dev_fill_cube(rvll_handle* h, int64_t B, uint64_t seed)
{
    int rc = rvll_dev_reserve(h, B);
    if (rc) return rc;
    HIP_TRY(rvll::launch_fill_cube(h->d_cube, (long long)B * h->L.ndim, seed, h->compute));
    return RVLL_OK;
}

int rvll_dev_prior(rvll_handle* h, int64_t B)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (!h->have_priors) return fail(RVLL_E_NOPRIORS, "rvll_set_priors has not been called");
    RVLL_TRY(rvll::host::check_capacity(h, B));
    rc = sync_other_lanes(h);                                       // other lanes may still be reading the old theta
    if (rc) return rc;
    rvll::PriorArgs a{h->d_cube, h->d_theta, (long long)B, h->L.ndim, h->d_priors, h->d_heavy, h->n_heavy};
    HIP_TRY(rvll::launch_prior(a, h->compute));
    h->theta_async = true;
    return RVLL_OK;
}

int rvll_dev_loglike(rvll_handle* h, int64_t B)
{
    int rc = use_device(h);
    if (rc) return rc;
    RVLL_TRY(rvll::host::check_capacity(h, B));
    if (B == 0) return RVLL_OK;
    const int lane = h->logl_cur;
    if (lane != 0 && h->theta_async) {        // theta was produced on lane 0's stream: order this lane behind it
        HIP_TRY(hipStreamSynchronize(h->compute));
        h->theta_async = false;
    }
    // launches that alternate pipeline lanes keep two kernels in flight: that decides the launch form and geometry
    // (choose_cu_form, choose_points_per_block) and is re-derived per launch, so a handle that went back to one lane
    // goes back to the single-stream choices
    const bool alternating = lane != h->logl_last;
    if (alternating != h->pipelined) { h->pipelined = alternating; h->geo.clear(); }
    rvll::LoglikeArgs a;
    int cu = 0;
    rc = build_args(h, h->d_theta, h->d_logL2[lane], h->d_flags2[lane], B, &a, &cu);
    if (rc) return rc;
    HIP_TRY(launch_form(a, cu, lane_stream(h, lane)));
    h->logl_last = lane;
    return RVLL_OK;
}

int rvll_dev_prior_loglike(rvll_handle* h, int64_t B)
{
    // Back-to-back one-launch batches over the same buffers stay asynchronous: the deferral word is sticky (cleared
    // only by resolve_fused), only the LATEST batch's results can still be looked at, and whoever looks at them goes
    // through use_device -> resolve_fused first — so the pending mark is carried over instead of resolved here.
    if (h) h->fused_pending = 0;
    int rc = use_device(h);
    if (rc) return rc;
    if (!h->have_priors) return fail(RVLL_E_NOPRIORS, "rvll_set_priors has not been called");
    RVLL_TRY(rvll::host::check_capacity(h, B));
    if (B == 0) return RVLL_OK;
    // One launch (the prior transform in the log-L tile's staging step) needs every Beta / Gamma prior to have a
    // verified table (the slim stage); otherwise: the prior kernels, then the log-L kernel.
    if (!h->all_direct) {
        rc = rvll_dev_prior(h, B);
        if (rc) return rc;
        if (h->logl_cur != 0) h->logl_cur = 0;     // results of this call live on lane 0, as the one-launch form's do
        return rvll_dev_loglike(h, B);
    }
    rc = sync_other_lanes(h);                  // theta is rewritten: no other lane may still be reading it
    if (rc) return rc;
    rvll::LoglikeArgs a;
    int cu = 0;                                // small batches: 256-thread tiles; larger ones: the CU-wide form, as for plain log-L
    h->pipelined = false;
    rc = build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], B, &a, B > kFusedMaxPoints ? &cu : nullptr);
    if (rc) return rc;
    make_fused(h, h->d_cube, h->d_theta, &a);
    if (cu > 0) HIP_TRY(rvll::launch_loglike_cu(a, cu, h->compute));
    else        HIP_TRY(rvll::launch_prior_loglike(a, h->compute));
    h->theta_async = true;
    h->logl_last = 0;
    h->fused_pending = B;                      // whoever touches the results next looks at the defer word first
    return RVLL_OK;
}

int rvll_dev_mark(rvll_handle* h, int32_t which)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (which < 0 || which > 1) return fail(RVLL_E_INVALID, "which must be 0 (start) or 1 (stop)");
    if (!h->marks[which]) HIP_TRY(hipEventCreate(&h->marks[which]));
    HIP_TRY(hipEventRecord(h->marks[which], h->compute));
    return RVLL_OK;
}

int rvll_dev_mark_elapsed(rvll_handle* h, double* ms)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (!ms || !h->marks[0] || !h->marks[1]) return fail(RVLL_E_INVALID, "both marks must have been recorded");
    HIP_TRY(hipEventSynchronize(h->marks[1]));
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, h->marks[0], h->marks[1]));
    *ms = (double)f;
    return RVLL_OK;
}

int rvll_dev_sync(rvll_handle* h)
{
    int rc = use_device(h);
    if (rc) return rc;
    // A blocking hipStreamSynchronize wakes the caller some tens of microseconds after the stream has drained; a caller
    // that is about to read a result (a sampler's proposal round, bench.py's 20-step timed region: 1.3 ms) waits on the
    // stream's status first — a poll costs well under a microsecond — and only falls back to the blocking call when the
    // work is long (the poll gives up after ~2 ms).
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(h->compute);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) HIP_TRY(q);
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    HIP_TRY(hipStreamSynchronize(h->compute));
    rc = sync_other_lanes(h);
    if (rc) return rc;
    h->theta_async = false;
    return RVLL_OK;
}

int rvll_dev_flip_lane(rvll_handle* h)
{
    if (!h) return fail(RVLL_E_INVALID, "null handle");
    h->logl_cur = (h->logl_cur + 1) % (h->nccl_comm[0] ? h->nlanes : h->nlanes_dev);
    return h->logl_cur;
}

int rvll_dev_time_loglike(rvll_handle* h, int64_t B, int32_t warmup, int32_t iters, rvll_timing* out)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (!out || iters < 1 || warmup < 0) return fail(RVLL_E_INVALID, "bad timing arguments");
    RVLL_TRY(rvll::host::check_capacity(h, B, 1));
    rvll::LoglikeArgs a;
    rc = sync_other_lanes(h);
    if (rc) return rc;
    int cu = 0;
    rc = build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], B, &a, &cu);
    if (rc) return rc;
    h->logl_last = 0;
    for (int i = 0; i < warmup; ++i) HIP_TRY(launch_form(a, cu, h->compute));
    std::vector<hipEvent_t> ev((size_t)iters + 1, nullptr);
    int status = RVLL_OK;
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) { status = fail(RVLL_E_HIP, "hipEventCreate failed"); break; }
    if (status == RVLL_OK) {
        hipError_t e = hipEventRecord(ev[0], h->compute);
        for (int i = 0; i < iters && e == hipSuccess; ++i) {
            e = launch_form(a, cu, h->compute);
            if (e == hipSuccess) e = hipEventRecord(ev[(size_t)i + 1], h->compute);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->compute);
        if (e != hipSuccess) status = fail(RVLL_E_HIP, "timed launches failed: %s", hipGetErrorString(e));
    }
    if (status == RVLL_OK) {
        std::vector<double> ms((size_t)iters);
        double sum = 0.;
        for (int i = 0; i < iters; ++i) {
            float f = 0.f;
            (void)hipEventElapsedTime(&f, ev[(size_t)i], ev[(size_t)i + 1]);
            ms[(size_t)i] = f;
            sum += f;
        }
        float total = 0.f;
        (void)hipEventElapsedTime(&total, ev.front(), ev.back());
        std::sort(ms.begin(), ms.end());
        out->kernel_ms_mean = sum / iters;
        out->kernel_ms_min = ms.front();
        out->kernel_ms_median = ms[(size_t)iters / 2];
        out->total_ms = total;
        out->evals = (int64_t)B * iters;
        out->launches = iters;
        out->points_per_block = a.PB;
        out->blocks = (int32_t)((B + a.PB - 1) / a.PB);
        out->threads = cu > 0 ? rvll::kCuThreads : rvll::kThreads;
    }
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    return status;
}

// Diagnostic: ONE launch of the stamped twin of the fp64 log-L kernel over the resident theta (after `warmup`
// ordinary launches, so the clocks are where a bench run has them); returns kTraceWords stamps per workgroup.
int rvll_dev_trace_loglike(rvll_handle* h, int64_t B, int32_t warmup, uint64_t* out, int64_t out_words,
                           int32_t* blocks, int32_t* points_per_block)
{
    int rc = use_device(h);
    if (rc) return rc;
    RVLL_TRY(rvll::host::check_capacity(h, B, 1));
    if (h->L.precision != RVLL_PREC_FP64) return fail(RVLL_E_UNSUPPORTED, "the trace kernel exists for fp64 only");
    rc = sync_other_lanes(h);
    if (rc) return rc;
    rvll::LoglikeArgs a;
    int cu = 0;
    rc = build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], B, &a, &cu);
    if (rc) return rc;
    const long long nb = (B + a.PB - 1) / a.PB;
    if (blocks) *blocks = (int32_t)nb;
    if (points_per_block) *points_per_block = a.PB;
    if (!out) return RVLL_OK;                               // size query
    const long long words = nb * rvll::kTraceWords;
    if (out_words < words) return fail(RVLL_E_INVALID, "trace buffer too small: %lld < %lld words", (long long)out_words, words);
    unsigned long long* d_trace = nullptr;
    HIP_TRY(hipMalloc(&d_trace, sizeof(unsigned long long) * (size_t)words));
    int status = RVLL_OK;
    hipError_t e = hipMemsetAsync(d_trace, 0, sizeof(unsigned long long) * (size_t)words, h->compute);
    for (int i = 0; i < warmup && e == hipSuccess; ++i) e = launch_form(a, cu, h->compute);
    a.trace = d_trace;
    if (e == hipSuccess) e = cu > 0 ? rvll::launch_loglike_cu(a, cu, h->compute) : rvll::launch_loglike_trace(a, h->compute);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_trace, sizeof(unsigned long long) * (size_t)words, hipMemcpyDeviceToHost, h->compute);
    if (e == hipSuccess) e = hipStreamSynchronize(h->compute);
    if (e != hipSuccess) status = fail(RVLL_E_HIP, "trace launch failed: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->compute);
    dev_free(d_trace);
    h->logl_last = 0;
    return status;
}

// ---- the one-launch batch's deferral, the scalar-call server ------------------------------------
}  // extern "C"

namespace {

// A one-launch cube -> log-L batch is in flight or finished: wait for it and, if its slim prior stage deferred any
// element (a quantile outside its table: |logit q| > 30, q = 0 or 1, ...), redo the batch with the prior kernels
// that carry the full solvers — the same rows, the same buffers, bit-identical results for every other point.
int resolve_fused(rvll_handle* h)
{
    const long long B = h->fused_pending;
    h->fused_pending = 0;
    HIP_TRY(hipStreamSynchronize(h->compute));
    if (__atomic_load_n(h->pin_defer, __ATOMIC_ACQUIRE) == 0) return RVLL_OK;
    *h->pin_defer = 0;
    int rc = rvll_dev_prior(h, B);
    if (rc) return rc;
    h->logl_cur = 0;
    return rvll_dev_loglike(h, B);
}

int server_start(rvll_handle* h)
{
    HIP_TRY(hipSetDevice(h->device));
    rvll::LoglikeArgs a;
    int rc = build_args(h, h->srv_dev->theta, h->d_srv_out, reinterpret_cast<int32_t*>(h->d_srv_out + 1), 1, &a);
    if (rc) return rc;
    if (a.PB != 1) { a.PB = 1; a.CH = std::max(rvll::kThreads, std::min(h->chunk_items, h->Ne)); a.CH = (a.CH + 1) & ~1; }
    if (h->have_priors) make_fused(h, h->srv_dev->theta, h->srv_dev->theta, &a);   // the prior op needs the tables
    __atomic_store_n(&h->srv->state, rvll::kServerRunning, __ATOMIC_RELEASE);
    HIP_TRY(rvll::launch_scalar_server(a, h->srv_dev, h->srv_last, h->srv_idle_ticks, h->srv_stream));
    h->srv_running = true;
    return RVLL_OK;
}

// One log-L through the persistent kernel: write theta and a new request number into the control block, spin on
// the answer.  If the kernel left in the meantime (idle timeout) it is started again with the request pending.
int scalar_call(rvll_handle* h, unsigned op, const double* theta, double* logL, int32_t* flags, double* theta_out)
{
    rvll::ServerCtl* c = h->srv;
    if (h->L.ndim > rvll::kServerMaxDim)
        return fail(RVLL_E_UNSUPPORTED, "scalar server supports up to %d parameters", rvll::kServerMaxDim);
    if (h->srv_dead)
        return fail(RVLL_E_HIP, "the scalar server of this handle stopped answering earlier; destroy the handle");
    if (h->srv_running && __atomic_load_n(&c->state, __ATOMIC_ACQUIRE) == rvll::kServerExited) {
        HIP_TRY(hipStreamSynchronize(h->srv_stream));
        h->srv_running = false;
    }
    if (!h->srv_running) {
        HIP_TRY(hipSetDevice(h->device));
        // the server reads the resident epoch table: anything still queued on the other streams goes first
        HIP_TRY(hipStreamSynchronize(h->compute));
        int rc = sync_other_lanes(h);
        if (rc) return rc;
    }
    const unsigned number = (unsigned)++h->srv_seq;
    const unsigned long long request = ((unsigned long long)op << 32) | number;
    server_post(h, request, theta);
    if (!h->srv_running) { int rc = server_start(h); if (rc) return rc; }
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(&c->answer.number, __ATOMIC_ACQUIRE) == number) break;
        __builtin_ia32_pause();
        if ((spins & 0xfff) != 0xfff) continue;
        if (__atomic_load_n(&c->state, __ATOMIC_ACQUIRE) == rvll::kServerExited &&
            __atomic_load_n(&c->answer.number, __ATOMIC_ACQUIRE) != number) {
            HIP_TRY(hipStreamSynchronize(h->srv_stream));           // left before it saw this request
            h->srv_running = false;
            int rc = server_start(h);
            if (rc) return rc;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
            // Post the quit word and mark the server dead WITHOUT waiting for the stream: if the persistent kernel is
            // really stuck, a stream synchronisation would never return.  The kernel also leaves by itself after its
            // idle timeout; the handle refuses further scalar calls and the caller should exit, not retry.
            const unsigned long long quit = ((unsigned long long)rvll::kServerQuit << 32) | (unsigned)++h->srv_seq;
            server_post(h, quit, nullptr);
            h->srv_last = quit;
            h->srv_dead = true;
            h->srv_enabled = false;
            return fail(RVLL_E_HIP, "scalar server did not answer within 5 s (handle marked dead)");
        }
    }
    h->srv_last = request;
    if (op == rvll::kServerPrior) {
        memcpy(theta_out, c->theta, sizeof(double) * (size_t)h->L.ndim);
        return RVLL_OK;
    }
    if (op == rvll::kServerPriorLogLike && theta_out) memcpy(theta_out, c->theta, sizeof(double) * (size_t)h->L.ndim);
    if (logL) *logL = c->answer.logL;          // same 16-byte store as the number just seen
    if (flags) *flags = c->answer.flags;
    return RVLL_OK;
}

}  // namespace

extern "C" {

int rvll_scalar_server(rvll_handle* h, int32_t enable)
{
    int rc = use_device(h);                   // also stops a running server
    if (rc) return rc;
    if (enable && h->L.ndim > rvll::kServerMaxDim)
        return fail(RVLL_E_UNSUPPORTED, "scalar server supports up to %d parameters", rvll::kServerMaxDim);
    h->srv_enabled = enable != 0;
    return RVLL_OK;
}

int rvll_set_wander_exact(rvll_handle* h, int32_t on)
{
    if (!h) return fail(RVLL_E_INVALID, "null handle");
    h->wander_exact = on != 0;
    return RVLL_OK;
}

int rvll_set_slim_table_range(rvll_handle* h, double umax)
{
    if (!h) return fail(RVLL_E_INVALID, "null handle");
    if (!(umax >= 0.)) return fail(RVLL_E_INVALID, "umax must be >= 0");
    h->slim_umax = std::min(umax, rvll::prior_table_umax());
    return RVLL_OK;
}

// ---- Keplerian curves (post-processing helper) ------------------------------------------------------
int rvll_kep_rv_batch(rvll_handle* h, const double* theta, int64_t B, const double* times, int32_t n_times,
                      uint32_t include_mask, double* out)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (B < 0 || n_times < 0) return fail(RVLL_E_INVALID, "negative size");
    if (B == 0 || n_times == 0) return RVLL_OK;
    if (!theta || !times || !out) return fail(RVLL_E_INVALID, "null buffer");
    rc = rvll_dev_upload_theta(h, theta, B);
    if (rc) return rc;
    double *d_times = nullptr, *d_out = nullptr;
    int status = RVLL_OK;
    hipError_t e = hipMalloc(&d_times, sizeof(double) * (size_t)n_times);
    if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(double) * (size_t)B * (size_t)n_times);
    if (e == hipSuccess) e = hipMemcpyAsync(d_times, times, sizeof(double) * (size_t)n_times, hipMemcpyHostToDevice, h->compute);
    if (e == hipSuccess) {
        rvll::LoglikeArgs a;
        status = build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], B, &a);
        if (status == RVLL_OK) e = rvll::launch_keprv(a, d_times, n_times, include_mask, d_out, h->compute);
    }
    if (status == RVLL_OK && e == hipSuccess)
        e = hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)B * (size_t)n_times, hipMemcpyDeviceToHost, h->compute);
    if (status == RVLL_OK && e == hipSuccess) e = hipStreamSynchronize(h->compute);
    if (status == RVLL_OK && e != hipSuccess) status = fail(RVLL_E_HIP, "kep_rv_batch: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->compute);
    dev_free(d_times); dev_free(d_out);
    return status;
}

// ---- order statistics of groups of Keplerian curves (post-processing; rvll_bands.hip) ----------------------------------------
int rvll_kep_rv_bands(rvll_handle* h, const double* theta, int64_t n_groups, int32_t n, const double* times, int32_t n_times,
                      uint32_t include_mask, const double* levels, int32_t n_q, double* q, double* mean, int32_t* n_valid,
                      int64_t chunk_bytes, double* phase_ms)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (n_groups < 0 || n_times < 0 || chunk_bytes < 0) return fail(RVLL_E_INVALID, "negative size");
    if (n < 1 || n > 4096) return fail(RVLL_E_INVALID, "n must be in [1, 4096]");
    if (n_q < 1 || n_q > 16) return fail(RVLL_E_INVALID, "n_q must be in [1, 16]");
    if (!levels) return fail(RVLL_E_INVALID, "null buffer");
    for (int32_t k = 0; k < n_q; ++k)
        if (!(levels[k] > 0.0 && levels[k] < 1.0)) return fail(RVLL_E_INVALID, "level %d is outside (0, 1)", (int)k);
    if (phase_ms) phase_ms[0] = phase_ms[1] = 0.0;
    if (n_groups == 0 || n_times == 0) return RVLL_OK;
    if (!theta || !times || !q || !mean || !n_valid) return fail(RVLL_E_INVALID, "null buffer");
    const long long group_bytes = (long long)sizeof(double) * n * n_times;
    const long long bound = chunk_bytes > 0 ? chunk_bytes : 256ll << 20;
    const long long gc = std::min<long long>(n_groups, std::max<long long>(1, bound / group_bytes));   // whole groups a chunk
    double *d_times = nullptr, *d_levels = nullptr, *d_vals = nullptr, *d_q = nullptr, *d_mean = nullptr;
    int32_t* d_nv = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int status = RVLL_OK;
    hipError_t e = hipMalloc(&d_times, sizeof(double) * (size_t)n_times);
    if (e == hipSuccess) e = hipMalloc(&d_levels, sizeof(double) * (size_t)n_q);
    if (e == hipSuccess) e = hipMalloc(&d_vals, (size_t)(gc * group_bytes));
    if (e == hipSuccess) e = hipMalloc(&d_q, sizeof(double) * (size_t)(gc * n_q * n_times));
    if (e == hipSuccess) e = hipMalloc(&d_mean, sizeof(double) * (size_t)(gc * n_times));
    if (e == hipSuccess) e = hipMalloc(&d_nv, sizeof(int32_t) * (size_t)(gc * n_times));
    for (auto& x : ev)
        if (e == hipSuccess) e = hipEventCreate(&x);
    if (e == hipSuccess) e = hipMemcpyAsync(d_times, times, sizeof(double) * (size_t)n_times, hipMemcpyHostToDevice, h->compute);
    if (e == hipSuccess) e = hipMemcpyAsync(d_levels, levels, sizeof(double) * (size_t)n_q, hipMemcpyHostToDevice, h->compute);
    for (long long g0 = 0; g0 < n_groups && status == RVLL_OK && e == hipSuccess; g0 += gc) {
        const long long gb = std::min<long long>(gc, n_groups - g0);
        status = rvll_dev_upload_theta(h, theta + g0 * n * (long long)h->L.ndim, gb * n);
        if (status != RVLL_OK) break;
        rvll::LoglikeArgs a;
        status = build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], gb * n, &a);
        if (status != RVLL_OK) break;
        e = hipEventRecord(ev[0], h->compute);
        if (e == hipSuccess) e = rvll::launch_keprv(a, d_times, n_times, include_mask, d_vals, h->compute);
        if (e == hipSuccess) e = hipEventRecord(ev[1], h->compute);
        if (e == hipSuccess) e = rvll::launch_bands(d_vals, gb, n, n_times, d_levels, n_q, d_q, d_mean, d_nv, h->compute);
        if (e == hipSuccess) e = hipEventRecord(ev[2], h->compute);
        if (e == hipSuccess)
            e = hipMemcpyAsync(q + g0 * n_q * n_times, d_q, sizeof(double) * (size_t)(gb * n_q * n_times), hipMemcpyDeviceToHost,
                               h->compute);
        if (e == hipSuccess)
            e = hipMemcpyAsync(mean + g0 * n_times, d_mean, sizeof(double) * (size_t)(gb * n_times), hipMemcpyDeviceToHost, h->compute);
        if (e == hipSuccess)
            e = hipMemcpyAsync(n_valid + g0 * n_times, d_nv, sizeof(int32_t) * (size_t)(gb * n_times), hipMemcpyDeviceToHost,
                               h->compute);
        if (e == hipSuccess) e = hipStreamSynchronize(h->compute);
        float ms = 0.f;
        if (e == hipSuccess && phase_ms && (e = hipEventElapsedTime(&ms, ev[0], ev[1])) == hipSuccess) phase_ms[0] += ms;
        if (e == hipSuccess && phase_ms && (e = hipEventElapsedTime(&ms, ev[1], ev[2])) == hipSuccess) phase_ms[1] += ms;
    }
    if (status == RVLL_OK && e != hipSuccess)
        status = fail(e == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, "kep_rv_bands: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->compute);
    for (auto& x : ev)
        if (x) (void)hipEventDestroy(x);
    dev_free(d_times); dev_free(d_levels); dev_free(d_vals); dev_free(d_q); dev_free(d_mean); dev_free(d_nv);
    return status;
}

// ---- diagnostics ---------------------------------------------------------------------
int rvll_debug_eval(rvll_handle* h, int32_t op, const double* x, const double* y, int64_t n, double* out)
{
    int rc = use_device(h);
    if (rc) return rc;
    if (!x || !out || n < 1) return fail(RVLL_E_INVALID, "bad debug_eval arguments");
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t nb = sizeof(double) * (size_t)n;
    int status = RVLL_OK;
    hipError_t e = hipMalloc(&dx, nb);
    if (e == hipSuccess) e = hipMalloc(&dout, nb);
    if (e == hipSuccess && y) e = hipMalloc(&dy, nb);
    if (e == hipSuccess) e = hipMemcpy(dx, x, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess && y) e = hipMemcpy(dy, y, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rvll::launch_debug_eval(op, dx, dy, (long long)n, dout, h->compute);
    if (e == hipSuccess) e = hipStreamSynchronize(h->compute);
    if (e == hipSuccess) e = hipMemcpy(out, dout, nb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) status = fail(RVLL_E_HIP, "debug_eval: %s", hipGetErrorString(e));
    dev_free(dx); dev_free(dy); dev_free(dout);
    return status;
}

}  // extern "C"

// ---- the helpers the other host units call (rvll_host.h) ----
namespace rvll {
namespace host {
int use_device(rvll_handle* h) { return ::use_device(h); }
int sync_other_lanes(rvll_handle* h) { return ::sync_other_lanes(h); }
int build_args(rvll_handle* h, const double* d_theta, double* d_logL, int32_t* d_flags, long long B, rvll::LoglikeArgs* out, int* cu_grid)
{
    return ::build_args(h, d_theta, d_logL, d_flags, B, out, cu_grid);
}
void make_fused(const rvll_handle* h, const double* d_cube, double* d_theta_out, rvll::LoglikeArgs* a) { ::make_fused(h, d_cube, d_theta_out, a); }
hipError_t launch_form(const rvll::LoglikeArgs& a, int cu_grid, hipStream_t stream) { return ::launch_form(a, cu_grid, stream); }
int scalar_call(rvll_handle* h, unsigned op, const double* theta, double* logL, int32_t* flags, double* theta_out)
{
    return ::scalar_call(h, op, theta, logL, flags, theta_out);
}
}  // namespace host
}  // namespace rvll
