// rvll_walk_host.hip — host side of the sampler's proposal step: the device-resident slice-sampling walk
// in its forms (rvll_slice_walk*).  Entry points of include/rvll.h; the kernels are in rvll_walk.hip and rvll_rounds.hip.  The
// live set of nested sampling kept in HBM (rvll_live_*) is rvll_live_host.hip, which walks through walk_core (rvll_host.h).
// Every integer decision — switches, geometry, arena layout, row order — is rvll_walk_plan.h's; here are the buffers, the launches
// and the copies: walk_rounds (plan, reserve, bind, streams, issue, totals) and walk_core (a sequence of passes over one Walk).
#include <chrono>
#include <thread>
#include "rvll_host.h"
#include "rvll_walk_plan.h"

using rvll::report_error;
using namespace rvll::host;
using namespace std::chrono;

namespace {

static_assert(walkplan::kThreads == rvll::kThreads && walkplan::kWave == rvll::kWave && walkplan::kMaxPoints == rvll::kMaxPointsPerBlock &&
              walkplan::kCuThreads == rvll::kCuThreads && walkplan::kCuMaxPoints == rvll::kCuMaxPoints && walkplan::kRing == rvll::kRoundsRing &&
              walkplan::kMaxGroups == kMaxLanes && walkplan::kCuLds == rvll::kCuLdsBudget, "rvll_walk_plan.h plans for these limits");

// the bound of the stepout walk's basis scratch (basis_for), in doubles: 512 MiB
constexpr size_t kStepoutBasisMax = (size_t)1 << 26;

// run mode: d_walk_cost [n] down and added to rw->row_calls (at rows[j], or at j when rows is null); synchronises the stream
int run_calls_add(rvll_handle* h, RunWalk* rw, int64_t n, const int32_t* rows)
{
    std::vector<int32_t> c((size_t)n);
    HIP_TRY(hipMemcpyAsync(c.data(), h->d_walk_cost, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, h->compute));
    HIP_TRY(hipStreamSynchronize(h->compute));
    for (int64_t j = 0; j < n; ++j) rw->row_calls[(size_t)(rows ? rows[j] : j)] += c[(size_t)j];
    return RVLL_OK;
}

// the first K walkers' rows (unit cube, theta, log-L: K of each) from host buffers into the walk's, behind one another on the compute stream
int walk_rows_upload(rvll_handle* h, const double* cube, const double* theta, const double* logl, int64_t K)
{
    const size_t D = (size_t)h->L.ndim;
    hipStream_t st = h->compute;
    HIP_TRY(hipMemcpyAsync(h->d_walk_u, cube, sizeof(double) * D * (size_t)K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_walk_theta, theta, sizeof(double) * D * (size_t)K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_walk_logl, logl, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, st));
    return RVLL_OK;
}

// ... and back to the host buffers; synchronises the stream
int walk_rows_download(rvll_handle* h, double* cube, double* theta, double* logl, int64_t K)
{
    const size_t D = (size_t)h->L.ndim;
    hipStream_t st = h->compute;
    HIP_TRY(hipMemcpyAsync(cube, h->d_walk_u, sizeof(double) * D * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(theta, h->d_walk_theta, sizeof(double) * D * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(logl, h->d_walk_logl, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

// the rows form runs neither the stepout proposal nor run mode
int rows_form_refusal(const WalkSwitches& sw, bool stepout, bool run_mode)
{
    if (sw.rows >= 1 && stepout) return report_error(RVLL_E_UNSUPPORTED, "the rows form (RVLL_WALK_ROWS) has no stepout proposal");
    if (sw.rows >= 1 && run_mode) return report_error(RVLL_E_UNSUPPORTED, "rvll_slice_walk_runs: the rows form (RVLL_WALK_ROWS) has no run mode");
    return RVLL_OK;
}

// ---- the walk as rounds of launches (rvll_rounds.h, rvll_kernels.hip; which walks take it: rounds_wanted) --------------------
// A walk in rounds in progress: G groups of rows; a group's round = its step, then the batch log-L tiles over its candidates, the
// groups on streams of their own (rvll_kernels.hip, rounds_step_kernel / rounds_tiles_kernel).  How the rounds are issued: a
// stream per group; a group's round = a step launch, then a tiles launch (256-thread form, or CU-wide: RVLL_ROUNDS_FORM=cu, a
// measurement switch).  (A third structure — one stream, every launch one group's tiles next to another group's step in one
// kernel — was measured slower, 1.2e8 against 1.7e8 calls/s, its kernel spilled, and it is gone: profiles/r04_rounds_sweep.txt.)
struct Rounds {
    rvll_handle* h;
    const WalkSwitches& sw;
    const RunWalk* rw;
    RoundsPlan p;
    std::vector<rvll::RoundsArgs> ga;
    std::vector<rvll::LoglikeArgs> la;
    std::vector<rvll::RoundsTiles> ta;
    std::vector<hipStream_t> gs;
    std::vector<long long> n_tile;                  // per group: rounds launched (a step, then its tiles)
    std::vector<char> done;
    int ndone = 0;
    bool chain = false;
    long long launch_ns = 0, n_launch = 0;
    std::vector<unsigned long long> listed_seen;    // RVLL_ROUNDS_LISTED_DUMP: group 0's progress words, as the host saw them change
    unsigned long long* d_stamps = nullptr;         // RVLL_ROUNDS_STAMPS
};

// the plan of a walk of K rows and the tiles' arguments (theta, log-L, flags, B: per group, rounds_bind)
int rounds_plan(rvll_handle* h, int64_t K, int32_t nsteps, int32_t max_rounds, const WalkSwitches& sw, rvll::LoglikeArgs* a, RoundsPlan* p)
{
    const RoundsStart s = rounds_start(K, h->n_cu, h->Ne, h->walk_spec_rounds, sw);
    RVLL_TRY(build_args(h, nullptr, nullptr, nullptr, s.batch(), a));
    auto tile_lds = [&](int pb, int ch) { rvll::LoglikeArgs b = *a; b.PB = pb; b.CH = ch; return rvll::loglike_lds_bytes(b); };
    RoundsIn in{K, h->L.ndim, h->Ne, h->n_cu, nsteps, max_rounds, h->walk_spec_rounds, h->chunk_items, a->PB, a->CH, 0,
                rvll::rounds_walkers_per_block(h->L.ndim, s.spec, walkplan::kLds)};
    if (in.W >= 1 && !sw.cu_form) in.occ = rvll::rounds_blocks_per_cu(tile_lds(a->PB, a->CH));
    *p = plan_rounds(in, sw, tile_lds);
    if (!p->ok) return RVLL_E_UNSUPPORTED;
    a->PB = p->PB;  a->CH = p->CH;
    a->cr_redo = sw.cr;                               // (the walk's tiles leave the exact redo of wandering solves to redo_wandering: see walk_tile_args)
    if (sw.geom_dump)
        fprintf(stderr, "[rounds] K=%lld G=%d %s %s per=%lld C=%lld c_free=%lld W=%d step blocks=%lld PB=%d tiles=%d lds=%zu spec=%d\n", (long long)K, p->G,
                "streams", p->cu_form ? "cu" : "tile", p->per, p->C, p->c_free, p->W, p->nblk, p->PB, p->tiles, p->lds, p->spec);
    return RVLL_OK;
}

// the arena, the groups' progress words, and the directions of every move of every walker, ahead of the rounds (rvll_rounds.h, rounds_dirs)
int rounds_reserve(Rounds& R, const RoundsArena& ar, int64_t K, int32_t nsteps, uint64_t seed, int64_t walker_base)
{
    rvll_handle* h = R.h;
    const int D = h->L.ndim;
    RVLL_TRY(grow(h, &h->d_rounds, &h->rounds_bytes, (size_t)R.p.G * ar.g_bytes));
    if (!h->pin_rounds) {
        void *p = nullptr, *pd = nullptr;
        HIP_TRY(hipHostMalloc(&p, sizeof(unsigned long long) * kMaxLanes, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer(&pd, p, 0));
        h->pin_rounds = static_cast<unsigned long long*>(p);
        h->pin_rounds_dev = static_cast<unsigned long long*>(pd);
    }
    RVLL_TRY(grow(h, &h->d_walk_dirs, &h->walk_dirs_cap, (size_t)K * (size_t)nsteps * (size_t)D));
    rvll::RoundsDirs dg{h->d_walk_dirs, h->d_walk_chol, (long long)K, (unsigned long long)walker_base, (unsigned long long)seed, D, nsteps};
    if (R.rw) { dg.run = h->d_walk_run; dg.rid = h->d_walk_wid; dg.run_seed = h->d_run_seed; dg.run_chol = h->d_run_chol; }
    HIP_TRY(R.rw ? rvll::launch_rounds_dirs_runs(dg, 16 * h->n_cu, h->compute) : rvll::launch_rounds_dirs(dg, 16 * h->n_cu, h->compute));
    return RVLL_OK;
}

// every group's step and tiles arguments: its rows of the walk's buffers, its slice of the arena (base + offset); its counters zeroed
int rounds_bind(Rounds& R, const RoundsArena& ar, const rvll::LoglikeArgs& a, int64_t K, double lstar, int32_t nsteps, int32_t max_rounds,
                uint64_t seed, int64_t walker_base)
{
    rvll_handle* h = R.h;
    const RoundsPlan& p = R.p;
    const int D = h->L.ndim;
    R.ga.resize((size_t)p.G);  R.la.assign((size_t)p.G, a);  R.ta.resize((size_t)p.G);
    for (int g = 0; g < p.G; ++g) {
        char* base = static_cast<char*>(h->d_rounds) + (size_t)g * ar.g_bytes;
        auto dbl = [&](size_t o) { return reinterpret_cast<double*>(base + o); };
        auto i32 = [&](size_t o) { return reinterpret_cast<int32_t*>(base + o); };
        const long long row0 = (long long)g * p.per;
        rvll::RoundsArgs& r = R.ga[(size_t)g];
        r.u = h->d_walk_u + (size_t)row0 * D;  r.theta = h->d_walk_theta + (size_t)row0 * D;  r.logl = h->d_walk_logl + row0;
        r.step = h->d_walk_steps + row0;  r.wflag = h->d_walk_wflag + row0;
        r.dirs = h->d_walk_dirs + (size_t)row0 * nsteps * D;
        r.dir = dbl(ar.dir);  r.dirnext = dbl(ar.dirnext);  r.tmin = dbl(ar.tmin);  r.tmax = dbl(ar.tmax);
        r.theta_c[0] = dbl(ar.theta_c[0]);  r.theta_c[1] = dbl(ar.theta_c[1]);  r.wt = dbl(ar.wt);  r.wres_logl = dbl(ar.wres_logl);
        r.calls_part = reinterpret_cast<long long*>(base + ar.calls_part);
        r.slots_part = reinterpret_cast<unsigned long long*>(base + ar.slots_part);
        r.ring = i32(ar.ring);
        r.ws = i32(ar.ws);  r.wres_flags = i32(ar.wres_flags);  r.wdef = i32(ar.wdef);  r.owner = i32(ar.owner);
        r.priors = h->d_priors;  r.heavy_dims = h->d_heavy;  r.n_heavy = h->n_heavy;  r.light_dims = h->d_heavy + h->n_heavy;
        r.inplace = h->priors_rowwise ? 0 : 1;  r.slim_umax = h->slim_umax;
        r.K = std::min<long long>(p.per, K - row0);  r.wid0 = (unsigned long long)(walker_base + row0);
        r.C = (int)p.C;  r.c_free = (int)p.c_free;
        r.wrapped = h->d_walk_wrapped;
        r.D = D;  r.W = p.W;  r.nsteps = nsteps;  r.max_rounds = max_rounds;  r.spec_max = p.spec;
        r.seed = seed;  r.lstar = lstar;
        if (R.rw) {
            r.run = h->d_walk_run + row0;  r.rid = h->d_walk_wid + row0;  r.wcost = h->d_walk_cost + row0;
            r.run_lstar = h->d_run_lstar;  r.run_seed = h->d_run_seed;
        }
        rvll::LoglikeArgs& l = R.la[(size_t)g];
        l.theta = r.theta_c[0];  l.logL = dbl(ar.res_logl);  l.flags = i32(ar.res_flags);  l.B = p.C;      // the tiles: theta -> log-L
        R.ta[(size_t)g] = rvll::RoundsTiles{nullptr, h->pin_rounds_dev + g, r.owner, dbl(ar.wres_logl), i32(ar.wres_flags)};
        r.stamps = nullptr;  r.stamp_rounds = 0;
        HIP_TRY(hipMemsetAsync(base + ar.calls_part, 0, ar.words_bytes(), h->compute));          // the partial sums and the ring
        h->pin_rounds[g] = 0;
    }
    return RVLL_OK;
}

// diagnostic (RVLL_ROUNDS_STAMPS=n): time stamps of group 0's step workgroups over its first n rounds, dumped to stderr
int stamps_begin(Rounds& R)
{
    if (!R.sw.stamps) return RVLL_OK;
    const size_t nb = sizeof(unsigned long long) * 8 * (size_t)R.sw.stamps * (size_t)R.p.nblk;
    HIP_TRY(hipMalloc(&R.d_stamps, nb));
    HIP_TRY(hipMemsetAsync(R.d_stamps, 0, nb, R.h->compute));
    R.ga[0].stamps = R.d_stamps;  R.ga[0].stamp_rounds = R.sw.stamps;
    return RVLL_OK;
}

void stamps_dump(Rounds& R)
{
    if (!R.d_stamps) return;
    const int stamp_rounds = R.sw.stamps;
    std::vector<unsigned long long> sv((size_t)8 * stamp_rounds * R.p.nblk);
    (void)hipMemcpy(sv.data(), R.d_stamps, sizeof(unsigned long long) * sv.size(), hipMemcpyDeviceToHost);
    (void)hipFree(R.d_stamps);
    const long long nb0 = (R.ga[0].K + R.p.W - 1) / R.p.W;
    for (int r = 0; r < stamp_rounds && r < R.n_tile[0]; ++r) {
        unsigned long long t0 = ~0ull, t_last_start = 0, t_end = 0, n = 0;
        double seg[7] = {};
        for (long long b = 0; b < nb0; ++b) {
            const unsigned long long* q = &sv[8 * ((size_t)r * nb0 + b)];
            if (!q[7]) continue;
            t0 = std::min(t0, q[0]); t_last_start = std::max(t_last_start, q[0]); t_end = std::max(t_end, q[7]);
            for (int k = 0; k < 7; ++k) seg[k] += (q[k + 1] >= q[k] && q[k + 1]) ? (double)(q[k + 1] - q[k]) / 100. : 0.;
            ++n;
        }
        if (n) fprintf(stderr, "[step stamps] round %d: %llu blocks, last start +%.2f, end +%.2f us; per block: fetch %.2f, accept+atomic %.2f, move-in+directions %.2f, "
                       "t-phase %.2f, rows %.2f, prior %.2f, store %.2f us\n", r, n, (t_last_start - t0) / 100., (t_end - t0) / 100.,
                       seg[0] / n, seg[1] / n, seg[2] / n, seg[3] / n, seg[4] / n, seg[5] / n, seg[6] / n);
    }
}

// diagnostic (RVLL_ROUNDS_LISTED_DUMP): group 0's walkers listed, round by round
void listed_dump(const Rounds& R)
{
    const std::vector<unsigned long long>& seen = R.listed_seen;
    if (seen.empty()) return;
    long long below[4] = {0, 0, 0, 0};
    const long long full = R.ga[0].K;
    for (unsigned long long p : seen) {
        const long long l = (long long)(unsigned)p;
        if (l * 2 < full) ++below[0];
        if (l * 4 < full) ++below[1];
        if (l * 10 < full) ++below[2];
        if (l * 50 < full) ++below[3];
    }
    fprintf(stderr, "[rounds listed] group 0: %lld walkers, %lld rounds to the end (%zu seen by the host); rounds with fewer than 1/2, 1/4, 1/10, 1/50 of the walkers listed: %lld %lld %lld %lld (of the seen);",
            full, (long long)(seen.back() >> 32), seen.size(), below[0], below[1], below[2], below[3]);
    for (size_t k = 0; k < seen.size(); k += std::max<size_t>(1, seen.size() / 24))
        fprintf(stderr, " r%lld:%u", (long long)(seen[k] >> 32), (unsigned)seen[k]);
    fprintf(stderr, "\n");
}

// The groups' streams: the handle's lanes (RVLL_ROUNDS_PRIO=1, a measurement switch: streams of DIFFERENT priorities — it did
// not keep the groups out of lock step: 1.45 against 1.51e8 calls/s); the events of the chained issue
int rounds_streams(Rounds& R)
{
    rvll_handle* h = R.h;
    const int G = R.p.G;
    R.gs.assign((size_t)G, h->compute);
    R.chain = G > 1 && R.sw.chain;
    if (R.chain)
        for (int g = 0; g < G; ++g)
            if (!h->ev_chain[g]) HIP_TRY(hipEventCreateWithFlags(&h->ev_chain[g], hipEventDisableTiming));
    if (G == 1) return RVLL_OK;
    int lo_p = 0, hi_p = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);      // (numerically: hi_p <= lo_p)
    for (int g = 0; g < G; ++g) {
        if (!R.sw.prio) { R.gs[(size_t)g] = h->lanes[g]; continue; }
        if (!h->rounds_streams[g]) {
            const int p = std::max(hi_p, std::min(lo_p, hi_p + g));
            HIP_TRY(hipStreamCreateWithPriority(&h->rounds_streams[g], hipStreamNonBlocking, p));
        }
        R.gs[(size_t)g] = h->rounds_streams[g];
    }
    // they start behind what lane 0 holds (uploads, the live step's gathers, the zeroing above)
    if (!h->ev_rounds) HIP_TRY(hipEventCreateWithFlags(&h->ev_rounds, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->ev_rounds, h->compute));
    for (int g = 0; g < G; ++g) if (R.gs[(size_t)g] != h->compute) HIP_TRY(hipStreamWaitEvent(R.gs[(size_t)g], h->ev_rounds, 0));
    return RVLL_OK;
}

// A group's progress word, published by its tiles as they start: (round + 1) << 32 | walkers listed.  The group is done when a
// round listed nobody (what is already queued behind it finds nothing to do), ready while fewer than `depth` rounds are queued
// beyond the last one seen starting.
enum class Poll { kDone, kReady, kWait };

Poll rounds_poll(Rounds& R, int g, unsigned long long* sum)
{
    const unsigned long long p = __atomic_load_n(&R.h->pin_rounds[g], __ATOMIC_ACQUIRE);
    const long long pub = (long long)(p >> 32);
    *sum += p;
    if (R.sw.listed_dump && !R.chain && g == 0 && (R.listed_seen.empty() || R.listed_seen.back() != p)) R.listed_seen.push_back(p);
    if (pub > 0 && (unsigned)p == 0u) { R.done[(size_t)g] = 1; ++R.ndone; return Poll::kDone; }
    return R.n_tile[(size_t)g] - pub >= R.p.depth ? Poll::kWait : Poll::kReady;
}

// group g's next round on its stream: its step, then its tiles; chained: the step behind group prev's step of this round (prev < 0: none)
int rounds_launch(Rounds& R, int g, int prev)
{
    rvll_handle* h = R.h;
    if (R.n_tile[(size_t)g] >= R.p.r_max) return report_error(RVLL_E_HIP, "rounds walk: group %d did not finish in %lld rounds", g, R.p.r_max);
    const int r = (int)R.n_tile[(size_t)g];
    hipStream_t s = R.gs[(size_t)g];
    const auto t0 = steady_clock::now();
    hipError_t e = prev >= 0 ? hipStreamWaitEvent(s, h->ev_chain[prev], 0) : hipSuccess;
    if (e == hipSuccess) e = R.rw ? rvll::launch_rounds_step_runs(R.ga[(size_t)g], r, s) : rvll::launch_rounds_step(R.ga[(size_t)g], r, s);
    if (e == hipSuccess && R.chain) e = hipEventRecord(h->ev_chain[g], s);
    if (e == hipSuccess) {
        R.ta[(size_t)g].ring_entry = R.ga[(size_t)g].ring + 2 * (r % rvll::kRoundsRing);
        R.la[(size_t)g].theta = R.ga[(size_t)g].theta_c[r & 1];
        e = R.p.cu_form ? rvll::launch_rounds_cu(R.la[(size_t)g], R.ta[(size_t)g], R.p.tiles, r, s)
                        : rvll::launch_rounds_tiles(R.la[(size_t)g], R.ta[(size_t)g], R.p.tiles, r, s);
    }
    R.launch_ns += duration_cast<nanoseconds>(steady_clock::now() - t0).count();
    if (e != hipSuccess) return report_error(RVLL_E_HIP, "rounds walk launch failed: %s", hipGetErrorString(e));
    R.n_tile[(size_t)g] += 1;
    R.n_launch += 2;
    return RVLL_OK;
}

// The host only keeps the queues a few rounds deep.  A turn polls every group that is not done and issues a ready group's next
// round at once.  (RVLL_ROUNDS_CHAIN=1, a measurement switch.)  Left to themselves the groups fall into lock step: all step
// together (the chip idle for a step's 20 us), then all run their tiles together.  Chained, group g's step of a round waits (an
// event, on the device) for group g - 1's step of that round — it starts when g - 1's tiles do and runs beside them — and the
// host issues a round for all groups at once, when all are ready.  Slower: the groups then all wait for the slowest of them, and
// every link adds an event's latency.  Returns when every group is done, with the groups' streams synchronised.
int rounds_issue(Rounds& R)
{
    const int G = R.p.G;
    R.n_tile.assign((size_t)G, 0);  R.done.assign((size_t)G, 0);
    int status = RVLL_OK;
    auto last_progress = steady_clock::now();
    unsigned long long seen_sum = 0;
    while (R.ndone < G && status == RVLL_OK) {
        unsigned long long sum = 0;
        bool any = false, all_ready = true;
        for (int g = 0; g < G && status == RVLL_OK; ++g) {
            if (R.done[(size_t)g]) continue;
            const Poll s = rounds_poll(R, g, &sum);
            if (s == Poll::kWait) all_ready = false;
            if (s != Poll::kReady || R.chain) continue;
            status = rounds_launch(R, g, -1);
            any = status == RVLL_OK;
        }
        if (R.chain && all_ready && R.ndone < G)
            for (int g = 0, prev = -1; g < G && status == RVLL_OK; ++g) {
                if (R.done[(size_t)g]) continue;
                status = rounds_launch(R, g, prev);
                prev = g;
                any = status == RVLL_OK;
            }
        if (status != RVLL_OK) break;
        if (any || sum != seen_sum) { last_progress = steady_clock::now(); seen_sum = sum; continue; }
        if (R.ndone < G && steady_clock::now() - last_progress > seconds(20)) {
            status = report_error(RVLL_E_HIP, "rounds walk made no progress for 20 s");
            break;
        }
        std::this_thread::yield();
    }
    for (int g = 0; g < G; ++g) {
        const hipError_t e = hipStreamSynchronize(R.gs[(size_t)g]);
        if (e != hipSuccess && status == RVLL_OK) status = report_error(RVLL_E_HIP, "rounds walk: %s", hipGetErrorString(e));
    }
    return status;
}

// The K rows of d_walk_u / d_walk_theta / d_walk_logl (chol, wrapped uploaded) walked in rounds.  Leaves the end points in the walk
// buffers, moves completed in d_walk_steps (a walker the slim prior stage deferred: < nsteps), and synchronises the stream.
// *calls: likelihood calls consumed; *slots: candidates evaluated.
// Returns RVLL_E_UNSUPPORTED without having launched anything if the step's state does not fit (huge D).
// rw != null: run mode (RunWalk; d_walk_cost zeroed by the caller receives every walker's calls, the scalars lstar / seed /
// walker_base are not used)
int walk_rounds(rvll_handle* h, const WalkSwitches& sw, int64_t K, double lstar, int32_t nsteps, int32_t max_rounds, uint64_t seed,
                int64_t walker_base, long long* calls, long long* slots, const RunWalk* rw)
{
    Rounds R{h, sw, rw};
    rvll::LoglikeArgs a;
    RVLL_TRY(rounds_plan(h, K, nsteps, max_rounds, sw, &a, &R.p));
    const RoundsArena ar = rounds_arena(R.p, h->L.ndim);
    RVLL_TRY(rounds_reserve(R, ar, K, nsteps, seed, walker_base));
    RVLL_TRY(rounds_bind(R, ar, a, K, lstar, nsteps, max_rounds, seed, walker_base));
    RVLL_TRY(stamps_begin(R));
    RVLL_TRY(rounds_streams(R));
    const auto t_walk0 = steady_clock::now();
    const int status = rounds_issue(R);
    listed_dump(R);
    if (sw.geom_dump)
        fprintf(stderr, "[rounds host] %lld launches, %.2f us each inside the launch calls, walk %.2f ms\n", R.n_launch,
                R.n_launch ? R.launch_ns / 1e3 / R.n_launch : 0., duration_cast<nanoseconds>(steady_clock::now() - t_walk0).count() / 1e6);
    stamps_dump(R);
    if (status != RVLL_OK) return status;
    long long total = 0, evaluated = 0, rounds = 0;
    std::vector<long long> part(2 * (size_t)R.p.nblk);
    for (int g = 0; g < R.p.G; ++g) {
        HIP_TRY(hipMemcpy(part.data(), R.ga[(size_t)g].calls_part, sizeof(long long) * part.size(), hipMemcpyDeviceToHost));
        for (long long b = 0; b < R.p.nblk; ++b) { total += part[(size_t)b]; evaluated += part[(size_t)(R.p.nblk + b)]; }
        rounds = std::max(rounds, R.n_tile[(size_t)g]);
    }
    h->walk_rounds_used = (int)std::min<long long>(rounds, 0x7fffffff);
    *calls = total;
    *slots = evaluated;
    return RVLL_OK;
}

// ---- walk_core's passes ------------------------------------------------------------------------------------------------------
// a walk of the K rows in the walk's buffers in progress
struct Walk {
    rvll_handle* h;
    WalkSwitches sw;
    int64_t K;
    int32_t nsteps, max_rounds;
    RunWalk* rw;                          // run mode, or null
    bool so;                              // the stepout proposal
    // Slim walk (verified-table quantiles only, 4 waves per SIMD) when every Beta / Gamma prior has such a table;
    // walkers it could not finish come back with steps_done < nsteps and are finished by the fat kernel (finish_deferred).
    bool slim;
    // no more workgroups than the chip holds at once; freed walker slots draw the remaining rows from a queue
    // (RVLL_WALK_QUEUE, a measurement / test switch: 0 = one workgroup per PB rows, as many residency rounds as that
    // takes; n > 0 = as many workgroups as n compute units hold, so that a small walk goes through the queue too)
    int max_cus;
    rvll::LoglikeArgs a;                  // the tile of a launch over all K rows
    rvll::WalkArgs w;
    rvll::StepoutArgs so_args;
    long long total = 0;                  // likelihood calls so far
    std::vector<int32_t> steps, wf;       // [K] moves completed (slim), wandering ends: host copies (walk_totals)
    rvll::StepoutArgs* sop() { return so ? &so_args : nullptr; }   // (null: the chord walk)
};

// the tile and the fused arguments of a single-kernel launch over n rows
int walk_tile_args(const Walk& c, long long n, rvll::LoglikeArgs* a)
{
    rvll_handle* h = c.h;
    RVLL_TRY(build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], n, a));
    make_fused(h, h->d_cube, h->d_theta, a);
    a->defer = nullptr;                            // deferrals are per walker here (steps_done), not per batch
    // A Kepler solve that wanders is 30 - 350 sequential Newton steps, and its exact redo (correctly rounded sin / cos in
    // double-double, ~2 us a step per wave) holds up whatever waits for its tile — a whole round of the rounds form: with
    // the redo inside the walk's tiles 1.65e8 calls/s became 1.04e8 (a candidate in ten thousand wanders; a round of 16384
    // candidates nearly always has one).  So the walk's tiles evaluate such candidates with the ordinary sin / cos — the
    // accept decision cannot tell the two values apart unless they straddle lstar, 1e-9 of |log-L| apart — and report which
    // walkers END on one (w.wflag); their log-L is put right by redo_wandering, by the batch kernel, which carries the redo.
    a->cr_redo = c.sw.cr;                          // (measurement switch)
    const WalkTile t = walk_tile(a->PB, a->D, h->Ne, h->chunk_items, h->pb_override, n, [&](int pb, int ch) {
        rvll::LoglikeArgs b = *a;
        b.PB = pb;  b.CH = ch;
        return rvll::walk_lds_bytes(b, h->walk_prop);
    });
    if (!t.ok) return report_error(RVLL_E_UNSUPPORTED, "%d parameters exceed the walk kernel's LDS budget", a->D);
    a->PB = t.PB;  a->CH = t.CH;
    return RVLL_OK;
}

// stepout: scratch for the basis of every walker slot of a launch of n rows — grid x PB x D^2 doubles, not K x D^2; grown on
// demand, bounded (a walk that would need more is refused before anything is launched)
int basis_for(Walk& c, const rvll::LoglikeArgs& aa, long long n, bool fat)
{
    if (!c.so) return RVLL_OK;
    rvll_handle* h = c.h;
    const size_t D = (size_t)h->L.ndim;
    const long long nb = rvll::slice_walk_stepout_blocks(aa, n, fat, c.rw != nullptr, c.max_cus);
    if (nb < 1) return report_error(RVLL_E_HIP, "stepout walk: the occupancy query failed");
    const size_t need = (size_t)nb * (size_t)aa.PB * D * D;
    if (need > kStepoutBasisMax)
        return report_error(RVLL_E_UNSUPPORTED, "stepout walk: %lld walker slots x %zu^2 exceed the basis scratch's bound", nb * aa.PB, D);
    RVLL_TRY(grow(h, &h->d_walk_basis, &h->walk_basis_cap, need));
    c.so_args.basis = h->d_walk_basis;
    c.so_args.basis_slots = (long long)(h->walk_basis_cap / (D * D));
    return RVLL_OK;
}

int launch_walk(Walk& c, const rvll::LoglikeArgs& a, const rvll::WalkArgs& w, bool fat)
{
    RVLL_TRY(basis_for(c, a, w.K, fat));
    HIP_TRY(rvll::launch_slice_walk(a, w, fat, c.max_cus, c.h->compute, c.sop()));
    return RVLL_OK;
}

// the second part in the rows form: `order` [K2] in as many launches as the parked rows take
int second_rows(Walk& c, const std::vector<int32_t>& order, int64_t K2, long long resident)
{
    rvll_handle* h = c.h;
    hipStream_t st = h->compute;
    rvll::LoglikeArgs ar = c.a;
    int64_t G = walk_blocks(K2, c.a.PB, resident);
    const int nt = rows_threads(c.sw, c.slim);
    auto rows_lds = [&](int pb, int ch, int rows) { rvll::LoglikeArgs b = ar; b.PB = pb; b.CH = ch; return rvll::walk_rows_lds_bytes(b, rows); };
    if (nt != rvll::kThreads) {
        const WideRows wide = wide_rows(K2, c.max_cus > 0 ? c.max_cus : h->n_cu, nt, h->Ne, h->L.ndim, rows_lds);
        if (!wide.ok) return report_error(RVLL_E_UNSUPPORTED, "the wide walk does not fit %lld rows per workgroup", (long long)wide.rows);
        G = wide.G;  ar.PB = wide.PB;  ar.CH = wide.CH;
        RVLL_TRY(rvll_dev_reserve(h, std::max<int64_t>(c.K, G * ar.PB) + rvll::kMaxPointsPerBlock));   // the tiles' scratch rows
        ar.theta = h->d_theta; ar.logL = h->d_logL2[0]; ar.flags = h->d_flags2[0];
        make_fused(h, h->d_cube, h->d_theta, &ar);
        ar.defer = nullptr;
    }
    const int64_t chunk = G * rows_parked_max(rows_budget(nt), [&](int rows) { return rows_lds(ar.PB, ar.CH, rows); });
    HIP_TRY(hipMemcpyAsync(h->d_walk_order, order.data(), sizeof(int32_t) * (size_t)K2, hipMemcpyHostToDevice, st));
    for (int64_t lo = 0; lo < K2; lo += chunk) {
        const int64_t n = std::min<int64_t>(chunk, K2 - lo);
        rvll::WalkArgs wr = c.w;
        wr.K = n;
        wr.order = h->d_walk_order + lo;
        const int64_t g = std::min<int64_t>(G, (n + ar.PB - 1) / ar.PB);
        wr.rows_per_wg = (int)((n + g - 1) / g);
        HIP_TRY(rvll::launch_slice_walk_rows(ar, wr, !c.slim, (int)g, nt, st));
    }
    return RVLL_OK;
}

// ... through the queue, the most expensive rows dealt round the workgroups
int second_queue(Walk& c, std::vector<int32_t>& order, int64_t K2, long long resident)
{
    rvll_handle* h = c.h;
    deal_first_rows(&order, K2, walk_blocks(K2, c.a.PB, resident), c.a.PB);
    HIP_TRY(hipMemcpyAsync(h->d_walk_order, order.data(), sizeof(int32_t) * (size_t)K2, hipMemcpyHostToDevice, h->compute));
    HIP_TRY(hipMemsetAsync(h->d_walk_ncalls + kWalkWords - 1, 0, sizeof(unsigned long long), h->compute));   // the queue; the counts go on
    c.w.K = K2;
    c.w.order = h->d_walk_order;
    return launch_walk(c, c.a, c.w, !c.slim);
}

// the rest of a two-part walk, after its first c.w.nsteps moves: the rows by what they cost so far, then the moves left
int second_part(Walk& c, long long resident, bool rows_form)
{
    rvll_handle* h = c.h;
    hipStream_t st = h->compute;
    const int64_t K = c.K;
    const int first = c.w.nsteps;
    std::vector<int32_t> cost((size_t)K), done((size_t)K), order;
    HIP_TRY(hipMemcpyAsync(cost.data(), h->d_walk_cost, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(done.data(), h->d_walk_steps, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t K2 = order_by_cost(cost, done, first, c.max_rounds, &order);
    if (c.sw.cost_dump) {
        std::vector<int32_t> cs(cost);
        std::sort(cs.begin(), cs.end());
        double sum = 0; for (int32_t v : cs) sum += v;
        fprintf(stderr, "[walk cost, first %d moves] K=%lld mean %.1f  p50 %d  p90 %d  p99 %d  p99.9 %d  max %d\n", first, (long long)K,
                sum / (double)K, cs[(size_t)(K / 2)], cs[(size_t)(K * 9 / 10)], cs[(size_t)(K * 99 / 100)], cs[(size_t)(K * 999 / 1000)], cs.back());
    }
    c.w.nsteps = c.nsteps;
    c.w.cost = nullptr;
    if (c.rw) {                                        // the first part's calls; the second part counts afresh
        for (int64_t i = 0; i < K; ++i) c.rw->row_calls[(size_t)i] += cost[(size_t)i];
        HIP_TRY(hipMemsetAsync(h->d_walk_cost, 0, sizeof(int32_t) * (size_t)K, st));
        c.w.cost = h->d_walk_cost;
    }
    c.w.step_start = h->d_walk_steps;      // every row resumes where the first part left it (read before it is rewritten)
    if (K2 > 0) {
        RVLL_TRY(rows_form ? second_rows(c, order, K2, resident) : second_queue(c, order, K2, resident));
        HIP_TRY(hipStreamSynchronize(st));             // `order` goes out of scope
    }
    c.w.K = K;
    c.w.order = nullptr;
    c.w.step_start = nullptr;
    return RVLL_OK;
}

// the walk in one kernel, or in two parts (rvll_walk_plan.h, walk_two_parts)
int single_kernel_walk(Walk& c)
{
    rvll_handle* h = c.h;
    const long long resident = c.max_cus > 0 ? rvll::slice_walk_resident_blocks(c.a, !c.slim, c.max_cus) : 0;
    const bool two_parts = walk_two_parts(c.K, resident, c.a.PB, c.nsteps, c.sw);
    const bool rows_form = walk_rows_form(c.sw, c.a.PB, c.a.D, c.a.CH);
    if (two_parts) {
        c.w.nsteps = first_part_steps(c.nsteps, rows_form, c.sw);
        c.w.cost = h->d_walk_cost;
    }
    RVLL_TRY(launch_walk(c, c.a, c.w, !c.slim));
    return two_parts ? second_part(c, resident, rows_form) : RVLL_OK;
}

// the calls and slots of the launches so far (run mode: per row), the walkers' flags and moves completed; synchronises the stream
int walk_totals(Walk& c, long long rounds_calls, long long rounds_slots)
{
    rvll_handle* h = c.h;
    hipStream_t st = h->compute;
    const size_t K = (size_t)c.K;
    if (c.rw) RVLL_TRY(run_calls_add(h, c.rw, c.K, nullptr));   // the calls of the single-kernel launch (or its second part), or of the rounds
    unsigned long long evaluated[kWalkWords] = {};
    h->walk_evaluated = 0;
    c.steps.resize(c.slim ? K : 0);  c.wf.resize(K);
    HIP_TRY(hipMemcpyAsync(c.wf.data(), h->d_walk_wflag, sizeof(int32_t) * K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(evaluated, h->d_walk_ncalls, sizeof evaluated, hipMemcpyDeviceToHost, st));
    if (c.slim) HIP_TRY(hipMemcpyAsync(c.steps.data(), h->d_walk_steps, sizeof(int32_t) * K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c.total = (long long)evaluated[0] + rounds_calls;
    h->walk_evaluated = (long long)evaluated[1] + rounds_slots;
    for (int k = 0; k < 6; ++k) h->walk_phase[k] = evaluated[2 + k];
    if (c.sw.tile_dump && evaluated[6])       // diagnostic build: the tile's own phases inside the walk (100 MHz ticks)
        fprintf(stderr, "[walk tile phases, summed over %llu workgroups] stage %llu  decode %llu  items %llu  reduce+write %llu ticks\n",
                evaluated[6], evaluated[8], evaluated[9], evaluated[10], evaluated[11]);
    return RVLL_OK;
}

// Finish the walkers the slim stage interrupted with the full solvers inline: same seed, same walker index in the random-number
// counters, resumed at the start of the move that was interrupted.  Rare: the rows travel through the host (the whole buffers
// down, the interrupted rows compacted to their front, walked, and everything put back)
int finish_deferred(Walk& c)
{
    rvll_handle* h = c.h;
    hipStream_t st = h->compute;
    RunWalk* rw = c.rw;
    const size_t D = (size_t)h->L.ndim, K = (size_t)c.K;
    std::vector<int32_t> ids, start;
    for (size_t i = 0; i < c.steps.size(); ++i) {
        const int32_t ni = rw && rw->nsteps ? std::min(c.nsteps, rw->nsteps[rw->run[i]]) : c.nsteps;
        if (c.steps[i] < ni) { ids.push_back((int32_t)i); start.push_back(c.steps[i]); }
    }
    if (ids.empty()) return RVLL_OK;
    const size_t M = ids.size();
    std::vector<double> hu(D * K), hth(D * K), hl(K), su(M * D), sth(M * D), sl(M);
    RVLL_TRY(walk_rows_download(h, hu.data(), hth.data(), hl.data(), c.K));
    for (size_t j = 0; j < M; ++j) {
        memcpy(&su[j * D], &hu[(size_t)ids[j] * D], sizeof(double) * D);
        memcpy(&sth[j * D], &hth[(size_t)ids[j] * D], sizeof(double) * D);
        sl[j] = hl[(size_t)ids[j]];
    }
    RVLL_TRY(walk_rows_upload(h, su.data(), sth.data(), sl.data(), (int64_t)M));
    std::vector<int32_t> wid_sub(ids), run_sub;
    if (rw) {                                  // run mode: the rows' indices inside their runs, and their runs
        run_sub.resize(M);
        for (size_t j = 0; j < M; ++j) { wid_sub[j] = rw->rid[(size_t)ids[j]]; run_sub[j] = rw->run[(size_t)ids[j]]; }
        HIP_TRY(hipMemcpyAsync(h->d_walk_run, run_sub.data(), sizeof(int32_t) * M, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(h->d_walk_cost, 0, sizeof(int32_t) * M, st));
    }
    HIP_TRY(hipMemcpyAsync(h->d_walk_wid, wid_sub.data(), sizeof(int32_t) * M, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_walk_start, start.data(), sizeof(int32_t) * M, hipMemcpyHostToDevice, st));
    std::vector<int32_t> wf_sub(M);
    for (size_t j = 0; j < M; ++j) wf_sub[j] = c.wf[(size_t)ids[j]];
    HIP_TRY(hipMemcpyAsync(h->d_walk_wflag, wf_sub.data(), sizeof(int32_t) * M, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->d_walk_ncalls, 0, kWalkWords * sizeof(unsigned long long), st));
    rvll::LoglikeArgs a2;
    RVLL_TRY(walk_tile_args(c, (long long)M, &a2));
    rvll::WalkArgs w2 = c.w;
    w2.K = (long long)M;
    w2.walker_id = h->d_walk_wid;
    w2.step_start = h->d_walk_start;
    if (rw) w2.cost = h->d_walk_cost;
    RVLL_TRY(launch_walk(c, a2, w2, true));
    unsigned long long evaluated[kWalkWords] = {};
    HIP_TRY(hipMemcpyAsync(wf_sub.data(), h->d_walk_wflag, sizeof(int32_t) * M, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(evaluated, h->d_walk_ncalls, sizeof evaluated, hipMemcpyDeviceToHost, st));
    RVLL_TRY(walk_rows_download(h, su.data(), sth.data(), sl.data(), (int64_t)M));
    c.total += (long long)evaluated[0];
    if (rw) RVLL_TRY(run_calls_add(h, rw, (int64_t)M, ids.data()));
    h->walk_evaluated += (long long)evaluated[1];
    for (int k = 0; k < 6; ++k) h->walk_phase[k] += evaluated[2 + k];
    for (size_t j = 0; j < M; ++j) {
        memcpy(&hu[(size_t)ids[j] * D], &su[j * D], sizeof(double) * D);
        memcpy(&hth[(size_t)ids[j] * D], &sth[j * D], sizeof(double) * D);
        hl[(size_t)ids[j]] = sl[j];
        c.wf[(size_t)ids[j]] = wf_sub[j];
    }
    RVLL_TRY(walk_rows_upload(h, hu.data(), hth.data(), hl.data(), c.K));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

// the walkers that END on a candidate with a wandering solve: their log-L as the batch kernel gives it (the exact redo the
// walk's tiles leave out) — a handful of rows in a million candidates, gathered, evaluated, scattered back
int redo_wandering(Walk& c)
{
    rvll_handle* h = c.h;
    hipStream_t st = h->compute;
    std::vector<int32_t> rows;
    for (int64_t i = 0; h->wander_exact && i < c.K; ++i) if (c.wf[(size_t)i]) rows.push_back((int32_t)i);
    if (rows.empty()) return RVLL_OK;
    const int64_t n = (int64_t)rows.size();
    HIP_TRY(hipMemcpyAsync(h->d_walk_order, rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(rvll::launch_gather_rows(h->d_walk_theta, h->d_walk_order, n, h->L.ndim, h->d_theta, st));
    rvll::LoglikeArgs ax;
    int cu = 0;
    RVLL_TRY(build_args(h, h->d_theta, h->d_logL2[0], h->d_flags2[0], n, &ax, &cu));
    HIP_TRY(cu > 0 ? rvll::launch_loglike_cu(ax, cu, st) : rvll::launch_loglike(ax, st));
    HIP_TRY(rvll::launch_scatter_rows(h->d_logL2[0], h->d_walk_order, n, 1, h->d_walk_logl, st));
    HIP_TRY(hipStreamSynchronize(st));         // `rows` goes out of scope
    return RVLL_OK;
}

}  // namespace

namespace rvll {
namespace host {

// device buffers of the walk for K rows (grown on demand)
int walk_reserve(rvll_handle* h, int64_t K)
{
    const size_t D = (size_t)h->L.ndim;
    RVLL_TRY(rvll_dev_reserve(h, K + rvll::kMaxPointsPerBlock));   // scratch rows (one tile per workgroup): d_theta, log-L / flags of lane 0
    RVLL_TRY(sync_other_lanes(h));
    if (K <= h->walk_cap && h->d_walk_chol) return RVLL_OK;
    const size_t cap = (size_t)std::max<long long>(K, 1024);
    h->walk_cap = 0;                               // (the rows' buffers share it)
    RVLL_TRY(renew(h, &h->d_walk_u, D * cap));  RVLL_TRY(renew(h, &h->d_walk_theta, D * cap));  RVLL_TRY(renew(h, &h->d_walk_logl, cap));
    RVLL_TRY(renew(h, &h->d_walk_steps, cap));  RVLL_TRY(renew(h, &h->d_walk_wid, cap));  RVLL_TRY(renew(h, &h->d_walk_start, cap));
    RVLL_TRY(renew(h, &h->d_walk_cost, cap));  RVLL_TRY(renew(h, &h->d_walk_order, cap));  RVLL_TRY(renew(h, &h->d_walk_wflag, cap));
    if (!h->d_walk_chol) {
        HIP_TRY(hipMalloc(&h->d_walk_chol, sizeof(double) * D * D));
        HIP_TRY(hipMalloc(&h->d_walk_wrapped, sizeof(int32_t) * D));
        HIP_TRY(hipMalloc(&h->d_walk_ncalls, kWalkWords * sizeof(unsigned long long)));   // calls used, tile slots evaluated, diagnostic bins
    }
    h->walk_cap = (long long)cap;
    return RVLL_OK;
}

// the walk's buffers for K rows in run mode, and the tables of R runs (grown on demand)
int runs_reserve(rvll_handle* h, int64_t K, int64_t R)
{
    const size_t D = (size_t)h->L.ndim;
    RVLL_TRY(walk_reserve(h, K));
    RVLL_TRY(grow(h, &h->d_walk_run, &h->runs_rows_cap, (size_t)K, (size_t)h->walk_cap));
    if (R <= h->runs_cap) return RVLL_OK;
    const size_t cap = (size_t)std::max<int64_t>(R, 64);
    h->runs_cap = 0;                               // (the runs' tables share it)
    RVLL_TRY(renew(h, &h->d_run_nsteps, cap));  RVLL_TRY(renew(h, &h->d_run_lstar, cap));  RVLL_TRY(renew(h, &h->d_run_seed, cap));
    RVLL_TRY(renew(h, &h->d_run_chol, D * D * cap));
    h->runs_cap = (long long)cap;
    return RVLL_OK;
}

// The walk of the K rows resident in d_walk_u / d_walk_theta / d_walk_logl (chol and wrapped already uploaded): every
// launch it takes — the rounds, or the first part and the rest (rows dealt to the workgroups by what they cost so far), the
// full-solver finish of rows the slim kernel deferred — leaves the end points in those buffers.  Synchronises the compute stream.
// rw != null: run mode (RunWalk; lstar / seed are not used, walker_base is 0): every launch also counts the calls of each
// row into rw->row_calls.  The rows form (RVLL_WALK_ROWS) has no run mode.
int walk_core(rvll_handle* h, int64_t K, double lstar, int32_t nsteps, int32_t max_rounds, uint64_t seed,
              int64_t walker_base, int64_t* ncalls, RunWalk* rw = nullptr)
{
    hipStream_t st = h->compute;
    Walk c{h, read_walk_switches(), K, nsteps, max_rounds, rw};
    // the stepout proposal (rvll_set_walk_proposal) runs in the single-kernel forms only: not in the rounds form
    // (its direction table holds one unit direction per move), not in the rows form
    c.so = h->walk_prop == RVLL_PROPOSAL_STEPOUT;
    RVLL_TRY(rows_form_refusal(c.sw, c.so, rw != nullptr));
    if (c.so && h->L.ndim > rvll::kStepoutMaxD) return report_error(RVLL_E_UNSUPPORTED, "stepout walks take at most %d parameters", rvll::kStepoutMaxD);
    if (rw) HIP_TRY(hipMemsetAsync(h->d_walk_cost, 0, sizeof(int32_t) * (size_t)K, st));
    HIP_TRY(hipMemsetAsync(h->d_walk_ncalls, 0, kWalkWords * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(h->d_walk_wflag, 0, sizeof(int32_t) * (size_t)K, st));
    RVLL_TRY(walk_tile_args(c, K, &c.a));
    c.slim = h->all_direct && !c.sw.fat;
    c.max_cus = walk_max_cus(c.sw, h->n_cu);
    const int spec = c.sw.spec ? c.sw.spec : std::max(1, std::min(h->walk_spec, rvll::kMaxPointsPerBlock));   // (RVLL_WALK_SPEC=1: no speculation)
    c.w = rvll::WalkArgs{h->d_walk_u, h->d_walk_theta, h->d_walk_logl, h->d_walk_chol, h->d_walk_wrapped, (long long)K,
                         nsteps, max_rounds, (unsigned long long)seed, lstar, h->d_walk_ncalls,
                         h->d_walk_steps, nullptr, nullptr, (long long)walker_base, spec, h->d_walk_ncalls + 1,
                         h->d_walk_ncalls + kWalkWords - 1, nullptr, nullptr, 0, h->d_walk_wflag};
    if (rw) {
        c.w.run = h->d_walk_run;  c.w.run_lstar = h->d_run_lstar;  c.w.run_seed = h->d_run_seed;  c.w.run_chol = h->d_run_chol;
        c.w.walker_id = h->d_walk_wid;                   // the row's index inside its run
        c.w.cost = h->d_walk_cost;                       // every launch counts every row's calls
        if (rw->nsteps) c.w.run_nsteps = h->d_run_nsteps;
    }
    c.so_args = rvll::StepoutArgs{h->walk_width, nullptr, 0};
    // the rounds form takes every walk the slim stage applies to; the single-kernel forms remain for the full-solver walk, for
    // the rows the rounds form hands back (deferred at a candidate the tables do not cover), and behind their switches
    long long rounds_calls = 0, rounds_slots = 0;
    bool by_rounds = false;
    h->walk_rounds_used = 0;
    if (c.slim && !c.so && rounds_wanted(K, c.sw) && !(rw && rw->nsteps)) {
        const int rc = walk_rounds(h, c.sw, K, lstar, nsteps, max_rounds, seed, walker_base, &rounds_calls, &rounds_slots, rw);
        if (rc != RVLL_OK && rc != RVLL_E_UNSUPPORTED) return rc;
        by_rounds = rc == RVLL_OK;
    }
    if (!by_rounds) RVLL_TRY(single_kernel_walk(c));
    RVLL_TRY(walk_totals(c, rounds_calls, rounds_slots));
    RVLL_TRY(finish_deferred(c));
    RVLL_TRY(redo_wandering(c));
    if (ncalls) *ncalls = (int64_t)c.total;
    h->theta_async = false;
    return RVLL_OK;
}

int walk_check_args(rvll_handle* h, int64_t K, int32_t nsteps, int32_t max_rounds, int64_t walker_base, const int32_t* wrapped)
{
    if (!h->have_priors) return report_error(RVLL_E_NOPRIORS, "rvll_set_priors has not been called");
    if (K < 0 || nsteps < 0) return report_error(RVLL_E_INVALID, "negative size");
    if (max_rounds < 1 || max_rounds > 4096 || nsteps >= (1 << 18) || K >= (1LL << 31) || walker_base < 0 ||
        walker_base + K >= (1LL << 32))
        return report_error(RVLL_E_INVALID, "nsteps / max_rounds / K / walker_base out of range");
    if (h->L.ndim < 1) return report_error(RVLL_E_INVALID, "no free parameter to walk in");
    if (h->walk_prop == RVLL_PROPOSAL_STEPOUT) {       // nothing would bound the bracket's stepping out
        bool all = wrapped != nullptr;
        for (int k = 0; all && k < h->L.ndim; ++k) all = wrapped[k] != 0;
        if (all) return report_error(RVLL_E_INVALID, "a stepout walk needs at least one parameter that is not wrapped");
    }
    return RVLL_OK;
}

// chol may be null (run mode: the factors are the runs')
int walk_upload_frame(rvll_handle* h, const double* chol, const int32_t* wrapped)
{
    const size_t D = (size_t)h->L.ndim;
    std::vector<int32_t> wr(D, 0);
    if (wrapped) for (size_t k = 0; k < D; ++k) wr[k] = wrapped[k] != 0;
    if (chol) HIP_TRY(hipMemcpyAsync(h->d_walk_chol, chol, sizeof(double) * D * D, hipMemcpyHostToDevice, h->compute));
    HIP_TRY(hipMemcpyAsync(h->d_walk_wrapped, wr.data(), sizeof(int32_t) * D, hipMemcpyHostToDevice, h->compute));
    HIP_TRY(hipStreamSynchronize(h->compute));         // wr (and pageable sources) may go out of scope
    return RVLL_OK;
}

// a per-run step table nsteps [n] (rvll_slice_walk_runs_steps, rvll_live_runs_step_steps): every count in range; *most its largest,
// *uniform whether all are equal (then the walk is the scalar one of `most` moves, every form open to it)
int steps_range(const char* who, const int32_t* nsteps, int32_t n, int32_t* most, bool* uniform)
{
    if (n > 0 && !nsteps) return report_error(RVLL_E_INVALID, "%s: null step table", who);
    int32_t hi = 0, lo = n > 0 ? nsteps[0] : 0;
    for (int32_t r = 0; r < n; ++r) {
        if (nsteps[r] < 0 || nsteps[r] >= (1 << 18))
            return report_error(RVLL_E_INVALID, "%s: nsteps[%d] = %d out of range", who, (int)r, (int)nsteps[r]);
        hi = std::max(hi, nsteps[r]);
        lo = std::min(lo, nsteps[r]);
    }
    *most = hi;
    *uniform = lo == hi;
    return RVLL_OK;
}

}  // namespace host
}  // namespace rvll

namespace {

// rvll_slice_walk_runs (steps = null: every run makes nsteps moves) and rvll_slice_walk_runs_steps (steps [R]: run r makes
// steps[r]; nsteps is their largest)
int slice_walk_runs_impl(rvll_handle* h, double* cube, double* theta, double* logl, const int64_t* run_start, int32_t R,
                         const double* lstar, const double* chol, const uint64_t* seed, const int32_t* wrapped,
                         const int32_t* steps, int32_t nsteps, int32_t max_rounds, int64_t* ncalls)
{
    RVLL_TRY(use_device(h));
    if (R < 0 || (R > 0 && !run_start)) return report_error(RVLL_E_INVALID, "rvll_slice_walk_runs: bad run table");
    if (ncalls) for (int32_t r = 0; r < R; ++r) ncalls[r] = 0;
    if (R > 0 && run_start[0] != 0) return report_error(RVLL_E_INVALID, "rvll_slice_walk_runs: run_start[0] must be 0");
    for (int32_t r = 0; r < R; ++r)
        if (run_start[r + 1] < run_start[r]) return report_error(RVLL_E_INVALID, "rvll_slice_walk_runs: run_start decreases at run %d", (int)r);
    const int64_t K = R > 0 ? run_start[R] : 0;
    RVLL_TRY(walk_check_args(h, K, nsteps, max_rounds, 0, wrapped));
    if (K == 0 || nsteps == 0) return RVLL_OK;
    if (!cube || !theta || !logl || !lstar || !chol || !seed) return report_error(RVLL_E_INVALID, "null buffer");
    RVLL_TRY(rows_form_refusal(read_walk_switches(), false, true));      // (before anything is reserved or uploaded)
    const size_t D = (size_t)h->L.ndim;
    RVLL_TRY(runs_reserve(h, K, R));
    hipStream_t st = h->compute;
    std::vector<int32_t> run((size_t)K), rid((size_t)K);
    for (int32_t r = 0; r < R; ++r)
        for (int64_t i = run_start[r]; i < run_start[r + 1]; ++i) { run[(size_t)i] = r; rid[(size_t)i] = (int32_t)(i - run_start[r]); }
    RVLL_TRY(walk_rows_upload(h, cube, theta, logl, K));
    HIP_TRY(hipMemcpyAsync(h->d_walk_run, run.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_walk_wid, rid.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_run_lstar, lstar, sizeof(double) * (size_t)R, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_run_seed, seed, sizeof(uint64_t) * (size_t)R, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_run_chol, chol, sizeof(double) * D * D * (size_t)R, hipMemcpyHostToDevice, st));
    if (steps) HIP_TRY(hipMemcpyAsync(h->d_run_nsteps, steps, sizeof(int32_t) * (size_t)R, hipMemcpyHostToDevice, st));
    RVLL_TRY(walk_upload_frame(h, nullptr, wrapped));       // (synchronises: the host tables above may go out of scope after it)
    RunWalk rw{run.data(), rid.data(), std::vector<long long>((size_t)K, 0), steps};
    RVLL_TRY(walk_core(h, K, 0., nsteps, max_rounds, 0, 0, nullptr, &rw));
    RVLL_TRY(walk_rows_download(h, cube, theta, logl, K));
    if (ncalls)
        for (int32_t r = 0; r < R; ++r)
            for (int64_t i = run_start[r]; i < run_start[r + 1]; ++i) ncalls[r] += rw.row_calls[(size_t)i];
    return RVLL_OK;
}

}  // namespace

extern "C" {

int rvll_slice_walk(rvll_handle* h, double* cube, double* theta, double* logl, int64_t K, double lstar,
                    const double* chol, const int32_t* wrapped, int32_t nsteps, int32_t max_rounds,
                    uint64_t seed, int64_t walker_base, int64_t* ncalls)
{
    RVLL_TRY(use_device(h));
    if (ncalls) *ncalls = 0;
    RVLL_TRY(walk_check_args(h, K, nsteps, max_rounds, walker_base, wrapped));
    if (K == 0 || nsteps == 0) return RVLL_OK;
    if (!cube || !theta || !logl || !chol) return report_error(RVLL_E_INVALID, "null buffer");
    RVLL_TRY(walk_reserve(h, K));
    RVLL_TRY(walk_rows_upload(h, cube, theta, logl, K));
    RVLL_TRY(walk_upload_frame(h, chol, wrapped));
    RVLL_TRY(walk_core(h, K, lstar, nsteps, max_rounds, seed, walker_base, ncalls));
    return walk_rows_download(h, cube, theta, logl, K);
}

int rvll_slice_walk_runs(rvll_handle* h, double* cube, double* theta, double* logl, const int64_t* run_start, int32_t R,
                         const double* lstar, const double* chol, const uint64_t* seed, const int32_t* wrapped,
                         int32_t nsteps, int32_t max_rounds, int64_t* ncalls)
{
    return slice_walk_runs_impl(h, cube, theta, logl, run_start, R, lstar, chol, seed, wrapped, nullptr, nsteps, max_rounds, ncalls);
}

int rvll_slice_walk_runs_steps(rvll_handle* h, double* cube, double* theta, double* logl, const int64_t* run_start, int32_t R,
                               const double* lstar, const double* chol, const uint64_t* seed, const int32_t* wrapped,
                               const int32_t* nsteps, int32_t max_rounds, int64_t* ncalls)
{
    int32_t most = 0;
    bool uniform = true;
    RVLL_TRY(steps_range("rvll_slice_walk_runs_steps", nsteps, R, &most, &uniform));
    // a uniform table is the scalar walk (every form open to it); otherwise the rows stop at their run's count
    return slice_walk_runs_impl(h, cube, theta, logl, run_start, R, lstar, chol, seed, wrapped, uniform ? nullptr : nsteps, most,
                                max_rounds, ncalls);
}

int rvll_set_walk_proposal(rvll_handle* h, int32_t kind, double width)
{
    if (!h) return report_error(RVLL_E_INVALID, "null handle");
    if (kind != RVLL_PROPOSAL_CHORD && kind != RVLL_PROPOSAL_STEPOUT) return report_error(RVLL_E_INVALID, "unknown proposal %d", kind);
    if (!(width > 0.) || !std::isfinite(width)) return report_error(RVLL_E_INVALID, "the step width must be positive and finite");
    h->walk_prop = kind;
    h->walk_width = width;
    return RVLL_OK;
}

int rvll_set_walk_speculation(rvll_handle* h, int32_t max_ahead)
{
    if (!h) return report_error(RVLL_E_INVALID, "null handle");
    if (max_ahead < 1 || max_ahead > rvll::kMaxPointsPerBlock)
        return report_error(RVLL_E_INVALID, "max_ahead must be in [1, %d]", rvll::kMaxPointsPerBlock);
    h->walk_spec = max_ahead;
    h->walk_spec_rounds = max_ahead;
    return RVLL_OK;
}

int rvll_slice_walk_evaluated(rvll_handle* h, int64_t* evaluated)
{
    if (!h || !evaluated) return report_error(RVLL_E_INVALID, "null argument");
    *evaluated = h->walk_evaluated;
    return RVLL_OK;
}

int rvll_slice_walk_rounds(rvll_handle* h, int32_t* rounds)
{
    if (!h || !rounds) return report_error(RVLL_E_INVALID, "null argument");
    *rounds = h->walk_rounds_used;
    return RVLL_OK;
}

int rvll_slice_walk_phases(rvll_handle* h, uint64_t out[6])
{
    if (!h || !out) return report_error(RVLL_E_INVALID, "null argument");
    for (int k = 0; k < 6; ++k) out[k] = h->walk_phase[k];
    return RVLL_OK;
}

}  // extern "C"
