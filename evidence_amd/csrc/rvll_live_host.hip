// rvll_live_host.hip — host side of nested sampling's live set kept in HBM: the one-run live set (rvll_live_*)
// and the resident ensemble (rvll_live_runs_*), their dead stores and birth contours, and the stages their steps are built from.
// Entry points of include/rvll.h; the kernels are in rvll_live.hip, the walk itself is walk_core of rvll_walk_host.hip.
#include <chrono>
#include "rvll_host.h"
#include "rvll_step_groups.h"

using rvll::report_error;
using namespace rvll::host;

namespace {

// The whitening factor of the resident live set: the lower Cholesky - Banachiewicz factor of cov + 1e-14 on the diagonal (as
// evidence_amd/nested.py adds), factor [D, D] zero above the diagonal.  Host arithmetic (19 x 19 at most in practice), shared by
// every resident step so that they cannot drift apart.  False: not positive definite.
bool whitening_factor(const double* cov, size_t D, double* factor)
{
    std::fill(factor, factor + D * D, 0.);
    for (size_t j = 0; j < D; ++j) {
        for (size_t l = 0; l <= j; ++l) {
            double sum = cov[j * D + l] + (j == l ? 1e-14 : 0.);
            for (size_t m = 0; m < l; ++m) sum -= factor[j * D + m] * factor[l * D + m];
            if (j == l) {
                if (!(sum > 0.)) return false;
                factor[j * D + j] = std::sqrt(sum);
            } else {
                factor[j * D + l] = sum / factor[l * D + l];
            }
        }
    }
    return true;
}

// room in the dead store for `add` more rows (grown to at least dead_n + 4 grow rows, the rows kept)
int dead_reserve(rvll_handle* h, long long add, long long grow, const char* who)
{
    if (h->dead_n + add <= h->dead_cap) return RVLL_OK;
    const size_t D = (size_t)h->L.ndim;
    hipStream_t st = h->compute;
    const long long cap = std::max<long long>(2 * h->dead_cap, h->dead_n + 4 * grow);
    double *nt = nullptr, *nl = nullptr, *nb = nullptr;
    HIP_TRY(hipMalloc(&nt, sizeof(double) * D * (size_t)cap));
    {
        hipError_t e = hipMalloc(&nl, sizeof(double) * (size_t)cap);
        if (e == hipSuccess) e = hipMalloc(&nb, sizeof(double) * (size_t)cap);
        if (e != hipSuccess) {
            (void)hipFree(nt); if (nl) (void)hipFree(nl);
            return report_error(e == hipErrorOutOfMemory ? RVLL_E_NOMEM : RVLL_E_HIP, "%s: dead store: %s", who, hipGetErrorString(e));
        }
    }
    if (h->dead_n) {
        hipError_t e = hipMemcpyAsync(nt, h->d_dead_theta, sizeof(double) * D * (size_t)h->dead_n, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(nl, h->d_dead_logl, sizeof(double) * (size_t)h->dead_n, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(nb, h->d_dead_birth, sizeof(double) * (size_t)h->dead_n, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(nt); (void)hipFree(nl); (void)hipFree(nb);
            return report_error(RVLL_E_HIP, "%s: dead store: %s", who, hipGetErrorString(e));
        }
    }
    dev_free(h->d_dead_theta); dev_free(h->d_dead_logl); dev_free(h->d_dead_birth);
    h->d_dead_theta = nt; h->d_dead_logl = nl; h->d_dead_birth = nb; h->dead_cap = cap;
    return RVLL_OK;
}

// N unit-cube rows -> prior transform -> log-L into the resident live buffers d_live_u / _theta / _logl (grown on demand), births
// -inf;
// logl_out [N] may be NULL.  Shared by the one-run live set and the ensemble; the caller keeps the state.
int live_load(rvll_handle* h, const double* cube, int64_t N, double* logl_out)
{
    const size_t D = (size_t)std::max(1, h->L.ndim);
    RVLL_TRY(rvll_dev_upload_cube(h, cube, N));
    RVLL_TRY(rvll_dev_prior_loglike(h, N));
    RVLL_TRY(rvll_dev_sync(h));
    RVLL_TRY(use_device(h));                                  // (elements the table-only prior stage handed over are redone here)
    if (N > h->live_cap) {
        dev_free(h->d_live_u); dev_free(h->d_live_theta); dev_free(h->d_live_logl); dev_free(h->d_live_birth); dev_free(h->d_live_idx);
        dev_free(h->d_sort_keys); dev_free(h->d_sort_rows);
        h->live_cap = 0;
        HIP_TRY(hipMalloc(&h->d_live_u, sizeof(double) * D * (size_t)N));
        HIP_TRY(hipMalloc(&h->d_live_theta, sizeof(double) * D * (size_t)N));
        HIP_TRY(hipMalloc(&h->d_live_logl, sizeof(double) * (size_t)N));
        HIP_TRY(hipMalloc(&h->d_live_birth, sizeof(double) * (size_t)N));
        HIP_TRY(hipMalloc(&h->d_live_idx, sizeof(int32_t) * 2 * (size_t)N));
        HIP_TRY(hipMalloc(&h->d_sort_keys, sizeof(unsigned long long) * 2 * (size_t)N));
        HIP_TRY(hipMalloc(&h->d_sort_rows, sizeof(int32_t) * (size_t)N));
        h->live_cap = N;
    }
    if (!h->d_live_mom) HIP_TRY(hipMalloc(&h->d_live_mom, sizeof(double) * (rvll::moments_scratch_doubles((int)D) + D + D * D)));
    hipStream_t st = h->compute;
    HIP_TRY(hipMemcpyAsync(h->d_live_u, h->d_cube, sizeof(double) * D * (size_t)N, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_live_theta, h->d_theta, sizeof(double) * D * (size_t)N, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_live_logl, h->d_logL2[h->logl_last], sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, st));
    HIP_TRY(rvll::launch_fill(h->d_live_birth, N, -INFINITY, st));       // drawn from the whole prior: born at -inf
    if (logl_out) HIP_TRY(hipMemcpyAsync(logl_out, h->d_live_logl, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

// the sorts' scratch d_sort_temp grown to `need` bytes
int sort_temp_reserve(rvll_handle* h, size_t need)
{
    return grow(h, &h->d_sort_temp, &h->sort_temp_bytes, need);
}

// ---- the stages of a resident step (DESIGN §4d "Resident ensemble", §4e): rvll_live_step and the two ensemble steps list them ------
// A step that fails leaves every run as it was: nothing before finish_and_commit changes a live row, and the dead store's rows behind
// dead_n, which retire_rows writes, are nobody's until finish_and_commit moves dead_n on — last, and nowhere else.

// the dying rows d_dying [K] copied behind the dead store's dead_n rows (room made by dead_reserve) before the step overwrites them
int retire_rows(rvll_handle* h, const int32_t* d_dying, int64_t K)
{
    const int Di = h->L.ndim;
    HIP_TRY(rvll::launch_gather_rows(h->d_live_theta, d_dying, K, Di, h->d_dead_theta + (size_t)h->dead_n * (size_t)Di, h->compute));
    HIP_TRY(rvll::launch_gather_rows(h->d_live_logl, d_dying, K, 1, h->d_dead_logl + h->dead_n, h->compute));
    return RVLL_OK;
}

// the walkers start from the live rows d_rows [K]: walk row e from row d_rows[e]
int gather_walkers(rvll_handle* h, const int32_t* d_rows, int64_t K)
{
    const int Di = h->L.ndim;
    HIP_TRY(rvll::launch_gather_rows(h->d_live_u, d_rows, K, Di, h->d_walk_u, h->compute));
    HIP_TRY(rvll::launch_gather_rows(h->d_live_theta, d_rows, K, Di, h->d_walk_theta, h->compute));
    HIP_TRY(rvll::launch_gather_rows(h->d_live_logl, d_rows, K, 1, h->d_walk_logl, h->compute));
    return RVLL_OK;
}

// The end of a step.  The dying rows d_dying [K] (the dead store's order: run a's kdead at a kdead) hand their births to the dead
// store and are born again at `lstar`, or with lstar_slot at their run's: its highest dying log-L, slot a kdead + kdead - 1 of this
// step's block in the dead store.  The walk's end points replace the rows d_scatter [K] (the dying rows in the walk's order), the new
// log-L comes down into logl_walk [K] and the stream is synchronised.  Only then — the commit point — the listed runs (null: the
// one-run live set) get their pieces of the dead store and dead_n moves on.
int finish_and_commit(rvll_handle* h, const int32_t* d_dying, const int32_t* d_scatter, int64_t K, int64_t kdead, bool lstar_slot,
                      double lstar, double* logl_walk, const int32_t* runs, int32_t A)
{
    const int Di = h->L.ndim;
    hipStream_t st = h->compute;
    HIP_TRY(rvll::launch_births_step(d_dying, K, kdead, lstar_slot ? h->d_dead_logl + h->dead_n + (kdead - 1) : nullptr, lstar,
                                     h->d_live_birth, h->d_dead_birth + h->dead_n, st));
    HIP_TRY(rvll::launch_scatter_rows(h->d_walk_u, d_scatter, K, Di, h->d_live_u, st));
    HIP_TRY(rvll::launch_scatter_rows(h->d_walk_theta, d_scatter, K, Di, h->d_live_theta, st));
    HIP_TRY(rvll::launch_scatter_rows(h->d_walk_logl, d_scatter, K, 1, h->d_live_logl, st));
    HIP_TRY(hipMemcpyAsync(logl_walk, h->d_walk_logl, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int32_t a = 0; a < A; ++a) h->runs_dead[(size_t)runs[a]].emplace_back(h->dead_n + (long long)a * kdead, (long long)kdead);
    h->dead_n += K;
    return RVLL_OK;
}

// The step-count adaptation's distances of an ensemble step (on: the caller passed move_out or pair_out), over the walk's
// groups G.  stage() keeps the walkers' start rows and groups before the walk (walk_core may reuse d_walk_run); measure(), behind the
// walk, takes group g's survivors as rows d_idx[gofs[g] .. + gcnt[g]] of d_rows and its factor as the walk's, and starts the downloads
// that finish_and_commit's synchronisation completes.
struct StepDistances {
    bool on;
    double* d_wstart = nullptr;
    int32_t* d_wgroup = nullptr;
    std::vector<int32_t> tables;
    std::vector<double> hmove, hpair;

    int stage(rvll_handle* h, const StepGroups& G)
    {
        if (!on) return RVLL_OK;
        const size_t K = G.perm.size(), D = (size_t)h->L.ndim;
        RVLL_TRY(adapt_in_reserve(h, 8 * K * D + 4 * K + 16));
        d_wstart = static_cast<double*>(h->d_adapt_in);
        d_wgroup = reinterpret_cast<int32_t*>(d_wstart + K * D);
        HIP_TRY(hipMemcpyAsync(d_wstart, h->d_walk_u, 8 * K * D, hipMemcpyDeviceToDevice, h->compute));
        HIP_TRY(hipMemcpyAsync(d_wgroup, G.grun.data(), 4 * K, hipMemcpyHostToDevice, h->compute));
        return RVLL_OK;
    }
    int measure(rvll_handle* h, const double* d_rows, const int32_t* d_idx, const StepGroups& G, const int32_t* wrapped)
    {
        if (!on) return RVLL_OK;
        const size_t K = G.perm.size();
        double *d_pair = nullptr, *d_move = nullptr;
        RVLL_TRY(walk_distances_core(h, d_rows, d_idx, G.gofs, G.gcnt, h->d_run_chol, wrapped_mask(wrapped, h->L.ndim), d_wstart,
                                     h->d_walk_u, d_wgroup, (int64_t)K, &d_pair, &d_move, tables));
        hmove.resize(K); hpair.resize(G.gofs.size());
        HIP_TRY(hipMemcpyAsync(hmove.data(), d_move, 8 * K, hipMemcpyDeviceToHost, h->compute));
        if (!G.gofs.empty()) HIP_TRY(hipMemcpyAsync(hpair.data(), d_pair, 8 * G.gofs.size(), hipMemcpyDeviceToHost, h->compute));
        return RVLL_OK;
    }
};

// walk order -> the caller's walker order (walk row e is walker G.perm[e] = a kdead + i): new log-L, calls per listed run, distances
void step_outputs(const StepGroups& G, int64_t kdead, const double* logl_walk, const std::vector<long long>& row_calls,
                  const StepDistances& dist, double* logl_new, int64_t* ncalls, double* move_out, double* pair_out)
{
    for (size_t e = 0; e < G.perm.size(); ++e) {
        const int32_t w = G.perm[e];
        logl_new[w] = logl_walk[e];
        if (ncalls) ncalls[w / kdead] += row_calls[e];
        if (move_out) move_out[w] = dist.hmove[e];
        if (pair_out) pair_out[w] = dist.hpair[(size_t)G.grun[e]];
    }
}

// the listed runs of a rvll_live_runs_sort / _step: distinct, ascending, below R
int runs_check(rvll_handle* h, const int32_t* runs, int32_t A, int64_t kdead, const char* who)
{
    if (h->runs_R < 1) return report_error(RVLL_E_INVALID, "%s: rvll_live_runs_init has not been called", who);
    if (!runs || A < 1 || A > h->runs_R) return report_error(RVLL_E_INVALID, "%s: bad run list", who);
    if (kdead < 1 || kdead >= h->runs_n) return report_error(RVLL_E_INVALID, "%s: kdead must be in [1, n)", who);
    for (int32_t a = 0; a < A; ++a)
        if (runs[a] < 0 || runs[a] >= h->runs_R || (a > 0 && runs[a] <= runs[a - 1]))
            return report_error(RVLL_E_INVALID, "%s: runs must be distinct, ascending and below R (runs[%d] = %d)", who, (int)a, (int)runs[a]);
    return RVLL_OK;
}

// How an ensemble step opens: four stages up to the runs' global whitening, in the order both steps take them.  The clustered step
// puts its own checks, its reservations and the packing of the survivors between them.
struct EnsembleStep {
    rvll_handle* h;
    const char* who;
    const int32_t* runs;                                   // [A] the listed runs, kdead dying rows each
    int32_t A;
    int64_t kdead;
    const int32_t *ranks;                                  // [A kdead] the walkers' start rows, as ranks among the survivors
    const double* lstar;                                   // [A]
    long long n = 0, R = 0;
    int64_t K = 0;                                         // A kdead: the step's walkers
    int32_t *d_order = nullptr, *d_rank = nullptr, *d_dying = nullptr, *d_start = nullptr;   // of d_runs_idx, [R n] each
    double *d_part = nullptr, *d_cov = nullptr;            // of d_runs_mom: the moments' scratch, the A covariances
    std::vector<double> cov;                               // [A D D] the survivors' covariances (whiten)
    std::chrono::steady_clock::time_point synced;          // when whiten's synchronisation returned

    // the call itself: the device, ncalls zeroed, the run list; buffers: every buffer the step cannot do without is there
    int check_call(bool buffers, int64_t* ncalls)
    {
        RVLL_TRY(use_device(h));
        if (ncalls && A > 0) for (int32_t a = 0; a < A; ++a) ncalls[a] = 0;
        RVLL_TRY(runs_check(h, runs, A, kdead, who));
        if (!buffers) return report_error(RVLL_E_INVALID, "%s: bad arguments", who);
        n = h->runs_n; R = h->runs_R; K = (int64_t)A * kdead;
        return RVLL_OK;
    }
    // the walk's arguments; the sort of these runs that lstar and ranks must fit, spent from here on whatever happens below (the step
    // changes the rows); room for the walk with tables of `groups` groups and for K more rows in the dead store
    int check_sort_and_reserve(const int32_t* wrapped, int32_t nsteps, int32_t max_rounds, int64_t groups)
    {
        RVLL_TRY(walk_check_args(h, K, nsteps, max_rounds, 0, wrapped));
        if (h->runs_sorted_kdead != kdead || h->runs_sorted.size() != (size_t)A || !std::equal(runs, runs + A, h->runs_sorted.begin()))
            return report_error(RVLL_E_INVALID, "%s: no rvll_live_runs_sort of these runs with kdead = %lld precedes", who, (long long)kdead);
        for (int32_t a = 0; a < A; ++a)
            if (!(lstar[a] == h->runs_sorted_lstar[(size_t)a]))
                return report_error(RVLL_E_INVALID, "%s: lstar[%d] is not the one rvll_live_runs_sort returned", who, (int)a);
        for (int64_t i = 0; i < K; ++i)
            if (ranks[i] < 0 || ranks[i] >= n - kdead)
                return report_error(RVLL_E_INVALID, "%s: ranks[%lld] is not a rank among the survivors", who, (long long)i);
        h->runs_sorted.clear();
        h->runs_sorted_kdead = -1;
        if (h->dead_n + K >= (1LL << 31)) return report_error(RVLL_E_NOMEM, "%s: the dead store is full (2^31 rows)", who);
        RVLL_TRY(runs_reserve(h, K, groups));
        return dead_reserve(h, K, K, who);
    }
    // one kernel turns the ranks into dying rows, start rows and the run-mode tables of one group per run (walker i of listed run a
    // is row a kdead + i); the dying rows go to the dead store; every run's survivors (ranks kdead .. n) in one set of moments launches
    int retire_and_sum()
    {
        const int Di = h->L.ndim;
        d_order = h->d_runs_idx;                         // [A n] from the sort
        d_rank = d_order + R * n;                        // [A kdead] each
        d_dying = d_rank + R * n;
        d_start = d_dying + R * n;
        HIP_TRY(hipMemcpyAsync(d_rank, ranks, sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, h->compute));
        HIP_TRY(rvll::launch_runs_compose(d_order, A, n, kdead, d_rank, d_dying, d_start, h->d_walk_run, h->d_walk_wid, h->compute));
        RVLL_TRY(retire_rows(h, d_dying, K));
        d_part = h->d_runs_mom;
        double* d_mean = d_part + rvll::moments_runs_scratch_doubles(Di) * (size_t)A;
        d_cov = d_mean + (size_t)Di * (size_t)A;
        HIP_TRY(rvll::launch_moments_runs(h->d_live_u, d_order + kdead, n, A, n - kdead, Di, d_part, d_mean, d_cov, h->compute));
        return RVLL_OK;
    }
    // the A covariances down in one copy (a synchronisation) and factored: factor [A D D]
    int whiten(double* factor)
    {
        const size_t D = (size_t)h->L.ndim;
        cov.resize(D * D * (size_t)A);
        HIP_TRY(hipMemcpyAsync(cov.data(), d_cov, sizeof(double) * cov.size(), hipMemcpyDeviceToHost, h->compute));
        HIP_TRY(hipStreamSynchronize(h->compute));
        synced = std::chrono::steady_clock::now();
        for (int32_t a = 0; a < A; ++a)
            if (!whitening_factor(cov.data() + D * D * (size_t)a, D, factor + D * D * (size_t)a))
                return report_error(RVLL_E_INVALID, "%s: the live points' covariance of run %d is not positive definite", who, (int)runs[a]);
        return RVLL_OK;
    }
};

// run r's rows in the dead store: how many, and their slots in death order, `want` of them at most
int64_t run_dead_count(const rvll_handle* h, int32_t run)
{
    int64_t have = 0;
    for (const auto& p : h->runs_dead[(size_t)run]) have += p.second;
    return have;
}
std::vector<int32_t> run_dead_rows(const rvll_handle* h, int32_t run, int64_t want)
{
    std::vector<int32_t> rows;
    rows.reserve((size_t)want);
    for (const auto& p : h->runs_dead[(size_t)run])
        for (long long i = 0; i < p.second && (int64_t)rows.size() < want; ++i) rows.push_back((int32_t)(p.first + i));
    return rows;
}

// `rows` of the dead store, gathered through the walk's buffers a chunk at a time: per chunk one download for every column that is
// wanted (dst not null): `width` doubles a row of d_src, through the walk buffer `scratch`
struct DeadColumn { const double* d_src; int width; double* rvll_handle::*scratch; double* dst; };
int dead_rows_download(rvll_handle* h, const std::vector<int32_t>& rows, std::initializer_list<DeadColumn> columns)
{
    RVLL_TRY(walk_reserve(h, 1));
    const int64_t want = (int64_t)rows.size();
    hipStream_t st = h->compute;
    for (int64_t lo = 0; lo < want; lo += h->walk_cap) {
        const size_t m = (size_t)std::min<int64_t>(h->walk_cap, want - lo);
        HIP_TRY(hipMemcpyAsync(h->d_walk_order, rows.data() + lo, sizeof(int32_t) * m, hipMemcpyHostToDevice, st));
        for (const DeadColumn& c : columns) {
            if (!c.dst) continue;
            HIP_TRY(rvll::launch_gather_rows(c.d_src, h->d_walk_order, (long long)m, c.width, h->*c.scratch, st));
            HIP_TRY(hipMemcpyAsync(c.dst + (size_t)lo * c.width, h->*c.scratch, sizeof(double) * c.width * m, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    return RVLL_OK;
}

}  // namespace

extern "C" {

// ---- nested sampling with the live points resident on the device -------------------------------------------
int rvll_live_init(rvll_handle* h, const double* cube, int64_t N, double* logl_out)
{
    RVLL_TRY(use_device(h));
    if (!h->have_priors) return report_error(RVLL_E_NOPRIORS, "rvll_set_priors has not been called");
    if (N < 1 || N >= (1LL << 31) || !cube) return report_error(RVLL_E_INVALID, "rvll_live_init: bad arguments");
    // a new run starts here: whatever fails below, no earlier run's live set is left looking valid (rvll_live_step and
    // rvll_live_get refuse live_n = 0) — live_n is set again as the last thing, on success
    h->live_n = 0;
    h->dead_n = 0;
    h->sorted_kdead = -1;
    h->runs_R = 0;                                       // (and no ensemble's either)
    h->cl_A = 0;
    RVLL_TRY(live_load(h, cube, N, logl_out));
    h->live_n = N;
    h->dead_n = 0;
    return RVLL_OK;
}

int rvll_live_step(rvll_handle* h, const int32_t* order, int64_t kdead, const int32_t* start, double lstar,
                   const double* chol, const int32_t* wrapped, int32_t nsteps, int32_t max_rounds, uint64_t seed,
                   int64_t walker_base, int64_t* ncalls, double* logl_new, double* chol_out)
{
    RVLL_TRY(use_device(h));
    if (ncalls) *ncalls = 0;
    const int64_t N = h->live_n;
    if (N < 1) return report_error(RVLL_E_INVALID, "rvll_live_init has not been called");
    if (!start || !logl_new || kdead < 1 || kdead >= N) return report_error(RVLL_E_INVALID, "rvll_live_step: bad arguments");
    RVLL_TRY(walk_check_args(h, kdead, nsteps, max_rounds, walker_base, wrapped));
    const bool dev_order = order == nullptr;             // the order rvll_live_sort left on the device; start[] are ranks among the survivors
    if (dev_order) {
        if (h->sorted_kdead != kdead) return report_error(RVLL_E_INVALID, "rvll_live_step: order is NULL but no rvll_live_sort(kdead = %lld) precedes", (long long)kdead);
        if (!(lstar == h->sorted_lstar)) return report_error(RVLL_E_INVALID, "rvll_live_step: lstar is not the one rvll_live_sort returned");
        for (int64_t i = 0; i < kdead; ++i)
            if (start[i] < 0 || start[i] >= N - kdead) return report_error(RVLL_E_INVALID, "rvll_live_step: start[%lld] is not a rank among the survivors", (long long)i);
        h->sorted_kdead = -1;                            // (used up, whatever happens below: the step changes the rows)
    }
    for (int64_t i = 0; !dev_order && i < N; ++i)
        if (order[i] < 0 || order[i] >= N) return report_error(RVLL_E_INVALID, "rvll_live_step: order[%lld] out of range", (long long)i);
    if (!dev_order) {
        // the dying rows are scattered into in parallel and appended to the dead store: a row listed twice would race and be counted twice
        std::vector<uint64_t> seen(((size_t)N + 63) / 64, 0);
        for (int64_t i = 0; i < kdead; ++i) {
            uint64_t& word = seen[(size_t)order[i] >> 6];
            const uint64_t bit = 1ull << (order[i] & 63);
            if (word & bit) return report_error(RVLL_E_INVALID, "rvll_live_step: row %d is listed twice among the dying rows", (int)order[i]);
            word |= bit;
        }
    }
    for (int64_t i = 0; !dev_order && i < kdead; ++i)
        if (start[i] < 0 || start[i] >= N) return report_error(RVLL_E_INVALID, "rvll_live_step: start[%lld] out of range", (long long)i);
    const size_t D = (size_t)h->L.ndim;
    const int Di = h->L.ndim;
    RVLL_TRY(walk_reserve(h, kdead));
    hipStream_t st = h->compute;
    int32_t* d_order = h->d_live_idx;
    int32_t* d_start = h->d_live_idx + h->live_cap;
    if (dev_order) {
        // d_order holds the device's own order; the ranks go up through the sort's row scratch and become rows on the device
        HIP_TRY(hipMemcpyAsync(h->d_sort_rows, start, sizeof(int32_t) * (size_t)kdead, hipMemcpyHostToDevice, st));
        HIP_TRY(rvll::launch_compose_index(d_order, kdead, h->d_sort_rows, kdead, d_start, st));
    } else {
        h->sorted_kdead = -1;
        HIP_TRY(hipMemcpyAsync(d_order, order, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_start, start, sizeof(int32_t) * (size_t)kdead, hipMemcpyHostToDevice, st));
    }
    // the points that die (rows order[0 .. kdead)) go to the dead store before their rows are overwritten
    RVLL_TRY(dead_reserve(h, kdead, kdead, "rvll_live_step"));
    RVLL_TRY(retire_rows(h, d_order, kdead));
    // (dead_n moves on in finish_and_commit: a step that fails below — a covariance that is not positive definite, a walk that
    // fails — leaves the dead store as it was, so a retry does not append the same rows twice)
    // whitening: the caller's factor, or the covariance of the surviving rows order[kdead .. N) summed on the device (in a
    // fixed order) and factored here (19 x 19: host arithmetic; + 1e-14 on the diagonal as evidence_amd/nested.py adds)
    std::vector<double> factor(D * D, 0.);
    if (chol) {
        memcpy(factor.data(), chol, sizeof(double) * D * D);
    } else {
        double* scratch = h->d_live_mom;
        double* d_mean = scratch + rvll::moments_scratch_doubles(Di);
        double* d_cov = d_mean + D;
        HIP_TRY(rvll::launch_moments(h->d_live_u, d_order + kdead, N - kdead, Di, scratch, d_mean, d_cov, st));
        std::vector<double> cov(D * D);
        HIP_TRY(hipMemcpyAsync(cov.data(), d_cov, sizeof(double) * D * D, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!whitening_factor(cov.data(), D, factor.data()))
            return report_error(RVLL_E_INVALID, "rvll_live_step: the live points' covariance is not positive definite");
    }
    if (chol_out) memcpy(chol_out, factor.data(), sizeof(double) * D * D);
    // the walkers start from rows start[0 .. kdead)
    RVLL_TRY(gather_walkers(h, d_start, kdead));
    RVLL_TRY(walk_upload_frame(h, factor.data(), wrapped));
    RVLL_TRY(walk_core(h, kdead, lstar, nsteps, max_rounds, seed, walker_base, ncalls, nullptr));
    // ... and their end points replace the dead rows, born at lstar (the dying rows' births go to the dead store first)
    return finish_and_commit(h, d_order, d_order, kdead, kdead, false, lstar, logl_new, nullptr, 0);
}

int rvll_live_sort(rvll_handle* h, int64_t kdead, double* dead_logl, double* lstar, double* max_logl)
{
    RVLL_TRY(use_device(h));
    const int64_t N = h->live_n;
    if (N < 1) return report_error(RVLL_E_INVALID, "rvll_live_init has not been called");
    if (kdead < 1 || kdead >= N || !dead_logl || !lstar || !max_logl) return report_error(RVLL_E_INVALID, "rvll_live_sort: bad arguments");
    h->sorted_kdead = -1;
    hipStream_t st = h->compute;
    RVLL_TRY(sort_temp_reserve(h, rvll::sort_temp_bytes(N)));
    int32_t* d_order = h->d_live_idx;
    HIP_TRY(rvll::launch_sort_logl(h->d_live_logl, N, h->d_sort_keys, h->d_sort_keys + h->live_cap, h->d_sort_rows, d_order,
                                   h->d_sort_temp, h->sort_temp_bytes, st));
    // the log-L of the kdead lowest, in order, and of the highest: gathered into the walk's log-L scratch, one download
    RVLL_TRY(walk_reserve(h, kdead + 1));
    HIP_TRY(rvll::launch_gather_rows(h->d_live_logl, d_order, kdead, 1, h->d_walk_logl, st));
    HIP_TRY(rvll::launch_gather_rows(h->d_live_logl, d_order + (N - 1), 1, 1, h->d_walk_logl + kdead, st));
    std::vector<double> got((size_t)kdead + 1);
    HIP_TRY(hipMemcpyAsync(got.data(), h->d_walk_logl, sizeof(double) * ((size_t)kdead + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(dead_logl, got.data(), sizeof(double) * (size_t)kdead);
    *lstar = got[(size_t)kdead - 1];
    *max_logl = got[(size_t)kdead];
    h->sorted_kdead = kdead;
    h->sorted_lstar = *lstar;
    return RVLL_OK;
}

int rvll_live_get(rvll_handle* h, double* cube, double* theta, double* logl)
{
    RVLL_TRY(use_device(h));
    if (h->live_n < 1) return report_error(RVLL_E_INVALID, "rvll_live_init has not been called");
    const size_t D = (size_t)h->L.ndim, N = (size_t)h->live_n;
    hipStream_t st = h->compute;
    const bool staged = sizeof(double) * D * N >= kDownloadStagedMin;
    if (cube && staged) RVLL_TRY(download_rows(h, cube, h->d_live_u, sizeof(double) * D * N));
    else if (cube) HIP_TRY(hipMemcpyAsync(cube, h->d_live_u, sizeof(double) * D * N, hipMemcpyDeviceToHost, st));
    if (theta && staged) RVLL_TRY(download_rows(h, theta, h->d_live_theta, sizeof(double) * D * N));
    else if (theta) HIP_TRY(hipMemcpyAsync(theta, h->d_live_theta, sizeof(double) * D * N, hipMemcpyDeviceToHost, st));
    if (logl) HIP_TRY(hipMemcpyAsync(logl, h->d_live_logl, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

int rvll_live_dead(rvll_handle* h, int64_t* n_dead, double* theta, double* logl)
{
    RVLL_TRY(use_device(h));
    if (!n_dead) return report_error(RVLL_E_INVALID, "n_dead is null");
    if (h->runs_R > 0) return report_error(RVLL_E_INVALID, "rvll_live_dead: the resident rows are an ensemble's (rvll_live_runs_dead)");
    const int64_t have = h->dead_n, want = (theta || logl) ? std::min<int64_t>(*n_dead, have) : 0;
    *n_dead = have;
    const size_t D = (size_t)h->L.ndim;
    hipStream_t st = h->compute;
    if (want > 0 && theta && sizeof(double) * D * (size_t)want >= kDeadStagedMin) {
        RVLL_TRY(download_rows(h, theta, h->d_dead_theta, sizeof(double) * D * (size_t)want));
    } else if (want > 0 && theta) {
        HIP_TRY(hipMemcpyAsync(theta, h->d_dead_theta, sizeof(double) * D * (size_t)want, hipMemcpyDeviceToHost, st));
    }
    if (want > 0 && logl) HIP_TRY(hipMemcpyAsync(logl, h->d_dead_logl, sizeof(double) * (size_t)want, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

// ---- the resident ensemble: R independent live sets in one handle (rvll_live_runs_*) ----------------------------------------
int rvll_live_runs_init(rvll_handle* h, const double* cube, int32_t R, int64_t n, double* logl_out)
{
    RVLL_TRY(use_device(h));
    if (!h->have_priors) return report_error(RVLL_E_NOPRIORS, "rvll_set_priors has not been called");
    if (R < 1 || n < 2 || (int64_t)R * n >= (1LL << 31) || !cube) return report_error(RVLL_E_INVALID, "rvll_live_runs_init: bad arguments");
    // a new ensemble starts here: no earlier live set — one run's or an ensemble's — is left looking valid, whatever fails below
    h->live_n = 0;
    h->dead_n = 0;
    h->sorted_kdead = -1;
    h->runs_R = 0;
    h->runs_sorted.clear();
    h->runs_sorted_kdead = -1;
    h->cl_A = 0;
    const int64_t N = (int64_t)R * n;
    RVLL_TRY(live_load(h, cube, N, logl_out));
    const int Di = h->L.ndim;
    const size_t D = (size_t)Di;
    const long long idx_need = 4 * N + 2 * (long long)R + 1;
    if (idx_need > h->runs_idx_cap) {
        dev_free(h->d_runs_idx);
        h->runs_idx_cap = 0;
        HIP_TRY(hipMalloc(&h->d_runs_idx, sizeof(int32_t) * (size_t)idx_need));
        h->runs_idx_cap = idx_need;
    }
    if (R > h->runs_mom_cap) {
        dev_free(h->d_runs_mom);
        h->runs_mom_cap = 0;
        HIP_TRY(hipMalloc(&h->d_runs_mom, sizeof(double) * (rvll::moments_runs_scratch_doubles(Di) + D + D * D) * (size_t)R));
        h->runs_mom_cap = R;
    }
    h->runs_dead.assign((size_t)R, {});
    h->runs_n = n;
    h->runs_R = R;
    return RVLL_OK;
}

int rvll_live_runs_sort(rvll_handle* h, const int32_t* runs, int32_t A, int64_t kdead, double* dead_logl, double* lstar,
                        double* max_logl)
{
    RVLL_TRY(use_device(h));
    RVLL_TRY(runs_check(h, runs, A, kdead, "rvll_live_runs_sort"));
    if (!dead_logl || !lstar || !max_logl) return report_error(RVLL_E_INVALID, "rvll_live_runs_sort: bad arguments");
    h->runs_sorted.clear();
    h->runs_sorted_kdead = -1;
    const long long n = h->runs_n, R = h->runs_R;
    hipStream_t st = h->compute;
    RVLL_TRY(sort_temp_reserve(h, rvll::runs_sort_temp_bytes(A, n)));
    int32_t* d_order = h->d_runs_idx;                    // [A n]: the listed runs' orders, packed
    int32_t* d_runs = h->d_runs_idx + 4 * R * n;         // [A], then the segments [A + 1]
    int32_t* d_seg = d_runs + R;
    RVLL_TRY(walk_reserve(h, (int64_t)A * (kdead + 1)));      // (the walk's log-L scratch takes the rows that come down)
    HIP_TRY(hipMemcpyAsync(d_runs, runs, sizeof(int32_t) * (size_t)A, hipMemcpyHostToDevice, st));
    HIP_TRY(rvll::launch_runs_sort(h->d_live_logl, d_runs, A, n, h->d_sort_keys, h->d_sort_keys + h->live_cap, h->d_sort_rows, d_seg,
                                   d_order, h->d_sort_temp, h->sort_temp_bytes, st));
    HIP_TRY(rvll::launch_runs_sorted_logl(h->d_live_logl, d_order, A, n, kdead, h->d_walk_logl, st));
    std::vector<double> got((size_t)A * (size_t)(kdead + 1));
    HIP_TRY(hipMemcpyAsync(got.data(), h->d_walk_logl, sizeof(double) * got.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<double> ls((size_t)A);
    for (int32_t a = 0; a < A; ++a) {
        const double* g = got.data() + (size_t)a * (size_t)(kdead + 1);
        memcpy(dead_logl + (size_t)a * (size_t)kdead, g, sizeof(double) * (size_t)kdead);
        ls[(size_t)a] = lstar[a] = g[kdead - 1];
        max_logl[a] = g[kdead];
    }
    h->runs_sorted.assign(runs, runs + A);
    h->runs_sorted_kdead = kdead;
    h->runs_sorted_lstar = ls;
    return RVLL_OK;
}

// rvll_live_runs_step, and rvll_live_runs_step_steps unclustered: steps [A] or null (every run nsteps; else nsteps is their
// largest), move_out / pair_out [A kdead] or null (the step-count adaptation's distances).  The groups of its walk are
// the listed runs themselves (step_groups_identity): the run-mode tables come from launch_runs_compose, lstar, seeds, steps and
// factors are the per-run arrays.
static int live_runs_step_impl(rvll_handle* h, const int32_t* runs, int32_t A, int64_t kdead, const int32_t* ranks, const double* lstar,
                               const int32_t* wrapped, int32_t nsteps, const int32_t* steps, int32_t max_rounds, const uint64_t* seeds,
                               int64_t* ncalls, double* logl_new, double* chol_out, double* move_out, double* pair_out)
{
    EnsembleStep S{h, "rvll_live_runs_step", runs, A, kdead, ranks, lstar};
    RVLL_TRY(S.check_call(ranks && lstar && seeds && logl_new, ncalls));
    RVLL_TRY(S.check_sort_and_reserve(wrapped, nsteps, max_rounds, A));
    RVLL_TRY(S.retire_and_sum());
    const int64_t K = S.K;
    const size_t D = (size_t)h->L.ndim;
    std::vector<double> factor(D * D * (size_t)A);
    RVLL_TRY(S.whiten(factor.data()));
    if (chol_out) memcpy(chol_out, factor.data(), sizeof(double) * factor.size());
    // the walkers (walker i of listed run a is row a kdead + i of the walk) start from their rows ...
    hipStream_t st = h->compute;
    RVLL_TRY(gather_walkers(h, S.d_start, K));
    HIP_TRY(hipMemcpyAsync(h->d_run_lstar, lstar, sizeof(double) * (size_t)A, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_run_seed, seeds, sizeof(uint64_t) * (size_t)A, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_run_chol, factor.data(), sizeof(double) * factor.size(), hipMemcpyHostToDevice, st));
    RVLL_TRY(walk_upload_frame(h, nullptr, wrapped));         // (synchronises: `factor` may go out of scope after it)
    StepGroups G;
    step_groups_identity(A, kdead, S.n, &G);
    StepDistances dist{move_out || pair_out};
    RVLL_TRY(dist.stage(h, G));
    if (steps) HIP_TRY(hipMemcpyAsync(h->d_run_nsteps, steps, sizeof(int32_t) * (size_t)A, hipMemcpyHostToDevice, st));
    RunWalk rw{G.grun.data(), G.grid.data(), std::vector<long long>((size_t)K, 0), steps};
    RVLL_TRY(walk_core(h, K, 0., nsteps, max_rounds, 0, 0, nullptr, &rw));
    // the distances (group = the run: its survivors, ranks kdead .. n of its sort order, and its factor), behind the walk
    RVLL_TRY(dist.measure(h, h->d_live_u, S.d_order, G, wrapped));
    // ... and their end points replace the dying rows, born at their run's lstar
    std::vector<double> wl((size_t)K);
    RVLL_TRY(finish_and_commit(h, S.d_dying, S.d_dying, K, kdead, true, 0., wl.data(), runs, A));
    step_outputs(G, kdead, wl.data(), rw.row_calls, dist, logl_new, ncalls, move_out, pair_out);
    return RVLL_OK;
}

int rvll_live_runs_step(rvll_handle* h, const int32_t* runs, int32_t A, int64_t kdead, const int32_t* ranks, const double* lstar,
                        const int32_t* wrapped, int32_t nsteps, int32_t max_rounds, const uint64_t* seeds, int64_t* ncalls,
                        double* logl_new, double* chol_out)
{
    return live_runs_step_impl(h, runs, A, kdead, ranks, lstar, wrapped, nsteps, nullptr, max_rounds, seeds, ncalls, logl_new, chol_out,
                               nullptr, nullptr);
}

// The covariances of the clustered step's segments (StepSegments: the clusters that get a factor of their own) in one segmented
// moments pass over the packed survivors d_surv in their (label, rank) order d_slot_sorted; segcov [S D D] comes down behind a
// synchronisation.  d_part: the global moments' scratch, spent by now (its block holds runs_mom_cap scratches).
static int segment_moments(rvll_handle* h, const StepSegments& seg, const double* d_surv, const int32_t* d_slot_sorted, double* d_part,
                           std::vector<double>* segcov)
{
    const int Di = h->L.ndim;
    const size_t D = (size_t)Di, S = seg.seg_of.size();
    hipStream_t st = h->compute;
    segcov->resize(D * D * S);
    if (S == 0) return RVLL_OK;
    const size_t o_sc = sizeof(long long) * 2 * S, o_mean = o_sc + sizeof(double) * 2 * S;
    const size_t o_cov = o_mean + sizeof(double) * D * S, bytes = o_cov + sizeof(double) * D * D * S;
    if (bytes > h->clseg_cap) {
        HIP_TRY(hipStreamSynchronize(st));
        if (h->d_clseg) { (void)hipFree(h->d_clseg); h->d_clseg = nullptr; }
        h->clseg_cap = 0;
        HIP_TRY(hipMalloc(&h->d_clseg, 2 * bytes));
        h->clseg_cap = 2 * bytes;
    }
    std::vector<char> tab(o_mean);
    memcpy(tab.data(), seg.segtab.data(), o_sc);
    memcpy(tab.data() + o_sc, seg.segsc.data(), o_mean - o_sc);
    char* dseg = static_cast<char*>(h->d_clseg);
    HIP_TRY(hipMemcpyAsync(dseg, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(rvll::launch_moments_segs(d_surv, d_slot_sorted, reinterpret_cast<const long long*>(dseg),
                                      reinterpret_cast<const double*>(dseg + o_sc), (int)S, Di, d_part, (int)std::min<long long>(h->runs_mom_cap, 65535),
                                      reinterpret_cast<double*>(dseg + o_mean), reinterpret_cast<double*>(dseg + o_cov), st));
    HIP_TRY(hipMemcpyAsync(segcov->data(), dseg + o_cov, sizeof(double) * segcov->size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

// The clustered step ("Clustering inside the resident ensemble"; the numbers below are its stages).  Host
// synchronisations before the walk: the global covariances (as rvll_live_runs_step), the labels and cluster counts, and — only when
// some run has more than one cluster with at least 2 ndim rows — the per-cluster covariances; then those of the walk and the final
// download, as rvll_live_runs_step.
// rvll_live_runs_step_clustered, and rvll_live_runs_step_steps clustered (steps, move_out, pair_out as live_runs_step_impl; the
// distances' groups are the walk's (run, cluster) groups)
static int live_runs_step_clustered_impl(rvll_handle* h, const int32_t* runs, int32_t A, int64_t kdead, const int32_t* ranks,
                                         const double* lstar, const int32_t* wrapped, int32_t nsteps, const int32_t* steps,
                                         int32_t max_rounds, const uint64_t* seeds, int32_t nboot, const uint64_t* boot_seeds,
                                         int64_t* ncalls, double* logl_new, int32_t* nclusters, double* move_out, double* pair_out)
{
    const char* who = "rvll_live_runs_step_clustered";
    EnsembleStep S{h, who, runs, A, kdead, ranks, lstar};
    RVLL_TRY(S.check_call(ranks && lstar && seeds && logl_new && boot_seeds && nclusters, ncalls));
    if (nboot < 0 || nboot > rvll::kClusterMaxBoot)
        return report_error(RVLL_E_INVALID, "%s: nboot = %d is outside [0, %d]", who, (int)nboot, rvll::kClusterMaxBoot);
    const int Di = h->L.ndim;
    if (Di < 1 || Di > rvll::kClusterMaxDims)
        return report_error(RVLL_E_UNSUPPORTED, "%s: %d parameters (the clustering takes 1 .. %d)", who, Di, rvll::kClusterMaxDims);
    const long long n = S.n, R = S.R, m = n - kdead;
    const int64_t K = S.K, M = (int64_t)A * m;
    const size_t D = (size_t)h->L.ndim;
    RVLL_TRY(S.check_sort_and_reserve(wrapped, nsteps, max_rounds, K));   // (group tables for up to A kdead groups: one walker each)
    // the clustering's blocks: rows a m .. a m + m - 1 are listed run a's survivors in rank order; the workgroup table depends on
    // (A, m) alone
    std::vector<int64_t> cstart((size_t)A + 1);
    for (int32_t a = 0; a <= A; ++a) cstart[(size_t)a] = (int64_t)a * m;
    const std::vector<int32_t> blocks = cluster_blocks(cstart.data(), A);
    const ClusterLayout L = cluster_layout(M, A, Di, blocks.size());
    RVLL_TRY(cluster_reserve(h, L, who));
    RVLL_TRY(sort_temp_reserve(h, rvll::label_sort_temp_bytes(A, M)));
    hipStream_t st = h->compute;
    // the sort keys' block as ints [4 live_cap]: labels in (label, rank) order | their slots | the walkers' start rows | their
    // dying rows, in group order (live_cap >= R n >= A m, A kdead)
    int32_t* kscr = reinterpret_cast<int32_t*>(h->d_sort_keys);
    const long long lc = h->live_cap;
    int32_t *d_lab_sorted = kscr, *d_slot_sorted = kscr + lc, *d_gstart = kscr + 2 * lc, *d_gdying = kscr + 3 * lc;
    // 1. the dying rows to the dead store and the global moments, exactly as rvll_live_runs_step; the survivors packed for the
    // clustering meanwhile; the covariances down (sync 1), the global factors
    RVLL_TRY(S.retire_and_sum());
    int32_t* d_seg = S.d_start + R * n + R;              // [A + 1]: the sort's segments, now the label sort's (a m)
    char* din = static_cast<char*>(h->d_cl_in);
    double* d_surv = reinterpret_cast<double*>(din + L.o_cube);
    HIP_TRY(rvll::launch_runs_survivors(h->d_live_u, S.d_order, A, n, kdead, Di, d_surv, h->d_sort_rows, d_seg, st));
    std::vector<double> gfac(D * D * (size_t)A);
    RVLL_TRY(S.whiten(gfac.data()));
    const std::vector<double>& cov = S.cov;
    const auto t1 = S.synced;
    // 2. the metric (evidence_amd/nested.py's _cluster_scale of the device covariance), the bootstrap seeds and the block table go
    // up behind the packed survivors; clustering, then every run's (label, rank) order; labels and counts down (sync 2)
    std::vector<double> scale(D * (size_t)A);
    for (int32_t a = 0; a < A; ++a)
        for (size_t d = 0; d < D; ++d) scale[(size_t)a * D + d] = 1.0 / std::sqrt(cov[(size_t)a * D * D + d * D + d] + 1e-14);
    std::vector<char> in(L.in_bytes - L.o_scale);
    memcpy(in.data(), scale.data(), sizeof(double) * scale.size());
    memcpy(in.data() + (L.o_start - L.o_scale), cstart.data(), sizeof(int64_t) * cstart.size());
    memcpy(in.data() + (L.o_seed - L.o_scale), boot_seeds, sizeof(uint64_t) * (size_t)A);
    if (!blocks.empty()) memcpy(in.data() + (L.o_blk - L.o_scale), blocks.data(), sizeof(int32_t) * blocks.size());
    HIP_TRY(hipMemcpyAsync(din + L.o_scale, in.data(), in.size(), hipMemcpyHostToDevice, st));
    const rvll::ClusterArgs ca = cluster_args(h, L, Di, nboot, wrapped);
    RVLL_TRY(cluster_core(h, ca));
    HIP_TRY(rvll::launch_label_sort(ca.labels, d_lab_sorted, h->d_sort_rows, d_slot_sorted, A, M, d_seg, h->d_sort_temp,
                                    h->sort_temp_bytes, st));
    std::vector<char> out(L.out_bytes);
    HIP_TRY(hipMemcpyAsync(out.data(), h->d_cl_out, L.out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();
    const int32_t* ncl = reinterpret_cast<const int32_t*>(out.data() + L.p_ncl);
    const int32_t* lab = reinterpret_cast<const int32_t*>(out.data() + L.p_lab);
    // 3. per (run, cluster) its rows, and the segments: the clusters that get moments of their own (rvll_step_groups.h)
    StepSegments seg;
    const StepGroupsError bad = step_segments(lab, ncl, A, m, Di, &seg);
    if (bad.what == StepGroupsError::kClusterCount)
        return report_error(RVLL_E_HIP, "%s: the clustering of run %d returned %d clusters", who, (int)runs[bad.a], (int)bad.value);
    if (bad.what == StepGroupsError::kLabelRange)
        return report_error(RVLL_E_HIP, "%s: label %d of run %d is out of range", who, (int)bad.value, (int)runs[bad.a]);
    // 4. their covariances (sync 3, skipped without segments) and the factors of every run: the global one alone (one cluster), else
    // one per cluster — its own or the global one
    std::vector<double> segcov;
    RVLL_TRY(segment_moments(h, seg, d_surv, d_slot_sorted, S.d_part, &segcov));
    const auto t3 = std::chrono::steady_clock::now();
    std::vector<std::vector<double>> fac((size_t)A);
    for (int32_t a = 0; a < A; ++a) {
        const size_t k = ncl[a] > 1 ? (size_t)ncl[a] : 1;
        fac[(size_t)a].resize(D * D * k);
        for (size_t c = 0; c < k; ++c) memcpy(fac[(size_t)a].data() + D * D * c, gfac.data() + D * D * (size_t)a, sizeof(double) * D * D);
    }
    for (size_t s = 0; s < seg.seg_of.size(); ++s) {
        const int32_t a = seg.seg_of[s].first, c = seg.seg_of[s].second;
        if (!whitening_factor(segcov.data() + D * D * s, D, fac[(size_t)a].data() + D * D * (size_t)c))
            return report_error(RVLL_E_INVALID, "%s: the covariance of cluster %d of run %d is not positive definite", who, (int)c, (int)runs[a]);
    }
    // 5. the walker groups (rvll_step_groups.h), every group with the factor of its cluster; the group tables and the walker
    // permutation go up, the start and dying rows follow the permutation
    StepGroups G;
    step_groups(seg.cnt, lab, ranks, lstar, seeds, steps, nsteps, A, kdead, m, &G);
    std::vector<double> gchol;
    gchol.reserve(D * D * G.gofs.size());
    for (const auto& f : G.gfac)
        gchol.insert(gchol.end(), fac[(size_t)f.first].begin() + D * D * (size_t)f.second, fac[(size_t)f.first].begin() + D * D * ((size_t)f.second + 1));
    HIP_TRY(hipMemcpyAsync(S.d_rank, G.perm.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, st));
    HIP_TRY(rvll::launch_compose_index(S.d_start, 0, S.d_rank, K, d_gstart, st));
    HIP_TRY(rvll::launch_compose_index(S.d_dying, 0, S.d_rank, K, d_gdying, st));
    HIP_TRY(hipMemcpyAsync(h->d_walk_run, G.grun.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_walk_wid, G.grid.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_run_lstar, G.glstar.data(), sizeof(double) * G.glstar.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_run_seed, G.gseed.data(), sizeof(uint64_t) * G.gseed.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_run_chol, gchol.data(), sizeof(double) * gchol.size(), hipMemcpyHostToDevice, st));
    // 6. one run-mode walk for every group of every run
    RVLL_TRY(gather_walkers(h, d_gstart, K));
    StepDistances dist{move_out || pair_out};
    RVLL_TRY(dist.stage(h, G));
    if (steps) HIP_TRY(hipMemcpyAsync(h->d_run_nsteps, G.gsteps.data(), sizeof(int32_t) * G.gsteps.size(), hipMemcpyHostToDevice, st));
    RVLL_TRY(walk_upload_frame(h, nullptr, wrapped));         // (synchronises: the host tables above may go out of scope after it)
    RunWalk rw{G.grun.data(), G.grid.data(), std::vector<long long>((size_t)K, 0), steps ? G.gsteps.data() : nullptr};
    RVLL_TRY(walk_core(h, K, 0., nsteps, max_rounds, 0, 0, nullptr, &rw));
    // the distances: group g's survivors are the packed rows of its cluster (d_surv through the label sort's slots), its factor the
    // walk's
    RVLL_TRY(dist.measure(h, d_surv, d_slot_sorted, G, wrapped));
    // 7. births in the dead store's order (d_dying), each run's rows at its lstar; the end points back to the dying rows in the
    // walk's order (d_gdying); commit; log-L, calls and distances back in walker order
    std::vector<double> wl((size_t)K);
    RVLL_TRY(finish_and_commit(h, S.d_dying, d_gdying, K, kdead, true, 0., wl.data(), runs, A));
    const auto t4 = std::chrono::steady_clock::now();
    step_outputs(G, kdead, wl.data(), rw.row_calls, dist, logl_new, ncalls, move_out, pair_out);
    for (int32_t a = 0; a < A; ++a) nclusters[a] = ncl[a];
    h->cl_A = A;
    h->cl_m = m;
    h->cl_labels.assign(lab, lab + M);
    h->cl_ncl.assign(ncl, ncl + A);
    h->cl_scale = std::move(scale);
    h->cl_factors = std::move(fac);
    h->cl_phase_s[0] = std::chrono::duration<double>(t2 - t1).count();
    h->cl_phase_s[1] = std::chrono::duration<double>(t3 - t2).count();
    h->cl_phase_s[2] = std::chrono::duration<double>(t4 - t3).count();
    return RVLL_OK;
}

int rvll_live_runs_step_clustered(rvll_handle* h, const int32_t* runs, int32_t A, int64_t kdead, const int32_t* ranks,
                                  const double* lstar, const int32_t* wrapped, int32_t nsteps, int32_t max_rounds,
                                  const uint64_t* seeds, int32_t nboot, const uint64_t* boot_seeds, int64_t* ncalls,
                                  double* logl_new, int32_t* nclusters)
{
    return live_runs_step_clustered_impl(h, runs, A, kdead, ranks, lstar, wrapped, nsteps, nullptr, max_rounds, seeds, nboot, boot_seeds,
                                         ncalls, logl_new, nclusters, nullptr, nullptr);
}

int rvll_live_runs_step_steps(rvll_handle* h, const int32_t* runs, int32_t A, int64_t kdead, const int32_t* ranks, const double* lstar,
                              const int32_t* wrapped, const int32_t* nsteps, int32_t max_rounds, const uint64_t* seeds, int32_t clustered,
                              int32_t nboot, const uint64_t* boot_seeds, int64_t* ncalls, double* logl_new, int32_t* nclusters,
                              double* move, double* pair)
{
    int32_t most = 0;
    bool uniform = true;
    RVLL_TRY(steps_range("rvll_live_runs_step_steps", nsteps, A, &most, &uniform));
    const int32_t* steps = uniform ? nullptr : nsteps;               // a uniform table is the scalar step
    if (clustered)
        return live_runs_step_clustered_impl(h, runs, A, kdead, ranks, lstar, wrapped, most, steps, max_rounds, seeds, nboot, boot_seeds,
                                             ncalls, logl_new, nclusters, move, pair);
    return live_runs_step_impl(h, runs, A, kdead, ranks, lstar, wrapped, most, steps, max_rounds, seeds, ncalls, logl_new, nullptr,
                               move, pair);
}

int rvll_live_runs_clusters(rvll_handle* h, int32_t a, int64_t* nsurv, int32_t* nclusters, int32_t* labels, double* scale, double* factors,
                            double* phase_s)
{
    if (!h) return report_error(RVLL_E_INVALID, "null handle");
    if (h->cl_A < 1) return report_error(RVLL_E_INVALID, "rvll_live_runs_clusters: no rvll_live_runs_step_clustered since the live sets were loaded");
    if (a < 0 || a >= h->cl_A) return report_error(RVLL_E_INVALID, "rvll_live_runs_clusters: listed run %d of %d", (int)a, (int)h->cl_A);
    const size_t D = (size_t)h->L.ndim, m = (size_t)h->cl_m;
    if (nsurv) *nsurv = (int64_t)m;
    if (nclusters) *nclusters = h->cl_ncl[(size_t)a];
    if (labels) memcpy(labels, h->cl_labels.data() + (size_t)a * m, sizeof(int32_t) * m);
    if (scale) memcpy(scale, h->cl_scale.data() + (size_t)a * D, sizeof(double) * D);
    if (factors) memcpy(factors, h->cl_factors[(size_t)a].data(), sizeof(double) * h->cl_factors[(size_t)a].size());
    if (phase_s) for (int k = 0; k < 3; ++k) phase_s[k] = h->cl_phase_s[k];
    return RVLL_OK;
}

int rvll_live_runs_get(rvll_handle* h, int32_t run, double* cube, double* theta, double* logl)
{
    RVLL_TRY(use_device(h));
    if (h->runs_R < 1) return report_error(RVLL_E_INVALID, "rvll_live_runs_init has not been called");
    if (run < 0 || run >= h->runs_R) return report_error(RVLL_E_INVALID, "rvll_live_runs_get: run %d out of range", (int)run);
    const size_t D = (size_t)h->L.ndim, n = (size_t)h->runs_n, r0 = (size_t)run * n;
    hipStream_t st = h->compute;
    if (cube) HIP_TRY(hipMemcpyAsync(cube, h->d_live_u + r0 * D, sizeof(double) * D * n, hipMemcpyDeviceToHost, st));
    if (theta) HIP_TRY(hipMemcpyAsync(theta, h->d_live_theta + r0 * D, sizeof(double) * D * n, hipMemcpyDeviceToHost, st));
    if (logl) HIP_TRY(hipMemcpyAsync(logl, h->d_live_logl + r0, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

int rvll_live_runs_dead(rvll_handle* h, int32_t run, int64_t* n_dead, double* theta, double* logl)
{
    RVLL_TRY(use_device(h));
    if (!n_dead) return report_error(RVLL_E_INVALID, "n_dead is null");
    if (h->runs_R < 1) return report_error(RVLL_E_INVALID, "rvll_live_runs_init has not been called");
    if (run < 0 || run >= h->runs_R) return report_error(RVLL_E_INVALID, "rvll_live_runs_dead: run %d out of range", (int)run);
    const int64_t have = run_dead_count(h, run), want = (theta || logl) ? std::min<int64_t>(*n_dead, have) : 0;
    *n_dead = have;
    if (want <= 0) return RVLL_OK;
    return dead_rows_download(h, run_dead_rows(h, run, want), {{h->d_dead_theta, h->L.ndim, &rvll_handle::d_walk_theta, theta},
                                                               {h->d_dead_logl, 1, &rvll_handle::d_walk_logl, logl}});
}

// ---- birth contours of the resident rows ----------------------------------------------------------------------------------------
int rvll_live_births(rvll_handle* h, int64_t* n_dead, double* dead_birth, double* live_birth)
{
    RVLL_TRY(use_device(h));
    if (!n_dead) return report_error(RVLL_E_INVALID, "n_dead is null");
    if (h->runs_R > 0) return report_error(RVLL_E_INVALID, "rvll_live_births: the resident rows are an ensemble's (rvll_live_runs_births)");
    if (live_birth && h->live_n < 1) return report_error(RVLL_E_INVALID, "rvll_live_init has not been called");
    const int64_t have = h->dead_n, want = dead_birth ? std::min<int64_t>(*n_dead, have) : 0;
    *n_dead = have;
    hipStream_t st = h->compute;
    if (want > 0) HIP_TRY(hipMemcpyAsync(dead_birth, h->d_dead_birth, sizeof(double) * (size_t)want, hipMemcpyDeviceToHost, st));
    if (live_birth) HIP_TRY(hipMemcpyAsync(live_birth, h->d_live_birth, sizeof(double) * (size_t)h->live_n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RVLL_OK;
}

int rvll_live_runs_births(rvll_handle* h, int32_t run, int64_t* n_dead, double* dead_birth, double* live_birth)
{
    RVLL_TRY(use_device(h));
    if (!n_dead) return report_error(RVLL_E_INVALID, "n_dead is null");
    if (h->runs_R < 1) return report_error(RVLL_E_INVALID, "rvll_live_runs_init has not been called");
    if (run < 0 || run >= h->runs_R) return report_error(RVLL_E_INVALID, "rvll_live_runs_births: run %d out of range", (int)run);
    const int64_t have = run_dead_count(h, run), want = dead_birth ? std::min<int64_t>(*n_dead, have) : 0;
    *n_dead = have;
    hipStream_t st = h->compute;
    if (live_birth) {
        const size_t n = (size_t)h->runs_n, r0 = (size_t)run * n;
        HIP_TRY(hipMemcpyAsync(live_birth, h->d_live_birth + r0, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (want <= 0) return RVLL_OK;
    // the run's rows of the store in death order, as rvll_live_runs_dead gathers them
    return dead_rows_download(h, run_dead_rows(h, run, want), {{h->d_dead_birth, 1, &rvll_handle::d_walk_logl, dead_birth}});
}

}  // extern "C"
