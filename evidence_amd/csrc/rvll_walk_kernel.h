// rvll_walk_kernel.h — the single-kernel proposal walk, slice_walk_kernel: included by rvll_walk.hip (its chord
// instantiations and the other walk forms) and by rvll_walk_stepout.hip (its stepout instantiations).  The stepout
// instantiations live in a translation unit of their own so that the chord instantiations compile to the instructions they
// compiled to before the stepout proposal existed: in one unit, the extra callers of the tile's helpers changed the inliner's
// decisions inside those helpers, and with them the chord kernels' register allocation.  Both units are built with the
// same flags (csrc/Makefile: -disable-machine-licm; rvll_walk.hip's header says why).
#pragma once
#include <algorithm>
#include <type_traits>
#include "rvll_tile.h"

namespace rvll {

namespace {

// Device-resident slice-sampling walk (rvll_kernels.h, WalkArgs; the scheme of evidence_amd/nested.py
// run_nested_slice, which follows the reference's UltraNest wrapper: region slice sampling, nsteps moves per new
// point, circular omega / ml0 — evidence/ultranest/__init__.py:159-175).  Everything a move needs stays on the
// chip: counter-based random numbers, directions, chords, candidates (written to the workgroup's scratch rows),
// prior transform + log-L of the candidates through the same loglike_tile as every other path, accept / shrink.
// The walkers of a workgroup are NOT in lock step: every iteration evaluates one candidate for every walker that
// still has moves left, and a walker whose candidate was accepted draws its next direction in the following
// iteration — so the tile stays full until the walkers run out of moves (their totals over nsteps moves are
// close), instead of idling behind the slowest walker of every move.  Trip counts are bounded by
// nsteps * max_rounds and shared through LDS, so all waves loop alike.
// SPECULATION.  The moves of a walker are a chain of dependent evaluations, and chains differ a lot in length (a
// walker in a narrow mode shrinks its bracket many more times per move): towards the end of a workgroup's life most
// of its tile is empty while the last walkers crawl on, one candidate per iteration.  Free tile slots are therefore
// given to the walkers that are left: a walker with S slots evaluates candidates r, r+1, .. r+S-1 of its move in ONE
// iteration, where candidate r+j is exactly the one it would draw in round r+j if r .. r+j-1 are all rejected (the
// bracket after a rejection is known before the rejection is: it ends at the rejected candidate).  The results are
// then consumed in order — accept the first one above lstar, shrink past the others — so positions, log-L, counters
// and ncalls are bit for bit those of the one-candidate-per-iteration walk, whatever the workgroup geometry; only
// the iterations a slow walker needs drop (nslots counts what was evaluated, ncalls what was used).
// WALKER QUEUE.  The launch has at most as many workgroups as the chip holds at once; a workgroup's PB walker slots
// start with walkers blockIdx * PB .. and every slot whose walker has finished (or was deferred) sends that walker's
// row home and takes the next one from a global ticket counter, so all slots stay busy until no walker is left —
// with a static split (one workgroup per PB walkers, two residency rounds at 16384 walkers) 28 % of the kernel's
// duration was its tail, workgroups waiting for their slowest walker while the rest of the chip had drained.  The
// random-number counters name the WALKER (row index + walker_base), never the slot, so which slot walks which row
// changes nothing in the results.  The order in which the rows are taken is the host's (w.order): it hands the second
// part of a walk out longest-expected first, from what every row cost in the first part (w.cost, rvll_api.hip).
// FAT = false: the prior stage evaluates Beta / Gamma quantiles by their verified tables only (rvll_tile.h,
// prior_heavy_slim).  A walker whose candidate needs anything else stops at the START of that move and reports the
// number of completed moves in steps_done; the host finishes those walkers with the FAT instantiation (full solvers
// inline, 2 waves per SIMD), whose counter-based random numbers make it retrace the interrupted move exactly — so
// the pair returns what a FAT-only walk would.
// RUNS (run mode, rvll_slice_walk_runs; w.run != null): the rows belong to independent runs, each with its own lstar, seed
// and whitening factor (WalkArgs).  The factor is read from global memory, per walker that starts a move (the walkers of a
// workgroup may belong to different runs); the instantiation without it is the one-run walk, instruction for instruction.
// With w.run_nsteps a row stops after its run's own number of moves (w.nsteps is then the largest, which bounds the loop).
// STEPOUT (PROP = kPropStepout): move m of a walker goes along d = L q_{m mod D}, q_i vector i of the random
// orthonormal basis b = m div D (modified Gram-Schmidt of D counter-based normals), d NOT normalised.  Its bracket, one w wide
// around the walker and cut by the cube's walls (the wrapped coordinates set no limit), steps out by w at each end whose
// log-L is above lstar — right end first, then left — one end per iteration, and then shrinks as the chord walk does.
// Expansions and shrink candidates count alike against max_rounds.  The basis lives in w.basis per walker SLOT, tagged
// in LDS with the (row, basis) it holds: a slot builds the vectors it is missing when its walker starts a move.  The
// counters name (walker, basis, 2 (i D + k)) for the normals, (walker, move, 8192 + round) for the shrink draws as in the
// chord walk and (walker, move, 12288) for the bracket's offset: disjoint ranges, and no slot in them.
template <int PROP> struct WalkKernelArgs { using type = WalkArgs; };
template <> struct WalkKernelArgs<kPropStepout> { using type = WalkArgsStepout; };
template <int PREC, bool FAT, int NP = 0, bool RUNS = false, int PROP = kPropChord>   // NP: the planet count at compile time (rvll_tile.h, eval_item), 0 = a.Np
__global__ __launch_bounds__(kThreads, FAT ? 2 : RVLL_WALK_WAVES) __attribute__((flatten))
void slice_walk_kernel(const LoglikeArgs a, const typename WalkKernelArgs<PROP>::type w)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const Carve cv = carve(a.PB, a.D, a.Np, a.Ni, a.nlin, a.CH);
    const int D = a.D, PB = a.PB, tid = threadIdx.x;
    const long long w0 = (long long)blockIdx.x * PB;
    const int nw = (int)min((long long)PB, w.K - w0);
    if (nw <= 0) return;
    double* wu   = smem + ((cv.total_doubles + 1) & ~1);   // [PB][D] current positions
    double* dir  = wu + PB * D;                            // [PB][D] unit directions
    double* tmin = dir + PB * D;                           // [PB]
    double* tmax = tmin + PB;
    double* slot_t = tmax + PB;                            // [PB] per tile slot: position along its walker's direction
    double* wl   = slot_t + PB;
    // The candidates' unit-cube rows [PB][D] and the per-coordinate chord limits of a starting move (2 x [PB][D]) live in the
    // tile's contribution window (round 3): the tile's staging step has read the candidates, and a barrier has passed,
    // before its items write the first contribution, and nothing outside the tile needs them afterwards — an accepted
    // candidate is recomputed from its walker's position, direction and step (the same arithmetic: the same bits).  That is
    // 3 PB D doubles less LDS per workgroup: twelve walker slots now fit four workgroups per compute unit, and the walk's own
    // phases — paid per workgroup iteration whatever the number of slots — are spread over half as many again.
    double* cand = smem + cv.contrib;
    double* lo_s = cand + PB * D;
    double* hi_s = lo_s + PB * D;
    const bool chol_in_lds = !RUNS && D <= kWalkCholLds;
    double* chol_s = wl + PB;                              // [D][D] the whitening factor, when it is small enough to stage
    int* act     = reinterpret_cast<int*>(chol_s + (chol_in_lds ? D * D : 0));   // [2][PB] walkers with moves left (local index),
                                                            // compacted; the list of the next iteration is written while this one's is read
    int* state   = act + 2 * PB;                              // [PB] 0: needs a new direction, 1: in a move, 2: accepted just now, 3: deferred
    int* step_of = state + PB;                              // [PB] moves completed
    int* round_of = step_of + PB;                           // [PB] candidates tried in the current move
    int* first_of = round_of + PB;                          // [PB] per walker: its first tile slot of this iteration ...
    int* nsp_of  = first_of + PB;                           // [PB] ... and how many it has (>= 1)
    int* acc_slot = nsp_of + PB;                            // [PB] per walker: the slot whose candidate was accepted
    int* used_of = acc_slot + PB;                           // [PB] per walker: candidates consumed this iteration
    int* slot_pl = used_of + PB;                            // [PB] per tile slot: its walker
    int* gid     = slot_pl + PB;                            // [PB] per walker slot: the row it is walking
    int* gold    = gid + PB;                                // [PB] ... the row that has just finished there (to be sent home)
    int* refill  = gold + PB;                               // [PB] 0 / 1: send gold home and load gid / 2: send gold home, slot stays empty
    int* acc_g   = refill + PB;                             // [PB] row of the walker whose candidate was accepted (= gid then)
    int* cost_of = acc_g + PB;                              // [PB] candidates the slot's current row has used in this launch
    int* starts  = cost_of + PB;                            // [PB] the listed walkers that start a move in this iteration
    int* nact_s  = starts + PB;                             // [4]  active walkers, tile slots, slots to refill, walkers starting a move
    int* wrapped_s = nact_s + 4;                            // [D]  circular parameters
    constexpr bool SO = PROP == kPropStepout;
    // stepout only (walk_lds_bytes(a, kPropStepout)): per walker slot its wall chord, its phase and the basis its slot holds.
    // (Declared with a type that depends on PROP, so that a lambda naming them in a discarded `if constexpr` branch does not
    // capture them in the chord instantiations: with the capture, the chord kernels compiled to different instructions.)
    using DblP = std::conditional_t<SO, double*, double*>;
    using IntP = std::conditional_t<SO, int*, int*>;
    DblP cmin_s = SO ? smem + ((reinterpret_cast<char*>(wrapped_s + D) - reinterpret_cast<char*>(smem) + 15) / 16) * 2 : nullptr;   // [PB]
    DblP cmax_s = SO ? cmin_s + PB : nullptr;                               // [PB]
    IntP phase_of = SO ? reinterpret_cast<int*>(cmax_s + PB) : nullptr;     // [PB] 0: stepping out right, 1: left, 2: shrinking
    IntP bas_g   = SO ? phase_of + PB : nullptr;                            // [PB] the row whose basis the slot holds (-1: none) ...
    IntP bas_b   = SO ? bas_g + PB : nullptr;                               // [PB] ... which of its bases ...
    IntP bas_n   = SO ? bas_b + PB : nullptr;                               // [PB] ... and how many of its vectors
    const double* chol = chol_in_lds ? chol_s : w.chol;
    const TileLds L = tile_views(a, smem);                  // the tile's results are read back from LDS (tile_point_result)
    const double one_below = 0.99999999999999988898;        // nextafter(1, 0)

    // the k-th row to be handed out (k: position in the host's order, or the row itself)
    auto row_at = [&](long long k) -> int { return w.order ? w.order[k] : (int)k; };
    // the moves row g makes in this launch: nsteps, or (run mode with a per-run table) its run's count if that is fewer
    auto moves_of = [&](int g) -> int {
        if constexpr (RUNS) { if (w.run_nsteps) return min(w.nsteps, w.run_nsteps[w.run[g]]); }
        return w.nsteps;
    };
    for (int i = tid; i < nw * D; i += kThreads) wu[i] = w.u[(long long)row_at(w0 + i / D) * D + i % D];
    if (chol_in_lds) for (int i = tid; i < D * D; i += kThreads) chol_s[i] = w.chol[i];
    for (int i = tid; i < D; i += kThreads) wrapped_s[i] = w.wrapped[i];
    for (int i = tid; i < nw; i += kThreads) {
        const int g = row_at(w0 + i);
        wl[i] = w.logl[g]; state[i] = 0; round_of[i] = 0; refill[i] = 0; gid[i] = g; cost_of[i] = 0;
        step_of[i] = w.step_start ? w.step_start[g] : 0;
    }
    if constexpr (SO) for (int i = tid; i < PB; i += kThreads) { bas_g[i] = -1; bas_b[i] = -1; bas_n[i] = 0; phase_of[i] = 0; }
    __syncthreads();
    // ---- bookkeeping by the LAST WAVE, one lane per walker slot (round 3; as one thread walking the slots it was a chain of
    //      dependent LDS reads — a tenth of a workgroup's life) ----
    // A lane accounts for its walker's candidates, moves it on after an accept, and — when the walker is done (all moves
    // made, or deferred) — marks its row to go home at the top of the next iteration and draws the next row nobody walks yet
    // from the global ticket counter (rows with nothing left to do are ticked off on the way); a slot that finds none stays
    // empty (gid = -1).  Then the next iteration's list, its tile slots (every listed walker one, the free ones dealt out
    // evenly, at most spec_max per walker and never past the move's last round; dealt by each row's own rejection rate
    // instead, 0.5 % more of the evaluated slots were used and the kernel was 3 % slower) and the walkers that start a move,
    // all by ballots.  Which slot draws which row is not deterministic any more — nor need it be: the random-number
    // counters name the row.
    const long long qbase = (long long)gridDim.x * PB;
    const int lane = tid & (kWave - 1);
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    bool queue_empty = false;                               // (per lane; a lane stops asking once it has seen the end)
    long long calls = 0;                                    // per lane of the bookkeeping wave
    unsigned long long slots = 0;
    auto bookkeep = [&](int* act_out, bool first) {
        const int pl = lane;
        const bool slot = pl < nw;
        const bool active = slot && gid[pl] >= 0;
        int st = active ? state[pl] : 1, stp = active ? step_of[pl] : 0;
        if (active && !first) { const int u = used_of[pl]; calls += u; cost_of[pl] += u; }
        if (active && st == 2) { st = 0; stp += 1; }
        const bool done = active && !(stp < moves_of(gid[pl]) && st != 3);
        int g = active ? gid[pl] : -1, rf = 0;
        if (done) {
            gold[pl] = g;
            used_of[pl] = cost_of[pl];                      // (carried to the top of the next iteration, where the row goes home)
            cost_of[pl] = 0;
            g = -1;
            while (!queue_empty) {
                const long long k = qbase + (long long)atomicAdd(w.queue, 1ull);
                if (k >= w.K) { queue_empty = true; break; }
                const int q = w.order ? w.order[k] : (int)k;
                const int ss = w.step_start ? w.step_start[q] : 0;
                if (ss < moves_of(q)) { g = q; break; }
                if (w.steps_done) w.steps_done[q] = ss;
                if (w.cost) w.cost[q] = 0;
            }
            rf = g >= 0 ? 1 : 2;
            if (g >= 0) { st = 0; round_of[pl] = 0; }
        }
        if (slot) { refill[pl] = rf; gid[pl] = g; }
        if (active) { state[pl] = st == 3 ? 0 : st; step_of[pl] = stp; }
        const bool listed = slot && g >= 0;
        const unsigned long long m_act = __ballot(listed);
        const int n = __popcll(m_act), ai = __popcll(m_act & lanes_below);
        int S = 0;
        if (listed) {
            act_out[ai] = pl;
            S = min(w.spec_max, n ? nw / n + (ai < nw % n ? 1 : 0) : 0);
            S = max(1, min(S, w.max_rounds - (st == 0 ? 0 : round_of[pl])));
            if constexpr (SO) { if (st == 0 || phase_of[pl] != 2) S = 1; }     // (an end of the bracket: one per iteration)
        }
        if (slot) nsp_of[pl] = S;
        // (the lanes of this wave read each other's word next: a wave-scope release + barrier, so that the order holds by the
        // memory model and not only by how the hardware happens to run a wave — ADVICE r3)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int f = 0;
        for (int k = 0; k < pl && k < nw; ++k) f += nsp_of[k];
        if (listed) first_of[pl] = f;
        if (lane == 63 - __builtin_clzll(m_act | 1ull) && listed) nact_s[1] = f + S;       // the last listed slot: the total
        const bool begins = listed && st == 0;
        const unsigned long long m_begin = __ballot(begins), m_done = __ballot(done);
        if (begins) starts[__popcll(m_begin & lanes_below)] = pl;
        if (lane == 0) {
            nact_s[0] = n;
            if (n == 0) nact_s[1] = 0;
            nact_s[2] = __popcll(m_done);
            nact_s[3] = __popcll(m_begin);
        }
    };
    int* const act0 = act;
    if (tid >= kThreads - kWave) bookkeep(act, true);       // walkers that still have moves to make; rows with none go home at once
    __syncthreads();

    // phase clock of a diagnostic build (make walktrace; scripts/walk_phase_probe.py): thread 0 sums the time between
    // barriers into four bins — directions and chord limits / candidates / prior transform + log-L tile / accept + copy
#ifdef RVLL_WALK_TRACE
    unsigned long long ph[5] = {0, 0, 0, 0, 0}, tph[4] = {0, 0, 0, 0}, last = __builtin_amdgcn_s_memrealtime();
#define WALK_STAMP(k) do { if (tid == 0) { const unsigned long long now = __builtin_amdgcn_s_memrealtime(); ph[k] += now - last; last = now; } } while (0)
#else
#define WALK_STAMP(k) do { } while (0)
#endif
    // every iteration consumes at least one candidate of every listed walker, so a slot's walkers end after at most
    // nsteps * max_rounds iterations each; the bound below is the formal exit for the case that all rows pass one slot
    const long long max_iters = ((long long)w.nsteps * w.max_rounds + 1) * (w.K + 1);
    for (long long iter = 0; iter < max_iters; ++iter) {
        const int nact = nact_s[0], nslots = nact_s[1], nref = nact_s[2];
        if (nref) {                                         // finished rows go home, the rows taking their slots come in
            for (int i = tid; i < nw * D; i += kThreads) {
                const int pl = i / D, k = i - pl * D, r = refill[pl];
                if (!r) continue;
                const long long go = gold[pl];
                w.u[go * D + k] = wu[i];
                if (k == 0) {
                    w.logl[go] = wl[pl];
                    if (w.steps_done) w.steps_done[go] = step_of[pl];
                    if (w.cost) w.cost[go] = used_of[pl];
                }
                if (r == 1) {
                    const long long gn = gid[pl];
                    wu[i] = w.u[gn * D + k];
                    if (k == 0) { wl[pl] = w.logl[gn]; step_of[pl] = w.step_start ? w.step_start[gn] : 0; }
                }
            }
            __syncthreads();
        }
        if (nact == 0) break;
        act = act0 + (iter & 1) * PB;
        int* const act_next = act0 + ((iter + 1) & 1) * PB;
        // walkers starting a move: standard normals (Box-Muller on two counter-based uniforms), parked in lo_s ...
        // (only the walkers that START a move — a third of them per iteration at cfg3 — draw directions; profiles/r03_walk_forms.txt)
        const int nstart = nact_s[3];
        if constexpr (SO) {
            // ... (stepout) vector i = m mod D of basis b = m div D, built by the walker's lane in its slot's scratch from the
            // first vector the slot does not hold yet, and parked in lo_s
            for (int si = tid; si < nstart; si += kThreads) {
                const int pl = starts[si], g = gid[pl], m = step_of[pl], b = m / D, iv = m - b * D;
                const unsigned long long wid = (unsigned long long)(w.walker_base + (w.walker_id ? (long long)w.walker_id[g] : (long long)g));
                const unsigned long long seed = RUNS ? w.run_seed[w.run[g]] : w.seed;
                double* q = w.so.basis + ((long long)blockIdx.x * PB + pl) * D * D;
                if (bas_g[pl] != g || bas_b[pl] != b) { bas_g[pl] = g; bas_b[pl] = b; bas_n[pl] = 0; }
                for (int v = bas_n[pl]; v <= iv; ++v) {
                    double* qv = q + v * D;
                    for (int k = 0; k < D; ++k)
                        qv[k] = walk_normal(seed, (wid << 32) | ((unsigned long long)b << 14) | (unsigned)(2 * (v * D + k)));
                    for (int j = 0; j < v; ++j) {                // modified Gram-Schmidt, j ascending
                        const double* qj = q + j * D;
                        double dot = 0.;
                        for (int k = 0; k < D; ++k) dot += qj[k] * qv[k];
                        for (int k = 0; k < D; ++k) qv[k] -= dot * qj[k];
                    }
                    double n2 = 0.;
                    for (int k = 0; k < D; ++k) n2 += qv[k] * qv[k];
                    const double nrm = sqrt(n2);
                    for (int k = 0; k < D; ++k) qv[k] /= nrm;
                }
                bas_n[pl] = max(bas_n[pl], iv + 1);
                for (int k = 0; k < D; ++k) lo_s[pl * D + k] = q[iv * D + k];
            }
        } else {
        for (int i = tid; i < nstart * D; i += kThreads) {
            const int pl = starts[i / D], k = i % D;
            const unsigned long long wid = (unsigned long long)(w.walker_base + (w.walker_id ? (long long)w.walker_id[gid[pl]] : (long long)gid[pl]));
            const unsigned long long ctr = (wid << 32) | ((unsigned long long)step_of[pl] << 14) | (unsigned)(2 * k);
            lo_s[pl * D + k] = walk_normal(RUNS ? w.run_seed[w.run[gid[pl]]] : w.seed, ctr);
        }
        }
        __syncthreads();
        // ... direction = chol * z (lower triangular), parked in the candidate rows, which are free until the tile ...
        for (int i = tid; i < nstart * D; i += kThreads) {
            const int pl = starts[i / D], k = i % D;
            const double* cf = RUNS ? w.run_chol + (long long)w.run[gid[pl]] * D * D : chol;
            double acc = 0.;
            for (int j = 0; j <= k; ++j) acc += cf[k * D + j] * lo_s[pl * D + j];
            cand[pl * D + k] = acc;
        }
        __syncthreads();
        // ... unit direction and the chord limits of every coordinate, one lane per (walker, coordinate); every lane
        // sums the walker's norm itself (same order, same bits) rather than wait a barrier for one lane to do it ...
        if constexpr (SO) {
            // ... (stepout) the direction as it is — t in whitened units — and the wall limits of the coordinates that are not
            // wrapped (no half-turn limit: centred on the walker, it would break reversibility)
            for (int i = tid; i < nstart * D; i += kThreads) {
                const int pl = starts[i / D], k = i % D;
                const double d = cand[pl * D + k], u = wu[pl * D + k];
                dir[pl * D + k] = d;
                double lo = -INFINITY, hi = INFINITY;
                if (d != 0. && !wrapped_s[k]) {
                    const double t0 = (0. - u) / d, t1 = (1. - u) / d;
                    lo = fmin(t0, t1); hi = fmax(t0, t1);
                }
                lo_s[pl * D + k] = lo; hi_s[pl * D + k] = hi;
            }
        } else {
        for (int i = tid; i < nstart * D; i += kThreads) {
            const int pl = starts[i / D], k = i % D;
            double n2 = 0.;
            for (int j = 0; j < D; ++j) n2 += cand[pl * D + j] * cand[pl * D + j];
            const double d = cand[pl * D + k] * (1. / sqrt(n2)), u = wu[pl * D + k];
            dir[pl * D + k] = d;
            double lo = -INFINITY, hi = INFINITY;
            if (d != 0.) {
                if (wrapped_s[k]) {
                    const double half = 0.5 / fabs(d);
                    lo = -half; hi = half;
                } else {
                    const double t0 = (0. - u) / d, t1 = (1. - u) / d;
                    lo = fmin(t0, t1); hi = fmax(t0, t1);
                }
            }
            lo_s[pl * D + k] = lo; hi_s[pl * D + k] = hi;
        }
        }
        __syncthreads();
        WALK_STAMP(0);
        // ... the chord (same max / min sequence over the coordinates as before); then the candidate position along it
        for (int ai = tid; ai < nact; ai += kThreads) {
            const int pl = act[ai];
            if (state[pl] == 0) {
                double lo = -INFINITY, hi = INFINITY;
                for (int k = 0; k < D; ++k) { lo = fmax(lo, lo_s[pl * D + k]); hi = fmin(hi, hi_s[pl * D + k]); }
                if constexpr (SO) {
                    // the bracket: [-w v, w - w v] cut by the wall chord; an end on the chord's limit is out
                    const unsigned long long wid = (unsigned long long)(w.walker_base + (w.walker_id ? (long long)w.walker_id[gid[pl]] : (long long)gid[pl]));
                    const double v = uniform01(RUNS ? w.run_seed[w.run[gid[pl]]] : w.seed, (wid << 32) | ((unsigned long long)step_of[pl] << 14) | 12288u);
                    const double blo = -w.so.step_width * v, bhi = blo + w.so.step_width;
                    cmin_s[pl] = lo; cmax_s[pl] = hi;
                    tmin[pl] = fmax(blo, lo); tmax[pl] = fmin(bhi, hi);
                    phase_of[pl] = tmax[pl] < hi ? 0 : tmin[pl] > lo ? 1 : 2;
                } else {
                tmin[pl] = lo; tmax[pl] = hi;
                }
                round_of[pl] = 0;
                state[pl] = 1;
            }
            if constexpr (SO) {
                if (phase_of[pl] != 2) {                    // an end of the bracket (S = 1)
                    slot_t[first_of[pl]] = phase_of[pl] == 0 ? tmax[pl] : tmin[pl]; slot_pl[first_of[pl]] = pl;
                    continue;
                }
            }
            // this round's candidate and, in the walker's further slots, the ones the next rounds draw if it is rejected
            const unsigned long long wid = (unsigned long long)(w.walker_base + (w.walker_id ? (long long)w.walker_id[gid[pl]] : (long long)gid[pl]));
            const unsigned long long ctr = (wid << 32) | ((unsigned long long)step_of[pl] << 14) | (unsigned)(8192 + round_of[pl]);
            double lo = tmin[pl], hi = tmax[pl];
            const int first = first_of[pl], S = nsp_of[pl];
            const unsigned long long seed = RUNS ? w.run_seed[w.run[gid[pl]]] : w.seed;
            for (int j = 0; j < S; ++j) {
                const double t = lo + (hi - lo) * uniform01(seed, ctr + (unsigned)j);
                slot_t[first + j] = t; slot_pl[first + j] = pl;
                if (t < 0.) lo = t; else hi = t;
            }
        }
        __syncthreads();
        for (int i = tid; i < nslots * D; i += kThreads) {
            const int sl = i / D, k = i - sl * D, pl = slot_pl[sl];
            double c = wu[pl * D + k] + slot_t[sl] * dir[pl * D + k];
            if (wrapped_s[k]) c -= floor(c);
            cand[i] = fmin(fmax(c, 0.), one_below);
        }
        __syncthreads();
        WALK_STAMP(1);
        // prior transform + log-L of the candidates: rows read from LDS, results left in LDS (and in the scratch rows)
#ifdef RVLL_WALK_TRACE
        loglike_tile<PREC, FAT ? kFusedFull : kFusedSlim, false, kThreads, false, true, false, NP>(a, smem, w0, nslots, cand, LogdetPre{}, tph);
#else
        loglike_tile<PREC, FAT ? kFusedFull : kFusedSlim, false, kThreads, false, true, false, NP>(a, smem, w0, nslots, cand);
#endif
        // the walk's own phases are short and serial (a lane per walker, one thread for the bookkeeping): at the
        // default priority they get every fourth issue slot next to three workgroups in their item loops and a
        // barrier-to-barrier phase of ~50 instructions takes 1-2 us (phase clock: 33 % of a workgroup's life for a
        // few per cent of its instructions).  Raised here, lowered again by the tile in front of its item loop.
        __builtin_amdgcn_s_setprio(3);
        __syncthreads();
        WALK_STAMP(2);
        for (int ai = tid; ai < nact; ai += kThreads) {
            const int pl = act[ai];
            const int first = first_of[pl], S = nsp_of[pl];
            const double lstar = RUNS ? w.run_lstar[w.run[gid[pl]]] : w.lstar;
            int used = 0;
            acc_slot[pl] = -1;
            for (int j = 0; j < S; ++j) {                               // in the order the walker would have met them
                int fl;
                const double cl = tile_point_result(a, L, first + j, fl);
                used = j + 1;
                if (!FAT && (fl & kFlagDeferred)) {
                    // leave at the start of this move; the full-solver pass retraces it from its first candidate, so none
                    // of this move's candidates count here (round_of: the ones of earlier iterations, counted then) —
                    // ncalls is what the full-solver walk alone reports
                    state[pl] = 3;
                    used = -(round_of[pl] - j);
                    break;
                }
                if constexpr (SO) {
                    const int ph = phase_of[pl];
                    if (ph != 2) {                          // an end: step out past it while it is inside the slice
                        if (ph == 0) {
                            if (cl > lstar) tmax[pl] = fmin(tmax[pl] + w.so.step_width, cmax_s[pl]);
                            if (!(cl > lstar) || !(tmax[pl] < cmax_s[pl])) phase_of[pl] = tmin[pl] > cmin_s[pl] ? 1 : 2;
                        } else {
                            if (cl > lstar) tmin[pl] = fmax(tmin[pl] - w.so.step_width, cmin_s[pl]);
                            if (!(cl > lstar) || !(tmin[pl] > cmin_s[pl])) phase_of[pl] = 2;
                        }
                        if (++round_of[pl] >= w.max_rounds) { state[pl] = 0; step_of[pl] += 1; }     // give the move up, stay put
                        break;
                    }
                }
                if (cl > lstar) {
                    state[pl] = 2; wl[pl] = cl; acc_slot[pl] = first + j; acc_g[pl] = gid[pl];
                    if (w.wflag) w.wflag[gid[pl]] = (fl & RVLL_FLAG_WANDERED) ? 1 : 0;
                    break;
                }
                const double t = slot_t[first + j];
                if (t < 0.) tmin[pl] = t; else tmax[pl] = t;
                if (++round_of[pl] >= w.max_rounds) { state[pl] = 0; step_of[pl] += 1; break; }     // give the move up, stay put
            }
            used_of[pl] = used;
        }
        __syncthreads();
        // accepted rows move in (every thread but the last) while the last thread does the bookkeeping: it writes the
        // NEXT iteration's list and touches nothing the copy reads
        for (int i = tid; i < nact * D; i += kThreads) {
            const int ai = i / D, k = i - ai * D, pl = act[ai];
            const int sl = acc_slot[pl];
            if (sl < 0) continue;
            double c = wu[pl * D + k] + slot_t[sl] * dir[pl * D + k];      // the accepted candidate, as it was made above
            if (wrapped_s[k]) c -= floor(c);
            wu[pl * D + k] = fmin(fmax(c, 0.), one_below);
            w.theta[(long long)acc_g[pl] * D + k] = L.theta_s[sl * D + k];
        }
        if (tid >= kThreads - kWave) {
            if (lane == 0) slots += (unsigned long long)nslots;
            bookkeep(act_next, false);
        }
        __syncthreads();
        WALK_STAMP(3);
    }
    // (only if the formal bound above ended the loop: rows still being walked go home as they are)
    for (int i = tid; i < nact_s[0] * D; i += kThreads) {
        const int pl = (act0 + (max_iters & 1) * PB)[i / D], k = i % D;
        const long long g = gid[pl];
        w.u[g * D + k] = wu[pl * D + k];
        if (k == 0) { w.logl[g] = wl[pl]; if (w.steps_done) w.steps_done[g] = step_of[pl]; if (w.cost) w.cost[g] = cost_of[pl]; }
    }
    if (tid >= kThreads - kWave && calls) atomicAdd(w.ncalls, (unsigned long long)calls);   // (two's complement: a negative share adds up right)
    if (tid >= kThreads - kWave && slots && w.nslots) atomicAdd(w.nslots, slots);
#ifdef RVLL_WALK_TRACE
    if (tid == 0 && w.nslots) {
        for (int k = 0; k < 4; ++k) atomicAdd(w.nslots + 1 + k, ph[k]);
        atomicAdd(w.nslots + 5, 1ull);
        atomicMax(w.nslots + 6, ph[0] + ph[1] + ph[2] + ph[3]);         // the longest workgroup life of the launch(es)
        for (int k = 0; k < 4; ++k) atomicAdd(w.nslots + 7 + k, tph[k]);  // the tile's own phases: stage, decode, items, reduce + write
    }
#endif
#undef WALK_STAMP
}


}  // namespace

}  // namespace rvll
