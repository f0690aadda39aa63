// rvll_walk_plan.h — the integer decisions of the device walk's host driver (rvll_walk_host.hip): the measurement switches, the
// geometry of a walk in rounds and the layout of its arena, the tile of the single-kernel walk, the two-part rule, the order and
// the deal of the second part's rows, the wide rows form.  No HIP call and no handle: what the kernels' launch interface knows
// (the LDS a tile, a step or a workgroup of parked rows takes; occupancy) comes in as numbers or as callables, so
// tests/test_walk_plan_host.py builds the header with a host compiler and holds it against the same rules stated in numpy.
#pragma once
#include <unistd.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace rvll {
namespace host {

// limits of the kernels and of the handle that the plans are made for (rvll_kernels.h, rvll_host.h: rvll_walk_host.hip asserts
// that they agree)
namespace walkplan {
constexpr int kThreads = 256, kWave = 64, kMaxPoints = 32, kCuThreads = 1024, kCuMaxPoints = 128, kRing = 16, kMaxGroups = 4;
constexpr size_t kLds = 60 * 1024, kLdsMax = 64 * 1024, kCuLds = 156 * 1024;   // a 256-thread workgroup's budget and limit; a CU's budget
}  // namespace walkplan

// ---- the switches: read on every walk (tests and scripts/*_probe.py change them between the calls of a live handle) ----
struct WalkSwitches {
    int rounds = -1;            // RVLL_WALK_ROUNDS: 0 never in rounds, else whenever the slim prior stage applies (-1: by size)
    bool single_kernel = false; // one of the switches that select a single-kernel form is set, whatever to: _QUEUE / _PARTS / _ROWS / _FAT
    int queue = -1;             // RVLL_WALK_QUEUE >= 0: compute units whose workgroups a launch fills (-1: all; 0: a workgroup per PB rows)
    bool one_part = false;      // RVLL_WALK_PARTS=1: one launch
    int rows = 0;               // RVLL_WALK_ROWS: 0 the queue form, 1 the rows form, 2 its CU-wide form, 3 two 512-thread workgroups a CU
    bool fat = false;           // RVLL_WALK_FAT: the full solvers inline
    int spec = 0;               // RVLL_WALK_SPEC in 1 .. kMaxPoints: candidates ahead (0: the handle's)
    int cr = 0;                 // RVLL_WALK_CR: the exact redo of wandering solves inside the walk's tiles
    bool first_set = false;     // RVLL_WALK_FIRST: moves of the first part ...
    int first = 0;              // ... (clamped to 1 .. nsteps - 1 by first_part_steps)
    bool geom_dump = false, cost_dump = false, tile_dump = false;   // RVLL_WALK_GEOM_DUMP / _COST_DUMP / _TILE_DUMP
    int groups = 3;             // RVLL_ROUNDS_GROUPS (measured at cfg3: 2: 1.64, 3: 1.72, 4: 1.67e8 calls/s; profiles/r04_rounds_sweep.txt)
    long long free_slots = 0;   // RVLL_ROUNDS_FREE >= 1 (0: by the chip and the epochs)
    bool cu_form = false;       // RVLL_ROUNDS_FORM=cu: the rounds' tiles CU-wide
    bool per_set = false;       // RVLL_ROUNDS_PER: rows a group (the last group takes the rest: unequal groups) ...
    long long per = 0;          // ... (clamped to 1 .. K by rounds_start)
    int w = 0;                  // RVLL_ROUNDS_W >= 1: at most this many walkers a step workgroup (0: what fits)
    int pb = 0;                 // RVLL_ROUNDS_PB in 1 .. kMaxPoints: points per tile (0: by the room beside the steps)
    int stamps = 0;             // RVLL_ROUNDS_STAMPS in 0 .. 4096: rounds of group 0 whose step workgroups are time-stamped
    int depth = 4;              // RVLL_ROUNDS_DEPTH >= 1: rounds queued beyond the last one seen starting
    bool listed_dump = false;   // RVLL_ROUNDS_LISTED_DUMP
    bool chain = false;         // RVLL_ROUNDS_CHAIN != 0 (measured: 1.57 against 1.71e8 calls/s unchained)
    bool prio = false;          // RVLL_ROUNDS_PRIO != 0: the groups' streams at different priorities
};

// one pass over the environment, as read_batch_switches (rvll_batch_route.h)
inline WalkSwitches read_walk_switches()
{
    WalkSwitches s;
    for (char** e = environ; e && *e; ++e) {
        const char* p = *e;
        if (p[0] != 'R' || p[1] != 'V' || p[2] != 'L' || p[3] != 'L' || p[4] != '_') continue;
        const char* name = p + 5;
        const char* eq = strchr(name, '=');
        if (!eq) continue;
        auto is = [&](const char* key) { return strlen(key) == (size_t)(eq - name) && strncmp(name, key, (size_t)(eq - name)) == 0; };
        const int v = atoi(eq + 1);
        if (is("WALK_ROUNDS")) s.rounds = v != 0;
        else if (is("WALK_QUEUE")) { s.queue = std::max(0, v); s.single_kernel = true; }
        else if (is("WALK_PARTS")) { s.one_part = v == 1; s.single_kernel = true; }
        else if (is("WALK_ROWS")) { s.rows = v < 1 ? 0 : v == 2 || v == 3 ? v : 1; s.single_kernel = true; }
        else if (is("WALK_FAT")) s.fat = s.single_kernel = true;
        else if (is("WALK_SPEC")) s.spec = std::max(1, std::min(v, walkplan::kMaxPoints));
        else if (is("WALK_CR")) s.cr = v;
        else if (is("WALK_FIRST")) { s.first_set = true; s.first = v; }
        else if (is("WALK_GEOM_DUMP")) s.geom_dump = true;
        else if (is("WALK_COST_DUMP")) s.cost_dump = true;
        else if (is("WALK_TILE_DUMP")) s.tile_dump = true;
        else if (is("ROUNDS_GROUPS")) s.groups = v;
        else if (is("ROUNDS_FREE")) s.free_slots = std::max(1, v);
        else if (is("ROUNDS_FORM")) s.cu_form = !strcmp(eq + 1, "cu");
        else if (is("ROUNDS_PER")) { s.per_set = true; s.per = atoll(eq + 1); }
        else if (is("ROUNDS_W")) s.w = std::max(1, v);
        else if (is("ROUNDS_PB")) s.pb = std::max(1, std::min(v, walkplan::kMaxPoints));
        else if (is("ROUNDS_STAMPS")) s.stamps = std::max(0, std::min(v, 4096));
        else if (is("ROUNDS_DEPTH")) s.depth = std::max(1, v);
        else if (is("ROUNDS_LISTED_DUMP")) s.listed_dump = true;
        else if (is("ROUNDS_CHAIN")) s.chain = v != 0;
        else if (is("ROUNDS_PRIO")) s.prio = v != 0;
    }
    return s;
}

// ---- the walk as rounds of launches (rvll_rounds.h, rvll_kernels.hip) ----
// Which walks take it: RVLL_WALK_ROUNDS = 0 never / 1 whenever the slim prior stage applies.  By default the walks it was
// measured to win (profiles/r04_rounds_sizes.txt, cfg3, nested sampling end to end, calls/s inside the walk against the
// single-kernel form): 8192 walkers 1.23 against 1.05e8, 16384: 1.72 against 1.62e8 — and not the ones it loses: 4096 walkers
// and fewer (a round's fixed ~35 us against a workgroup iteration of the single kernel: 5.2 against 5.8e7), 32768 (1.86 against
// 1.90e8: the single kernel's queue has enough rows per slot there).  None of the switches that select a single-kernel form
// may be set (the tests and the measurements of those forms).
inline bool rounds_wanted(long long K, const WalkSwitches& sw)
{
    if (sw.rounds >= 0) return sw.rounds != 0;
    return !sw.single_kernel && K >= 6144 && K <= 24576;
}

// What is settled before the tile and the step's workgroup are known: groups, rows a group, free slots, candidates a walker may
// hold.  The cost model chooses the base tile for batch() points.
struct RoundsStart {
    int G, spec;
    long long per, c_free;
    long long batch() const { return std::max(per, c_free); }
};

inline RoundsStart rounds_start(long long K, int n_cu, int Ne, int spec, const WalkSwitches& sw)
{
    RoundsStart s;
    s.spec = std::max(1, std::min(sw.spec ? sw.spec : spec, walkplan::kMaxPoints));   // (1: no candidates ahead)
    s.G = (int)std::max<long long>(1, std::min<long long>(std::min(sw.groups, walkplan::kMaxGroups), K));
    // Slots a round may hold before walkers stop getting candidates AHEAD: while a group lists fewer walkers than this, the free
    // slots go to its walkers' next candidates (consumed in order: the results do not change).  A round costs ~35 us whatever it
    // holds (a step, a launch, a tile's prologue and last wave round) plus ~3 ns a slot, and a walk is a chain of such rounds:
    // below ~6000 slots at 200 epochs a round is cheaper filled with candidates of which two in three go unused than run again
    // (measured, 16384 walkers: 1300: 1.50, 2600: 1.61, 4000: 1.68, 6000: 1.72, 8000: 1.71e8 calls/s).  Scaled by the epochs.
    s.c_free = sw.free_slots ? sw.free_slots : std::max<long long>(256, (long long)n_cu * 4608 / std::max(1, Ne));
    s.per = sw.per_set ? std::max<long long>(1, std::min<long long>(K, sw.per)) : (K + s.G - 1) / s.G;
    return s;
}

struct RoundsIn {
    long long K;
    int D, Ne, n_cu, nsteps, max_rounds;
    int spec;                   // the handle's candidates ahead (rvll_set_walk_speculation)
    int chunk_items;            // the tile's contribution window at most
    int PB, CH;                 // the cost model's tile for rounds_start().batch() points
    int occ;                    // workgroups of the tiles kernel a compute unit holds with that tile's LDS (0: unknown)
    int W;                      // walkers a step workgroup holds within walkplan::kLds at rounds_start().spec (0: none: refused)
};

// G groups of `per` rows (the last one what is left), a step workgroup per W of them; C candidate slots a group, of which c_free
// may go to candidates ahead; `tiles` tiles of PB points (CH contributions in LDS, lds bytes); a group has listed nobody by
// round r_max.  !ok: the walk does not fit the rounds form (RVLL_E_UNSUPPORTED, nothing launched).
struct RoundsPlan {
    bool ok = false, cu_form = false;
    int G = 0, W = 0, spec = 0, PB = 0, CH = 0, tiles = 0, depth = 0;
    long long per = 0, C = 0, c_free = 0, nblk = 0, r_max = 0;
    size_t lds = 0;
};

template <class TileLds>          // size_t tile_lds(int PB, int CH)
RoundsPlan plan_rounds(const RoundsIn& in, const WalkSwitches& sw, TileLds tile_lds)
{
    using namespace walkplan;
    RoundsPlan p;
    const RoundsStart s = rounds_start(in.K, in.n_cu, in.Ne, in.spec, sw);
    p.spec = s.spec;  p.cu_form = sw.cu_form;  p.depth = sw.depth;
    // the step's walkers per workgroup: within what leaves four workgroups a compute unit when it shares its launches (and with
    // them the size of the dynamic LDS) with the tiles, up to a wave's lanes otherwise
    if (in.W < 1) return p;
    p.W = sw.w ? std::min(in.W, sw.w) : in.W;
    p.per = (s.per + p.W - 1) / p.W * p.W;
    p.G = (int)((in.K + p.per - 1) / p.per);
    p.C = std::max(p.per, s.c_free);  p.nblk = p.per / p.W;
    p.c_free = std::min(s.c_free, p.C);
    if (p.C >= (1LL << 30) || p.per * p.spec >= (1LL << 31)) return p;
    if (p.G > kMaxGroups) return p;            // (RVLL_ROUNDS_PER below K / kMaxGroups: the handle has a stream and a progress word for kMaxGroups)
    auto window = [&](int pb) { return (std::min(in.chunk_items, std::max(kThreads, pb * in.Ne)) + 1) & ~1; };
    p.PB = in.PB;  p.CH = in.CH;
    if (sw.cu_form) {
        // one CU-wide tile per compute unit: every contribution of the tile resident in LDS
        int pb = (int)std::min<long long>(kCuMaxPoints, (p.C + in.n_cu - 1) / in.n_cu);
        auto fits = [&](int q) { return tile_lds(q, (q * in.Ne + 1) & ~1) <= kCuLds; };
        while (pb > 1 && !fits(pb)) --pb;
        if (!fits(pb)) return p;
        p.PB = pb;  p.CH = (pb * in.Ne + 1) & ~1;
    } else {
        // 256-thread tiles sized to the wave slots the chip has left beside one group's step workgroups (but never smaller
        // than the cost model's choice): a tile that waits for a step's slot ends its launch a step's latency late
        const long long room = (long long)std::max(1, in.occ) * in.n_cu - (p.G > 1 ? p.nblk : 0);
        const long long want = room > 0 ? (p.C + room - 1) / room : p.PB;
        if (want > p.PB && want <= kMaxPoints && tile_lds((int)want, window((int)want)) <= kLds) { p.PB = (int)want; p.CH = window(p.PB); }
        if (sw.pb && tile_lds(sw.pb, window(sw.pb)) <= kLds) { p.PB = sw.pb; p.CH = window(p.PB); }
    }
    p.lds = tile_lds(p.PB, p.CH);
    p.tiles = (int)((p.C + p.PB - 1) / p.PB);
    // Every round consumes a candidate of every listed walker, so a group has listed nobody by round nsteps * max_rounds + 1 — and the
    // host may have queued `depth` rounds beyond the last one it has seen start (without that allowance a walk with max_rounds = 1
    // was refused while its last rounds were still in the queue: found by scripts/walk_soak.py).
    p.r_max = (long long)in.nsteps * in.max_rounds + 2 + p.depth;
    p.ok = true;
    return p;
}

// A group's slice of the arena: doubles | 64-bit words | ints, each section from a multiple of 16 bytes; byte offsets of its arrays
struct RoundsArena {
    size_t n_dbl, n_ll, n_int, g_bytes;
    size_t dir, dirnext, tmin, tmax, theta_c[2], wt, wres_logl, res_logl;   // doubles (RoundsArgs; res_logl [C]: the tiles' log-L)
    size_t calls_part, slots_part, ring;                                     // 64-bit words (the ring: 8-byte aligned pairs, one 64-bit atomic a workgroup)
    size_t ws, wres_flags, wdef, res_flags, owner;                           // ints (res_flags [C]: the tiles' flags)
    size_t words_bytes() const { return ws - calls_part; }                   // the partial sums and the ring: zeroed before a walk
};

inline RoundsArena rounds_arena(const RoundsPlan& p, int D)
{
    const size_t per = (size_t)p.per, C = (size_t)p.C, spec = (size_t)p.spec, nblk = (size_t)p.nblk, d = (size_t)D;
    RoundsArena a;
    size_t at = 0;
    auto take = [&](size_t n, size_t width) { const size_t o = at; at += n * width; return o; };
    a.dir = take(per * d, 8);  a.dirnext = take(per * d, 8);  a.tmin = take(per, 8);  a.tmax = take(per, 8);
    a.theta_c[0] = take(C * d, 8);  a.theta_c[1] = take(C * d, 8);
    a.wt = take(per * spec, 8);  a.wres_logl = take(per * spec, 8);  a.res_logl = take(C, 8);
    a.n_dbl = at / 8;
    at = (at + 15) & ~(size_t)15;
    a.calls_part = take(nblk, 8);  a.slots_part = take(nblk, 8);  a.ring = take(walkplan::kRing, 8);
    a.n_ll = (at - a.calls_part) / 8;
    at = (at + 15) & ~(size_t)15;
    a.ws = take(4 * per, 4);  a.wres_flags = take(per * spec, 4);  a.wdef = take(per * spec, 4);  a.res_flags = take(C, 4);  a.owner = take(C, 4);
    a.n_int = (at - a.ws) / 4;
    a.g_bytes = (at + 15) & ~(size_t)15;
    return a;
}

// ---- the single-kernel forms ----
inline int walk_max_cus(const WalkSwitches& sw, int n_cu) { return sw.queue >= 0 ? std::min(sw.queue, n_cu) : n_cu; }

// The tile of a single-kernel walk of n rows, from the cost model's PB0: the walk keeps per-walker state in LDS next to the tile's
// carve, so the group shrinks until both fit.  !ok: not even one walker does.
struct WalkTile { bool ok; int PB, CH; };

template <class WalkLds>          // size_t walk_lds(int PB, int CH)
WalkTile walk_tile(int PB0, int D, int Ne, int chunk_items, int pb_override, long long n, WalkLds walk_lds)
{
    using namespace walkplan;
    auto window = [&](int pb) {                    // the tile's contribution window also holds 3 PB D doubles of the walk
        const int ch = std::max(std::min(chunk_items, std::max(kThreads, pb * Ne)), 3 * pb * D);
        return (ch + 1) & ~1;
    };
    int pb = PB0;
    // Walker slots per workgroup: the walk's own phases cost a workgroup iteration the same whatever the number of
    // slots, so more slots spread them thinner — as long as four workgroups still fit a compute unit's LDS.  Measured at
    // cfg3 (profiles/r03_walk_forms.txt): 8: 1.54, 10: 1.58, 12: 1.58, 14: 1.53, 16: 1.47e8 calls/s inside the walk.
    if (pb_override <= 0 && n >= 4096) {
        pb = std::min(10, kMaxPoints);
        while (pb > 1 && 4 * walk_lds(pb, window(pb)) > kCuLds) --pb;
    }
    auto too_big = [&](int q, size_t lds) { return walk_lds(q, window(q)) > lds || (long long)q * D > 4 * kThreads; };
    while (pb > 1 && too_big(pb, kLds)) --pb;
    return {!too_big(pb, kLdsMax), pb, window(pb)};
}

// With more rows than walker slots a row handed out late still takes a whole walk — nsteps sequential moves — and the
// kernel ends in a drain (phase clock: mean workgroup life 7.2 ms of a 9.5 ms kernel at 16384 rows).  What a row costs
// per move is a property of where it walks, so the walk is launched in two parts: the first moves of every row through
// the queue (short rows: a fine grain), counting the candidates each one needs; then the rest in the "rows" form —
// every workgroup OWNS an equal share of the rows by that cost and interleaves them over its walker slots, so all rows
// of the launch end together (rvll_walk.hip, slice_walk_rows_kernel).  Results are those of one launch (the moves of
// a row do not care which launch makes them).  RVLL_WALK_PARTS=1: one launch (measurement / test switch).
// RVLL_WALK_ROWS=1 selects the rows form; the DEFAULT is the second part through the queue as well, most expensive
// rows first (round 2's form): measured on bench.py's nested run (profiles/r03_walk_forms.txt) the rows form balances
// the workgroups as designed — and is 7 % slower (1.38 vs 1.48e8 calls/s inside the walk): with every slot always
// holding a walker no tile slot is ever free for candidates ahead, and the kernel is bound by what a workgroup's
// iteration costs (2600 vector instructions per candidate against the batch kernel's 1990, VALUs busy 75 %), not by
// its tail.  Kept, tested bit-identical, for walks whose rows differ more than cfg3's.
// `resident`: workgroups the chip holds at once (0: a workgroup per PB rows)
inline bool walk_two_parts(long long K, long long resident, int PB, int nsteps, const WalkSwitches& sw)
{
    return resident > 0 && K > resident * PB && nsteps >= 8 && !sw.one_part;
}
inline bool walk_rows_form(const WalkSwitches& sw, int PB, int D, int CH) { return sw.rows >= 1 && 3LL * PB * D <= CH; }   // (the rows kernels park their candidates in the tile's window)
inline int first_part_steps(int nsteps, bool rows_form, const WalkSwitches& sw)
{
    return std::max(1, sw.first_set ? std::min(nsteps - 1, sw.first) : rows_form ? nsteps / 8 : nsteps / 4);
}

// The rows in the order the second part hands them out: counting sort by the candidates the first `first` moves cost (held to
// 0 .. min(first * max_rounds, 65536)), most expensive first, stable; rows that did not complete the first part (the slim stage
// deferred them: left to the full-solver pass) last.  Returns K2, the rows that go on.
inline int64_t order_by_cost(const std::vector<int32_t>& cost, const std::vector<int32_t>& done, int first, int max_rounds,
                             std::vector<int32_t>* order)
{
    const int64_t K = (int64_t)cost.size();
    const int32_t cmax = std::min<int32_t>(first * max_rounds, 1 << 16);
    std::vector<int32_t> count((size_t)cmax + 2, 0);
    auto key = [&](int64_t i) { return done[(size_t)i] >= first ? std::min(std::max(cost[(size_t)i], 0), cmax) + 1 : 0; };
    for (int64_t i = 0; i < K; ++i) ++count[(size_t)key(i)];
    const int32_t deferred = count[0];
    int32_t pos = 0;
    for (int32_t c = cmax + 1; c >= 0; --c) { const int32_t n_c = count[(size_t)c]; count[(size_t)c] = pos; pos += n_c; }
    order->resize((size_t)K);
    for (int64_t i = 0; i < K; ++i) (*order)[(size_t)count[(size_t)key(i)]++] = (int32_t)i;
    return K - deferred;
}

// workgroups of a launch over K2 ordered rows
inline int64_t walk_blocks(int64_t K2, int PB, long long resident) { return std::min<int64_t>((K2 + PB - 1) / PB, resident); }

// The workgroups' first rows: deal the G * PB most expensive ones round the workgroups like cards, so that every workgroup
// starts with one of the G longest, one of the next G, ... — eight long rows in one workgroup would leave it no free tile slot
// to evaluate candidates ahead with, and they are the critical path.  Slot b * PB + pl receives entry pl * G + b.
inline void deal_first_rows(std::vector<int32_t>* order, int64_t K2, int64_t G, int PB)
{
    const int64_t first_rows = std::min<int64_t>(G * PB, K2);
    std::vector<int32_t> dealt((size_t)first_rows);
    int64_t k = 0;
    for (int64_t pl = 0; pl < PB; ++pl)
        for (int64_t b = 0; b < G; ++b) {
            const int64_t slot = b * PB + pl;
            if (slot < first_rows && k < first_rows) dealt[(size_t)slot] = (*order)[(size_t)k++];
        }
    std::copy(dealt.begin(), dealt.end(), order->begin());
}

// The rows form: every workgroup an equal share of the rows (snake deal of the sorted order, in the kernel); a share that does not
// fit the kernel's LDS goes in several launches, one after the other.  RVLL_WALK_ROWS=2: the CU-wide form — one 1024-thread
// workgroup per compute unit with as many walker slots (<= 64) as its LDS holds next to the parked rows, the tile in its CU-wide
// form; 3: two 512-thread workgroups.  (The wide forms exist for the slim stage only: the full-solver instantiation does not fit
// 128 VGPRs unspilled.)
inline int rows_threads(const WalkSwitches& sw, bool slim) { return !slim || sw.rows < 2 ? walkplan::kThreads : sw.rows == 2 ? walkplan::kCuThreads : 512; }
inline size_t rows_budget(int nt) { return nt == walkplan::kThreads ? walkplan::kLds : nt == walkplan::kCuThreads ? walkplan::kCuLds : walkplan::kCuLds / 2; }

struct WideRows { bool ok; int64_t G, rows; int PB, CH; };

template <class RowsLds>          // size_t rows_lds(int PB, int CH, int rows_per_wg)
WideRows wide_rows(int64_t K2, int cus, int nt, int Ne, int D, RowsLds rows_lds)
{
    WideRows r;
    r.G = std::min<int64_t>((int64_t)cus * (walkplan::kCuThreads / nt), K2);
    r.rows = (K2 + r.G - 1) / r.G;
    auto ch = [&](int sl) { return (std::max(sl * Ne, 3 * sl * D) + 1) & ~1; };
    auto fits = [&](int sl) { return rows_lds(sl, ch(sl), (int)r.rows) <= rows_budget(nt); };
    r.PB = (int)std::min<int64_t>(walkplan::kWave, r.rows);
    while (r.PB > 1 && !fits(r.PB)) --r.PB;
    r.CH = ch(r.PB);
    r.ok = fits(r.PB);
    return r;
}

// rows a workgroup can park: a launch takes G times as many
template <class RowsLds>          // size_t rows_lds(int rows_per_wg)
int64_t rows_parked_max(size_t budget, RowsLds rows_lds)
{
    int64_t rmax = 1;
    while (rmax < 4096 && rows_lds((int)rmax + 1) <= budget) ++rmax;
    return rmax;
}

}  // namespace host
}  // namespace rvll
