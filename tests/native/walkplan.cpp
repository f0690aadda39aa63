// The integer decisions of the device walk's host driver (evidence_amd/csrc/rvll_walk_plan.h) behind C functions, for
// tests/test_walk_plan_host.py: host code only, the header alone.  The switches are read from the environment, as the library reads
// them.  What the library asks the kernels' launch interface (the LDS a tile, a walk workgroup or a workgroup of parked rows takes)
// is a stand-in here, affine in what it depends on; the test states the same stand-ins.
#include "rvll_walk_plan.h"

using namespace rvll::host;

namespace {
size_t tile_lds(int D, int PB, int CH) { return 8 * ((size_t)CH + (size_t)PB * (2 * D + 24)) + 2048; }
size_t walk_lds(int D, int PB, int CH) { return 8 * ((size_t)CH + (size_t)PB * (5 * D + 40)) + 4096; }
size_t rows_lds(int D, int PB, int CH, int rows) { return walk_lds(D, PB, CH) + 8 * (size_t)rows * (2 * D + 4); }
}  // namespace

extern "C" {

// out = the switches in the order of the struct (bools as 0 / 1)
void wp_switches(int64_t* out)
{
    const WalkSwitches s = read_walk_switches();
    const int64_t v[24] = {s.rounds, s.single_kernel, s.queue, s.one_part, s.rows, s.fat, s.spec, s.cr, s.first_set, s.first, s.geom_dump,
                           s.cost_dump, s.tile_dump, s.groups, s.free_slots, s.cu_form, s.per_set, s.per, s.w, s.pb, s.stamps, s.depth,
                           s.listed_dump, (int64_t)s.chain | (int64_t)s.prio << 1};
    for (int i = 0; i < 24; ++i) out[i] = v[i];
}

int wp_rounds_wanted(int64_t K) { return rounds_wanted(K, read_walk_switches()); }
int wp_max_cus(int n_cu) { return walk_max_cus(read_walk_switches(), n_cu); }

// out = {G, spec, per, c_free, batch}
void wp_start(int64_t K, int n_cu, int Ne, int spec, int64_t* out)
{
    const RoundsStart s = rounds_start(K, n_cu, Ne, spec, read_walk_switches());
    out[0] = s.G; out[1] = s.spec; out[2] = s.per; out[3] = s.c_free; out[4] = s.batch();
}

// in = the fields of RoundsIn in their order; plan = {ok, cu_form, G, W, spec, PB, CH, tiles, depth, per, C, c_free, nblk, r_max, lds};
// arena = {n_dbl, n_ll, n_int, g_bytes, the 17 offsets in the struct's order, words_bytes}
void wp_plan(const int64_t* in, int64_t* plan, int64_t* arena)
{
    const RoundsIn r{in[0], (int)in[1], (int)in[2], (int)in[3], (int)in[4], (int)in[5], (int)in[6], (int)in[7], (int)in[8], (int)in[9],
                     (int)in[10], (int)in[11]};
    const RoundsPlan p = plan_rounds(r, read_walk_switches(), [&](int pb, int ch) { return tile_lds(r.D, pb, ch); });
    const int64_t v[15] = {p.ok, p.cu_form, p.G, p.W, p.spec, p.PB, p.CH, p.tiles, p.depth, p.per, p.C, p.c_free, p.nblk, p.r_max, (int64_t)p.lds};
    for (int i = 0; i < 15; ++i) plan[i] = v[i];
    if (!p.ok) return;
    const RoundsArena a = rounds_arena(p, r.D);
    const size_t w[22] = {a.n_dbl, a.n_ll, a.n_int, a.g_bytes, a.dir, a.dirnext, a.tmin, a.tmax, a.theta_c[0], a.theta_c[1], a.wt, a.wres_logl,
                          a.res_logl, a.calls_part, a.slots_part, a.ring, a.ws, a.wres_flags, a.wdef, a.res_flags, a.owner, a.words_bytes()};
    for (int i = 0; i < 22; ++i) arena[i] = (int64_t)w[i];
}

// out = {ok, PB, CH}
void wp_walk_tile(int PB0, int D, int Ne, int chunk_items, int pb_override, int64_t n, int64_t* out)
{
    const WalkTile t = walk_tile(PB0, D, Ne, chunk_items, pb_override, n, [&](int pb, int ch) { return walk_lds(D, pb, ch); });
    out[0] = t.ok; out[1] = t.PB; out[2] = t.CH;
}

// out = {two parts, rows form, moves of the first part in the rows form, ... in the queue form}
void wp_parts(int64_t K, int64_t resident, int PB, int D, int CH, int nsteps, int64_t* out)
{
    const WalkSwitches sw = read_walk_switches();
    out[0] = walk_two_parts(K, resident, PB, nsteps, sw); out[1] = walk_rows_form(sw, PB, D, CH);
    out[2] = first_part_steps(nsteps, true, sw); out[3] = first_part_steps(nsteps, false, sw);
}

// order [K] out; returns K2
int64_t wp_order(const int32_t* cost, const int32_t* done, int64_t K, int first, int max_rounds, int32_t* order)
{
    std::vector<int32_t> o;
    const int64_t K2 = order_by_cost(std::vector<int32_t>(cost, cost + K), std::vector<int32_t>(done, done + K), first, max_rounds, &o);
    std::copy(o.begin(), o.end(), order);
    return K2;
}

// order [n] in place; returns the workgroups the deal went round
int64_t wp_deal(int32_t* order, int64_t n, int64_t K2, int PB, int64_t resident)
{
    std::vector<int32_t> o(order, order + n);
    const int64_t G = walk_blocks(K2, PB, resident);
    deal_first_rows(&o, K2, G, PB);
    std::copy(o.begin(), o.end(), order);
    return G;
}

// out = {threads, budget, ok, G, rows, PB, CH, rows a workgroup can park with that tile}
void wp_rows(int64_t K2, int cus, int slim, int Ne, int D, int PB, int CH, int64_t* out)
{
    const int nt = rows_threads(read_walk_switches(), slim != 0);
    out[0] = nt; out[1] = (int64_t)rows_budget(nt);
    WideRows w{true, 0, 0, PB, CH};
    if (nt != walkplan::kThreads) w = wide_rows(K2, cus, nt, Ne, D, [&](int pb, int ch, int rows) { return rows_lds(D, pb, ch, rows); });
    out[2] = w.ok; out[3] = w.G; out[4] = w.rows; out[5] = w.PB; out[6] = w.CH;
    out[7] = rows_parked_max(rows_budget(nt), [&](int rows) { return rows_lds(D, w.PB, w.CH, rows); });
}

}  // extern "C"
