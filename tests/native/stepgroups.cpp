// The walker groups of a resident ensemble step (evidence_amd/csrc/rvll_step_groups.h) behind one C function, for
// tests/test_step_groups_host.py: host code only.  With -DSTEPGROUPS_MAIN the same function behind a program that reads cases
// from a text file and prints what it built (the build under the address and undefined-behaviour sanitizers).
#include <cinttypes>
#include <cstdio>
#include "rvll_step_groups.h"

using namespace rvll::host;

// Returns 0, or what step_segments refused (1: a cluster count, 2: a label) with sizes = {listed run, value}.  On success
// sizes = {segments S, groups G}; cnt [A m] holds run a's counts at a m (-1 beyond its clusters); segtab, segsc, seg_of [2 S];
// perm, grun, grid [A kdead]; gofs, gcnt, glstar, gseed, gsteps [G], gfac [2 G].  steps may be null.
extern "C" int sg_build(const int32_t* lab, const int32_t* ncl, const int32_t* ranks, const double* lstar, const uint64_t* seeds,
                        const int32_t* steps, int32_t nsteps, int32_t A, int64_t kdead, int64_t m, int32_t D, int64_t* sizes,
                        int64_t* cnt, int64_t* segtab, double* segsc, int32_t* seg_of, int32_t* perm, int32_t* grun, int32_t* grid,
                        int64_t* gofs, int64_t* gcnt, double* glstar, uint64_t* gseed, int32_t* gsteps, int32_t* gfac)
{
    StepSegments seg;
    const StepGroupsError bad = step_segments(lab, ncl, A, m, D, &seg);
    if (bad.what != StepGroupsError::kNone) {
        sizes[0] = bad.a; sizes[1] = bad.value;
        return (int)bad.what;
    }
    StepGroups G;
    step_groups(seg.cnt, lab, ranks, lstar, seeds, steps, nsteps, A, kdead, m, &G);
    const size_t S = seg.seg_of.size(), NG = G.gofs.size();
    sizes[0] = (int64_t)S; sizes[1] = (int64_t)NG;
    for (int64_t i = 0; i < (int64_t)A * m; ++i) cnt[i] = -1;
    for (int32_t a = 0; a < A; ++a)
        for (size_t c = 0; c < seg.cnt[(size_t)a].size(); ++c) cnt[a * m + (int64_t)c] = seg.cnt[(size_t)a][c];
    for (size_t s = 0; s < S; ++s) {
        segtab[2 * s] = seg.segtab[2 * s]; segtab[2 * s + 1] = seg.segtab[2 * s + 1];
        segsc[2 * s] = seg.segsc[2 * s]; segsc[2 * s + 1] = seg.segsc[2 * s + 1];
        seg_of[2 * s] = seg.seg_of[s].first; seg_of[2 * s + 1] = seg.seg_of[s].second;
    }
    for (size_t e = 0; e < G.perm.size(); ++e) { perm[e] = G.perm[e]; grun[e] = G.grun[e]; grid[e] = G.grid[e]; }
    for (size_t g = 0; g < NG; ++g) {
        gofs[g] = G.gofs[g]; gcnt[g] = G.gcnt[g]; glstar[g] = G.glstar[g]; gseed[g] = G.gseed[g]; gsteps[g] = G.gsteps[g];
        gfac[2 * g] = G.gfac[g].first; gfac[2 * g + 1] = G.gfac[g].second;
    }
    return 0;
}

#ifdef STEPGROUPS_MAIN
#include <vector>

// Cases: "A kdead m D nsteps has_steps", then lab [A m], ncl [A], ranks [A kdead], lstar [A] (hex floats), seeds [A], and steps [A]
// when has_steps.  Prints per case the return code and the sizes, then every array sg_build filled, one per line.
int main(int argc, char** argv)
{
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    int A, D, nsteps, has_steps;
    long long kdead, m;
    while (fscanf(f, "%d %lld %lld %d %d %d", &A, &kdead, &m, &D, &nsteps, &has_steps) == 6) {
        const size_t K = (size_t)A * (size_t)kdead, M = (size_t)A * (size_t)m;
        std::vector<int32_t> lab(M), ncl((size_t)A), ranks(K), steps((size_t)A);
        std::vector<double> lstar((size_t)A);
        std::vector<uint64_t> seeds((size_t)A);
        bool ok = true;
        for (auto& v : lab) ok = ok && fscanf(f, "%" SCNd32, &v) == 1;
        for (auto& v : ncl) ok = ok && fscanf(f, "%" SCNd32, &v) == 1;
        for (auto& v : ranks) ok = ok && fscanf(f, "%" SCNd32, &v) == 1;
        for (auto& v : lstar) ok = ok && fscanf(f, "%la", &v) == 1;
        for (auto& v : seeds) ok = ok && fscanf(f, "%" SCNu64, &v) == 1;
        if (has_steps) for (auto& v : steps) ok = ok && fscanf(f, "%" SCNd32, &v) == 1;
        if (!ok) { fprintf(stderr, "bad case file\n"); return 2; }
        int64_t sizes[2] = {0, 0};
        std::vector<int64_t> cnt(M), segtab(2 * M), gofs(K), gcnt(K);
        std::vector<double> segsc(2 * M), glstar(K);
        std::vector<int32_t> seg_of(2 * M), perm(K), grun(K), grid(K), gsteps(K), gfac(2 * K);
        std::vector<uint64_t> gseed(K);
        const int rc = sg_build(lab.data(), ncl.data(), ranks.data(), lstar.data(), seeds.data(), has_steps ? steps.data() : nullptr, nsteps,
                                A, kdead, m, D, sizes, cnt.data(), segtab.data(), segsc.data(), seg_of.data(), perm.data(), grun.data(),
                                grid.data(), gofs.data(), gcnt.data(), glstar.data(), gseed.data(), gsteps.data(), gfac.data());
        printf("%d %" PRId64 " %" PRId64 "\n", rc, sizes[0], sizes[1]);
        if (rc) continue;
        const size_t S = (size_t)sizes[0], G = (size_t)sizes[1];
        auto ints = [](const auto& v, size_t n) { for (size_t i = 0; i < n; ++i) printf("%lld ", (long long)v[i]); printf("\n"); };
        ints(cnt, M); ints(segtab, 2 * S);
        for (size_t i = 0; i < 2 * S; ++i) printf("%a ", segsc[i]);
        printf("\n");
        ints(seg_of, 2 * S); ints(perm, K); ints(grun, K); ints(grid, K); ints(gofs, G); ints(gcnt, G);
        for (size_t i = 0; i < G; ++i) printf("%a ", glstar[i]);
        printf("\n");
        for (size_t i = 0; i < G; ++i) printf("%" PRIu64 " ", gseed[i]);
        printf("\n");
        ints(gsteps, G); ints(gfac, 2 * G);
    }
    fclose(f);
    return 0;
}
#endif
