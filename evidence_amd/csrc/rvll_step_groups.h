// rvll_step_groups.h — the walker groups of a resident ensemble step (stages 3 and 5): index arithmetic on host arrays
// without a HIP call or a handle, so tests/test_step_groups_host.py builds it with a host compiler and holds it against
// nested._walk_groups.  Listed run a has m survivors in rank order, labelled lab[a m ..], and kdead walkers that start from the
// survivors of ranks ranks[a kdead ..].
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace rvll {
namespace host {

constexpr uint64_t kGroupSeedMul = 0xD1B54A32D192ED03ull;   // walk seed of cluster c > 0: seed + c kGroupSeedMul (nested._GROUP_MUL)

// what step_segments found wrong (it looks run by run: the cluster count, then the labels in rank order): listed run a's cluster
// count `value`, or its label `value`
struct StepGroupsError {
    enum What { kNone = 0, kClusterCount = 1, kLabelRange = 2 } what = kNone;
    int32_t a = 0, value = 0;
};

// Stage 3.  cnt[a][c]: rows of cluster c of listed run a.  The clusters of at least 2 D rows of the runs with more than one cluster
// are the segments of one moments pass: segment s = seg_of[s] (listed run, cluster) is segtab[2 s + 1] rows from slot segtab[2 s] of
// the packed (label, rank) order (run a's block starts at a m, its clusters in label order), folded with segsc[2 s] = 1 / rows and
// segsc[2 s + 1] = 1 / (rows - 1).
struct StepSegments {
    std::vector<std::vector<long long>> cnt;
    std::vector<long long> segtab;
    std::vector<double> segsc;
    std::vector<std::pair<int32_t, int32_t>> seg_of;
};

inline StepGroupsError step_segments(const int32_t* lab, const int32_t* ncl, int32_t A, long long m, int D, StepSegments* out)
{
    *out = StepSegments{};
    out->cnt.resize((size_t)A);
    for (int32_t a = 0; a < A; ++a) {
        const int32_t k = ncl[a];
        if (k < 1 || k > m) return {StepGroupsError::kClusterCount, a, k};
        std::vector<long long>& cnt = out->cnt[(size_t)a];
        cnt.assign((size_t)k, 0);
        for (long long j = 0; j < m; ++j) {
            const int32_t c = lab[a * m + j];
            if (c < 0 || c >= k) return {StepGroupsError::kLabelRange, a, c};
            ++cnt[(size_t)c];
        }
        if (k == 1) continue;
        long long off = (long long)a * m;
        for (int32_t c = 0; c < k; ++c) {
            const long long rows = cnt[(size_t)c];
            if (rows >= 2 * (long long)D) {
                out->segtab.push_back(off); out->segtab.push_back(rows);
                out->segsc.push_back(1.0 / (double)rows); out->segsc.push_back(1.0 / (double)(rows > 1 ? rows - 1 : 1));
                out->seg_of.emplace_back(a, c);
            }
            off += rows;
        }
    }
    return {};
}

// The group tables of a step's walk.  Walk row e is walker perm[e] = a kdead + i (walker i of listed run a), in group grun[e] with
// the index grid[e] inside it; group g's survivors are slots gofs[g] .. + gcnt[g] of the order the step names, it walks above
// glstar[g] with seed gseed[g], gsteps[g] moves and the factor of gfac[g] = (listed run, cluster).
struct StepGroups {
    std::vector<int32_t> perm, grun, grid;
    std::vector<int64_t> gofs, gcnt;
    std::vector<double> glstar;
    std::vector<uint64_t> gseed;
    std::vector<int32_t> gsteps;
    std::vector<std::pair<int32_t, int32_t>> gfac;
};

// Stage 5 (nested.py's _walk_groups): per run the non-empty clusters of the start rows in label order, walkers in their order inside
// a group; slots of the packed (label, rank) order.  cnt and lab as step_segments left and checked them, ranks in [0, m).
inline void step_groups(const std::vector<std::vector<long long>>& cnt, const int32_t* lab, const int32_t* ranks, const double* lstar,
                        const uint64_t* seeds, const int32_t* steps, int32_t nsteps, int32_t A, int64_t kdead, long long m,
                        StepGroups* out)
{
    const int64_t K = (int64_t)A * kdead;
    *out = StepGroups{};
    out->perm.resize((size_t)K); out->grun.resize((size_t)K); out->grid.resize((size_t)K);
    int64_t e = 0;
    std::vector<int32_t> wc((size_t)kdead);
    std::vector<long long> first;
    for (int32_t a = 0; a < A; ++a) {
        const size_t k = cnt[(size_t)a].size();
        first.assign(k + 1, 0);
        for (int64_t i = 0; i < kdead; ++i) {
            wc[(size_t)i] = lab[a * m + ranks[(size_t)a * kdead + i]];
            ++first[(size_t)wc[(size_t)i] + 1];
        }
        for (size_t c = 0; c < k; ++c) first[c + 1] += first[c];
        std::vector<int32_t> gof(k, -1);             // group number of cluster c (-1: no walker starts in it)
        long long offc = (long long)a * m;
        for (size_t c = 0; c < k; ++c) {
            offc += c > 0 ? cnt[(size_t)a][c - 1] : 0;
            if (first[c + 1] == first[c]) continue;
            gof[c] = (int32_t)out->gofs.size();
            out->gofs.push_back(offc);
            out->gcnt.push_back(cnt[(size_t)a][c]);
            out->gsteps.push_back(steps ? steps[a] : nsteps);
            out->glstar.push_back(lstar[a]);
            out->gseed.push_back(c == 0 ? seeds[a] : seeds[a] + (uint64_t)c * kGroupSeedMul);
            out->gfac.emplace_back(a, (int32_t)c);
        }
        std::vector<long long> at(first.begin(), first.end() - 1);
        for (int64_t i = 0; i < kdead; ++i) {
            const size_t c = (size_t)wc[(size_t)i];
            const long long r = at[c]++;
            const int64_t row = e + r;
            out->perm[(size_t)row] = (int32_t)((int64_t)a * kdead + i);
            out->grun[(size_t)row] = gof[c];
            out->grid[(size_t)row] = (int32_t)(r - first[c]);
        }
        e += kdead;
    }
}

// The unclustered step: one group per listed run, walkers in their own order, group a's survivors the ranks kdead .. n of run a's
// sort order (slots a n + kdead .. of the packed orders); lstar, seed, steps and factor per group are the caller's per-run arrays.
inline void step_groups_identity(int32_t A, int64_t kdead, long long n, StepGroups* out)
{
    const int64_t K = (int64_t)A * kdead;
    *out = StepGroups{};
    out->perm.resize((size_t)K); out->grun.resize((size_t)K); out->grid.resize((size_t)K);
    for (int64_t e = 0; e < K; ++e) {
        out->perm[(size_t)e] = (int32_t)e;
        out->grun[(size_t)e] = (int32_t)(e / kdead);
        out->grid[(size_t)e] = (int32_t)(e % kdead);
    }
    out->gofs.resize((size_t)A); out->gcnt.assign((size_t)A, n - kdead);
    for (int32_t a = 0; a < A; ++a) out->gofs[(size_t)a] = (int64_t)a * n + kdead;
}

}  // namespace host
}  // namespace rvll
