// Host program for tests/test_sched_units.py: walks the work lists of algp_amd/csrc/gemm_sched.h over a grid of launch shapes and
// checks the schedule's invariants.  Prints one line per violated invariant and "checked <n> shapes"; exit status 1 on any.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../algp_amd/csrc/gemm_sched.h"

using namespace algp;

static int bad = 0;
#define CHECK(cond, what)                                                                                      \
    do {                                                                                                       \
        if (!(cond)) {                                                                                         \
            ++bad;                                                                                             \
            printf("FAIL %s: tiles_m %d tiles_n %d kblocks %d slots %d kcut %d\n", what, tm, tn, kb, slots, kcut); \
        }                                                                                                      \
    } while (0)

static void check(int tm, int tn, int kb, int slots, int kcut) {
    const Sched s = sched_make(slots, tm, tn, kb, kcut, 1);
    const int tiles = tm * tn;
    CHECK(s.G == std::min(tiles, slots) && s.G >= 1, "grid");
    CHECK(s.tiles == tiles, "tile count");
    if (!kcut) {
        CHECK(s.full == tiles / s.G * s.G && s.left == tiles - s.full, "whole-tile share");
        if (s.left > 0) CHECK(s.S == std::max(1, std::min(s.G / s.left, kb)), "slices per leftover tile");
        else CHECK(s.S == 0, "no leftover, no slices");
    }
    std::vector<std::vector<int>> cover(tiles, std::vector<int>(kb, 0));
    std::vector<std::vector<std::pair<int, int>>> pieces(tiles);       // per tile: (kb0, kb1) of every unit
    std::vector<int> seen_slice(s.left * std::max(s.S, 1), 0);
    std::vector<long> total(s.G, 0);
    long longest_extra = 0;
    for (int wg = 0; wg < s.G; ++wg) {
        const int n = sched_count(s, wg);
        int slices = 0, prev_len = 1 << 30;
        for (int i = 0; i < n; ++i) {
            const SchedUnit u = sched_unit(s, wg, i);
            CHECK(u.tile >= 0 && u.tile < tiles, "tile in range");
            CHECK(u.kb0 >= 0 && u.kb0 < u.kb1 && u.kb1 <= kb, "k range non-empty and inside");
            if (u.tile < 0 || u.tile >= tiles || u.kb0 < 0 || u.kb1 > kb) continue;
            for (int q = u.kb0; q < u.kb1; ++q) cover[u.tile][q]++;
            pieces[u.tile].push_back({u.kb0, u.kb1});
            total[wg] += u.kb1 - u.kb0;
            if (u.slice >= 0) {
                ++slices;
                CHECK(!kcut, "no slices in the triangular form");
                CHECK(u.tile >= s.full, "only leftover tiles are cut");
                CHECK(u.slice < s.left * s.S, "slice index in range");
                if (u.slice < (int)seen_slice.size()) seen_slice[u.slice]++;
                // the finish kernel sums tile j's partials j * S .. j * S + S - 1 in this order: ascending k
                CHECK(u.slice / s.S == u.tile - s.full, "slice belongs to its tile");
                CHECK(u.kb0 == (long long)(u.slice % s.S) * kb / s.S, "slices ascend in k");
            } else if (!kcut) {
                CHECK(u.kb0 == 0 && u.kb1 == kb, "a whole tile walks the whole k range");
            }
            if (!kcut) CHECK((i >= s.rounds) == (u.tile >= s.full), "the leftover tiles are the last of the row-major list");
            if (!kcut && i >= s.rounds) longest_extra = std::max<long>(longest_extra, u.kb1 - u.kb0);
            if (kcut) {
                const int bn = u.tile % tn;
                CHECK(u.kb0 == 0 && u.kb1 == bn + 1, "column tile c walks c + 1 blocks");
                CHECK(u.kb1 - u.kb0 <= prev_len, "a workgroup's tiles never get longer");
                prev_len = u.kb1 - u.kb0;
            }
        }
        CHECK(slices <= 1, "at most one slice per workgroup");
    }
    for (int t = 0; t < tiles; ++t) {
        const int want = kcut ? t % tn + 1 : kb;
        bool once = true;
        for (int q = 0; q < kb; ++q) once = once && cover[t][q] == (q < want ? 1 : 0);
        CHECK(once, "every (tile, k block) exactly once");
        std::sort(pieces[t].begin(), pieces[t].end());
        bool contiguous = !pieces[t].empty() && pieces[t].front().first == 0 && pieces[t].back().second == want;
        for (size_t q = 1; q < pieces[t].size(); ++q) contiguous = contiguous && pieces[t][q].first == pieces[t][q - 1].second;
        CHECK(contiguous, "a tile's pieces are contiguous in k");
        // the leftover tiles, and only they, are the last ones of the row-major list
        if (!kcut && s.S >= 2) CHECK((pieces[t].size() > 1) == (t >= s.full) && (t < s.full || (int)pieces[t].size() == s.S), "leftover tiles are the last");
    }
    for (int v : seen_slice)
        if (!kcut && s.S >= 2) CHECK(v == 1, "every partial sum written once");
    const long hi = *std::max_element(total.begin(), total.end()), lo = *std::min_element(total.begin(), total.end());
    if (!kcut) {
        // every workgroup: rounds whole tiles, plus at most one leftover unit (a slice; the whole tile when S = 1)
        CHECK(hi - lo <= longest_extra + 1, "update form: totals within one slice plus one block");
    } else {
        // Dealing a never-increasing sequence round-robin: workgroup w < w' has, unit by unit, a tile no shorter than w' and no
        // longer than the PREVIOUS unit of w', so 0 <= total(w) - total(w') <= first unit of w <= tiles_n blocks.  (One block,
        // as for equal tiles, is not attainable with whole tiles: one row panel on four workgroups is 4, 3, 2, 1.)
        CHECK(hi - lo <= tn, "triangular form: totals within one longest tile");
    }
    if (!kcut) {
        // XCD groups (wg & 7): in every round the group's workgroups hold consecutive tiles, and the group's rounds follow each
        // other in the list -- a contiguous share
        for (int x = 0; x < 8 && x < s.G; ++x) {
            int expect = -1;
            for (int i = 0; i < s.rounds; ++i)
                for (int wg = x; wg < s.G; wg += 8) {
                    const int t = sched_unit(s, wg, i).tile;
                    if (expect >= 0) CHECK(t == expect, "group share contiguous, consecutive within a round");
                    expect = t + 1;
                }
        }
    }
}

int main() {
    const int tms[] = {1, 3, 127, 128, 129, 401, 512, 782}, tns[] = {1, 2, 4}, kbs[] = {1, 4, 5, 76}, gs[] = {8, 512};
    int n = 0;
    for (int tm : tms)
        for (int tn : tns)
            for (int g : gs) {
                for (int kb : kbs) { check(tm, tn, kb, g, 0); ++n; }
                check(tm, tn, tn, g, 1);                               // triangular: k == n
                ++n;
            }
    // the shapes the GPU tests and the headline run name: 401 x 4 tiles on 512 -> 68 leftover, 7 slices; 782 x 4 -> 56, 9
    const Sched a = sched_make(512, 401, 4, 8, 0, 1), b = sched_make(512, 782, 4, 40, 0, 1), c = sched_make(512, 475, 4, 8, 0, 1),
                d = sched_make(512, 448, 4, 8, 0, 1), e = sched_make(512, 512, 4, 8, 0, 1);
    if (a.left != 68 || a.S != 7 || b.left != 56 || b.S != 9 || c.left != 364 || c.S != 1 || d.left != 256 || d.S != 2 || e.left != 0) {
        printf("FAIL named shapes: %d %d | %d %d | %d %d | %d %d | %d\n", a.left, a.S, b.left, b.S, c.left, c.S, d.left, d.S, e.left);
        ++bad;
    }
    printf("checked %d shapes\n", n);
    return bad ? 1 : 0;
}
