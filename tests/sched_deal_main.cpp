// Host program for tests/test_sched_deal.py: the triangular form's deal of algp_amd/csrc/gemm_sched.h (whole tiles, longest
// first, odd rounds dealt down the workgroups) against the plain round-robin deal of the same sequence, which this program
// computes itself from d = wg + i * G.  Prints one line per violated expectation and "checked <n> shapes"; exit status 1 on any.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../algp_amd/csrc/gemm_sched.h"

using namespace algp;

static int bad = 0;
#define CHECK(cond, what)                                                                  \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            ++bad;                                                                         \
            printf("FAIL %s: tiles_m %d tiles_n %d slots %d\n", what, tm, tn, slots);      \
        }                                                                                  \
    } while (0)

struct Totals {
    long hi, lo, sum;
};

// per-workgroup totals of k blocks as the header deals the tiles; every tile must be dealt once
static Totals dealt(int tm, int tn, int slots) {
    const Sched s = sched_make(slots, tm, tn, tn, 1, 1);
    std::vector<int> seen(tm * tn, 0);
    std::vector<long> total(s.G, 0);
    for (int wg = 0; wg < s.G; ++wg) {
        const int n = sched_count(s, wg);
        for (int i = 0; i < n; ++i) {
            const SchedUnit u = sched_unit(s, wg, i);
            CHECK(u.tile >= 0 && u.tile < tm * tn, "tile in range");
            if (u.tile < 0 || u.tile >= tm * tn) continue;
            seen[u.tile]++;
            CHECK(u.kb0 == 0 && u.kb1 == u.tile % tn + 1 && u.slice < 0, "column tile c is a whole tile of c + 1 blocks");
            total[wg] += u.kb1 - u.kb0;
        }
    }
    CHECK(std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; }), "every tile exactly once");
    Totals t = {*std::max_element(total.begin(), total.end()), *std::min_element(total.begin(), total.end()), 0};
    for (long v : total) t.sum += v;
    return t;
}

// the same sequence (classes of tm tiles, tn blocks first) dealt round-robin: position d = wg + i * G
static Totals round_robin(int tm, int tn, int slots) {
    const int tiles = tm * tn, G = std::min(tiles, slots);
    std::vector<long> total(G, 0);
    for (int d = 0; d < tiles; ++d) total[d % G] += tn - d / tm;
    Totals t = {*std::max_element(total.begin(), total.end()), *std::min_element(total.begin(), total.end()), 0};
    for (long v : total) t.sum += v;
    return t;
}

static Totals check(int tm, int tn, int slots) {
    const Totals a = dealt(tm, tn, slots), b = round_robin(tm, tn, slots);
    CHECK(a.sum == b.sum && a.sum == (long)tm * tn * (tn + 1) / 2, "the same work");
    CHECK(a.hi <= b.hi, "the longest workgroup is no longer than under the round-robin deal");
    CHECK(a.hi - a.lo <= tn, "totals within one longest tile");
    return a;
}

int main() {
    const int tms[] = {1, 3, 127, 128, 129, 401, 512, 782}, tns[] = {1, 2, 4}, gs[] = {8, 512};
    int n = 0;
    for (int tm : tms)
        for (int tn : tns)
            for (int g : gs) { check(tm, tn, g); ++n; }
    // the shapes the GPU tests and the headline run name, on 512 slots
    {
        const int tm = 782, tn = 4, slots = 512;
        const Totals t = check(tm, tn, slots);
        CHECK(t.hi == (t.sum + slots - 1) / slots && t.hi == 16, "782 x 4: the longest workgroup holds the mean, rounded up (16)");
        ++n;
    }
    {
        const int tm = 401, tn = 4, slots = 512;
        const Totals t = check(tm, tn, slots);
        CHECK(t.hi == (t.sum + slots - 1) / slots && t.hi == 8, "401 x 4: the longest workgroup holds the mean, rounded up (8)");
        ++n;
    }
    {
        const int tm = 475, tn = 4, slots = 512;
        const Totals t = check(tm, tn, slots);
        CHECK(t.hi - t.lo <= 2, "475 x 4: totals within 2 blocks");
        ++n;
    }
    printf("checked %d shapes\n", n);
    return bad ? 1 : 0;
}
