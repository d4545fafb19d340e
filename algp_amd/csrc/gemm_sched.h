// The work list of a scheduled (persistent) launch of the GEMM tile kernel: which 128 x 128 output tiles, and which part of
// their k range, workgroup `wg` of a grid of G walks, in closed form.  One definition for the launcher, the kernel and the
// CPU test (tests/test_sched_units.py compiles this header with a host compiler): no HIP types in here.
//
// Update form (kcut = 0): the tiles are row-major, tile = bm * tiles_n + bn, each with the whole k range of `kblocks`
// 128-element blocks.
//   * full = (tiles / G) * G tiles from the front of the list are whole-tile units, tiles / G per workgroup.  Workgroups are
//     grouped as the hardware deals them to its 8 XCDs (wg & 7); group x owns a contiguous share of the list, and in round i
//     its workgroups hold consecutive tiles -- the column tiles of a row panel stay in flight together in one L2.
//   * the left = tiles - full tiles at the END of the list are cut along k into S = min(G / left, kblocks) slices of whole
//     128-blocks (split allowed and S >= 2), one slice per workgroup at most, none empty: slice s of leftover tile j covers
//     blocks [s kblocks / S, (s + 1) kblocks / S) and its partial sum has index j * S + s.  With S = 1 the leftover tiles are
//     whole tiles, one each for the first `left` workgroups.
// Triangular form (kcut = 1, k == n): column tile c walks blocks [0, c + 1).  Whole tiles only, dealt by descending length:
// class c = tiles_n - 1 first, tiles_m tiles each, in rounds of G over the workgroups from where the previous class stopped --
// boustrophedon: even rounds run up the workgroups, odd rounds down (deal position d = i G + (i odd ? G - 1 - wg : wg); the unit
// exists when d < tiles), so the workgroup that got the longest tile of one round gets the shortest of the next.  Per workgroup
// the lengths never increase from unit to unit, and two workgroups still differ by at most one longest tile (tiles_n blocks);
// where every round ran up, the first workgroups collected the long end of every round: 782 x 4 tiles on 512 workgroups were
// 18 blocks at most against a mean of 15.3, and are 16 now.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ALGP_SCHED_HD __host__ __device__ inline
#else
#define ALGP_SCHED_HD inline
#endif

namespace algp {

struct Sched {
    int G;                  // workgroups of the launch
    int tiles_m, tiles_n, kblocks, kcut;
    int tiles, rounds, full, left, S;   // S: slices per leftover tile (0: no leftover; 1: whole tiles)
};

struct SchedUnit {
    int tile;               // bm * tiles_n + bn
    int kb0, kb1;           // 128-element k blocks [kb0, kb1)
    int slice;              // -1: the unit writes its output tile; >= 0: index of its partial sum
};

ALGP_SCHED_HD Sched sched_make(int slots, int tiles_m, int tiles_n, int kblocks, int kcut, int allow_split) {
    Sched s;
    s.tiles_m = tiles_m; s.tiles_n = tiles_n; s.kblocks = kblocks; s.kcut = kcut;
    s.tiles = tiles_m * tiles_n;
    s.G = s.tiles < slots ? s.tiles : slots;
    s.rounds = s.G > 0 ? s.tiles / s.G : 0;
    s.full = s.rounds * s.G;
    s.left = s.tiles - s.full;
    s.S = 0;
    if (kcut) { s.full = s.tiles; s.left = 0; return s; }
    if (s.left > 0) {
        s.S = 1;
        if (allow_split) {
            s.S = s.G / s.left;
            if (s.S > kblocks) s.S = kblocks;
        }
    }
    return s;
}

// position of workgroup wg in group-major order (groups = wg & 7), the size of its group and the workgroups before the group
ALGP_SCHED_HD void sched_group(const Sched& s, int wg, int* before, int* size, int* local) {
    const int x = wg & 7, q = s.G >> 3, r = s.G & 7;
    *before = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    *size = q + (x < r ? 1 : 0);
    *local = wg >> 3;
}

// (TRI = false: for a kernel that never takes the triangular form -- the generating product, which sits at its register limit
// and is compiled without the branch)
template <bool TRI = true>
ALGP_SCHED_HD int sched_count(const Sched& s, int wg) {
    if (TRI && s.kcut) {                                                  // whole rounds, and the last one from its end of the workgroups
        const int r = s.tiles / s.G;
        return r + (((r & 1) ? s.G - 1 - wg : wg) < s.tiles - r * s.G ? 1 : 0);
    }
    int extra = 0;
    if (s.S >= 2) {
        int before, size, local;
        sched_group(s, wg, &before, &size, &local);
        extra = before + local < s.left * s.S ? 1 : 0;
    } else if (s.S == 1) {
        extra = wg < s.left ? 1 : 0;
    }
    return s.rounds + extra;
}

template <bool TRI = true>
ALGP_SCHED_HD SchedUnit sched_unit(const Sched& s, int wg, int i) {
    SchedUnit u;
    u.slice = -1;
    if (TRI && s.kcut) {
        const int d = i * s.G + ((i & 1) ? s.G - 1 - wg : wg);     // place in the deal: classes of tiles_m tiles, longest first
        const int cls = d / s.tiles_m, bm = d - cls * s.tiles_m, bn = s.tiles_n - 1 - cls;
        u.tile = bm * s.tiles_n + bn;
        u.kb0 = 0;
        u.kb1 = bn + 1 < s.kblocks ? bn + 1 : s.kblocks;
        return u;
    }
    int before, size, local;
    sched_group(s, wg, &before, &size, &local);
    u.kb0 = 0;
    u.kb1 = s.kblocks;
    if (i < s.rounds) {
        u.tile = s.rounds * before + i * size + local;
    } else if (s.S >= 2) {
        const int pos = before + local;                            // slice-major: neighbours hold the same k range of consecutive tiles
        const int sl = pos / s.left, j = pos - sl * s.left;
        u.tile = s.full + j;
        u.kb0 = (int)((long long)sl * s.kblocks / s.S);
        u.kb1 = (int)((long long)(sl + 1) * s.kblocks / s.S);
        u.slice = j * s.S + sl;
    } else {
        u.tile = s.full + wg;
    }
    return u;
}

}  // namespace algp
