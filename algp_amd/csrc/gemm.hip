// gemm.hip -- D = alpha * A * B^T + beta * C on the gfx950 matrix cores, fp64 and fp32.
//
// This one kernel carries the O(n^2 m) terms of the path outside the one-launch factorisation: the candidate
// solve V^T = B^T L^-T, the posterior covariance V^T V, the factor updates and the launch-sequence Cholesky.
// All are "NT" products with both operands contiguous along k, so one staging path serves.
//
// Shape: 128 x 128 output tile per 256-thread workgroup (4 waves as 2 x 2, each wave 64 x 64 =
// 4 x 4 MFMA tiles of 16 x 16).
//   fp64: v_mfma_f64_16x16x4_f64   (C/D: row = (lane>>4) + 4*reg, col = lane&15)
//   fp32: v_mfma_f32_16x16x4_f32   (C/D: row = (lane>>4)*4 + reg, col = lane&15)
// Both take ONE scalar of A and of B per lane (A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15]).
// Because the sum over k is order independent, lane group g = lane>>4 is handed the 16-byte chunk g of the
// row piece instead (2 f64 / 4 f32 consecutive k per chunk): one ds_read_b128 then feeds 2 (f64) or 4 (f32)
// MFMA k-steps, and A and B use the same permutation so products pair up.
//
// The kernel (gemm_nt_kernel_dma4): k advances 64 bytes per row per step (8 f64 / 16 f32); the operand pieces go
// global -> LDS by DMA (global_load_lds_dwordx4, no staging registers, no ds_write pass) into FOUR 16 KB stages,
// three k-tiles in flight while one is multiplied, with hand-placed s_waitcnt vmcnt(8/4/0) + s_barrier per k-tile;
// two workgroups per CU (64 KB LDS, 178 VGPRs each).
// LDS image per operand and stage: [128 rows][4 chunks of 16 B], chunk index XOR ((row>>2)&2).
// Round 1 measured its predecessors against it -- register-staged with one k-tile of prefetch (64.6 TFLOP/s at fp64
// 4096^3), two-stage LDS-DMA, fragment double-buffering, s_setprio around the MFMAs, 5 stages, 3 workgroups per CU --
// all slower (profiles/r01_gemm_ab_f64.txt); they are no longer in the source.
//   fp64 4096^3: 71.0 TFLOP/s (90 % of 78.6); candidate solve in situ 68 TFLOP/s.
//
// Requirements (the library pads every matrix to multiples of 128 with zeros / identity):
//   m % 128 == 0, n % 128 == 0, k % 128 == 0, leading dimensions multiples of 4 elements,
//   16-byte aligned base pointers.  In-place use (D aliasing A) is safe iff n == 128: a
//   workgroup then reads exactly the rows it later overwrites and finishes reading first.
#include "common.h"
#include <hip/hip_ext.h>
#include "mfma.h"
#include "gemm_sched.h"
#include <algorithm>
#include <type_traits>
#include <stdio.h>
#include <stdlib.h>

namespace algp {

template <typename T>
struct GemmArgs {
    const T* A;
    const T* B;
    const T* C;
    T* D;
    int64_t lda, ldb, ldc, ldd;
    int64_t sA, sB, sC, sD;        // batch strides in elements (blockIdx.y = batch index)
    int tiles_m, tiles_n, ktiles;
    T alpha, beta;
    int lower_only;
    int ktri;                      // lower_only products of an UPPER-triangular operand with itself (X X^T, X = L^-T): row tile bm of
                                   // X is zero left of column 128 bm, so tile (bm, bn <= bm) sums over k >= 128 bm only
    int kcut;                      // B is LOWER triangular by 128 x 128 tiles (X * inv(L_JJ)^T with an explicit block inverse): column
                                   // tile bn sums over k < 128 (bn + 1) only
    // STATS kernels only (the launches that write a column tile of V^T for the last time): per output row, the sums over
    // the tile's 128 columns of d^2 and of d * stat_w[column] go to stat_out[2 bn + 0 / 1][row] (second index: stat_ld apart)
    const T* stat_w;
    T* stat_out;
    int64_t stat_ld;
    // SCHED kernels only: the launch's work list (gemm_sched.h) and where the k slices of its leftover tiles leave their partial
    // sums (slice q: a row-major 128 x 128 tile at part + q * 128 * 128)
    Sched sch;
    T* part;
};

// GEN kernels only (the scheduled update products of the candidate sweep with fused right-hand sides, RhsGen in common.h): C is
// not read -- entry (row, column) of the C tile is the B^T entry (row, col0 + column), formed in the epilogue by bt_entry from
// the gathered coordinates rx / cx (DP per row / column) and the rows' kinds rk.  FAM: which kernel forms the instantiation holds
// a copy of its store loop for -- 0: RBF and Matern-3/2, 1: Matern-1/2 and Matern-5/2 (kernel_family, common.h).  Two forms per kernel and
// not four: the epilogue shares its registers with the k loop, and with four copies in one kernel the allocation of the whole
// kernel moved (fp64 256 -> 246 VGPRs, profiles/kernel_forms_resources.md): the RBF copy, which the headline step runs, would no
// longer be the code it was, in the one kernel here with no register to spare.
template <typename T, int DP_, int FAM_ = 0>
struct GenGemmArgs : GemmArgs<T> {
    static constexpr int DP = DP_;
    static constexpr int FAM = FAM_;
    const T* rx;
    const T* cx;
    const int* rk;
    int64_t col0;                  // global column of V^T that column 0 of this launch's output is
    int64_t ncols;                 // columns of the train set: the padding behind them is zero
    int kernel;
    T os;
};
template <typename A>
struct gen_dp { static constexpr int value = 0; };
template <typename T, int DP, int FAM>
struct gen_dp<GenGemmArgs<T, DP, FAM>> { static constexpr int value = DP; };

typedef __attribute__((address_space(3))) void* lds_vp;
typedef const __attribute__((address_space(1))) void* glb_vp;

// sum over the 16 lanes of a DPP row (the lanes that share lane >> 4), left in every lane: four rotate-and-add steps on
// the VALU (row_ror 8, 4, 2, 1), no LDS round trip (the same butterfly through __shfl_xor is 8 ds_bpermute per double with
// a wait each: 10 us per output tile in the epilogue below)
template <int CTRL>
__device__ __forceinline__ float dpp_row(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ double dpp_row(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <typename T>
__device__ __forceinline__ T row16_sum(T x) {
    x += dpp_row<0x128>(x);
    x += dpp_row<0x124>(x);
    x += dpp_row<0x122>(x);
    x += dpp_row<0x121>(x);
    return x;
}

// ---------------------------------------------------------------------------------------------
// Variance-reduction criterion (api_vr.hip): A = B = V^T, rows c against columns j.  The tile's accumulators hold
// G_cj = V_c . V_j; the epilogue forms E_cj = kappa_c C(c, j) - G_cj in registers (kappa_c = 1 for an ordinary row, 0 for a
// unit row; C from the scaled coordinates of the tile's 128 rows and 128 columns staged in LDS, with the one kernel-value
// definition kexp, or read from an explicit pool covariance), drops the columns that are not targets (unit rows, padding),
// squares, and sums over the tile's 128 columns per row exactly as the STATS epilogue does: stat_out[bn * stat_ld + row].
// With target weights attached (Args = VrWGemmArgs, an instantiation of its own, so that the unweighted one keeps the
// instructions and the bits it had) every column counts omega_j times (tw, per pool site).
// Neither a D tile nor a kernel-matrix block is written.  Fixed order: the same bits in every run.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct VrGemmArgs : GemmArgs<T> {
    const int64_t* cidx;           // pool index of every candidate row (M entries)
    const int* ckind;              // >= 0: a unit row
    int64_t M;                     // rows / columns beyond M are padding
    union {
        int64_t ncol0;             // candidate row that column 0 of this launch's B is
        const int64_t* cpool;      // VrxGemmArgs: the pool index of every column of B (negative: not a target), B being rows of its own
    };
    const T* Xs;                   // scaled coordinates, DP per site (coordinate pool)
    const T* Cp;                   // or the explicit pool covariance (n_pool x n_pool)
    int64_t n_pool;
    int DP, kernel;
    T os, noise;
    const T* tw;                   // target weight of every pool site (n_pool entries): VrWGemmArgs; PvrGemmArgs, or null there.
                                   // LAST: ahead of Xs it moved the fields behind it by 8 bytes in the kernel arguments, and the
                                   // unweighted product, the same instructions otherwise, took 2 % longer
};

template <typename T>
struct VrWGemmArgs : VrGemmArgs<T> {};   // the same launch with tw attached: the weighted epilogue
// The rectangular form (the criterion over the ranks of a communicator, api_vr.hip): the rows are this rank's V^T as above,
// the columns gathered rows of every rank's V^T -- B and ldb of their own, and on the column side cpool in the place of
// cidx / ckind / M.  The launch is batched over the ranks' slices (blockIdx.y): slice s of B lies sB elements further, its
// pool indices the same number of bytes behind cpool (they travel in front of their rows), and its column tile bn leaves its
// sums at stat_out[(s * tiles_n + bn) * stat_ld + row].  The same fields at the same offsets, tw still last.
template <typename T>
struct VrxGemmArgs : VrGemmArgs<T> {};
template <typename T>
struct VrxWGemmArgs : VrxGemmArgs<T> {};

// The additive form of any of the argument structs above (and of PvrGemmArgs below): part b's fields appended, which is what
// makes pool_cov take its additive branch (is_additive, common.h) and the launch a kernel of its own -- the single forms'
// kernels, their arguments and their instructions stay what they were.
template <typename T, typename Base>
struct AddGemmArgs : Base {
    int kernel_b, da, parts;
    T os_b;
};

// The relationship form of the same structs: the table's fields appended (is_rel, common.h), kernels of their own likewise
template <typename T, typename Base>
struct RelGemmArgs : Base {
    const T* G;
    int64_t Q;
    int da, parts;
    T os_g;
};

// The separable form of the same structs: its fields appended (is_sep, common.h), kernels of their own likewise
template <typename T, typename Base>
struct SepGemmArgs : Base {
    const T* sep_G;
    int64_t sep_Q;
    int sep_kb, sep_da, sep_dg, sep_hasg, sep_parts;
    T sep_osg;
};

// C(prow, pcol) for the two epilogues below: pool_cov (common.h) over the launch's own source fields, the coordinates of the
// row in registers and of the column staged in LDS, both at width MAXD
template <typename T, typename G>
__device__ __forceinline__ T vr_pool_cov(const G& g, int64_t prow, int64_t pcol, const T (&xrow)[MAXD], const T* xcol) {
    return pool_cov<MAXD>(g, prow, pcol, &xrow[0], xcol);
}

// RECT: the columns are described by cpool (this slice's 128 x tiles_n pool indices) instead of cidx / ckind / M
template <typename T, bool WEIGHTED, bool RECT, typename G, typename ACC>
__device__ __forceinline__ void vr_epilogue(const G& g, char* smem, const ACC (&acc)[4][4], int64_t m0, int64_t n0, int bn,
                                            int wr, int wc, int lane, int tid, const int64_t* cpool = nullptr) {
    using F = MF<T>;
    const int fr = lane & 15;
    // LDS: [2 column halves][128 rows] sums | coordinates of the rows, of the columns ([128][MAXD], zero padded) | pool
    // indices of the rows, of the columns | kappa of the rows | target mask of the columns (int), or WEIGHTED their target
    // weight (T; 0: not a target).  2 KB + 16 KB + 2 KB + 512 B + at most 128 doubles <= 21.5 KB of the main loop's 64 KB of
    // stages; the weights start 8-byte aligned.
    T* red = reinterpret_cast<T*>(smem);
    T* xr = reinterpret_cast<T*>(smem + 2048);
    T* xc = reinterpret_cast<T*>(smem + 2048 + 8192);
    int64_t* pr = reinterpret_cast<int64_t*>(smem + 2048 + 16384);
    int64_t* pc = pr + 128;
    int* kr = reinterpret_cast<int*>(pc + 128);
    int* mc = kr + 128;
    T* wcol = reinterpret_cast<T*>(kr + 128);
    __syncthreads();                                               // every wave is done with the last stage
    {
        const int t = tid & 127;
        const bool is_col = tid >= 128;
        int64_t p;
        int ordinary;
        if (RECT && is_col) {
            const int64_t hp = cpool[n0 + t];
            ordinary = hp >= 0 ? 1 : 0;
            p = ordinary ? hp : 0;
        } else {
            const int64_t gi = (!RECT && is_col) ? g.ncol0 + n0 + t : m0 + t;
            const bool valid = gi < g.M;
            p = valid ? g.cidx[gi] : 0;
            ordinary = (valid && g.ckind[gi] < 0) ? 1 : 0;
        }
        (is_col ? pc : pr)[t] = p;
        if constexpr (WEIGHTED) {
            if (is_col) wcol[t] = ordinary ? g.tw[p] : (T)0;
            else kr[t] = ordinary;
        } else {
            (is_col ? mc : kr)[t] = ordinary;
        }
        if (!g.Cp) {
            T* x = (is_col ? xc : xr) + t * MAXD;
#pragma unroll
            for (int d = 0; d < MAXD; ++d) x[d] = d < g.DP ? g.Xs[p * g.DP + d] : (T)0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wr * 64 + i * 16 + F::row_of(lane, r);
            const int64_t prow = pr[row];
            const T kap = kr[row] ? (T)1 : (T)0;
            T xrow[MAXD];
#pragma unroll
            for (int d = 0; d < MAXD; ++d) xrow[d] = xr[row * MAXD + d];
            T s2 = (T)0;
            if constexpr (WEIGHTED) {
                T es[4], we[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = wc * 64 + j * 16 + fr;
                    const int64_t pcol = pc[col];
                    const T cv = vr_pool_cov<T>(g, prow, pcol, xrow, xc + col * MAXD);
                    const T wgt = wcol[col];
                    const T e = kap * cv - acc[i][j][r];
                    es[j] = wgt != (T)0 ? e : (T)0;
                    we[j] = wgt * es[j];
                }
                // sum_j (omega_j e_j) e_j, written out: the second square rounded on its own, the first added to it by one fma,
                // then one fma per column -- what the compiler makes of the unweighted `s2 += e * e` below, so that all-ones
                // weights leave the unweighted bits (omega e is then e itself; omega (e e) would round every square first)
                s2 = kfma(we[0], es[0], we[1] * es[1]);
                s2 = kfma(we[2], es[2], s2);
                s2 = kfma(we[3], es[3], s2);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = wc * 64 + j * 16 + fr;
                    const int64_t pcol = pc[col];
                    const T cv = vr_pool_cov<T>(g, prow, pcol, xrow, xc + col * MAXD);
                    T e = kap * cv - acc[i][j][r];
                    e = mc[col] ? e : (T)0;
                    s2 += e * e;
                }
            }
            s2 = row16_sum<T>(s2);
            if (fr == 0) red[wc * 128 + row] = s2;
        }
    __syncthreads();
    if (tid < 128) g.stat_out[(int64_t)bn * g.stat_ld + m0 + tid] = red[tid] + red[128 + tid];
}

// ---------------------------------------------------------------------------------------------
// Variance reduction of whole paths (api_paths_vr.hip): A = R_U, the rows of V^T of the union U of the paths' sites (a site
// with a train row already: its second-row form), B = rows [ncol0, ncol0 + n) of V^T.  The accumulators hold R_u . V_j; the
// epilogue forms the cross covariance E_uj = C(u, j) - R_u . V_j in registers -- the kernel term as in vr_epilogue, but always
// present on the row side and with the row's pool index from uidx -- zeroes the columns that are not targets (unit rows,
// padding) and the padding rows behind U, scales column j by sqrt(omega_j) (tw as above: Phi = E Omega E^T), and WRITES the
// tile: E[row][n0 + col], the launch's columns only (Phi = E E^T is the caller's next product).  No kernel-matrix block is
// written.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct PvrGemmArgs : VrGemmArgs<T> {
    const int64_t* uidx;           // pool index of every union row (U entries)
    int64_t U;                     // rows beyond U are padding
    T* E;                          // mpad x n
    int64_t lde;
};

template <typename T, typename G, typename ACC>
__device__ __forceinline__ void pvr_epilogue(const G& g, char* smem, const ACC (&acc)[4][4], int64_t m0, int64_t n0, int wr,
                                             int wc, int lane, int tid) {
    using F = MF<T>;
    const int fr = lane & 15;
    // LDS: coordinates of the rows, of the columns ([128][MAXD], zero padded) | pool indices of the rows, of the columns |
    // which rows are union sites | sqrt of the target weight of the columns (0: not a target): 16 KB + 2 KB + 512 B + 128 T
    // <= 19.5 KB of the main loop's 64 KB of stages; the weights start 8-byte aligned.
    T* xr = reinterpret_cast<T*>(smem);
    T* xc = reinterpret_cast<T*>(smem + 8192);
    int64_t* pr = reinterpret_cast<int64_t*>(smem + 16384);
    int64_t* pc = pr + 128;
    int* kr = reinterpret_cast<int*>(pc + 128);
    T* wcol = reinterpret_cast<T*>(kr + 128);
    __syncthreads();                                               // every wave is done with the last stage
    {
        const int t = tid & 127;
        const bool is_col = tid >= 128;
        const int64_t gi = is_col ? g.ncol0 + n0 + t : m0 + t;
        const bool valid = is_col ? gi < g.M : gi < g.U;
        const int64_t p = valid ? (is_col ? g.cidx[gi] : g.uidx[gi]) : 0;
        (is_col ? pc : pr)[t] = p;
        if (is_col) wcol[t] = (valid && g.ckind[gi] < 0) ? (g.tw ? sqrt(g.tw[p]) : (T)1) : (T)0;
        else kr[t] = valid ? 1 : 0;
        if (!g.Cp) {
            T* x = (is_col ? xc : xr) + t * MAXD;
#pragma unroll
            for (int d = 0; d < MAXD; ++d) x[d] = d < g.DP ? g.Xs[p * g.DP + d] : (T)0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wr * 64 + i * 16 + F::row_of(lane, r);
            const int64_t prow = pr[row];
            const bool rowon = kr[row] != 0;
            T xrow[MAXD];
#pragma unroll
            for (int d = 0; d < MAXD; ++d) xrow[d] = xr[row * MAXD + d];
            T* Er = g.E + (m0 + row) * g.lde + n0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = wc * 64 + j * 16 + fr;
                const int64_t pcol = pc[col];
                const T cv = vr_pool_cov<T>(g, prow, pcol, xrow, xc + col * MAXD);
                const T sw = wcol[col];
                Er[col] = (rowon && sw != (T)0) ? sw * (cv - acc[i][j][r]) : (T)0;
                // the additive form evaluates two kernels per entry: one column after the other, or the scheduler overlaps the
                // four and the fp64 kernel no longer fits its registers beside the accumulators (the single forms: as before)
                if constexpr (is_additive<G>::value || is_rel<G>::value || is_sep<G>::value) __builtin_amdgcn_sched_barrier(0);
            }
        }
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA staging with FOUR stages of 64-byte rows (4 x 16 KB, two workgroups per CU) and hand-placed waits, so
// that the loads of THREE k-tiles (8 f64 / 16 f32 wide each) are in flight while one is multiplied.  Per k-tile and wave: s_waitcnt vmcnt(8) (own DMA of this tile landed, two
// younger tiles may still fly), s_barrier (everybody's DMA landed, everybody is done reading the stage
// that is refilled next), 4 global_load_lds for tile kt+3, then 8 ds_read_b128 + 32 MFMAs.
// LDS image per operand and stage: [128 rows][4 chunks of 16 B], chunk index XOR ((row>>2)&2).  A ds_read_b128 is served
// in four groups of 16 lanes -- {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32 (MI355X_MICROARCH.md, LDS), NOT the
// four quarter-waves -- and a group is one LDS cycle when its lanes touch 16 distinct 16-byte slots of the 256-byte bank
// row: with lane = row fr + 16 * chunk fg that holds for this XOR (tools/pmc_lds.sh: SQ_LDS_BANK_CONFLICT 0).  Rounds 1-4
// XORed with (row>>2)&3, conflict-free for quarter-waves and two-way for the real groups: half of all LDS-array cycles were
// conflict cycles (2.4e10 of 4.8e10 in the bench run) -- at no measurable cost in time (164.8-165.2 vs 165.2 ms per step, A/B on
// one box): the LDS array is busy for a tenth of the kernel either way.
// ---------------------------------------------------------------------------------------------
// (-DALGP_GEMM_XOR_MASK=3 builds the image of rounds 1-4, for the traffic A/B of round 6: tools/xor_traffic_ab.sh measured
// 0.93 GB of fabric reads per launch with it against 1.16 GB with this one at the same request count -- 18 % fewer L2
// misses -- and the same time; profiles/r06_xor_traffic_ab.txt)
#ifndef ALGP_GEMM_XOR_MASK
#define ALGP_GEMM_XOR_MASK 2
#endif
// Args = VrGemmArgs<T> / VrWGemmArgs<T>: the variance-reduction epilogue above instead of a D tile (STATS is then false); Args =
// PvrGemmArgs<T>: the path form's epilogue, which writes the E tile.
//
// SCHED: the scheduled sibling for the candidate sweep's products.  A grid of G = min(tiles, 2 x CUs) workgroups, each
// walking its fixed list of units (gemm_sched.h: whole tiles, or one k slice of a leftover tile whose alpha * acc goes to a
// partials scratch for gemm_finish_kernel).  Same stages, k order, fragment layout and epilogues, so a whole tile has the
// bits of the plain kernel's.  Between two units the first NST - 1 k-tiles of the NEXT unit are issued before the epilogue
// of the current one (the LDS-DMA needs no registers): they go to the stages that follow the last one read, which no wave
// can still be reading (every wave passed the last k-tile's barrier), so the stage rotation simply continues.  Wait
// accounting: arrive()'s vmcnt(8/4/0) counts stage DMAs only, and in the epilogue the C loads and D stores fly with the
// prefetched stages -- so the epilogue ends with an honest vmcnt(0), which covers the prefetched stages too, and the next
// unit's loop starts from a clean counter exactly like a fresh workgroup whose prologue has landed.  The STATS epilogue's
// `red` scratch has 4 KB of its own behind the stages (68 KB per workgroup, two per CU).  Workgroups never wait for,
// signal or poll each other: partial sums meet only in the finish kernel, a later launch on the same stream.
//
// Args = GenGemmArgs<T, DP> (SCHED only): the update product whose C tile is generated instead of loaded.  Per unit, thread t
// holds one entry of the unit's 128 rows (t < 128: coordinates and kind) or 128 columns (coordinates) in registers, loaded
// BEFORE the unit's first stage DMAs are issued (older than all of them: arrive()'s counts stay exact, and the k loop hides the
// latency).  After the k loop they go to an LDS region of their own behind the stages (4.5 KB at DP = 2, fp64) -- before the next
// unit's entries are loaded and its stages prefetched --, then lgkmcnt(0) + s_barrier (not __syncthreads(): no wait for the
// prefetched stages), and the store loop forms alpha * acc + beta * bt_entry(...) with no C loads queued behind the prefetch.
// The region's last readers (the previous unit's epilogue) have since passed the barriers of a whole k loop.  k-slice units
// write alpha * acc to the partials scratch as before; gemm_finish_gen_kernel generates their C term.
template <typename T, bool STATS = false, typename Args = GemmArgs<T>, bool SCHED = false>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel_dma4(Args g) {
    constexpr int GDP = gen_dp<Args>::value;
    constexpr bool GEN = GDP > 0;
    constexpr bool VR = std::is_base_of<VrGemmArgs<T>, Args>::value;
    static_assert(!(VR && STATS), "one epilogue per kernel");
    static_assert(!(VR && SCHED), "the scheduled form serves the sweep's products only");
    static_assert(!GEN || (SCHED && !STATS), "generated C tiles: the scheduled update product only");
    constexpr int NST = 4;
    using F = MF<T>;
    using acc_t = typename F::acc_t;
    using chunk_t = typename F::chunk_t;
    constexpr int EPC = F::EPC;
    constexpr int BK = 4 * EPC;                                    // elements per 64-byte row piece

    constexpr int GEN_LDS = GEN ? 2 * 128 * GDP * (int)sizeof(T) + 128 * (int)sizeof(int) : 0;
    __shared__ __attribute__((aligned(1024))) char smem[NST * 16384 + (SCHED && STATS ? 4096 : 0) + GEN_LDS];

    const int nwg = gridDim.x;
    int bm, bn;
    int kskip = 0;                                                 // 64-byte k-tiles this unit leaves out in front
    int nkt;                                                       // ... and walks
    int slice = -1, nunits = 1, ui = 0;
    if constexpr (SCHED) {
        nunits = sched_count<!GEN>(g.sch, blockIdx.x);
        const SchedUnit u = sched_unit<!GEN>(g.sch, blockIdx.x, 0);
        bm = u.tile / g.tiles_n;
        bn = u.tile - bm * g.tiles_n;
        kskip = u.kb0 * (128 / BK);
        nkt = (u.kb1 - u.kb0) * (128 / BK);
        slice = u.slice;
    } else {
    if (g.ktri) {
        // Tile row bm costs (bm + 1) tiles x K = k - 128 bm: a contiguous share of the tile list per XCD (below) would give the
        // XCD with the first rows several times the work of the last.  Instead XCD x takes the tile rows bm = x, x + 8, ...
        // (its rows' tiles share the row panel of X through its L2), longest K first; the grid holds 8 x the largest share
        // and the surplus workgroups of the other XCDs leave at once.
        int local = blockIdx.x >> 3;
        bm = blockIdx.x & 7;
        while (bm < g.tiles_m && local > bm) { local -= bm + 1; bm += 8; }
        if (bm >= g.tiles_m) return;
        bn = local;
    } else {
        int sid;
        {
            const int id = blockIdx.x, xcd = id & 7, q = nwg >> 3, r = nwg & 7;
            sid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
        }
        if (g.lower_only) {
            bm = (int)((sqrt(8.0 * (double)sid + 1.0) - 1.0) * 0.5);
            while ((int64_t)(bm + 1) * (bm + 2) / 2 <= sid) ++bm;
            while ((int64_t)bm * (bm + 1) / 2 > sid) --bm;
            bn = sid - (int)((int64_t)bm * (bm + 1) / 2);
        } else {
            bm = sid / g.tiles_n;
            bn = sid - bm * g.tiles_n;
        }
    }
    kskip = g.ktri ? bm * (128 / BK) : 0;
    nkt = g.ktiles * 2 - kskip;                                    // g.ktiles counts 128-byte tiles
    if (g.kcut && (bn + 1) * (128 / BK) < nkt) nkt = (bn + 1) * (128 / BK);
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t bz = blockIdx.y;

    // ---- DMA: wave w stages rows [32w, 32w+32) of each operand as two 16-row groups; lane l -> row l>>2 of
    // the group, LDS slot l&3, which must hold chunk (l&3) ^ ((row>>2)&2) = (l&3) ^ ((l>>4)&2)
    const int srow = lane >> 2;
    const int schunk = (lane & 3) ^ ((lane >> 4) & ALGP_GEMM_XOR_MASK);
    const T* Ag = g.A + bz * g.sA + ((int64_t)bm * 128 + 32 * wave + srow) * g.lda + schunk * EPC + (int64_t)kskip * BK;
    const T* Bg = g.B + bz * g.sB + ((int64_t)bn * 128 + 32 * wave + srow) * g.ldb + schunk * EPC + (int64_t)kskip * BK;
    auto stage = [&](int st, int kt) {
        char* As = smem + st * 16384 + wave * 2048;
        char* Bs = As + 8192;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_global_load_lds((glb_vp)(Ag + (int64_t)(16 * i) * g.lda + (int64_t)kt * BK),
                                             (lds_vp)(As + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((glb_vp)(Bg + (int64_t)(16 * i) * g.ldb + (int64_t)kt * BK),
                                             (lds_vp)(Bs + i * 1024), 16, 0, 0);
        }
    };

    // ---- fragment reads: row = w*64 + t*16 + (lane&15), chunk (lane>>4) ^ ((row>>2)&2) ----
    const int fr = lane & 15, fg = lane >> 4;
    const int coff = ((fg ^ ((fr >> 2) & ALGP_GEMM_XOR_MASK)) << 4);   // (row>>2)&2 == (fr>>2)&2: the row offsets are multiples of 16
    const int aoff = (wr * 64 + fr) * 64 + coff;
    const int boff = (wc * 64 + fr) * 64 + coff;

    acc_t acc[4][4];
    // GEN: this thread's entry of the unit's rows (waves 0, 1) or columns (waves 2, 3), ahead of the unit's first stage DMAs
    typedef T gen_vec_t __attribute__((ext_vector_type(GEN ? GDP : 1)));
    gen_vec_t gx;
    int gk = -1;
    auto gen_load = [&](int ubm, int ubn) {
        if constexpr (GEN) {
            // (no branches: a k-slice unit loads its entries too, and the column waves a row kind, both unused -- loads under
            // a condition made the compiler wait for them on the spot, in front of the stage prefetch)
            int t = tid & 127;
            asm volatile("" : "+v"(t));                            // (not hoisted out of the unit loop: see the epilogue)
            const int64_t row = (int64_t)ubm * 128 + t;
            const T* src = wave >= 2 ? g.cx + (g.col0 + (int64_t)ubn * 128 + t) * GDP : g.rx + row * GDP;
            gx = *reinterpret_cast<const gen_vec_t*>(src);
            gk = g.rk[row];
            asm volatile("" ::: "memory");
        }
    };
    gen_load(bm, bn);
    // prologue: tiles 0 .. NST-2 in flight
#pragma unroll
    for (int t = 0; t < NST - 1; ++t)
        if (t < nkt) stage(t, t);

    auto fread = [&](int st, chunk_t (&a)[4], chunk_t (&b)[4]) {
        const char* As = smem + st * 16384;
        const char* Bs = As + 8192;
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = *reinterpret_cast<const chunk_t*>(As + aoff + t * 1024);
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = *reinterpret_cast<const chunk_t*>(Bs + boff + t * 1024);
    };
    // column by column: the first four MFMAs need a[0..3] and b[0] only, the rest of b lands under them
    auto fmac = [&](const chunk_t (&a)[4], const chunk_t (&b)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < EPC; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][j] = F::mfma(a[i][e], b[j][e], acc[i][j]);
    };
    // wait until this wave's DMA of a tile has landed while `younger` (0..2) later tiles may still fly, then meet
    auto arrive = [&](int younger) {
        if (younger >= 2) __builtin_amdgcn_s_waitcnt(0x0F78);                   // vmcnt(8)
        else if (younger >= 1) __builtin_amdgcn_s_waitcnt(0x0F74);              // vmcnt(4)
        else __builtin_amdgcn_s_waitcnt(0x0F70);                                // vmcnt(0)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    int st = 0;                                                    // stage of tile kt; tile kt+NST-1 goes to st-1 (mod NST)
    for (;;) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = (T)0;
    for (int kt = 0; kt < nkt; ++kt) {
        arrive(nkt - 1 - kt);
        chunk_t a[4], b[4];
        fread(st, a, b);
        if (kt + NST - 1 < nkt) stage(st == 0 ? NST - 1 : st - 1, kt + NST - 1);   // the stage read in iteration kt-1
        fmac(a, b);
        st = (st + 1 == NST) ? 0 : st + 1;
    }
    const int64_t m0 = (int64_t)bm * 128, n0 = (int64_t)bn * 128;   // the unit whose accumulators are going out
    const int cur_bn = bn, cur_slice = slice;
    if constexpr (GEN) {
        // this unit's row and column entries into their LDS region (its last readers are a whole k loop behind), before the
        // registers take the next unit's
        if (cur_slice < 0) {
            T* xr = reinterpret_cast<T*>(smem + NST * 16384);
            T* xc = xr + 128 * GDP;
            int* kr = reinterpret_cast<int*>(xc + 128 * GDP);
            int t = tid & 127;
            asm volatile("" : "+v"(t));
            *reinterpret_cast<gen_vec_t*>((wave >= 2 ? xc : xr) + t * GDP) = gx;
            if (wave < 2) kr[t] = gk;
        }
        asm volatile("" ::: "memory");
    }
    if constexpr (SCHED) {
        // the next unit's first NST - 1 k-tiles, into the stages after the one read last (a unit has at least 128 / BK >= 8)
        if (++ui < nunits) {
            const SchedUnit u = sched_unit<!GEN>(g.sch, blockIdx.x, ui);
            bm = u.tile / g.tiles_n;
            bn = u.tile - bm * g.tiles_n;
            nkt = (u.kb1 - u.kb0) * (128 / BK);
            slice = u.slice;
            gen_load(bm, bn);
            Ag = g.A + ((int64_t)bm * 128 + 32 * wave + srow) * g.lda + schunk * EPC + (int64_t)u.kb0 * 128;
            Bg = g.B + ((int64_t)bn * 128 + 32 * wave + srow) * g.ldb + schunk * EPC + (int64_t)u.kb0 * 128;
#pragma unroll
            for (int t = 0; t < NST - 1; ++t) stage((st + t) & (NST - 1), t);
        }
    }

    if constexpr (std::is_base_of<PvrGemmArgs<T>, Args>::value) {
        pvr_epilogue<T>(g, smem, acc, m0, n0, wr, wc, lane, tid);
        return;
    } else if constexpr (VR) {
        constexpr bool WEIGHTED = std::is_base_of<VrWGemmArgs<T>, Args>::value || std::is_base_of<VrxWGemmArgs<T>, Args>::value;
        if constexpr (std::is_base_of<VrxGemmArgs<T>, Args>::value)
            vr_epilogue<T, WEIGHTED, true>(g, smem, acc, m0, n0, (int)bz * g.tiles_n + cur_bn, wr, wc, lane, tid,
                                           reinterpret_cast<const int64_t*>(reinterpret_cast<const char*>(g.cpool) +
                                                                            bz * g.sB * (int64_t)sizeof(T)));
        else
            vr_epilogue<T, WEIGHTED, false>(g, smem, acc, m0, n0, cur_bn, wr, wc, lane, tid);
        return;
    }
    const T alpha = g.alpha, beta = g.beta;
    const T* Cb = g.C + bz * g.sC;
    T* Db = g.D + bz * g.sD;
    if (SCHED && !STATS && cur_slice >= 0) {
        // a k slice of a leftover tile: alpha * acc to the partials scratch, gemm_finish_kernel adds C and the other slices
        T* P = g.part + (int64_t)cur_slice * (128 * 128);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 64 + i * 16 + F::row_of(lane, r);
#pragma unroll
                for (int j = 0; j < 4; ++j) P[row * 128 + wc * 64 + j * 16 + fr] = alpha * acc[i][j][r];
            }
    } else if constexpr (GEN) {
        // the C tile from the staged coordinates: own LDS writes done, then meet (no wait for the prefetched stages)
        const T* xr = reinterpret_cast<const T*>(smem + NST * 16384);
        const T* xc = xr + 128 * GDP;
        const int* kr = reinterpret_cast<const int*>(xc + 128 * GDP);
        __builtin_amdgcn_s_waitcnt(0xC07F);                        // lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // (the lane index through an opaque move: the per-lane row and column offsets below are the same in every unit, and
        // hoisted out of the unit loop they would live across the k loop -- 268 bytes of scratch per lane)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int gfr = ln & 15;
        T xcol[4][GDP];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int d = 0; d < GDP; ++d) xcol[j][d] = xc[(wc * 64 + j * 16 + gfr) * GDP + d];
        const int64_t gc = g.col0 + n0 + wc * 64 + gfr;            // global column of this lane's column j = 0; + 16 j
        const T os = g.os;
        const int64_t ncols = g.ncols;
        // one copy of the loop per kernel form of this instantiation's family: the form is uniform, and as a run-time argument of
        // kval every form's arithmetic (a square root per value) would be done and selected
        auto tile_out = [&](auto kform) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = wr * 64 + i * 16 + F::row_of(ln, r);
                    T xrow[GDP];
#pragma unroll
                    for (int d = 0; d < GDP; ++d) xrow[d] = xr[row * GDP + d];
                    const int kind = kr[row];
                    T* Dr = Db + (m0 + row) * g.ldd + n0 + wc * 64 + gfr;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const T cv = bt_entry<T, GDP>(decltype(kform)::value, os, xrow, xcol[j], kind, gc + 16 * j, ncols);
                        Dr[j * 16] = alpha * acc[i][j][r] + beta * cv;
                        // two kernel values at a time: interleaved further, their exp polynomials cost registers the k loop needs
                        if (j & 1) __builtin_amdgcn_sched_barrier(0);
                    }
                }
        };
        if constexpr (Args::FAM == 0) {
            if (g.kernel == ALGP_KERNEL_RBF) tile_out(std::integral_constant<int, ALGP_KERNEL_RBF>{});
            else tile_out(std::integral_constant<int, ALGP_KERNEL_MATERN15>{});
        } else {
            if (g.kernel == ALGP_KERNEL_MATERN05) tile_out(std::integral_constant<int, ALGP_KERNEL_MATERN05>{});
            else tile_out(std::integral_constant<int, ALGP_KERNEL_MATERN25>{});
        }
    } else if (beta != (T)0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            T cv[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gi = m0 + wr * 64 + i * 16 + F::row_of(lane, r);
#pragma unroll
                for (int j = 0; j < 4; ++j) cv[r][j] = Cb[gi * g.ldc + n0 + wc * 64 + j * 16 + fr];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gi = m0 + wr * 64 + i * 16 + F::row_of(lane, r);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    Db[gi * g.ldd + n0 + wc * 64 + j * 16 + fr] = alpha * acc[i][j][r] + beta * cv[r][j];
            }
        }
    } else if (!STATS) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gi = m0 + wr * 64 + i * 16 + F::row_of(lane, r);
#pragma unroll
                for (int j = 0; j < 4; ++j) Db[gi * g.ldd + n0 + wc * 64 + j * 16 + fr] = alpha * acc[i][j][r];
            }
    } else {
        // The tile goes out and, with it, its row statistics (the candidate solve's variance and mean, reference
        // utils.py:301-304: a second pass over V^T otherwise -- 8 GB at config 4).  A lane holds, of each of its 16 rows, the
        // four columns fr + 16 j of this wave's half: sum them, fold the 16 lanes of a row (DPP rotations inside the
        // 16-lane group), add the two column halves through LDS (free now), one store per row and statistic.  Fixed order:
        // the same bits in every run.  (Row by row, stores and sums together: kept for a second loop the 64 products
        // alpha * acc cost 20 spilled VGPRs.)
        T wv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wv[j] = g.stat_w[n0 + wc * 64 + j * 16 + fr];
        // [column half][row][2]; SCHED: behind the stages, which the next unit's k-tiles are landing in -- the last reader
        // of the previous unit's sums has since passed the barriers of a whole k loop
        T* red = reinterpret_cast<T*>(smem + (SCHED ? NST * 16384 : 0));
        if constexpr (!SCHED) __syncthreads();                     // every wave is done with the last stage
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr * 64 + i * 16 + F::row_of(lane, r);
                T s2 = (T)0, sw = (T)0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const T d = alpha * acc[i][j][r];
                    Db[(m0 + row) * g.ldd + n0 + wc * 64 + j * 16 + fr] = d;
                    s2 += d * d;
                    sw += d * wv[j];
                }
                s2 = row16_sum<T>(s2);
                sw = row16_sum<T>(sw);
                if (fr == 0) {
                    red[(wc * 128 + row) * 2 + 0] = s2;
                    red[(wc * 128 + row) * 2 + 1] = sw;
                }
            }
        if constexpr (SCHED) {
            // own LDS writes done, then meet: a __syncthreads() would also wait for the prefetched stages (vmcnt)
            __builtin_amdgcn_s_waitcnt(0xC07F);                    // lgkmcnt(0)
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        } else {
            __syncthreads();
        }
        const int row = tid >> 1, q = tid & 1;
        g.stat_out[(int64_t)(2 * cur_bn + q) * g.stat_ld + m0 + row] = red[row * 2 + q] + red[(128 + row) * 2 + q];
    }
    if constexpr (!SCHED) return;
    if (ui >= nunits) return;
    // every load and store of this epilogue and the next unit's prefetched k-tiles: the k loop's counted waits start clean
    __builtin_amdgcn_s_waitcnt(0x0F70);                            // vmcnt(0)
    }
}

// D = beta C + the partial sums of a scheduled launch's leftover tiles, slice by slice in ascending k: a fixed order, the
// same bits in every run.  A memory-bound pass, shaped for the memory system: FIN_STRIPS workgroups per leftover tile (tile
// tile0 + blockIdx.x / FIN_STRIPS of the row-major list), each a strip of 128 / FIN_STRIPS = 8 rows -- 56 leftover tiles are 896
// workgroups, where one workgroup per tile left four CUs in five idle.  A thread owns PPT 16-byte pieces (two fp64 / four fp32
// adjacent columns; a wave reads 1 KB of a row at a time), in the same columns of rows RSTEP apart, and loads the slices in
// batches of FIN_BATCH before the first add of a batch: FIN_BATCH * PPT independent 16-byte loads in flight per thread, where
// the element-by-element loop waited for every 8 bytes.  Per element the arithmetic is what it always was: v = beta * c
// rounded on its own (contraction is off in these kernels: unrolled, the compiler would make one fma of the multiplication and
// the first add, which rounds once where the loop rounded twice), then v += P[q] in ascending q, one add per slice.
constexpr int FIN_STRIPS = 16;
constexpr int FIN_BATCH = 8;
template <typename T>
struct Fin {
    static constexpr int EPV = 16 / (int)sizeof(T);                        // elements of a piece
    static constexpr int RPW = 256 * EPV / 128;                            // rows that the 256 threads cover at a time: 4 / 8
    static constexpr int PPT = (128 / FIN_STRIPS) / RPW;                   // pieces of a thread: 2 / 1
    static constexpr int RSTEP = RPW;
    typedef T V __attribute__((ext_vector_type(EPV)));
    static_assert(PPT >= 1 && PPT * RPW * FIN_STRIPS == 128, "a strip is whole passes of the workgroup");
};

// v[i] += the pieces of slices 0 .. NB - 1 at P (uniform: the first of them) + off (the thread's first piece), ascending: every
// load of the batch is issued before its first add (left alone, the scheduler interleaves them to save registers)
template <typename T, int NB>
__device__ __forceinline__ void finish_add(const T* P, unsigned off, typename Fin<T>::V (&v)[Fin<T>::PPT]) {
#pragma clang fp contract(off)
    using F = Fin<T>;
    typename F::V p[NB][F::PPT];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < F::PPT; ++i)
            p[b][i] = *reinterpret_cast<const typename F::V*>(P + b * (128 * 128) + (off + i * F::RSTEP * 128));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < F::PPT; ++i) v[i] += p[b][i];
}

// all S slices: whole batches, then the remainder as batches of 4, 2 and 1 (still ascending)
template <typename T>
__device__ __forceinline__ void finish_sum(const T* P, unsigned off, int S, typename Fin<T>::V (&v)[Fin<T>::PPT]) {
    int q = 0;
    for (; q + FIN_BATCH <= S; q += FIN_BATCH) finish_add<T, FIN_BATCH>(P + (int64_t)q * (128 * 128), off, v);
    static_assert(FIN_BATCH == 8, "the remainder below is 4 + 2 + 1");
    if ((S - q) & 4) { finish_add<T, 4>(P + (int64_t)q * (128 * 128), off, v); q += 4; }
    if ((S - q) & 2) { finish_add<T, 2>(P + (int64_t)q * (128 * 128), off, v); q += 2; }
    if ((S - q) & 1) finish_add<T, 1>(P + (int64_t)q * (128 * 128), off, v);
}

template <typename T>
__global__ __launch_bounds__(256) void gemm_finish_kernel(const T* part, int S, int tile0, int tiles_n, T beta, const T* C, int64_t ldc,
                                                          T* D, int64_t ldd) {
#pragma clang fp contract(off)
    using F = Fin<T>;
    using V = typename F::V;
    const int j = blockIdx.x / FIN_STRIPS, strip = blockIdx.x - j * FIN_STRIPS;
    const int tile = tile0 + j, bm = tile / tiles_n, bn = tile - bm * tiles_n;
    const int lrow = strip * (128 / FIN_STRIPS) + (int)threadIdx.x / (128 / F::EPV), lcol = ((int)threadIdx.x % (128 / F::EPV)) * F::EPV;
    const int64_t row = (int64_t)bm * 128 + lrow, col = (int64_t)bn * 128 + lcol;
    V v[F::PPT];
#pragma unroll
    for (int i = 0; i < F::PPT; ++i) v[i] = beta * *reinterpret_cast<const V*>(C + (row + i * F::RSTEP) * ldc + col);
    finish_sum<T>(part + (int64_t)j * S * (128 * 128), (unsigned)(lrow * 128 + lcol), S, v);
#pragma unroll
    for (int i = 0; i < F::PPT; ++i) *reinterpret_cast<V*>(D + (row + i * F::RSTEP) * ldd + col) = v[i];
}

// The same with the C term generated (GenGemmArgs): the leftover tiles of a scheduled update product with fused right-hand sides.
// The coordinates of a thread's columns are loaded once, the coordinates and the kind of a row once per piece; one copy of the C
// term per kernel form of the family FAM, as in the product's epilogue.
template <typename T, int DP, int FAM>
__global__ __launch_bounds__(256) void gemm_finish_gen_kernel(const T* part, int S, int tile0, int tiles_n, T beta, const T* rx, const T* cx,
                                                              const int* rk, int64_t col0, int64_t ncols, int kernel, T os, T* D, int64_t ldd) {
#pragma clang fp contract(off)
    using F = Fin<T>;
    using V = typename F::V;
    const int j = blockIdx.x / FIN_STRIPS, strip = blockIdx.x - j * FIN_STRIPS;
    const int tile = tile0 + j, bm = tile / tiles_n, bn = tile - bm * tiles_n;
    const int lrow = strip * (128 / FIN_STRIPS) + (int)threadIdx.x / (128 / F::EPV), lcol = ((int)threadIdx.x % (128 / F::EPV)) * F::EPV;
    const int64_t row = (int64_t)bm * 128 + lrow, col = (int64_t)bn * 128 + lcol;
    T xcol[F::EPV][DP];
#pragma unroll
    for (int e = 0; e < F::EPV; ++e)
#pragma unroll
        for (int d = 0; d < DP; ++d) xcol[e][d] = cx[(col0 + col + e) * DP + d];
    T xrow[F::PPT][DP];
    int kind[F::PPT];
#pragma unroll
    for (int i = 0; i < F::PPT; ++i) {
#pragma unroll
        for (int d = 0; d < DP; ++d) xrow[i][d] = rx[(row + i * F::RSTEP) * DP + d];
        kind[i] = rk[row + i * F::RSTEP];
    }
    V v[F::PPT];
    auto c_term = [&](auto kform) {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < F::PPT; ++i) {
            V cv;
#pragma unroll
            for (int e = 0; e < F::EPV; ++e)
                cv[e] = bt_entry<T, DP>(decltype(kform)::value, os, xrow[i], xcol[e], kind[i], col0 + col + e, ncols);
            v[i] = beta * cv;
        }
    };
    if constexpr (FAM == 0) {
        if (kernel == ALGP_KERNEL_RBF) c_term(std::integral_constant<int, ALGP_KERNEL_RBF>{});
        else c_term(std::integral_constant<int, ALGP_KERNEL_MATERN15>{});
    } else {
        if (kernel == ALGP_KERNEL_MATERN05) c_term(std::integral_constant<int, ALGP_KERNEL_MATERN05>{});
        else c_term(std::integral_constant<int, ALGP_KERNEL_MATERN25>{});
    }
    finish_sum<T>(part + (int64_t)j * S * (128 * 128), (unsigned)(lrow * 128 + lcol), S, v);
#pragma unroll
    for (int i = 0; i < F::PPT; ++i) *reinterpret_cast<V*>(D + (row + i * F::RSTEP) * ldd + col) = v[i];
}

// $ALGP_LAUNCH_LOG=<file>: one line per launch of gemm_nt_kernel_dma4 (any instantiation), in enqueue order (class m n k
// lower_only batch ktri element-size kcut): joined with a rocprofv3 kernel trace by dispatch order, it gives the trace the K
// its grid sizes do not show (tools/trace_shapes.py)
static void launch_log_line(int klass, int64_t m, int64_t n, int64_t k, int lower_only, int batch, int ktri, int es, int kcut) {
    static FILE* launch_log = getenv("ALGP_LAUNCH_LOG") ? fopen(getenv("ALGP_LAUNCH_LOG"), "w") : nullptr;
    if (!launch_log) return;
    fprintf(launch_log, "%d %lld %lld %lld %d %d %d %d %d\n", klass, (long long)m, (long long)n, (long long)k, lower_only, batch, ktri, es, kcut);
    fflush(launch_log);
}

// ---- the launch side: every form of gemm_nt_kernel_dma4 goes the same way ------------------------------------------------
// Its launcher describes the product as a GemmNt (common.h), makes the refusals that are its own, and then
//   gemm_check        refuses what no form can run (padding, k, leading dimensions, grid size) and counts the output tiles,
//   gemm_fill         sets the GemmArgs base of the form's argument struct from the description,
//   gemm_book         gives the launch's flop and byte figures and writes its line of the launch log,
//   dispatch          enqueues a kernel with its arguments on c->cur, timed where the profiler asks for events,
//   launch_scheduled  is the scheduled route with its finish launch (the loading and the generating form).
// A new form costs its own fields, its own checks and one dispatch line.
template <typename T>
static int gemm_check(algp_ctx* c, const char* who, const GemmNt<T>& p, int64_t* tiles) {
    if (p.m % 128 || p.n % 128 || p.k % 128 || p.k <= 0 || p.A.ld % 4 || p.B.ld % 4 || p.A.stride % 4 || p.B.stride % 4)
        return fail(c, ALGP_ERR_BAD_ARG, std::string(who) + ": operands must be padded to multiples of 128");
    const int64_t tm = p.m / 128, tn = p.n / 128;
    *tiles = p.lower_only ? tm * (tm + 1) / 2 : tm * tn;
    if (*tiles > 0x7fffffff) return fail(c, ALGP_ERR_BAD_ARG, std::string(who) + ": grid too large");
    return ALGP_OK;
}

template <typename T>
static void gemm_fill(GemmArgs<T>& g, const GemmNt<T>& p) {
    const bool inplace = !p.C.p;
    g.A = p.A.p; g.B = p.B.p; g.C = inplace ? p.D.p : p.C.p; g.D = p.D.p;
    g.lda = p.A.ld; g.ldb = p.B.ld; g.ldc = inplace ? p.D.ld : p.C.ld; g.ldd = p.D.ld;
    g.sA = p.A.stride; g.sB = p.B.stride; g.sC = inplace ? p.D.stride : p.C.stride; g.sD = p.D.stride;
    g.tiles_m = (int)(p.m / 128);
    g.tiles_n = (int)(p.n / 128);
    g.ktiles = (int)(p.k / (8 * MF<T>::EPC));
    g.alpha = p.alpha; g.beta = p.beta;
    g.lower_only = p.lower_only;
    g.ktri = p.ktri;
    g.kcut = p.kcut;
    g.stat_w = p.stat_w;
    g.stat_out = p.stat_out;
    g.stat_ld = p.stat_ld;
    g.sch = Sched();
    g.part = nullptr;
}

// Once per launch, behind its refusals: the figures the profile books, and the launch's line of the launch log (written here).
// tile_elems: what the form's epilogue moves per output tile -- a D tile or an E tile 128 x 128, D and C twice that, row sums
// only 128
struct Booking { double flops, bytes; };
template <typename T>
static Booking gemm_book(const GemmNt<T>& p, int64_t tiles, double tile_elems) {
    // ktri: tile row bm holds bm + 1 tiles of K = k - 128 bm: sum_bm (bm + 1)(tm - bm) = tm (tm + 1)(tm + 2) / 6 tile-steps of 128
    const double tm = (double)(p.m / 128), tn = (double)(p.n / 128);
    Booking b;
    b.flops = p.ktri ? 2.0 * 128.0 * 128.0 * 128.0 * tm * (tm + 1.0) * (tm + 2.0) / 6.0 * p.batch
              : p.kcut ? 2.0 * 128.0 * 128.0 * 128.0 * tm * tn * (tn + 1.0) / 2.0 * p.batch
                       : 2.0 * 128.0 * 128.0 * (double)p.k * (double)tiles * p.batch;
    b.bytes = sizeof(T) * p.batch * ((double)tiles * tile_elems + (double)p.k * 128.0 * (tm + tn));
    launch_log_line(p.klass, p.m, p.n, p.k, p.lower_only, p.batch, p.ktri, (int)sizeof(T), p.kcut);
    return b;
}

template <typename X>
struct as_is { typedef X type; };                                  // the arguments convert to the kernel's parameter types
template <typename... P>
static int dispatch(algp_ctx* c, int klass, double flops, double bytes, void (*kernel)(P...), dim3 grid, const typename as_is<P>::type&... args) {
    hipEvent_t ev_a, ev_b;
    if (prof_launch_events(c, klass, flops, bytes, &ev_a, &ev_b)) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, c->cur, ev_a, ev_b, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->cur, args...);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}

// The scheduled form (the candidate sweep's launches, potrf.hip): 2 x CUs resident workgroups walk the tile list; the leftover
// tiles of an update product are cut along k where the sweep has provided the partials scratch (row statistics and kcut rule
// that out), and `finish` (its arguments behind beta: tail) then sums the S slices onto beta C -- S + 2 tile passes where C is
// loaded, S + 1 where it is generated.
template <typename T, typename Args, typename... Tail>
static int launch_scheduled(algp_ctx* c, const char* who, const GemmNt<T>& p, const Booking& bk, Args& g, void (*product)(Args),
                            void (*finish)(const T*, int, int, int, T, Tail...), bool c_loaded, const typename as_is<Tail>::type&... tail) {
    const int slots = 2 * c->cu_count;
    const bool split = p.beta != (T)0 && !p.stat_out && !p.kcut && c->gemm_part.p &&
                       c->gemm_part.cap >= sizeof(T) * 128 * 128 * (size_t)slots;
    g.sch = sched_make(slots, g.tiles_m, g.tiles_n, (int)(p.k / 128), p.kcut, split ? 1 : 0);
    g.part = (T*)c->gemm_part.p;
    if (g.sch.S >= 2 && (g.ldd % 4 || ((uintptr_t)g.D & 15) || (c_loaded && (g.ldc % 4 || ((uintptr_t)g.C & 15)))))
        return fail(c, ALGP_ERR_BAD_ARG, std::string(who) + ": the finish kernel moves its tiles in 16-byte pieces");
    ALGP_TRY(dispatch(c, p.klass, bk.flops, bk.bytes, product, dim3((unsigned)g.sch.G), g));
    if (g.sch.S >= 2)
        ALGP_TRY(dispatch(c, p.klass, 0.0, sizeof(T) * 128.0 * 128.0 * (double)g.sch.left * (g.sch.S + (c_loaded ? 2.0 : 1.0)), finish,
                          dim3((unsigned)(g.sch.left * FIN_STRIPS)), g.part, g.sch.S, g.sch.full, g.tiles_n, g.beta, tail...));
    return ALGP_OK;
}

template <typename T>
int gemm_nt(algp_ctx* c, const GemmNt<T>& p) {
    if (p.m <= 0 || p.n <= 0 || p.batch <= 0) return ALGP_OK;
    if (p.stat_out && (p.beta != (T)0 || p.batch != 1 || p.lower_only || p.ktri))
        return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt: row statistics need beta = 0, no batch");
    if (p.kcut && (p.k != p.n || p.lower_only || p.ktri)) return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt: kcut needs k == n");
    int64_t tiles;
    ALGP_TRY(gemm_check(c, "gemm_nt", p, &tiles));
    if (p.lower_only && p.m != p.n) return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt: lower_only needs a square output");
    if (p.batch > 65535) return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt: batch too large");
    if (p.ktri && (!p.lower_only || p.k != p.m)) return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt: ktri needs a square lower-only product with k == m");
    GemmArgs<T> g;
    gemm_fill(g, p);
    const Booking bk = gemm_book(p, tiles, 128.0 * 128.0 * (p.beta != (T)0 ? 2.0 : 1.0));
    if (c->gemm_sched && c->cu_count > 0 && !p.lower_only && !p.ktri && p.batch == 1)
        return launch_scheduled(c, "gemm_nt", p, bk, g,
                                p.stat_out ? gemm_nt_kernel_dma4<T, true, GemmArgs<T>, true> : gemm_nt_kernel_dma4<T, false, GemmArgs<T>, true>,
                                gemm_finish_kernel<T>, true, g.C, g.ldc, g.D, g.ldd);
    int64_t gx = tiles;
    if (p.ktri) {                                                  // 8 x the largest per-XCD share (rows x, x + 8, ... of XCD x)
        int64_t most = 0;
        for (int x = 0; x < 8; ++x) {
            int64_t cnt = 0;
            for (int64_t r = x; r < g.tiles_m; r += 8) cnt += r + 1;
            most = std::max(most, cnt);
        }
        gx = 8 * most;
    }
    return dispatch(c, p.klass, bk.flops, bk.bytes, p.stat_out ? gemm_nt_kernel_dma4<T, true> : gemm_nt_kernel_dma4<T, false>,
                    dim3((unsigned)gx, (unsigned)p.batch), g);
}

bool rhs_gen_supported(int DP, bool pool_is_cov, bool additive) { return DP == 2 && !pool_is_cov && !additive; }

// The scheduled update product with its C tile generated (GEN above): booked like the loading form -- the same flop; the C
// tile's bytes are not read.
template <typename T>
int gemm_nt_launch_gen(algp_ctx* c, int klass, int64_t m, int64_t n, int64_t k, T alpha, const T* A, int64_t lda, const T* B,
                       int64_t ldb, T beta, const RhsGen& gen, int64_t col0, T* D, int64_t ldd) {
    if (m <= 0 || n <= 0) return ALGP_OK;
    if (!c->gemm_sched || c->cu_count <= 0 || !rhs_gen_supported(gen.DP, false) || !gen.rx || !gen.cx || !gen.rk)
        return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt_gen: the scheduled form with two gathered coordinates only");
    if (col0 < 0) return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt_gen: operands must be padded to multiples of 128");
    const GemmNt<T> p = {.klass = klass, .m = m, .n = n, .k = k, .alpha = alpha, .beta = beta, .A = {A, lda}, .B = {B, ldb}, .D = {D, ldd}};
    int64_t tiles;
    ALGP_TRY(gemm_check(c, "gemm_nt_gen", p, &tiles));
    auto launch = [&](auto fam) {
        constexpr int FAM = decltype(fam)::value;
        GenGemmArgs<T, 2, FAM> g;
        gemm_fill(g, p);                                           // (C, not read by this form, is D's pointer and strides)
        g.rx = (const T*)gen.rx; g.cx = (const T*)gen.cx; g.rk = gen.rk;
        g.col0 = col0; g.ncols = gen.ncols; g.kernel = gen.kernel; g.os = (T)gen.outputscale;
        return launch_scheduled(c, "gemm_nt_gen", p, gemm_book(p, tiles, 128.0 * 128.0), g,
                                gemm_nt_kernel_dma4<T, false, GenGemmArgs<T, 2, FAM>, true>, gemm_finish_gen_kernel<T, 2, FAM>, false, g.rx,
                                g.cx, g.rk, col0, g.ncols, g.kernel, g.os, D, ldd);
    };
    return kernel_family(gen.kernel) ? launch(std::integral_constant<int, 1>{}) : launch(std::integral_constant<int, 0>{});
}
ALGP_INSTANTIATE(gemm_nt_launch_gen);

// the fields the two variance-reduction forms share
template <typename T>
static void vr_fill(VrGemmArgs<T>& g, const KmatSrc& s, const int64_t* cidx, const int* ckind, int64_t M, int64_t ncol0, const T* tw) {
    g.cidx = cidx; g.ckind = ckind; g.M = M; g.ncol0 = ncol0; g.tw = tw;
    g.Xs = (const T*)s.Xs; g.Cp = (const T*)s.Cp; g.n_pool = s.n_pool; g.DP = s.DP; g.kernel = s.kernel;
    g.os = (T)s.outputscale; g.noise = (T)s.noise;
}

// the launch of one of the three forms below: the tile kernel for the argument struct as it is, or under the additive kernel for
// its additive form (AddGemmArgs) -- instantiations of their own
template <typename T, typename G>
static int vr_dispatch(algp_ctx* c, int klass, const Booking& bk, dim3 grid, const G& g, const KmatSrc& s) {
    if (s.sepf()) {
        SepGemmArgs<T, G> a;
        static_cast<G&>(a) = g;
        a.sep_G = (const T*)s.G; a.sep_Q = s.Q; a.sep_kb = s.kernel_b; a.sep_da = s.da; a.sep_dg = s.dg; a.sep_hasg = s.Q > 0 ? 1 : 0;
        a.sep_parts = 3; a.sep_osg = (T)s.outputscale_g;
        return dispatch(c, klass, bk.flops, bk.bytes, gemm_nt_kernel_dma4<T, false, SepGemmArgs<T, G>>, grid, a);
    }
    if (s.rel()) {
        RelGemmArgs<T, G> a;
        static_cast<G&>(a) = g;
        a.G = (const T*)s.G; a.Q = s.Q; a.da = s.da; a.parts = 3; a.os_g = (T)s.outputscale_g;
        return dispatch(c, klass, bk.flops, bk.bytes, gemm_nt_kernel_dma4<T, false, RelGemmArgs<T, G>>, grid, a);
    }
    if (!s.additive()) return dispatch(c, klass, bk.flops, bk.bytes, gemm_nt_kernel_dma4<T, false, G>, grid, g);
    AddGemmArgs<T, G> a;
    static_cast<G&>(a) = g;
    a.kernel_b = s.kernel_b; a.da = s.da; a.parts = 3; a.os_b = (T)s.outputscale_b;
    return dispatch(c, klass, bk.flops, bk.bytes, gemm_nt_kernel_dma4<T, false, AddGemmArgs<T, G>>, grid, a);
}

// The variance-reduction column sums of rows [0, mpad) of V^T against its rows [ncol0, ncol0 + n): per row and column
// tile bn of the launch, part[bn * part_ld + row] = sum over the tile's target columns j of (kappa_row C(row, j) - V_row . V_j)^2,
// the dot products over the first k columns, every column weighted by tw[its pool site] where tw is given.  Nothing else is
// written.
template <typename T>
int gemm_nt_launch_vr(algp_ctx* c, int klass, int64_t mpad, int64_t n, int64_t k, const T* Vt, int64_t ldv, int64_t ncol0,
                      const KmatSrc& s, const int64_t* cidx, const int* ckind, int64_t M, const T* tw, T* part, int64_t part_ld) {
    if (mpad <= 0 || n <= 0) return ALGP_OK;
    if (ncol0 % 128 || ncol0 + n > mpad || k > ldv || s.DP > MAXD)
        return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt_vr: operands must be padded to multiples of 128");
    const GemmNt<T> p = {.klass = klass, .m = mpad, .n = n, .k = k, .A = {Vt, ldv}, .B = {Vt + ncol0 * ldv, ldv}, .stat_out = part, .stat_ld = part_ld};
    int64_t tiles;
    ALGP_TRY(gemm_check(c, "gemm_nt_vr", p, &tiles));
    VrGemmArgs<T> g;
    gemm_fill(g, p);
    vr_fill(g, s, cidx, ckind, M, ncol0, tw);
    const Booking bk = gemm_book(p, tiles, 128.0);
    if (!tw) return vr_dispatch<T>(c, klass, bk, dim3((unsigned)tiles), g, s);
    VrWGemmArgs<T> gw;
    static_cast<VrGemmArgs<T>&>(gw) = g;
    return vr_dispatch<T>(c, klass, bk, dim3((unsigned)tiles), gw, s);
}
ALGP_INSTANTIATE(gemm_nt_launch_vr);

// The rectangular form: rows [0, mpad) of V^T (cidx / ckind / M describe them) against nslices blocks of n rows each, slice s at
// B + s * slice_bytes (leading dimension ldb) with its n pool indices at cpool + s * slice_bytes (negative: the column is no target);
// part[(s * n / 128 + bn) * part_ld + row] = the sum over the target columns j of slice s, tile bn, of
// (kappa_row C(row, j) - V_row . B_j)^2, weighted by tw[pool index of j] where tw is given.  One batched launch.
template <typename T>
int gemm_nt_launch_vrx(algp_ctx* c, int klass, int64_t mpad, int64_t n, int64_t k, const T* Vt, int64_t ldv, const T* B, int64_t ldb,
                       const int64_t* cpool, int nslices, int64_t slice_bytes, const KmatSrc& s, const int64_t* cidx, const int* ckind,
                       int64_t M, const T* tw, T* part, int64_t part_ld) {
    if (mpad <= 0 || n <= 0 || nslices <= 0) return ALGP_OK;
    if (k > ldv || k > ldb || s.DP > MAXD || !cpool || slice_bytes % 16 || ((uintptr_t)B & 15) || ((uintptr_t)cpool & 7) || nslices > 65535 ||
        (nslices > 1 && slice_bytes < (int64_t)sizeof(T) * n * ldb))
        return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt_vrx: operands must be padded to multiples of 128, the slices 16-byte aligned");
    const GemmNt<T> p = {.klass = klass, .m = mpad, .n = n, .k = k, .A = {Vt, ldv}, .B = {B, ldb, slice_bytes / (int64_t)sizeof(T)},
                         .batch = nslices, .stat_out = part, .stat_ld = part_ld};
    int64_t tiles;
    ALGP_TRY(gemm_check(c, "gemm_nt_vrx", p, &tiles));
    VrxGemmArgs<T> g;
    gemm_fill(g, p);
    vr_fill(g, s, cidx, ckind, M, 0, tw);
    g.cpool = cpool;
    const Booking bk = gemm_book(p, tiles, 128.0);
    const dim3 grid((unsigned)tiles, (unsigned)nslices);
    if (!tw) return vr_dispatch<T>(c, klass, bk, grid, g, s);
    VrxWGemmArgs<T> gw;
    static_cast<VrGemmArgs<T>&>(gw) = g;
    return vr_dispatch<T>(c, klass, bk, grid, gw, s);
}
ALGP_INSTANTIATE(gemm_nt_launch_vrx);

// The cross covariances of the union rows R (upad x k, the rows behind U zero) with rows [ncol0, ncol0 + n) of V^T:
// E[u][j] = C(uidx[u], cidx[ncol0 + j]) - R_u . V_(ncol0 + j) where column ncol0 + j is a target, 0 elsewhere and on the
// padding rows, times sqrt(tw[pool site of the column]) where tw is given; E is upad x n with leading dimension lde.
template <typename T>
int gemm_nt_launch_pvr(algp_ctx* c, int klass, int64_t upad, int64_t n, int64_t k, const T* R, int64_t ldr, const T* Vt, int64_t ldv,
                       int64_t ncol0, const KmatSrc& s, const int64_t* uidx, int64_t U, const int64_t* cidx, const int* ckind, int64_t M,
                       const T* tw, T* E, int64_t lde) {
    if (upad <= 0 || n <= 0) return ALGP_OK;
    if (ncol0 % 128 || ncol0 + n > (M + 127) / 128 * 128 || k > ldv || k > ldr || U > upad || lde < n || s.DP > MAXD)
        return fail(c, ALGP_ERR_BAD_ARG, "gemm_nt_pvr: operands must be padded to multiples of 128");
    const GemmNt<T> p = {.klass = klass, .m = upad, .n = n, .k = k, .A = {R, ldr}, .B = {Vt + ncol0 * ldv, ldv}};
    int64_t tiles;
    ALGP_TRY(gemm_check(c, "gemm_nt_pvr", p, &tiles));
    PvrGemmArgs<T> g;
    gemm_fill(g, p);
    vr_fill(g, s, cidx, ckind, M, ncol0, tw);
    g.uidx = uidx; g.U = U; g.E = E; g.lde = lde;
    const Booking bk = gemm_book(p, tiles, 128.0 * 128.0);
    return vr_dispatch<T>(c, klass, bk, dim3((unsigned)tiles), g, s);
}
ALGP_INSTANTIATE(gemm_nt_launch_pvr);

template <typename T>
int gemm_nt_launch(algp_ctx* c, int klass, int64_t m, int64_t n, int64_t k, T alpha, const T* A,
                   int64_t lda, const T* B, int64_t ldb, T beta, const T* C, int64_t ldc, T* D,
                   int64_t ldd, int lower_only) {
    return gemm_nt<T>(c, {.klass = klass, .m = m, .n = n, .k = k, .alpha = alpha, .beta = beta, .A = {A, lda}, .B = {B, ldb}, .C = {C, ldc},
                          .D = {D, ldd}, .lower_only = lower_only});
}
// D = alpha A B^T for ONE column tile (n = 128), and per output row the sums of d^2 and d * w[column] over the tile
template <typename T>
int gemm_nt_launch_stats(algp_ctx* c, int klass, int64_t m, int64_t k, T alpha, const T* A, int64_t lda, const T* B, int64_t ldb,
                         T* D, int64_t ldd, const T* w, T* stat_out, int64_t stat_ld) {
    return gemm_nt<T>(c, {.klass = klass, .m = m, .n = 128, .k = k, .alpha = alpha, .A = {A, lda}, .B = {B, ldb}, .D = {D, ldd},
                          .stat_w = w, .stat_out = stat_out, .stat_ld = stat_ld});
}
// D (m x n) = A B^T with B (n x n) lower triangular by 128-tiles -- X_J = T inv(L_JJ)^T with the explicit inverse of a 512-column
// block: column tile c walks k < 128 (c + 1) only; stat_out (or null): the row statistics of every column tile as above
template <typename T>
int gemm_nt_launch_tri(algp_ctx* c, int klass, int64_t m, int64_t n, const T* A, int64_t lda, const T* B, int64_t ldb, T* D,
                       int64_t ldd, const T* w, T* stat_out, int64_t stat_ld) {
    return gemm_nt<T>(c, {.klass = klass, .m = m, .n = n, .k = n, .A = {A, lda}, .B = {B, ldb}, .D = {D, ldd}, .kcut = 1,
                          .stat_w = stat_out ? w : nullptr, .stat_out = stat_out, .stat_ld = stat_ld});
}
ALGP_INSTANTIATE(gemm_nt_launch_tri);
ALGP_INSTANTIATE(gemm_nt_launch_stats);

ALGP_INSTANTIATE(gemm_nt_launch);
// (last: the object file holds the kernels in the order in which these instantiations first name them)
ALGP_INSTANTIATE(gemm_nt);

// ---------------------------------------------------------------------------------------------
// MFMA fragment-layout probe (exact integer data, asymmetric B).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void mfma_probe_kernel(int* mismatches) {
    using F = MF<T>;
    const int lane = threadIdx.x & 63;
    const int i = lane & 15, kk = lane >> 4;
    const T a = (T)(i * 4 + kk + 1);               // A[i][k]
    const T b = (T)((kk + 1) * 17 + i * 3);        // B[k][j], j = lane&15
    typename F::acc_t acc;
    for (int r = 0; r < 4; ++r) acc[r] = (T)0;
    acc = F::mfma(a, b, acc);
    int bad = 0;
    for (int r = 0; r < 4; ++r) {
        const int row = F::row_of(lane, r), col = lane & 15;
        double want = 0;
        for (int k = 0; k < 4; ++k) want += (double)(row * 4 + k + 1) * (double)((k + 1) * 17 + col * 3);
        if ((double)acc[r] != want) ++bad;
    }
    if (bad) atomicAdd(mismatches, bad);
}

template <typename T>
int test_mfma_launch(algp_ctx* c, int* mismatches_dev) {
    hipLaunchKernelGGL(mfma_probe_kernel<T>, dim3(1), dim3(64), 0, c->cur, mismatches_dev);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(test_mfma_launch);


// ---------------------------------------------------------------------------------------------
// device-resident GEMM benchmark (pseudo-random operands, no host traffic)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void fill_random_kernel(T* p, int64_t n, unsigned seed) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned x = (unsigned)(i * 2654435761u) ^ seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    p[i] = (T)((int)(x & 0xffff) - 32768) * (T)(1.0 / 32768.0);
}

template <typename T>
int bench_gemm(algp_ctx* c, int64_t m, int64_t n, int64_t k, int lower_only, int beta_one, int reps,
               double* ms_out, bool gen_c) {
    DevBuf a, b, cc;
    int rc = ensure(c, a, sizeof(T) * m * k);
    if (rc == ALGP_OK) rc = ensure(c, b, sizeof(T) * n * k);
    if (rc == ALGP_OK) rc = ensure(c, cc, sizeof(T) * m * n);
    if (rc != ALGP_OK) { hipFree(a.p); hipFree(b.p); hipFree(cc.p); return rc; }
    hipLaunchKernelGGL(fill_random_kernel<T>, dim3((unsigned)((m * k + 255) / 256)), dim3(256), 0, c->cur, (T*)a.p, m * k, 1u);
    hipLaunchKernelGGL(fill_random_kernel<T>, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, c->cur, (T*)b.p, n * k, 2u);
    hipLaunchKernelGGL(fill_random_kernel<T>, dim3((unsigned)((m * n + 255) / 256)), dim3(256), 0, c->cur, (T*)cc.p, m * n, 3u);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const T beta = beta_one ? (T)1 : (T)0;
    // gen_c: beta = 1 with the C tile GENERATED from (synthetic) coordinates, as the sweep's update products with fused
    // right-hand sides form it (gemm_nt_launch_gen; the scheduled form only) -- timed against beta_one, the C tile loaded
    DevBuf grx, gcx, grk;
    RhsGen gen;
    if (gen_c) {
        rc = ensure(c, grx, sizeof(T) * m * 2);
        if (rc == ALGP_OK) rc = ensure(c, gcx, sizeof(T) * n * 2);
        if (rc == ALGP_OK) rc = ensure(c, grk, sizeof(int) * m);
        if (rc == ALGP_OK) {
            hipLaunchKernelGGL(fill_random_kernel<T>, dim3((unsigned)((m * 2 + 255) / 256)), dim3(256), 0, c->cur, (T*)grx.p, m * 2, 4u);
            hipLaunchKernelGGL(fill_random_kernel<T>, dim3((unsigned)((n * 2 + 255) / 256)), dim3(256), 0, c->cur, (T*)gcx.p, n * 2, 5u);
            hipMemsetAsync(grk.p, 0xff, sizeof(int) * m, c->cur);         // every row ordinary (-1)
            gen.rx = grx.p; gen.cx = gcx.p; gen.rk = (const int*)grk.p;
            gen.ncols = n; gen.DP = 2; gen.kernel = ALGP_KERNEL_RBF; gen.outputscale = 1.0;
        }
    }
    auto one = [&]() {
        if (gen_c) return gemm_nt_launch_gen<T>(c, ALGP_PROF_GEMM_OTHER, m, n, k, (T)-1, (const T*)a.p, k, (const T*)b.p, k, beta, gen, 0, (T*)cc.p, n);
        return gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, m, n, k, (T)-1, (const T*)a.p, k, (const T*)b.p, k, beta, (const T*)cc.p, n,
                                 (T*)cc.p, n, lower_only);
    };
    // $ALGP_TRSM_SCHED (read per call, default on): the scheduled launcher the candidate sweep uses, with its partials scratch
    const bool sched = !lower_only && c->cu_count > 0 && env_switch("ALGP_TRSM_SCHED", true) &&
                       ensure(c, c->gemm_part, sizeof(T) * 128 * 128 * 2 * (size_t)c->cu_count) == ALGP_OK;
    c->gemm_sched = sched;
    for (int w = 0; w < 2 && rc == ALGP_OK; ++w) rc = one();
    hipEventRecord(e0, c->cur);
    for (int r = 0; r < reps && rc == ALGP_OK; ++r) rc = one();
    hipEventRecord(e1, c->cur);
    c->gemm_sched = false;
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    *ms_out = ms / (reps > 0 ? reps : 1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(a.p); hipFree(b.p); hipFree(cc.p); hipFree(grx.p); hipFree(gcx.p); hipFree(grk.p);
    c->dev_bytes -= (int64_t)(a.cap + b.cap + cc.cap + grx.cap + gcx.cap + grk.cap);
    return rc;
}
ALGP_INSTANTIATE(bench_gemm);

}  // namespace algp
