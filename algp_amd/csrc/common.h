// Internal declarations shared by the HIP translation units of libalgp_hip.so (gfx950 only).
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/algp_hip.h"

namespace algp {

constexpr int NB = 128;          // factor block / GEMM tile edge; every device matrix is padded to it
constexpr int MAXD = 8;          // coordinates are stored scaled by 1/lengthscale and zero-padded to DP
constexpr int MAX_APPEND = 128;  // rows a greedy run may append to V^T (ldv = Npad + MAX_APPEND)
constexpr double ENT_CONST = 1.4189385332046727;  // 1/2 log(2 pi e)  (reference utils.py:10)

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// slots (doubles) of ctx->scal, the context's device scalars
constexpr int SC_LOGDET = 0;
constexpr int SC_INFO = 1;       // int stored in a double slot
constexpr int SC_AUXLOGDET = 2;
constexpr int SC_AUXINFO = 3;
constexpr int SC_AMAXV = 4;
constexpr int SC_AMAXI = 5;
constexpr int SC_PROBE = 6;
constexpr int SC_COMMIT = 8;     // (d_c, scale) of the pick being committed
constexpr int SC_AMAXF = 10;     // fresh[argmax] of the lazy greedy
constexpr int SC_STALL = 12;     // int, sticky: a one-launch kernel with inter-workgroup hand-offs gave up (sync_checked)
constexpr int SC_GRAD = 16;      // 16..27: partial sums of the MLL gradient
constexpr int SC_COUNT = 32;

// fixed effects (fixed.hip): the basis is held zero-padded to FX_P columns; the slots (doubles) of fixed_gls_small's output
constexpr int FX_P = 16;
constexpr int FX_BETA = 0;                 // beta, FX_P entries
constexpr int FX_C = FX_P;                 // C (FX_P x FX_P, upper, zero-padded): A^-1 = C C^T
constexpr int FX_COV = FX_C + FX_P * FX_P; // C C^T, p x p
constexpr int FX_LOGDET_A = FX_COV + FX_P * FX_P;
constexpr int FX_QUAD = FX_LOGDET_A + 1;   // b' beta
constexpr int FX_ZZ = FX_QUAD + 1;         // z'z
constexpr int FX_INFO = FX_ZZ + 1;         // 0, or the 1-based column of H_A that is in the span of the ones before it
constexpr int FX_OUT = FX_INFO + 5;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct ProfSlot {
    double ms = 0, flops = 0, bytes = 0;
    int64_t launches = 0;
};

struct PendingEvent {
    hipEvent_t a, b;
    int klass;
};

struct Hypers {
    int kernel = ALGP_KERNEL_RBF;
    int D = 0, DP = 2;
    double inv_ls[MAXD] = {0};
    double outputscale = 1.0, noise = 1.0;
    bool set = false;
    // the additive form (algp_set_hypers_additive): k = os kappa_kernel(r_a) + os_b kappa_kernel_b(r_b), r_a over the first Da
    // coordinates and r_b over the others; kernel / outputscale above are part a's
    bool additive = false;
    int kernel_b = ALGP_KERNEL_RBF, Da = 0;
    double outputscale_b = 0.0;
    // the relationship form (algp_set_hypers_relationship): k = os kappa_kernel(r_a) + os_g G[g, g'], r_a over the first D - 1
    // coordinates (Da), g the integer id in coordinate D - 1 (inverse lengthscale exactly 1); kernel / outputscale are part a's.
    // The table lives in algp_ctx::Gtab in the context's dtype (has_table; else G = I); Ghash: the FNV-1a fingerprint of the
    // caller's Q x Q doubles (0 for the identity), what algp_factorize_from compares as it compares the sites' coordinates by
    // theirs; gdiag_max = max_q G_qq (1 for the identity)
    bool rel = false;
    bool has_table = false;
    int64_t Q = 0;
    double outputscale_g = 0.0, gdiag_max = 1.0;
    uint64_t Ghash = 0;
    // the separable form (algp_set_hypers_separable): k = os kappa_kernel(r_a) kappa_kernel_b(r_b) [+ os_g G[g, g']], r_a over the
    // first Da coordinates, r_b over the next Db; with the genotype term (Q >= 1; the table's fields above are then this form's,
    // rel stays false) the id sits in coordinate Da + Db = D - 1
    bool sep = false;
    int Db = 0;
    // a genotype id rides in coordinate idc() of every site (validated on the host wherever coordinates arrive)
    bool has_ids() const { return rel || (sep && Q > 0); }
    int idc() const { return sep ? Da + Db : Da; }
    // K_jj where it is one scalar (the single and additive forms); under the relationship form the LARGEST prior variance (the
    // jitter's scale) -- the per-site prior goes through algp_ctx::Gprior
    double prior_var() const {
        return has_ids() ? outputscale + outputscale_g * gdiag_max : additive ? outputscale + outputscale_b : outputscale;
    }
    // the gradient's layout [log ls (nl) | log outputscales (nos) | log sigma_n^2]: the id has no lengthscale
    int n_ls() const { return has_ids() ? D - 1 : D; }
    int n_os() const { return (additive || has_ids()) ? 2 : 1; }
    // the same covariance function of the sites' coordinates (algp_factorize_from): the form, and of each form the fields that
    // count under it, the table by its fingerprint
    bool same_model(const Hypers& b) const {
        bool same = D == b.D && kernel == b.kernel && outputscale == b.outputscale && noise == b.noise && additive == b.additive &&
                    (!additive || (kernel_b == b.kernel_b && Da == b.Da && outputscale_b == b.outputscale_b));
        same = same && rel == b.rel && (!rel || (Q == b.Q && outputscale_g == b.outputscale_g && Ghash == b.Ghash));
        same = same && sep == b.sep && (!sep || (kernel_b == b.kernel_b && Da == b.Da && Db == b.Db && Q == b.Q &&
                                                 (Q == 0 || (outputscale_g == b.outputscale_g && Ghash == b.Ghash))));
        for (int d = 0; same && d < D; ++d) same = inv_ls[d] == b.inv_ls[d];
        return same;
    }
};

struct PickRec {           // one committed greedy pick, host side (the device keeps a LazyPick with the row's scale)
    int64_t pool_idx;
    int in_train;          // winner was a mobile-sampled train site (rank-1 noise change)
};

struct DagCache {          // device copy of one task list of the dependency-driven Cholesky (chol_dag.hip)
    int64_t nt;
    int mt = 0, mode = 0, solve_only = 0, pshort = 0;   // the row panel carried below the factor (DagShape)
    DevBuf tasks;
    DevBuf init;           // template of the per-launch state for lists whose tiles do not all start at version 0 (or null)
    int ntasks;
    int workers;           // workgroups the schedule was simulated for = the grid it is launched with
};

struct LazyPick {          // device copy of a committed pick for the lazy greedy refresh (vecops.hip)
    int64_t pool_idx;
    int64_t ncols;         // columns of V^T the pick's dot product covers = the column its entry goes to
    double scale;
    int64_t in_train;
    double d;              // the winner's statistic (pv or s) when it was committed: what `scale` was computed from
};

// The MI criterion's state (api_mi.hip): X = L^-T of P = C_AbarAbar^-1 (Xbar) and of Q = (C + D_all)^-1 (Xall), built once
// per candidate solve, with the picks committed since folded into their diagonals.  form 0 (one GPU): both X whole, in place;
// form 1 (dealt over the ranks of a communicator, ncomp: the layout of algp_comm_set_mi_groups): Xbar / Xall hold only this
// rank's row blocks, everything else stays whole on every rank.
struct MiState {
    DevBuf Xbar, Xall;
    DevBuf DP, DQ;                       // diag(P), diag(Q)
    DevBuf Pos;                          // posbar on the device
    DevBuf U, W;                         // the rank-1 lists of P and of Q (MAX_APPEND columns each)
    DevBuf Col;                          // a pick's column of P or Q (form 1: of both, [mbpad | npad])
    DevBuf H;                            // [H(A), H(Abar), H(all) | signs of the rank-1 terms of P | of Q]
    DevBuf Full, Fold;                   // form 1: the matrix being factored and inverted (released after the build); a gathered column
    std::vector<int64_t> posbar;         // host: pool index -> row of the complement matrix when it was built (-1: sampled)
    bool valid = false;
    int form = 0;
    int64_t npicks = 0, base = 0, nbar = 0;   // picks folded in; picks.size() at the build; rank-1 terms of P so far
    int64_t mb = 0, mbpad = 0, npad = 0;
    double ss = 0, sm = 0;
    int ncomp = 0;                       // ranks [0, ncomp) hold P, the others Q (0: no layout; a world of one: 1, both)

    bool holds(int f) const { return valid && form == f; }
    // holds(f) for (ss, sm) with at most npicks_now picks folded in: catching up folds the later picks, nothing is rebuilt.
    // score_paths_mi asks only holds(0): it refuses to run with picks committed, and a state built with none (a solve
    // invalidates it and clears the picks) does not depend on ss or sm, which only set the noise of picked sites.
    bool current(int f, double ss_now, double sm_now, int64_t npicks_now) const {
        return holds(f) && ss == ss_now && sm == sm_now && npicks_now >= npicks;
    }
    // the communicator's layout goes, and with it a state dealt by that layout
    void drop_layout() {
        ncomp = 0;
        if (form == 1) valid = false;
    }
};

// The variance-reduction criterion's state (api_vr.hip): w_c = sum over the targets j (the ordinary rows of the candidate
// set, fixed by the solve) of omega_j E_jc^2, E the signed cross term of include/algp_hip.h and omega the target weights of
// the pool (algp_ctx::tw; 1 where none are attached), for the first npicks committed picks.
// Built by one fused product per candidate solve (gemm.hip, gemm_nt_kernel_dma4_vr); later picks are folded in by the rank-1
// identity, one pass over V^T each.  It does not depend on the noise levels (ss, sm): they enter when the utilities are formed.
struct VrState {
    DevBuf W;                            // w, one entry per candidate row
    DevBuf Part;                         // the product's sums per column tile, for one chunk of column tiles
    DevBuf R;                            // a pick's column of V^T: [all rows | omega_j r_j on the targets, zero elsewhere]
    DevBuf Tp, Tv;                       // t = V_T^T (omega r)_T: its partial sums per row block, and t
    DevBuf Y;                            // [sum_j C(c, j) omega_j r_j | V_c . t]
    DevBuf Nrm;                          // sum_{j in T} omega_j r_j^2
    DevBuf Obj;                          // one double: the objective sum_{j in T} omega_j pv_j (algp_get_target_variance)
    // over the ranks of a communicator (algp_comm_set_vr_exchange): the local candidates' marks by pool site and the hit flag of
    // the build's disjointness check; the gathered (pool index, omega r) pairs of a fold, made contiguous
    DevBuf Mark, Tidx, Trt;
    bool valid = false;
    bool over_ranks = false;             // w counts the targets of every rank (built by vr_shard_build), not this context's own
    int64_t npicks = 0;                  // picks folded in
    int64_t xrows = 0;                   // the layout: rows of V^T per rank and all-gather of the build (0: none, -1: the default)
    int64_t max_rows = 0;                // the largest shard's rows when the state was built (the padding of a fold's pairs)
    bool every_time = false;             // some rank of the last agreement runs with ALGP_VR_RANK1=0: every scoring builds

    void drop() { valid = false; npicks = 0; }
    // the communicator's layout goes, and with it a state built over its ranks
    void drop_layout() {
        xrows = 0;
        if (over_ranks) drop();
        over_ranks = false;
    }
};

}  // namespace algp

namespace algp {
// exp(x) for the kernel values, x <= 0 in every use (-r^2/2, -r, -sqrt(3) r, -sqrt(5) r): ONE definition for every kernel that evaluates
// k(x, x') -- the matrix build, the lazy refresh's b', the path scores, the mean-only posterior, the MLL gradient -- so
// that a value recomputed later has the bits of the one stored earlier.  fp64: Cody-Waite reduction x = k ln2 + r,
// |r| <= ln2 / 2, Taylor to r^13 (truncation 4e-18), v_ldexp: ~20 instructions where the library routine takes ~55 (the
// matrix build was VALU-bound on it: profiles/r02_valu_by_kernel.json); within 1 ulp of the correctly rounded value on
// [-745, 0], exact at 0, underflows to 0 like it.  fp32: the library's.
__device__ __forceinline__ float kexp(float x) { return expf(x); }
__device__ __forceinline__ double kexp(double x) {
    const double k = __builtin_rint(x * 1.4426950408889634074);
    double r = __builtin_fma(-k, 6.93147180369123816490e-01, x);
    r = __builtin_fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821614599e-10;                          // 1/13!
    p = __builtin_fma(p, r, 2.0876756987868098979e-09);            // 1/12!
    p = __builtin_fma(p, r, 2.5052108385441718775e-08);            // 1/11!
    p = __builtin_fma(p, r, 2.7557319223985890653e-07);            // 1/10!
    p = __builtin_fma(p, r, 2.7557319223985892511e-06);            // 1/9!
    p = __builtin_fma(p, r, 2.4801587301587301566e-05);            // 1/8!
    p = __builtin_fma(p, r, 1.9841269841269841253e-04);            // 1/7!
    p = __builtin_fma(p, r, 1.3888888888888889419e-03);            // 1/6!
    p = __builtin_fma(p, r, 8.3333333333333332177e-03);            // 1/5!
    p = __builtin_fma(p, r, 4.1666666666666664354e-02);            // 1/4!
    p = __builtin_fma(p, r, 1.6666666666666665741e-01);            // 1/3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)k);
}

__device__ __forceinline__ float kfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double kfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
// Matern-1/2 and Matern-5/2 of a squared scaled distance, and their derivative factors (kdk below): written once, here, with
// contraction off and the one fused multiply-add spelled out, so that every site that inlines them -- the matrix build, the
// product epilogues, the criteria, the gradient -- rounds the same way whatever surrounds the call.
//   nu = 1/2: os e^-r, dk = os e^-r / r (0 at r = 0: the limit of u_d^2 / r);  nu = 5/2, a = sqrt(5) r: os (1 + a + a^2/3) e^-a,
//   dk = 5/3 os (1 + a) e^-a
// One body for both: a = c r with c = 1 or sqrt 5 by the (uniform) form, one square root and one exponential, then the value
// os e^-a alone or times the polynomial.  A site that takes the form at run time thus holds one square root and one exponential
// for the two, not two of each (the variance-reduction epilogues inline this 64 times).
template <typename T>
__device__ __forceinline__ T kval_matern_05_25(int kernel, T os, T r2, T* dk) {
#pragma clang fp contract(off)
    const bool m25 = kernel == ALGP_KERNEL_MATERN25;
    const T r = sqrt(r2);
    const T a = r * (m25 ? (T)2.2360679774997896 : (T)1);
    const T oe = os * kexp(-a);
    const T a1 = (T)1 + a;
    if (dk) *dk = m25 ? (T)1.6666666666666667 * (a1 * oe) : (r > (T)0 ? oe / r : (T)0);
    // (selected, not multiplied by a run-time 0: a coordinate difference that overflows gives a = inf, e^-a = 0 and the value 0
    // for nu = 1/2 as os * kexp(-r) alone would, not 0 * inf)
    return m25 ? kfma(a * (T)0.33333333333333333, a, a1) * oe : oe;
}
// The forms come in two families: 0 = RBF and Matern-3/2, 1 = Matern-1/2 and Matern-5/2.  A kernel whose inner loop selects the
// form at run time is compiled once per family (kmat_kernel, the generating GEMM epilogues), so that the copy the first two forms
// run is the code it was before the second family existed: with all four in one loop the fp64 matrix build took 20 more VGPRs,
// and the fp64 gradient kernel (whose nu = 1/2 factor holds a division) 4 more, which cost it a wave of occupancy.
__host__ __device__ inline int kernel_family(int kernel) { return kernel == ALGP_KERNEL_MATERN05 || kernel == ALGP_KERNEL_MATERN25 ? 1 : 0; }
// ScaleKernel(RBF) / ScaleKernel(Matern-nu), nu = 1/2, 3/2, 5/2, of a squared scaled distance.  FAM: the family `kernel` is known
// to belong to (only its two forms are compiled in), or -1: any of the four, tested in the order RBF, Matern-3/2, second family
// (the order the criteria's kernels have always tested them in: pool_cov below keeps their instructions)
template <typename T, int FAM = -1>
__device__ __forceinline__ T kval(int kernel, T os, T r2) {
    if (FAM != 1 && kernel == ALGP_KERNEL_RBF) return os * kexp((T)-0.5 * r2);
    if (FAM != 1 && (FAM == 0 || kernel == ALGP_KERNEL_MATERN15)) {
        const T r = sqrt(r2) * (T)1.7320508075688772;
        return os * ((T)1 + r) * kexp(-r);
    }
    return kval_matern_05_25<T>(kernel, os, r2, nullptr);
}
// The kernel value (returned) and the factor dk of its length-scale derivative, dk * u_d^2 = dk/dlog ls_d with
// u_d = (x_d - x'_d) / ls_d, i.e. dk = -2 dk/dr^2: the MLL gradient (fit.hip).  FAM as for kval
template <typename T, int FAM = -1>
__device__ __forceinline__ T kdk(int kernel, T os, T r2, T& dk) {
    if (FAM != 1 && kernel == ALGP_KERNEL_RBF) {
        const T kv = os * kexp((T)-0.5 * r2);
        dk = kv;
        return kv;
    }
    if (FAM != 0 && (FAM == 1 || kernel_family(kernel) == 1)) return kval_matern_05_25<T>(kernel, os, r2, &dk);
    const T a = sqrt(r2) * (T)1.7320508075688772;
    const T e = kexp(-a);
    dk = (T)3 * os * e;
    return os * ((T)1 + a) * e;
}
// k(x, x') from the scaled, zero-padded coordinates of the two sites: ONE definition for the kernel-matrix build (kmat.hip)
// and for the product epilogue that forms the candidates' right-hand sides in registers (gemm.hip, GEN), which must leave the
// same bits.  Two coordinates (the form with two call sites): r^2 = fma(d0, d0, d1 * d1), the second square rounded on its own --
// what the compiler has always made of `r2 = 0; r2 += d0 * d0; r2 += d1 * d1` in the matrix build, written out so that no call
// site can be contracted differently.  Wider coordinates keep the plain sum (the matrix build is their only caller).
template <typename T, int DP, int FAM = -1>
__device__ __forceinline__ T kmat_value(int kernel, T os, const T (&xr)[DP], const T (&xc)[DP]) {
    T r2;
    if constexpr (DP == 2) {
        const T d0 = xr[0] - xc[0], d1 = xr[1] - xc[1];
        const T q1 = d1 * d1;
        r2 = kfma(d0, d0, q1);
    } else {
        r2 = (T)0;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xr[d] - xc[d];
            r2 += df * df;
        }
    }
    return kval<T, FAM>(kernel, os, r2);
}
// The additive form, a third family (2) beside the two above: k = os_a kappa_a(r_a) + os_b kappa_b(r_b), r_a over the first da
// scaled coordinates, r_b over the others (the zero padding adds nothing).  It is compiled as instantiations of its own (the
// matrix build's FAM = 2, a source type of its own for pool_cov below, a form type of its own for fit.hip's gradient kernel), so that the code the
// single forms run stays what it was.  ONE definition of the two squared distances and of the sum for every site: each
// square rounded on its own and added in coordinate order (contraction off), so the matrix build, the criteria and the gradient
// see the same r_a^2, r_b^2 and the same value for a pair of sites.
template <int DP, typename C, typename XA, typename XB>
__device__ __forceinline__ void split_r2(const XA* xa, const XB* xb, int da, C& ra, C& rb) {
#pragma clang fp contract(off)
    ra = (C)0;
    rb = (C)0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const C df = (C)xa[d] - (C)xb[d];
        const C q = df * df;
        ra += d < da ? q : (C)0;
        rb += d < da ? (C)0 : q;
    }
}
// parts: bit 0 = part a, bit 1 = part b (3: the kernel; one bit: a component of the posterior mean)
template <typename T>
__device__ __forceinline__ T kval_add(int ka, T osa, T ra, int kb, T osb, T rb, int parts = 3) {
#pragma clang fp contract(off)
    const T va = (parts & 1) ? kval<T>(ka, osa, ra) : (T)0;
    const T vb = (parts & 2) ? kval<T>(kb, osb, rb) : (T)0;
    return va + vb;
}
template <typename T, int DP>
__device__ __forceinline__ T kmat_value_add(int ka, T osa, int kb, T osb, int da, const T (&xr)[DP], const T (&xc)[DP]) {
    T ra, rb;
    split_r2<DP>(&xr[0], &xc[0], da, ra, rb);
    return kval_add<T>(ka, osa, ra, kb, osb, rb);
}
// The relationship form, a fourth family (3): k = os_a kappa_a(r_a) + os_g G[ia Q + ib], r_a over the first da scaled coordinates
// and ia, ib the two sites' integer ids, held exactly in coordinate da (its inverse lengthscale is 1; validated on the host to be
// integers in [0, Q) before any launch, and the zero padding reads id 0).  G null: the identity, the part's value os_g (ia == ib).
// Compiled as instantiations of its own like the additive form.  ONE definition for every site: r_a^2 as split_r2 sums it (each
// square rounded on its own, coordinate order, contraction off), the table index in 64 bits, one rounded product os_g G and one
// rounded sum of the two terms.
template <int DP, typename C, typename XA, typename XB>
__device__ __forceinline__ void rel_r2(const XA* xa, const XB* xb, int da, C& ra, int64_t& ia, int64_t& ib) {
#pragma clang fp contract(off)
    ra = (C)0;
    C ga = (C)0, gb = (C)0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const C va = (C)xa[d], vb = (C)xb[d];
        const C df = va - vb;
        const C q = df * df;
        ra += d < da ? q : (C)0;
        ga = d == da ? va : ga;
        gb = d == da ? vb : gb;
    }
    ia = (int64_t)ga;
    ib = (int64_t)gb;
}
// the genotype part's value os_g G[ia, ib]: kval_rel's, and every other site's that takes an entry of the table (fit.hip: the
// gradient, the genotype posterior's right-hand sides and prior, the per-site prior)
template <typename C, typename T>
__device__ __forceinline__ C rel_entry(const T* G, int64_t Q, C osg, int64_t ia, int64_t ib) {
#pragma clang fp contract(off)
    const C g = G ? (C)G[ia * Q + ib] : (ia == ib ? (C)1 : (C)0);
    return osg * g;
}
// parts: bit 0 = the spatial part, bit 1 = the genotype part (as kval_add)
template <typename C, typename T>
__device__ __forceinline__ C kval_rel(int ka, C osa, C ra, const T* G, int64_t Q, C osg, int64_t ia, int64_t ib, int parts = 3) {
#pragma clang fp contract(off)
    const C va = (parts & 1) ? kval<C>(ka, osa, ra) : (C)0;
    C vg = (C)0;
    if (parts & 2) vg = rel_entry<C>(G, Q, osg, ia, ib);
    return va + vg;
}
template <typename T, int DP>
__device__ __forceinline__ T kmat_value_rel(int ka, T osa, const T* G, int64_t Q, T osg, int da, const T (&xr)[DP], const T (&xc)[DP]) {
    T ra;
    int64_t ia, ib;
    rel_r2<DP>(&xr[0], &xc[0], da, ra, ia, ib);
    return kval_rel<T, T>(ka, osa, ra, G, Q, osg, ia, ib);
}
// The separable form, a fifth family (4): k = os kappa_a(r_a) kappa_b(r_b) [+ os_g G[ia Q + ib]], r_a over the scaled coordinates
// [0, da), r_b over [da, dg), and -- with the genotype term (hasg, uniform over the launch) -- the two sites' integer ids held
// exactly in coordinate dg, as under the relationship form.  Without the term dg is the padded width: no coordinate is read as
// an id.  Compiled as instantiations of its own like the two forms above.  ONE definition for every site: r_a^2 and r_b^2 as
// split_r2 sums them (each square rounded on its own, coordinate order, contraction off), the two factor values at outputscale
// 1, one rounded product kappa_a kappa_b, one rounded product with os, then (hasg) one rounded sum with rel_entry's value.
template <int DP, typename C, typename XA, typename XB>
__device__ __forceinline__ void sep_r2(const XA* xa, const XB* xb, int da, int dg, C& ra, C& rb, int64_t& ia, int64_t& ib) {
#pragma clang fp contract(off)
    ra = (C)0;
    rb = (C)0;
    C ga = (C)0, gb = (C)0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const C va = (C)xa[d], vb = (C)xb[d];
        const C df = va - vb;
        const C q = df * df;
        const bool isid = d == dg;                                // (behind the id there is only zero padding: it adds nothing)
        ra += d < da ? q : (C)0;
        rb += (d < da || isid) ? (C)0 : q;
        ga = isid ? va : ga;
        gb = isid ? vb : gb;
    }
    ia = (int64_t)ga;
    ib = (int64_t)gb;
}
// the product of the two factor values and the outputscale, in that order: kval_sep's, and the gradient's dS/dlog os
template <typename C>
__device__ __forceinline__ C sep_prod(C os, C fa, C fb) {
#pragma clang fp contract(off)
    const C p = fa * fb;
    return os * p;
}
// parts: bit 0 = the spatial product, bit 1 = the genotype term (as kval_rel)
template <typename C, typename T>
__device__ __forceinline__ C kval_sep(int ka, int kb, C os, C ra, C rb, bool hasg, const T* G, int64_t Q, C osg, int64_t ia, int64_t ib,
                                      int parts = 3) {
#pragma clang fp contract(off)
    C v = (C)0;
    if (parts & 1) v = sep_prod<C>(os, kval<C>(ka, (C)1, ra), kval<C>(kb, (C)1, rb));
    if (hasg && (parts & 2)) {
        const C vg = rel_entry<C>(G, Q, osg, ia, ib);
        v = v + vg;
    }
    return v;
}
template <typename T, int DP>
__device__ __forceinline__ T kmat_value_sep(int ka, int kb, T os, int da, int dg, bool hasg, const T* G, int64_t Q, T osg, const T (&xr)[DP],
                                            const T (&xc)[DP]) {
    T ra, rb;
    int64_t ia, ib;
    sep_r2<DP>(&xr[0], &xc[0], da, dg, ra, rb, ia, ib);
    return kval_sep<T, T>(ka, kb, os, ra, rb, hasg, G, Q, osg, ia, ib);
}
// Entry (row, global column gcol) of the candidates' right-hand side B^T = K(candidates, train) as the matrix build writes it:
// kind -1: an ordinary row, k(x_row, x_col) in the columns of the train set (gcol < ncols), 0 in the padding behind them;
// kind >= 0: the unit row e_kind (a candidate that is a train site under prior_includes_noise); kind -2: a padding row, 0.
template <typename T, int DP>
__device__ __forceinline__ T bt_entry(int kernel, T os, const T (&xr)[DP], const T (&xc)[DP], int kind, int64_t gcol, int64_t ncols) {
    const T v = kmat_value<T, DP>(kernel, os, xr, xc);
    const T ordinary = (kind == -1 && gcol < ncols) ? v : (T)0;
    const T unit = gcol == (int64_t)kind ? (T)1 : (T)0;
    return kind >= 0 ? unit : ordinary;
}

// The pool covariance as the vector kernels and the criteria's epilogues see it: KmatSrc (below) in the storage type T, with
// the outputscale and the noise in the type the site computes in (C: double in the path kernels, whatever T is).  DP stays a
// template argument of the kernels.  Made on the host by cov_src.
template <typename T, typename C = T>
struct CovSrc {
    const T* Xs;         // n x DP scaled, zero padded coordinates (coordinate pool)
    const T* Cp;         // n x n explicit covariance, or null
    int64_t n_pool;
    int kernel;
    C os, noise;         // noise: sigma_n^2 where the pool indices coincide; 0 for an explicit covariance, which holds it already
};
// C(pa, pb), ONE definition for every site outside the matrix build: the lazy refresh's b', the path kernels, the kernel-GEMV,
// the variance-reduction epilogues.  The entry of the explicit covariance if there is one; else r^2 as the plain sum from zero
// over the DP coordinate differences, the kernel value (kval), and sigma_n^2 where the pool indices coincide (NOISE = false: left
// out -- the kernel-GEMV, whose callers add that term themselves or have none).  The plain sum is NOT kmat_value's r^2: under
// contraction two coordinates come out as fma(d1, d1, d0 * d0) here and fma(d0, d0, d1 * d1) there, which round differently, and
// each side's stored results hold its own bits -- the two are not to be merged.
// xa, xb: the two sites' coordinates wherever the kernel holds them (registers, LDS, memory), in any type; computed in the type
// of s.os.  S: a CovSrc, or any argument struct with its fields (the GEMM's VrGemmArgs, read in place: a CovSrc made from it in
// the epilogue moved the address arithmetic around it).
// The additive form's source: CovSrc (kernel, os: part a) and part b, the split and the parts that count.  A source type of its
// own, so that a kernel instantiated for it is another kernel than the single forms' (never made for an explicit covariance)
template <typename T, typename C = T>
struct CovSrcAdd : CovSrc<T, C> {
    int kernel_b, da, parts;
    C os_b;
};
// S carries the additive fields (CovSrcAdd, or the GEMM's argument structs with the same fields appended)
template <typename S, typename = void>
struct is_additive : std::false_type {};
template <typename S>
struct is_additive<S, std::void_t<decltype(std::declval<S>().kernel_b)>> : std::true_type {};

// The relationship form's source: CovSrc (kernel, os: the spatial part), the table (null: the identity) in the storage type, its
// order, the genotype part's outputscale, the coordinate that holds the id (da = D - 1) and the parts that count.  A source type
// of its own for the reason CovSrcAdd is one.
template <typename T, typename C = T>
struct CovSrcRel : CovSrc<T, C> {
    const T* G;
    int64_t Q;
    int da, parts;
    C os_g;
};
// S carries the relationship fields (CovSrcRel, or the GEMM's argument structs with the same fields appended)
template <typename S, typename = void>
struct is_rel : std::false_type {};
template <typename S>
struct is_rel<S, std::void_t<decltype(std::declval<S>().os_g)>> : std::true_type {};

// The separable form's source: CovSrc (kernel: factor a, os: the product's outputscale), factor b, the split [0, sep_da) |
// [sep_da, sep_dg), and the genotype term's table, order and outputscale while sep_hasg (then sep_dg is the id's coordinate).  A
// source type of its own for the reason CovSrcAdd is one; its field names are its own so that neither trait above takes it.
template <typename T, typename C = T>
struct CovSrcSep : CovSrc<T, C> {
    const T* sep_G;
    int64_t sep_Q;
    int sep_kb, sep_da, sep_dg, sep_hasg, sep_parts;
    C sep_osg;
};
// S carries the separable fields (CovSrcSep, or the GEMM's argument structs with the same fields appended)
template <typename S, typename = void>
struct is_sep : std::false_type {};
template <typename S>
struct is_sep<S, std::void_t<decltype(std::declval<S>().sep_dg)>> : std::true_type {};

template <int DP, bool NOISE = true, typename S, typename XA, typename XB>
__device__ __forceinline__ auto pool_cov(const S& s, int64_t pa, int64_t pb, const XA* xa, const XB* xb) {
    using C = std::remove_cv_t<decltype(s.os)>;
    if constexpr (is_sep<S>::value) {
        C ra, rb;
        int64_t ia, ib;
        sep_r2<DP>(xa, xb, s.sep_da, s.sep_dg, ra, rb, ia, ib);
        C v = kval_sep<C>(s.kernel, s.sep_kb, s.os, ra, rb, s.sep_hasg != 0, s.sep_G, s.sep_Q, s.sep_osg, ia, ib, s.sep_parts);
        if (NOISE && pa == pb) v += s.noise;
        return v;
    } else if constexpr (is_rel<S>::value) {
        C ra;
        int64_t ia, ib;
        rel_r2<DP>(xa, xb, s.da, ra, ia, ib);
        C v = kval_rel<C>(s.kernel, s.os, ra, s.G, s.Q, s.os_g, ia, ib, s.parts);
        if (NOISE && pa == pb) v += s.noise;
        return v;
    } else if constexpr (is_additive<S>::value) {
        C ra, rb;
        split_r2<DP>(xa, xb, s.da, ra, rb);
        C v = kval_add<C>(s.kernel, s.os, ra, s.kernel_b, s.os_b, rb, s.parts);
        if (NOISE && pa == pb) v += s.noise;
        return v;
    }
    if (s.Cp) return (C)s.Cp[pa * s.n_pool + pb];
    C r2 = (C)0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const C df = (C)xa[d] - (C)xb[d];
        r2 += df * df;
    }
    C v = kval<C>(s.kernel, s.os, r2);
    if (NOISE && pa == pb) v += s.noise;
    return v;
}
// the row's coordinates in registers, the column's read from the pool; both read from the pool
template <int DP, bool NOISE = true, typename S, typename XA>
__device__ __forceinline__ auto pool_cov(const S& s, int64_t pa, int64_t pb, const XA* xa) {
    return pool_cov<DP, NOISE>(s, pa, pb, xa, s.Xs + pb * DP);
}
template <int DP, typename S>
__device__ __forceinline__ auto pool_cov(const S& s, int64_t pa, int64_t pb) {
    return pool_cov<DP>(s, pa, pb, s.Xs + pa * DP, s.Xs + pb * DP);
}
}  // namespace algp

struct algp_ctx {
    int device = 0;
    int dtype = ALGP_F64;
    size_t es = 8;
    hipStream_t stream = nullptr;    // main stream (all results are complete on it before an ABI call returns)
    hipStream_t stream2 = nullptr;   // helper streams: independent row chunks of the candidate solve overlap on them
    hipStream_t stream3 = nullptr, stream4 = nullptr;
    int trsm_chunks = 3;
    bool trsm_chunks_explicit = false;   // set by $ALGP_TRSM_CHUNKS or algp_debug_set_trsm_chunks(k >= 1): the chunked sweep, not the scheduled one
    int cu_count = 0;                // compute units of the device (the scheduled GEMM's grid is 2 x this)
    bool gemm_sched = false;         // the GEMM launcher takes its scheduled form (gemm_sched.h) while this is set: the candidate sweep, bench_gemm
    hipStream_t cur = nullptr;       // stream the launch helpers currently target
    std::vector<hipEvent_t> sync_events;
    std::string err;
    int64_t pivot = 0;
    double last_jitter = 0;          // diagonal jitter the last algp_get_posterior_cov needed for its MI term (0: none)
    algp::Hypers hyp;

    // pool
    int64_t n_pool = 0;
    bool pool_is_cov = false;
    algp::DevBuf Xs;        // n x DP scaled, zero padded coordinates
    algp::DevBuf Xraw;      // n x D raw coordinates (kept to rescale on a hyper change)
    algp::DevBuf Cp;        // n x n explicit covariance (pool_is_cov)
    algp::DevBuf tw;        // target weight of every pool site in the context's dtype (algp_set_target_weights), while has_tw
    bool has_tw = false;    // the weights belong to their pool: a new pool drops them
    uint64_t tw_hash = 0;   // FNV-1a of the weights as attached (while has_tw): ranks scoring together must hold the same ones
    algp::DevBuf fxH;       // the fixed effects' basis (algp_set_fixed_effects): n_pool x FX_P in the context's dtype, zero-padded, while fx_p > 0
    int fx_p = 0;           // its columns; 0: none attached.  The basis belongs to its pool: a new pool drops it
    std::vector<int64_t> pos_in_train;   // host: pool index -> position in train set or -1
    std::vector<uint64_t> site_hash;     // host: fingerprint of every pool site's coordinates (algp_factorize_from)

    // train set / factor
    int64_t N = 0, Npad = 0;
    int64_t Lld = 0;                     // leading dimension (= capacity) of L; >= Npad
    int64_t Nfact = 0;                   // rows of L that are valid for (fact_idx, fact_var)
    std::vector<int64_t> fact_idx;       // train set the resident factor was computed for
    std::vector<double> fact_var;
    std::vector<double> train_var_host;
    uint64_t fact_hyp_stamp = 0, hyp_stamp = 1;
    bool train_dirty = false;
    int64_t kept_rows_last = 0;
    std::vector<int64_t> train_idx;
    bool mean_override = false;          // algp_set_constant_mean: the GP's constant mean instead of mean(train y)
    double mean_value = 0;
    bool train_has_repeats = false;      // a pool index occurs in more than one train row
    algp::DevBuf Aidx, yA, varA, y0, L, invD, z, alpha, scal;   // scal: device doubles (logdet, info...)
    double ybar = 0, logdet = 0, yalpha = 0;
    bool factored = false;
    // z = L^-1 (y - ybar 1) = u - ybar w with u = L^-1 y, w = L^-1 1: both are prefix-stable under row appends, so a
    // factor update only extends them (uw_rows leading rows valid for fact_idx / fact_var / fact_y)
    algp::DevBuf yraw, uvec, wvec;
    std::vector<double> train_y_host, fact_y;
    int64_t uw_rows = 0;
    int64_t uw_stable = 0;               // leading entries of u, w unchanged since the row sums below were started
    // per candidate: sums over the kept columns [0, acc_cols) of V^T of v^2, v u, v w (incremental solve)
    algp::DevBuf acc3;
    algp::DevBuf rowstat;                // per column tile of V^T: row sums of v^2 and v z left by the solve's own launches
    algp::DevBuf splitk;                 // partial products of split-K launches (skinny solves)
    algp::DevBuf ldpart;                 // logdiag_kernel's per-wave partial sums
    algp::DevBuf tailPart;               // tail.hip: partial accumulators of the k-split form
    algp::DevBuf tailE;                  // tail.hip: inverse of the 128 x 128 window of L at the first new column (a range that straddles two blocks)
    algp::DevBuf gemm_part;              // scheduled GEMM: partial sums of the k slices of a launch's leftover tiles (2 x CUs tiles)
    algp::DevBuf inv512, inv512_scr, trsm_tmp;   // candidate solve: explicit inverses of the factor's 512-column blocks, their scratch, mpad x 512
    algp::DevBuf rhs_rx, rhs_cx, rhs_rk;         // fused right-hand sides (RhsGen): gathered coordinates of the candidate rows, of the train columns; row kinds
    int64_t rhs_rows = 0;                        // the leading candidate rows (a multiple of 128) that RhsGen::window writes: the sweep's
    std::vector<algp::DagCache> dag_cache;   // task lists of the dependency-driven Cholesky, per matrix size
    algp::DevBuf dag_state;              // its per-launch tile versions / control words / per-block log-determinants
    algp::DevBuf trsv_ctrl;              // ticket + per-block flags of the one-launch forward substitution (potrf.hip)
    algp::DevBuf dag_stats;              // its in-kernel task accounting (while profiling is on), see algp_cholesky_task_stats
    int64_t acc_cols = 0, acc_M = -1;
    int64_t factor_rows_from_vt = 0;     // last factor update: rows of L taken from V^T instead of a triangular solve
    bool alpha_valid = false;            // alpha = L^-T z is computed on first use (scoring does not need it)

    // candidates
    int64_t M = 0, Mpad = 0, ldv = 0;
    int64_t ncols = 0;       // active columns of V^T (Npad + appended)
    int prior_noise = 1;
    std::vector<int64_t> cand_idx;
    std::vector<int64_t> cand_pos;       // host: pool index -> local candidate position or -1
    algp::DevBuf Cidx, ckind, cextra, Vt, dstat, mu, alive, scores, lrow, tvec, amax;
    std::vector<algp::PickRec> picks;
    algp::DevBuf prevrows;   // MAX_APPEND x ldv: the l-rows of committed picks
    algp::DevBuf remote;     // one-row stand-ins for the per-candidate arrays while a remote winner's row is rebuilt
    // lazy greedy: fresh[j] = number of committed picks already applied to row j of V^T / dstat[j]
    algp::DevBuf fresh, lazypicks;
    bool lazy_stale = false;             // some rows lag behind picks.size(): flush before reading the full state
    bool bounds_valid = false;           // c->scores = entropy utility of each row as of fresh[row] picks, for (lazy_ss, lazy_delta)
    double lazy_ss = 0, lazy_delta = 0;
    bool solved = false;
    int64_t ldv_cap = 0;                 // allocated leading dimension of V^T
    // what the resident V^T columns were solved for (incremental candidate solve)
    std::vector<int64_t> vt_fact_idx, vt_cand_idx;
    std::vector<double> vt_fact_var;
    std::vector<int> vt_kind;            // per candidate: position in the train set it was solved as, or -1
    uint64_t vt_hyp_stamp = 0;
    int vt_prior_noise = -1;
    bool vt_has_extra = false;
    int64_t kept_cols_last = 0;

    algp::MiState mi;                    // the MI criterion's resident state (api_mi.hip)
    algp::VrState vr;                    // the variance-reduction criterion's column sums (api_vr.hip)

    // multi-GPU: transport of the sharded greedy loop's one all-gather (comm.hip): an RCCL communicator
    // (algp_comm_init), a caller-supplied host all-gather (algp_comm_init_host), or neither (one rank)
    void* comm = nullptr;
    algp_allgather_fn host_gather = nullptr;
    void* host_gather_user = nullptr;
    int comm_nranks = 1, comm_rank = 0;
    algp::DevBuf commbuf;    // [own payload | gathered payloads | winner record], see comm.hip
    void* comm_host = nullptr;           // pinned staging of the host transport: [own payload | gathered payloads]
    size_t comm_host_cap = 0;
    // the factor update's row exchange (comm.hip, api.hip: exchange_new_rows): which rank holds each pool site as a candidate
    // (algp_comm_set_owners; empty: no exchange), [own rows | gathered rows] on the device, pinned staging (host transport)
    std::vector<int32_t> site_owner;
    uint64_t site_owner_hash = 0;                              // FNV-1a of the whole map: part of the agreement word of a sharded factor update
    algp::DevBuf rowx;
    void* rowx_host = nullptr;
    size_t rowx_host_cap = 0;
    int64_t rows_from_peers = 0;         // last factor update: rows of L that arrived from other ranks
    int64_t row_exchanges = 0, row_fallbacks = 0;   // exchanges carried out / agreed fall-backs to the triangular solve, so far
    int debug_fail_next_rowx = 0;        // algp_debug_fail_at(3): this rank's next agreement word carries this code
    int pending_pick_error = 0;          // a commit that failed after an exchange: this rank's status word in its next pick
    std::string pending_pick_msg;
    int64_t n_syncs = 0;     // stream synchronisations issued by the library (algp_debug_counter)
    int debug_dag_stall_ticket = -1; // algp_debug_dag_stall: the next one-launch factorisation loses this ticket's publish
    int debug_trsv_stall_block = -1; // algp_debug_trsv_stall: the next one-launch substitution loses this block's flag
    int debug_fail_next_pick = 0;   // algp_debug_fail_next_pick: error code this rank reports in its next pick
    int debug_fail_next_commit = 0; // algp_debug_fail_at(1): the next commit of a greedy pick fails with this code (after the exchange)
    int debug_fail_next_pack = 0;   // algp_debug_fail_at(2): the next pick's pack launch counts as failed
    int debug_fail_next_mi = 0;     // algp_debug_fail_at(4): the next step of the sharded MI state (its build or a pick's fold) fails
    int debug_fail_next_vr = 0;     // algp_debug_fail_at(5): the next step of the variance-reduction state over ranks (build, else a fold) fails
    double xhdr[4] = {0, 0, 0, 0};  // comm_exchange: this rank's header of the next gather (host memory that outlives the copy)

    // scratch for auxiliary factorizations (entropy_from_cov, set entropies, MI terms, posterior cov)
    algp::DevBuf auxA, auxInv, auxW, auxIdx, auxVar, auxD, hostStage;
    algp::DevBuf smp;                    // algp_sample_posterior's scratch, one allocation carved up per call (api_sample.hip)
    algp::DevBuf grp;                    // algp_group_posterior's scratch, likewise (api_group.hip)
    // the relationship form (Hypers::rel): the Q x Q table in the context's dtype (while hyp.has_table), the prior variance
    // os_a + os_g G[g_j, g_j] of every pool site (the per-site prior of cand_finalize_launch, rebuilt with the scaled pool), and
    // algp_genotype_posterior's scratch, one allocation carved up per call (api_genotype.hip)
    algp::DevBuf Gtab, Gprior, gen;
    algp::DevBuf ai;                     // algp_get_mll_ai's scratch: the 128 x Npad panel U -> V and the P x P result (api_fit.hip)
    algp::DevBuf fx;                     // the fixed effects' scratch, one allocation carved up per call (api_fixed.hip)
    uint64_t gprior_stamp = 0;          // Gprior holds the priors for this hyp_stamp and gprior_noise (prior_includes_noise)
    int gprior_noise = -1;

    // profiling
    bool prof_on = false;
    algp::ProfSlot prof[ALGP_PROF_COUNT];
    std::vector<algp::PendingEvent> pending;
    std::vector<hipEvent_t> event_pool;
    int64_t dev_bytes = 0;
};

namespace algp {

int fail(algp_ctx* c, int code, const std::string& msg);
int ensure(algp_ctx* c, DevBuf& b, size_t bytes);
void prof_begin(algp_ctx* c, int klass, double flops, double bytes);
void prof_end(algp_ctx* c);
bool prof_launch_events(algp_ctx* c, int klass, double flops, double bytes, hipEvent_t* a, hipEvent_t* b);
void prof_collect(algp_ctx* c);
// un-nested wall-time span on the main stream (e.g. a whole candidate solve whose row chunks overlap on several streams)
void prof_span_begin(algp_ctx* c, int klass, double flops, double bytes);
void prof_span_end(algp_ctx* c);
void prof_span_end_on(algp_ctx* c, hipStream_t st);
void prof_span_begin2(algp_ctx* c, int klass, double flops, double bytes);   // second span, starts on c->cur
void prof_span_end2(algp_ctx* c);

// ---- environment switches: ALL of them, read through these two functions ------------------------------------------------
// Size-range fall-backs that are product paths for other sizes, each forced by its switch so that the tests can run both on
// one input:   ALGP_TAIL_COLS=0 (appended columns re-solved as whole 128-column blocks: what inputs below 2 048 rows take;
//   also: a from-scratch solve's narrow last tile goes through the sweep instead of the tail kernel),
//   ALGP_TAIL_SPLIT=0 (the tail kernel without its k-split), ALGP_SOLVE_DAG=0 (mid-sized solves as the right-looking push
//   instead of the task list), ALGP_FOLD=0 (fit and solve as two steps: what a candidate set beyond 51 200 rows takes),
//   ALGP_ROW_STATS=0 / ALGP_TRSM_INV512=0 (the chunked solve with a variance pass / with 128-column steps inside a block),
//   ALGP_TRSM_SCHED=0 (the big solve as row chunks on three streams instead of scheduled launches on one; read per call),
//   ALGP_RHS_FUSED=0 (the scheduled sweep reads the candidates' right-hand sides B^T from V^T, where a kernel-matrix launch has
//   put them, instead of forming them in its update products' epilogues; read per call),
//   ALGP_SPLIT_PANELS=n (fit_and_solve's sweep with its last n tile rows in the factorisation's launch; unset: the rule of
//   plan_route, 0: never; read per call),
//   ALGP_FACTOR_FROM_VT=0 (new rows of an updated factor solved, not gathered), ALGP_LAZY_GREEDY=0 (every row scored before
//   every pick), ALGP_TRSM_CHUNKS=n (row-chunk streams of the big solve; bench.py's one-stream leg sets it by the ABI).
// Cross-check routes: ALGP_CHOL_DAG=0 (launch-sequence factorisation), ALGP_GATHER_ROWS=0 (remote commits rebuild the row),
//   ALGP_VR_RANK1=0 (variance-reduction criterion: the full product at every scoring instead of one rank-1 fold per pick).
// Tooling: ALGP_LAUNCH_LOG=<file> (tools/trace_shapes.py), ALGP_RCCL_PATH=<file> (which librccl to dlopen).
inline bool env_switch(const char* name, bool dflt) {
    const char* e = getenv(name);
    return (e && *e) ? atoi(e) != 0 : dflt;
}
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}

#define ALGP_HIP(call)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return algp::fail(c, ALGP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define ALGP_TRY(call)          \
    do {                        \
        int r_ = (call);        \
        if (r_ != ALGP_OK) return r_; \
    } while (0)

struct ProfScope {
    algp_ctx* c;
    ProfScope(algp_ctx* c_, int klass, double flops, double bytes) : c(c_) { prof_begin(c, klass, flops, bytes); }
    ~ProfScope() { prof_end(c); }
};

// ---- typed kernels (definitions in the .hip files; explicit instantiation for float, double) ----
struct KmatSrc {
    // generator of C(pi, pj): coordinates (scaled, padded) or explicit pool covariance
    const void* Xs;      // n x DP
    const void* Cp;      // n x n or null
    int64_t n_pool;
    int DP;
    int kernel;
    double outputscale;
    double noise;        // sigma_n^2 added when pool indices coincide (coords mode only)
    // the additive form (kernel_b >= 0; kernel / outputscale are then part a's): part b, the first da coordinates are part a's,
    // parts: bit 0 = a, bit 1 = b counts (3 everywhere but in algp_posterior_mean_component)
    int kernel_b = -1, da = 0, parts = 3;
    double outputscale_b = 0;
    bool additive() const { return kernel_b >= 0 && !Cp && !sep; }
    // the relationship form (Q > 0; kernel / outputscale are then the spatial part's, da = D - 1 the id's coordinate, kernel_b
    // stays -1): the table in the context's dtype or null for the identity, its order, the genotype part's outputscale
    const void* G = nullptr;
    int64_t Q = 0;
    double outputscale_g = 0;
    bool rel() const { return Q > 0 && !Cp && !sep; }
    // the separable form (sep; kernel / kernel_b are then the two factors', outputscale the product's, da the split, dg the end
    // of factor b's coordinates -- the id's coordinate while Q > 0, the padded width DP else; the table's fields above are then
    // this form's): additive() and rel() are false under it
    bool sep = false;
    int dg = 0;
    bool sepf() const { return sep && !Cp; }
};
// the device-side view of a source (CovSrc above).  The one place that says what `noise` means per pool kind: an explicit
// covariance carries sigma_n^2 on its diagonal already, so nothing is added to it anywhere
template <typename T, typename C = T>
inline CovSrc<T, C> cov_src(const KmatSrc& s) {
    return {(const T*)s.Xs, (const T*)s.Cp, s.n_pool, s.kernel, (C)s.outputscale, (C)(s.Cp ? 0.0 : s.noise)};
}
// f(the typed source): a CovSrc, a CovSrcAdd under the additive form, a CovSrcRel under the relationship form or a CovSrcSep under
// the separable form -- the kernel's source type is a template argument, so those three forms run instantiations of their own
template <typename T, typename C = T, typename F>
inline void with_src(const KmatSrc& s, F&& f) {
    if (s.sepf()) {
        CovSrcSep<T, C> a;
        static_cast<CovSrc<T, C>&>(a) = cov_src<T, C>(s);
        a.sep_G = (const T*)s.G; a.sep_Q = s.Q; a.sep_kb = s.kernel_b; a.sep_da = s.da; a.sep_dg = s.dg; a.sep_hasg = s.Q > 0 ? 1 : 0;
        a.sep_parts = s.parts; a.sep_osg = (C)s.outputscale_g;
        f(a);
    } else if (s.rel()) {
        CovSrcRel<T, C> a;
        static_cast<CovSrc<T, C>&>(a) = cov_src<T, C>(s);
        a.G = (const T*)s.G; a.Q = s.Q; a.da = s.da; a.parts = s.parts; a.os_g = (C)s.outputscale_g;
        f(a);
    } else if (s.additive()) {
        CovSrcAdd<T, C> a;
        static_cast<CovSrc<T, C>&>(a) = cov_src<T, C>(s);
        a.kernel_b = s.kernel_b; a.da = s.da; a.parts = s.parts; a.os_b = (C)s.outputscale_b;
        f(a);
    } else {
        f(cov_src<T, C>(s));
    }
}
// The padded coordinate width (2, 4 or 8) as a compile-time constant: f(std::integral_constant<int, DP>{}), one launch line
// per kernel instead of three
template <typename F>
inline void with_dp(int DP, F&& f) {
    if (DP == 2) f(std::integral_constant<int, 2>{});
    else if (DP == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}
// explicit instantiation of a typed launcher for both element types, by name: the signature is the template's own
#define ALGP_INSTANTIATE(f) \
    template decltype(f<double>) f<double>; \
    template decltype(f<float>) f<float>

// The candidates' right-hand sides as a generator instead of a matrix (the scheduled sweep, potrf.hip: trsm_blocked): the update
// product of a column block forms its C tile in registers from these (gemm.hip, GEN), so B^T is never written to V^T and read
// back.  rx / cx: the scaled coordinates of the candidate rows and of the train columns, gathered once per solve (DP per entry,
// zero behind the last row / column); rk: per row -1 (ordinary), the train row of a unit row, -2 (padding).  window(): what the
// sweep cannot generate -- block 0's right-hand sides into its scratch, or all of them into V^T where the scheduled launches
// are not taken after all: columns [c0, c0 + w) of B^T to out (leading dimension ldo), by the kernel-matrix build.
struct RhsGen {
    const void* rx = nullptr;
    const void* cx = nullptr;
    const int* rk = nullptr;
    int64_t ncols = 0;   // N: the columns behind are zero
    int DP = 0, kernel = 0;
    double outputscale = 0;
    int (*window)(algp_ctx* c, int64_t c0, int64_t w, void* out, int64_t ldo) = nullptr;
};
// rx[i] = Xs[ridx[i]] (i < rows), cx[j] = Xs[cidx[j]] (j < cols), zero up to rows_pad / cols_pad; rk from unit (or null) as above
template <typename T>
int rhs_gather_launch(algp_ctx* c, const T* Xs, int DP, const int64_t* ridx, int64_t rows, int64_t rows_pad, const int* unit,
                      const int64_t* cidx, int64_t cols, int64_t cols_pad, T* rx, T* cx, int* rk);
// the scheduled update product D = alpha A B^T + beta C with C generated: C[i][j] = B^T entry (i, col0 + j) of `gen` (gemm.hip)
template <typename T>
int gemm_nt_launch_gen(algp_ctx* c, int klass, int64_t m, int64_t n, int64_t k, T alpha, const T* A, int64_t lda, const T* B,
                       int64_t ldb, T beta, const RhsGen& gen, int64_t col0, T* D, int64_t ldd);
// whether gemm_nt_launch_gen has a kernel for this generator (DP = 2; wider coordinates, the additive and the relationship form
// (additive = true for either) take the materialised route)
bool rhs_gen_supported(int DP, bool pool_is_cov, bool additive = false);

// out[r][c] for r<rows_pad, c<cols_pad (ld = ldo):
//   r<rows && c<cols : value(ridx[r], cidx[c])  [+ diag terms when the pool indices coincide]
//   unit != null && unit[r] >= 0 : (c == unit[r]) ? 1 : 0      (e_j rows of B^T)
//   padding: identity_pad ? (r==c) : 0
template <typename T>
int kmat_launch(algp_ctx* c, const KmatSrc& s, const int64_t* ridx, int64_t rows, int64_t rows_pad,
                const int64_t* cidx, int64_t cols, int64_t cols_pad, const T* diag_add,
                int add_noise_on_equal, const int* unit, int identity_pad, T* out, int64_t ldo,
                int64_t ident_shift = 0, int64_t col_shift = 0);

// plain (non-pool) kernel matrix between two scaled coordinate arrays, for algp_kernel_matrix
template <typename T>
int kmat_xy_launch(algp_ctx* c, const T* xs1, int64_t n1, const T* xs2, int64_t n2, int symmetric,
                   const T* diag_add, double add_noise, T* out, int64_t ldo);
template <typename T>
int scale_coords_launch(algp_ctx* c, const T* x, int64_t n, T* xs);

// One product D = alpha A B^T + beta C of the GEMM tile kernel, described by field name at the call site (designated
// initialisers: gemm_nt<T>(c, {.klass = ..., .m = ..., .A = {X, ldx}, ...})); a field that a call does not use stays unwritten.
// The library is built as C++17, where clang takes designated initialisers as an extension and warns: switched off on purpose
// for every file that includes this header (no push / pop), since the call sites are spread over them.
#pragma clang diagnostic ignored "-Wc++20-designator"
template <typename P>
struct Mat {                       // an operand: element (i, j) of problem b at p[b * stride + i * ld + j]
    P* p = nullptr;
    int64_t ld = 0;
    int64_t stride = 0;
};
template <typename T>
struct GemmNt {
    int klass = 0;                 // ALGP_PROF_* class the launch is booked under
    int64_t m = 0, n = 0, k = 0;
    T alpha = (T)1, beta = (T)0;
    Mat<const T> A, B, C;          // C left null: D, with D's leading dimension and stride (in place; the kernel reads C only
                                   // where beta != 0 and C is not generated)
    Mat<T> D;
    int batch = 1;                 // independent problems, one operand stride apart each (grid.y)
    int lower_only = 0;            // square output, only the tiles on / below the diagonal
    int ktri = 0, kcut = 0;        // GemmArgs::ktri, ::kcut (gemm.hip): the k range of a tile cut by its row / its column tile
    const T* stat_w = nullptr;     // row statistics (gemm_nt_launch_stats below): written where stat_out is set
    T* stat_out = nullptr;
    int64_t stat_ld = 0;
};
template <typename T>
int gemm_nt(algp_ctx* c, const GemmNt<T>& p);
// the BLAS-shaped call of one product
template <typename T>
int gemm_nt_launch(algp_ctx* c, int klass, int64_t m, int64_t n, int64_t k, T alpha, const T* A,
                   int64_t lda, const T* B, int64_t ldb, T beta, const T* C, int64_t ldc, T* D,
                   int64_t ldd, int lower_only);
// D (m x n) = A B^T, B (n x n) lower triangular by 128-tiles (column tile c sums over k < 128 (c + 1)); stat_out or null: the
// row statistics of every column tile written (stat_out[(2 tile + 0 / 1) * stat_ld + row])
template <typename T>
int gemm_nt_launch_tri(algp_ctx* c, int klass, int64_t m, int64_t n, const T* A, int64_t lda, const T* B, int64_t ldb, T* D,
                       int64_t ldd, const T* w, T* stat_out, int64_t stat_ld);
// D = alpha A B^T for ONE column tile (n = 128) and, per output row, the tile's sums of d^2 and of d * w[column] to
// stat_out[row] and stat_out[stat_ld + row] (the candidate solve's last write of a column tile of V^T: its share of the
// variance and the mean without a second pass over V^T)
template <typename T>
int gemm_nt_launch_stats(algp_ctx* c, int klass, int64_t m, int64_t k, T alpha, const T* A, int64_t lda, const T* B, int64_t ldb,
                         T* D, int64_t ldd, const T* w, T* stat_out, int64_t stat_ld);
// variance-reduction criterion: rows [0, mpad) of V^T against its rows [ncol0, ncol0 + n) over the first k columns; per row and
// column tile bn of the launch the sum over the tile's target columns of (kappa_row C(row, j) - V_row . V_j)^2 goes to
// part[bn * part_ld + row]; no matrix is written (gemm.hip)
template <typename T>
int gemm_nt_launch_vr(algp_ctx* c, int klass, int64_t mpad, int64_t n, int64_t k, const T* Vt, int64_t ldv, int64_t ncol0,
                      const KmatSrc& s, const int64_t* cidx, const int* ckind, int64_t M, const T* tw, T* part, int64_t part_ld);
// its rectangular form (the criterion over ranks): rows [0, mpad) of V^T against `nslices` blocks of n gathered rows B (leading
// dimension ldb; slice s starts slice_bytes * s behind B, and its n pool indices -- negative: not a target -- behind cpool by the same
// step) in ONE launch; slice s, column tile bn -> part[(s * n / 128 + bn) * part_ld + row]
template <typename T>
int gemm_nt_launch_vrx(algp_ctx* c, int klass, int64_t mpad, int64_t n, int64_t k, const T* Vt, int64_t ldv, const T* B, int64_t ldb,
                       const int64_t* cpool, int nslices, int64_t slice_bytes, const KmatSrc& s, const int64_t* cidx, const int* ckind,
                       int64_t M, const T* tw, T* part, int64_t part_ld);
// variance reduction of whole paths: E[u][j] = C(uidx[u], cidx[ncol0 + j]) - R_u . V_(ncol0 + j) on the target columns, 0 on the
// others and on the rows behind U; the E tile is written (upad x n, leading dimension lde), nothing else (gemm.hip)
template <typename T>
int gemm_nt_launch_pvr(algp_ctx* c, int klass, int64_t upad, int64_t n, int64_t k, const T* R, int64_t ldr, const T* Vt, int64_t ldv,
                       int64_t ncol0, const KmatSrc& s, const int64_t* uidx, int64_t U, const int64_t* cidx, const int* ckind, int64_t M,
                       const T* tw, T* E, int64_t lde);
// C (m x m, lower tiles) -= X X^T for a short, very wide X (m <= 512 rows, k columns): the k range is cut into
// chunks that run as one batched launch, the partial products are summed in chunk order (deterministic)
template <typename T>
int syrk_skinny_sub(algp_ctx* c, int klass, const T* X, int64_t m, int64_t k, int64_t ldx, T* C, int64_t ldc,
                    algp::DevBuf& scratch);

// factor the NB x NB diagonal block at A (ld = lda) in place, write its inverse (NB x NB, ld NB),
// add sum(log pivot) to *logdet_acc, record first bad pivot (block_row0 + j + 1) in *info (atomicMin style).
template <typename T>
int potrf_diag_launch(algp_ctx* c, T* A, int64_t lda, T* inv_out, double* logdet_acc, int* info,
                      int64_t block_row0);

template <typename T>
int potrf_diag_batched_launch(algp_ctx* c, T* A, int64_t sA, int64_t lda, T* inv_out, int64_t sInv, double* logdet, int* info, int batch);

int comm_unique_id(void* out128, std::string* why);
int comm_init(algp_ctx* c, int nranks, int rank, const void* unique_id128);
void comm_destroy(algp_ctx* c);
int comm_init_host(algp_ctx* c, int nranks, int rank, algp_allgather_fn fn, void* user);
int comm_pick_exchange(algp_ctx* c, const double* val_dev, const int64_t* pos_dev, const int64_t* cidx_dev,
                       const int* fresh_dev, int npicks, int status, double* rec5, const char** winner_payload);
int comm_reserve(algp_ctx* c);
// every rank's `nd` doubles (an agreement word: 4, or more where a protocol compares more), in rank order
int comm_agree(algp_ctx* c, const double* mine, std::vector<double>& all, int nd = 4);
int comm_rows_reserve(algp_ctx* c, size_t bytes_per_rank);
int comm_rows_gather(algp_ctx* c, size_t bytes_per_rank, const size_t* used_bytes = nullptr);
// The status-word protocol of a criterion's state kept over the ranks (api_mi.hip, api_vr.hip): described with these functions
// in comm.hip.  CommState: whose state a collective belongs to (an agreed failure names it and drops it); what: the step's name.
struct CommState {
    const char* name;
    void (*drop)(algp_ctx*);
};
int comm_first_failure(const double* words, int stride, int nranks, int* code);
int comm_agree_checked(algp_ctx* c, const CommState& s, const char* what, const double* mine, std::vector<double>& all, int nd = 4);
int comm_exchange(algp_ctx* c, const CommState& s, const char* what, size_t bytes, int st, const double* v3 = nullptr,
                  std::vector<double>* hdr = nullptr);
int comm_picks_agree(algp_ctx* c, const CommState& s, const char* who, const std::vector<double>& all, int nd, int need_at, bool* any_need);
int comm_fold_status(algp_ctx* c, int st, bool built, const char* state, int64_t q, const char* crit, int* inject);
int comm_catch_up(algp_ctx* c, int64_t rounds, int st, int (*fold)(algp_ctx*, int));
size_t comm_payload_bytes(const algp_ctx* c);
int comm_debug_first_max(algp_ctx* c, const double* triples, int nranks, double* out5);
void dag_release(algp_ctx* c);   // frees the cached task lists of the dependency-driven Cholesky
// Cholesky of the npad x npad matrix A (ld), inverse diagonal blocks to invD (one dependency-driven launch, or the
// blocked right-looking launch sequence for very small / very large matrices)
template <typename T>
int cholesky_blocked(algp_ctx* c, T* A, int64_t npad, int64_t ld, T* invD, double* logdet_acc,
                     int* info);
// Sizes the one-launch task list (chol_dag.hip) serves: the factor's tile count, and the tile rows of a panel carried along
constexpr int64_t DAG_MIN_TILES = 8, DAG_MAX_TILES = 192, DAG_MAX_PANEL_TILES = 400;
bool dag_enabled();       // $ALGP_CHOL_DAG != 0
// The factorisation and P <- P L^-T in one launch (P: mpad rows riding along as extra block rows of the task list;
// mode 1: dense rows, mode 2: P = I of the factor's size -> L^-T); and the same solve against a factor that is final.
template <typename T>
// (mode 2: the identity's nt tile rows may be followed by dense tile rows -- mpad > npad)
int cholesky_dag_panel(algp_ctx* c, T* A, int64_t npad, int64_t ld, T* invD, double* logdet_acc, int* info, T* P, int64_t ldp,
                       int64_t mpad, int mode, int pshort = 0);
template <typename T>
int solve_dag_panel(algp_ctx* c, const T* L, int64_t npad, int64_t ld, const T* invD, int* info, T* P, int64_t ldp, int64_t mpad,
                    int mode, int pshort = 0);
// ---- the blocked triangular solve X <- X L^-T on the GEMM (potrf.hip) ------------------------------------------------------
constexpr int WB = 512;                     // its column block (two-level blocking: potrf.hip)
constexpr int64_t TRSM_PUSH_TILES = 320;    // candidate solves of up to 320 x 128 rows run right-looking (trsm_push)
template <typename T>
struct TrsmOp {                  // the operands
    int klass = 0;               // ALGP_PROF_* class the launches are booked under
    T* X = nullptr;              // mpad x npad, leading dimension ldx: the right-hand sides, solved in place
    int64_t mpad = 0, ldx = 0;
    const T* L = nullptr;        // the factor: npad x npad, leading dimension ldl
    int64_t npad = 0, ldl = 0;
    const T* invD = nullptr;     // the explicit inverses of its 128 x 128 diagonal blocks
};
template <typename T>
struct TrsmStats {               // row statistics (with w and out; out null: none).  Where every row takes the left-looking order
    const T* w = nullptr;        // from column 0 (more than 320 tile rows), the launch that writes a column tile of X for the last
    T* out = nullptr;            // time also leaves the tile's row sums of x^2 and x * w[column] at out[(2 tile + 0 / 1) * ld + row];
    int64_t ld = 0;              // TrsmPlan::stats says whether that happened (else: take them in a pass over X)
};
template <typename T>
struct TrsmOpt {                 // what is optional
    int64_t col_start = 0;       // (multiple of 128): columns [0, col_start) of X already hold the solution
    TrsmStats<T> stats;
    const RhsGen* gen = nullptr; // X does not hold the right-hand sides of columns [0, npad) yet.  The scheduled sweep generates
                                 // them; where it is not taken after all, gen->window writes them into X first
};
// How a solve of this shape runs: decided once, by trsm_plan (allocates nothing, launches nothing; the switches are read per call,
// tests flip them), for trsm_blocked and for the candidate solve's plan (plan_route).
enum class TrsmOrder { Short, Push, LeftLooking };      // trsm_short / trsm_push / trsm_left (potrf.hip)
struct TrsmWants { bool stats = false, gen = false; };  // the caller has row statistics to take / a generator instead of a matrix
struct TrsmPlan {
    TrsmOrder order = TrsmOrder::Short;
    bool main_stream = false;    // enqueued on the context's own stream: helper streams may run beside it
    bool inv512 = false;         // LeftLooking: a full 512-column block is one product with its explicit inverse
    bool sched = false;          // ... and every product a scheduled launch, one after the other on the caller's stream
    bool stats = false;          // the launches leave the row statistics
    bool gen = false;            // the update products generate the right-hand sides (sched only)
    int chunks = 1;              // LeftLooking, not scheduled: row chunks on streams of their own
};
TrsmPlan trsm_plan(const algp_ctx* c, int64_t mpad, int64_t npad, int64_t col_start, TrsmWants wants);
template <typename T>
int trsm_blocked(algp_ctx* c, const TrsmOp<T>& op, const TrsmOpt<T>& opt = {}, TrsmPlan* ran = nullptr);   // *ran: its plan, less what no buffer was had for
// The right-looking step inside a column block [j0, j1), 128 columns at a time: the product with the diagonal inverse over the first
// rows_of(k0) rows (0: the column is skipped), then the push into the block's columns behind.  The short order's, and the L^-T sweeps'.
template <typename T>
int block_solve_right(algp_ctx* c, const TrsmOp<T>& op, int64_t j0, int64_t j1, const std::function<int64_t(int64_t)>& rows_of);
// Slots of algp_ctx::sync_events (sync_event, api.hip).  0 .. 16 are the blocked solve's, 20 and up the API layer's.
enum SyncSlot : size_t {
    EV_CHUNK = 0,                // + k, k < 4: row chunk k of the left-looking order is done (slot 0 first marks their common start)
    EV_PUSH_A = 8, EV_PUSH_B = 9, EV_PUSH_DONE = 16,   // the push order's rings a[J], b[J] (+ 2 (J & 3)); its helper stream has finished
    EV_INV_READY = 20, EV_INV_DONE = 21,   // factor_resident's S^-1 on the helper stream (api_factor.hip; api_fit.hip waits)
};
hipEvent_t sync_event(algp_ctx* c, size_t slot);
// columns [c0, c0 + w) of X <- the solution's new columns after rows c0.. were appended to L (tail.hip): c0 a multiple of 16,
// w <= 64, inside one 128-column block whose explicit inverse is invD_blk; lrows = rows of L that exist
template <typename T>
int tail_cols_launch(algp_ctx* c, int klass, T* X, int64_t mpad, int64_t ldx, const T* L, int64_t ldl, int64_t lrows, const T* invD_blk,
                     int64_t c0, int w, const T* E_window = nullptr);
// X (npad x npad, holding the identity) <- L^-T (upper triangular; zero parts are never touched)
template <typename T>
int trinv_upper(algp_ctx* c, int klass, T* X, int64_t npad, int64_t ldx, const T* L, int64_t ldl, const T* invD);
template <typename T>
int trinv_upper_inplace(algp_ctx* c, int klass, T* XL, int64_t npad, int64_t ld, const T* invD);
// C (lower tiles, npad x npad) <- X X^T for that upper-triangular X
template <typename T>
int syrk_upper(algp_ctx* c, int klass, const T* X, int64_t npad, int64_t ldx, T* C, int64_t ldc);

// b <- L^-1 b (forward) and b <- L^-T b (backward) for one vector of length npad
template <typename T>
int trsv_forward(algp_ctx* c, const T* L, int64_t npad, int64_t ldl, const T* invD, T* b, int64_t kb_start = 0);
template <typename T>
int trsv_forward2(algp_ctx* c, const T* L, int64_t npad, int64_t ldl, const T* invD, T* b0, T* b1, int64_t kb_start = 0);
// u[k:] -= L[k:, 0:k] u[0:k] (and the same for w): resume two forward substitutions at row k
template <typename T>
int tail_gemv2_launch(algp_ctx* c, const T* L, int64_t ldl, int64_t k, int64_t npad, T* u, T* w);
template <typename T>
int trsv_backward(algp_ctx* c, const T* L, int64_t npad, int64_t ldl, const T* invD, T* b);

// row reductions over V^T: ss[j] = sum_r V[j][r]^2 (if ss), dot[j] = sum_r V[j][r]*w[r] (if w)
template <typename T>
int rows_reduce_launch(algp_ctx* c, const T* Vt, int64_t rows, int64_t ldv, int64_t ncols, const T* w, T* ss, T* dot,
                       int64_t tri_c0 = -1);

// ---- joint posterior draws (sample.hip; algp_sample_posterior, api_sample.hip) ----
// Where a launch of the two kernels below leaves the prior draw g of (row, sample s), for one tile of at most 128 samples,
// sample-major: out[s * ld + row], every row < ld and every s < 128 written.
//   candidates (y0 == null): ybar + g for row < nrows, 0 behind
//   train rows: y0[row] - g - sqrt(var[row] + noise) eps[s * ld + row] for row < nrows and s < slive, 0 elsewhere -- the
//   right-hand side R^T of Z^T = R^T L^-T
template <typename T>
struct SampleEpi {
    T* out;
    int64_t ld, nrows;
    int slive;
    T ybar;
    const T* y0;
    const T* var;
    const T* eps;
    T noise;
};
constexpr int SAMPLE_TILE = 128;   // samples per pass
constexpr int SAMPLE_KT = 32;      // features per staged k-tile: F is padded to it with zero weights
// g[row][s] = scale sum_f cos(Xs[idx[row]] . om[f] + ph[f]) Wt[f][s] on the matrix cores, the A operand generated in registers;
// om: Fpad x DP, ph: Fpad, Wt: Fpad x 128 (feature-major, zero behind F and behind the live samples); flop_f: the true F
template <typename T>
int sample_features_launch(algp_ctx* c, const T* Xs, int DP, const int64_t* idx, const T* Wt, const T* om, const T* ph,
                           int64_t Fpad, int64_t flop_f, T scale, const SampleEpi<T>& e);
// g[row][s] = prior[s * n_pool + idx[row]] (prior: 128 x n_pool, zero rows behind the live samples)
template <typename T>
int sample_values_launch(algp_ctx* c, const T* prior, int64_t n_pool, const int64_t* idx, const SampleEpi<T>& e);
// dst (rows_pad x cols_pad, leading dimension ldd; transposed: cols_pad x rows_pad) = src (rows x cols doubles), zero padded
template <typename T>
int sample_convert_launch(algp_ctx* c, const double* src, int64_t rows, int64_t cols, T* dst, int64_t rows_pad, int64_t cols_pad,
                          int64_t ldd, int transposed);

template <typename T>
int test_mfma_launch(algp_ctx* c, int* mismatches_dev);
template <typename T>
int bench_gemm(algp_ctx* c, int64_t m, int64_t n, int64_t k, int lower_only, int beta_one, int reps,
               double* ms_out, bool gen_c = false);
// the rank-p fold on a rows x cols matrix beside a device-to-device copy of it (fold_ms, copy_ms; both or neither), the posterior
// pass over a rows x cols panel with a zero basis row (panel_ms, or null): average ms per launch (fixed.hip)
template <typename T>
int bench_fixed(algp_ctx* c, int64_t rows, int64_t cols, int p, int reps, double* fold_ms, double* copy_ms, double* panel_ms);

}  // namespace algp
