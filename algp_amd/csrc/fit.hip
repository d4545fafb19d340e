// fit.hip -- gradient of the exact-GP marginal log likelihood w.r.t. the D+2 log hyper-parameters
// (what gpytorch's autograd computes inside the reference's fit loop, models.py:145-158).
//
//   MLL = -1/2 y0' S^-1 y0 - 1/2 log det S - N/2 log 2pi,   S = K + diag(var) + sigma_n^2 I
//   dMLL/dtheta = 1/2 tr(W dS/dtheta),  W = alpha alpha' - S^-1
//   dS/dlog os = K ; dS/dlog ls_d = dk u_d^2, u_d = (x_d-x'_d)/ls_d, dk = -2 dk/dr^2 (kdk, common.h): K (RBF) | os e^-r / r, 0 where
//   r = 0 (Matern-1/2) | 3 os e^-a, a = sqrt(3) r (Matern-3/2) | 5/3 os (1 + a) e^-a, a = sqrt(5) r (Matern-5/2)
//   dS/dlog sigma_n^2 = sigma_n^2 E,  E_ij = 1 where rows i and j are the same pool site (I unless a site is listed more than
//   once: the kernel matrix gives such rows' cross entries sigma_n^2 too, algp_hip.h at algp_set_train)
// S^-1 = X X' with X = L^-T (trinv_upper + syrk_upper on the MFMA GEMM, both skipping X's zero half:
// N^3/6 + N^3/6 multiply-adds);
// the pairwise reduction below then streams the lower triangle of S^-1 once (HBM-bound, s*N^2/2
// bytes) while K and u_d are recomputed from the scaled coordinates.
#include "common.h"

namespace algp {

// ---------------------------------------------------------------------------------------------
// What a kernel form says about one pair of rows (i, j); the tiling, staging, accumulation and reduction are mll_grad_kernel's.
//   NOS              the number of outputscales, each with a sum of its own
//   pair<DP>         from the row's coordinates and alpha_i (both in LDS), the column's (registers) and s = S^-1_ij: returns the
//                    weight W_ij = alpha_i alpha_j - s and hands back the pair's terms, kv[q] = dS_ij/dlog os_q, dk[d] = the
//                    lengthscale factor of the part that owns coordinate d (dS_ij/dlog ls_d = dk[d] u2[d]), u2[d] = u_d^2.
//                    In this order: the squared distances, the weight, the kernel values.  alpha_i comes by reference so that
//                    its read from LDS stands where the weight is formed: read ahead of the distances it cost the fp32 DP = 8
//                    kernel two VGPRs and a wave, read behind the kernel values (which branch on the form) 1 % of the time at DP = 2
//   SINV_UP_FRONT    a thread's 16 entries of S^-1 are loaded ahead of a fully unrolled row loop (else: read pair by pair in a
//                    rolled one)
//   PAIR_FLOPS, SINV_ELEMS   the profile's accounting: flops per pair beyond 3 DP, elements read per N^2
// The rounding is part of each form and written out in it: the single forms are compiled with contraction on (the squared
// distance a running fused sum, the weight one fused multiply-add), the two-part forms with contraction off (each square and
// the weight's product rounded on their own, split_r2's and rel_r2's rule: the distances the matrix build sees).
// ---------------------------------------------------------------------------------------------
// One kernel of family FAM (kernel_family, common.h): one copy of the gradient kernel per family
template <typename T, int FAM>
struct GradSingle {
    static constexpr int NOS = 1;
    static constexpr bool SINV_UP_FRONT = true;
    static constexpr double PAIR_FLOPS = 8.0, SINV_ELEMS = 0.5;
    int kernel;
    T os;
    template <int DP>
    __device__ __forceinline__ T pair(const T (&xi)[DP], const T (&xj)[DP], const T& ai, T aj, T s, T (&kv)[NOS], T (&dk)[DP], T (&u2)[DP]) const {
        T r2 = (T)0;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xi[d] - xj[d];
            u2[d] = df * df;
            r2 += u2[d];
        }
        const T w = kfma(ai, aj, -s);                            // one fused multiply-add
        T k1;                                                    // 0 at r = 0 for nu = 1/2
        kv[0] = kdk<T, FAM>(kernel, os, r2, k1);
#pragma unroll
        for (int d = 0; d < DP; ++d) dk[d] = k1;
        return w;
    }
};

// The additive kernel (common.h: family 2): S = os_a kappa_a(r_a) + os_b kappa_b(r_b) + ..., so dS/dlog os_a = K_a, dS/dlog os_b
// = K_b, and coordinate d belongs to part a where d < da.  Two kdk values per pair.
template <typename T>
struct GradAdd {
    static constexpr int NOS = 2;
    static constexpr bool SINV_UP_FRONT = false;
    static constexpr double PAIR_FLOPS = 16.0, SINV_ELEMS = 0.5;
    int kernel_a;
    T os_a;
    int kernel_b;
    T os_b;
    int da;
    template <int DP>
    __device__ __forceinline__ T pair(const T (&xi)[DP], const T (&xj)[DP], const T& ai, T aj, T s, T (&kv)[NOS], T (&dk)[DP], T (&u2)[DP]) const {
#pragma clang fp contract(off)
        T ra, rb, dka, dkb;
        split_r2<DP>(&xi[0], &xj[0], da, ra, rb);
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xi[d] - xj[d];
            u2[d] = df * df;                                     // the squares split_r2 has just summed
        }
        const T aa = ai * aj;                                    // a rounded product, then the difference
        const T w = aa - s;
        kv[0] = kdk<T>(kernel_a, os_a, ra, dka);
        kv[1] = kdk<T>(kernel_b, os_b, rb, dkb);
#pragma unroll
        for (int d = 0; d < DP; ++d) dk[d] = d < da ? dka : dkb;
        return w;
    }
};

// The relationship kernel (common.h: family 3): S = os_a kappa_a(r_a) + os_g G[g_i, g_j] + ..., so dS/dlog os_a = K_a, dS/dlog os_g
// = os_g G[g_i, g_j] (rel_entry: one gather per pair), and only the spatial coordinates d < da have a lengthscale: the id's
// coordinate and the padding get the factor 0, their sums stay 0 and are not returned.
template <typename T>
struct GradRel {
    static constexpr int NOS = 2;
    static constexpr bool SINV_UP_FRONT = false;
    static constexpr double PAIR_FLOPS = 10.0, SINV_ELEMS = 1.0;
    int kernel_a;
    T os_a;
    const T* G;
    int64_t Q;
    T os_g;
    int da;
    template <int DP>
    __device__ __forceinline__ T pair(const T (&xi)[DP], const T (&xj)[DP], const T& ai, T aj, T s, T (&kv)[NOS], T (&dk)[DP], T (&u2)[DP]) const {
#pragma clang fp contract(off)
        T ra, dka;
        int64_t ia, ib;
        rel_r2<DP>(&xi[0], &xj[0], da, ra, ia, ib);
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xi[d] - xj[d];
            u2[d] = df * df;                                     // the squares rel_r2 has just summed
        }
        const T aa = ai * aj;                                    // a rounded product, then the difference
        const T w = aa - s;
        kv[0] = kdk<T>(kernel_a, os_a, ra, dka);
        kv[1] = rel_entry<T>(G, Q, os_g, ia, ib);
#pragma unroll
        for (int d = 0; d < DP; ++d) dk[d] = d < da ? dka : (T)0;
        return w;
    }
};

// The separable kernel (common.h: family 4): S = os kappa_a(r_a) kappa_b(r_b) [+ os_g G[g_i, g_j]] + ..., so dS/dlog os = os kappa_a
// kappa_b (sep_prod: the value the matrix build holds), dS/dlog os_g = os_g G (rel_entry; NOS_ = 2: the genotype term is there),
// and by kdk's factors at outputscale 1 dS/dlog ls_d = (os kappa_b dk_a) u_d^2 for d in part a, (os kappa_a dk_b) u_d^2 in part
// b; the id's coordinate and the padding get the factor 0.
template <typename T, int NOS_>
struct GradSep {
    static constexpr int NOS = NOS_;
    static constexpr bool SINV_UP_FRONT = false;
    static constexpr double PAIR_FLOPS = 20.0, SINV_ELEMS = NOS_ == 2 ? 1.0 : 0.5;
    int kernel_a, kernel_b;
    T os;
    const T* G;
    int64_t Q;
    T os_g;
    int da, dg;
    template <int DP>
    __device__ __forceinline__ T pair(const T (&xi)[DP], const T (&xj)[DP], const T& ai, T aj, T s, T (&kv)[NOS], T (&dk)[DP], T (&u2)[DP]) const {
#pragma clang fp contract(off)
        T ra, rb, dka, dkb;
        int64_t ia = 0, ib = 0;
        const int sa = da, sg = dg;
        if constexpr (NOS == 2) sep_r2<DP>(&xi[0], &xj[0], sa, sg, ra, rb, ia, ib);
        else split_r2<DP>(&xi[0], &xj[0], sa, ra, rb);            // no id: sep_r2's sums with dg behind the last coordinate
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xi[d] - xj[d];
            u2[d] = df * df;                                     // the squares sep_r2 has just summed
        }
        const T aa = ai * aj;                                    // a rounded product, then the difference
        const T w = aa - s;
        const T fa = kdk<T>(kernel_a, (T)1, ra, dka);
        const T fb = kdk<T>(kernel_b, (T)1, rb, dkb);
        kv[0] = sep_prod<T>(os, fa, fb);
        if constexpr (NOS == 2) kv[1] = rel_entry<T>(G, Q, os_g, ia, ib);
        const T ga = sep_prod<T>(os, dka, fb), gb = sep_prod<T>(os, fa, dkb);
#pragma unroll
        for (int d = 0; d < DP; ++d) dk[d] = d < sa ? ga : ((NOS == 2 && d == sg) ? (T)0 : gb);   // (the padding's u2 is 0)
        return w;
    }
};

// Per workgroup, and after the reduction: [0, NOS) = the outputscale sums, [NOS] = the noise trace, [NOS+1, NOS+1+DP) = the
// lengthscale sums -- 11 at most.
template <typename T, int DP, typename Form>
__global__ __launch_bounds__(256) void mll_grad_kernel(const T* Sinv, int64_t ld, int64_t N, const T* Xs, const int64_t* aidx,
                                                       const T* alpha, Form f,
                                                       int repeats /* a pool site occurs in more than one row */, double* partial) {
    constexpr int NOS = Form::NOS, NQ = NOS + 1 + DP;
    // one workgroup = a 64-row x 64-col tile of the lower triangle; the grid enumerates only those
    // (blockIdx.x -> (bi, bj <= bi)).  The 64 rows' coordinates and alpha are staged in LDS once.
    int bi = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((int64_t)(bi + 1) * (bi + 2) / 2 <= (int64_t)blockIdx.x) ++bi;
    while ((int64_t)bi * (bi + 1) / 2 > (int64_t)blockIdx.x) --bi;
    const int bj = (int)(blockIdx.x - (int64_t)bi * (bi + 1) / 2);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // tx: column, ty: 4 row groups of 16
    __shared__ T s_x[64][DP];
    __shared__ T s_a[64];
    __shared__ int64_t s_p[64];
    if (threadIdx.x < 64) {
        const int64_t i = (int64_t)bi * 64 + threadIdx.x;
        const bool ok = i < N;
        const int64_t pi = ok ? aidx[i] : 0;
#pragma unroll
        for (int d = 0; d < DP; ++d) s_x[threadIdx.x][d] = ok ? Xs[pi * DP + d] : (T)0;
        s_a[threadIdx.x] = ok ? alpha[i] : (T)0;
        s_p[threadIdx.x] = ok ? pi : (int64_t)-1;
    }
    const int64_t j = (int64_t)bj * 64 + tx;
    double g_os[NOS], g_tr = 0, g_ls[DP];
#pragma unroll
    for (int q = 0; q < NOS; ++q) g_os[q] = 0;
#pragma unroll
    for (int d = 0; d < DP; ++d) g_ls[d] = 0;
    T xj[DP], aj = (T)0;
    int64_t pj = -2;
#pragma unroll
    for (int d = 0; d < DP; ++d) xj[d] = (T)0;
    if (j < N) {
        pj = aidx[j];
#pragma unroll
        for (int d = 0; d < DP; ++d) xj[d] = Xs[pj * DP + d];
        aj = alpha[j];
    }
    __syncthreads();
    if (j < N) {
        // the rows li = ty * 16 + rr of this thread's column.  Their entries of S^-1 up front and the loop unrolled, or each read
        // where its pair is formed in a rolled loop: by the form.  (One loop with the body written out and the sums in variables
        // of their own: the body as a lambda called from two loops, or the sums as one array, gave the single forms' kernels 3 to
        // 6 % more instructions at DP = 2 -- exec-mask regions and moves -- and as much more time.)
        constexpr int UNROLL = Form::SINV_UP_FRONT ? 16 : 1;
        T sv[UNROLL];
        if constexpr (Form::SINV_UP_FRONT) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int64_t i = (int64_t)bi * 64 + ty * 16 + rr;
                sv[rr] = (i < N && j <= i) ? Sinv[i * ld + j] : (T)0;
            }
        }
#pragma unroll UNROLL
        for (int rr = 0; rr < 16; ++rr) {
            const int li = ty * 16 + rr;
            const int64_t i = (int64_t)bi * 64 + li;
            if (i >= N || j > i) continue;
            T s;
            if constexpr (Form::SINV_UP_FRONT) s = sv[rr];
            else s = Sinv[i * ld + j];
            T kv[NOS], dk[DP], u2[DP];
            const T w = f.template pair<DP>(s_x[li], xj, s_a[li], aj, s, kv, dk, u2);
            // m * x is exact (m = 1 or 2), so the sums are the same doubles with and without contraction
            const double m = (i == j) ? 1.0 : 2.0;               // symmetric: off-diagonal pairs count twice
#pragma unroll
            for (int q = 0; q < NOS; ++q) g_os[q] += m * (double)(w * kv[q]);
            if (i == j) g_tr += (double)w;
            else if (repeats && s_p[li] == pj) g_tr += 2.0 * (double)w;   // a second row of the same site: S_ij holds sigma_n^2 too
#pragma unroll
            for (int d = 0; d < DP; ++d) g_ls[d] += m * (double)((w * dk[d]) * u2[d]);
        }
    }
    // block reduction: wave shuffles, LDS across the 4 waves, then one partial per block and quantity (summed in fixed
    // order by mll_grad_reduce_kernel: the gradient, and with it a whole fit trajectory, is the same in every run)
    __shared__ double s_red[4][NQ];
    auto wsum = [](double v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        return v;
    };
#pragma unroll
    for (int q = 0; q < NOS; ++q) g_os[q] = wsum(g_os[q]);
    g_tr = wsum(g_tr);
#pragma unroll
    for (int d = 0; d < DP; ++d) g_ls[d] = wsum(g_ls[d]);
    if (tx == 0) {
#pragma unroll
        for (int q = 0; q < NOS; ++q) s_red[ty][q] = g_os[q];
        s_red[ty][NOS] = g_tr;
#pragma unroll
        for (int d = 0; d < DP; ++d) s_red[ty][NOS + 1 + d] = g_ls[d];
    }
    __syncthreads();
    if (threadIdx.x < NQ)
        partial[(int64_t)blockIdx.x * NQ + threadIdx.x] =
            (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}

// out[q] += sum over blocks of partial[b][q], q < nq: one workgroup, thread-strided then shuffle tree
__global__ __launch_bounds__(256) void mll_grad_reduce_kernel(const double* partial, int64_t nblocks, int nq, double* out) {
    __shared__ double part[4];
    for (int q = 0; q < nq; ++q) {
        double v = 0;
        for (int64_t b = threadIdx.x; b < nblocks; b += 256) v += partial[b * nq + q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) out[q] += (part[0] + part[1]) + (part[2] + part[3]);
        __syncthreads();
    }
}

// out_dev in the kernel's layout for the form of `s` (a coordinate pool's source, make_src): NOS + 1 + DP doubles
template <typename T>
int mll_grad_launch(algp_ctx* c, const T* Sinv, int64_t ld, int64_t N, const int64_t* aidx, const T* alpha, const KmatSrc& s,
                    double* out_dev, double* partial) {
    if (N <= 0) return ALGP_OK;
    const int rp = c->train_has_repeats ? 1 : 0;
    const unsigned nb = (unsigned)((N + 63) / 64);
    dim3 grid(nb * (nb + 1) / 2), blk(256);
    auto launch = [&](auto f) -> int {
        using Form = decltype(f);
        ProfScope ps(c, ALGP_PROF_KMAT, 0.5 * (double)N * N * (3.0 * s.DP + Form::PAIR_FLOPS), sizeof(T) * Form::SINV_ELEMS * (double)N * N);
        with_dp(s.DP, [&](auto dp) {
            hipLaunchKernelGGL((mll_grad_kernel<T, decltype(dp)::value, Form>), grid, blk, 0, c->cur, Sinv, ld, N, (const T*)s.Xs, aidx, alpha,
                               f, rp, partial);
        });
        ALGP_HIP(hipGetLastError());
        hipLaunchKernelGGL(mll_grad_reduce_kernel, dim3(1), dim3(256), 0, c->cur, partial, (int64_t)grid.x, Form::NOS + 1 + s.DP, out_dev);
        ALGP_HIP(hipGetLastError());
        return ALGP_OK;
    };
    const T os = (T)s.outputscale;
    if (s.sepf()) {
        if (s.Q > 0) return launch(GradSep<T, 2>{s.kernel, s.kernel_b, os, (const T*)s.G, s.Q, (T)s.outputscale_g, s.da, s.dg});
        return launch(GradSep<T, 1>{s.kernel, s.kernel_b, os, nullptr, 0, (T)0, s.da, s.dg});
    }
    if (s.rel()) return launch(GradRel<T>{s.kernel, os, (const T*)s.G, s.Q, (T)s.outputscale_g, s.da});
    if (s.additive()) return launch(GradAdd<T>{s.kernel, os, s.kernel_b, (T)s.outputscale_b, s.da});
    if (kernel_family(s.kernel)) return launch(GradSingle<T, 1>{s.kernel, os});
    return launch(GradSingle<T, 0>{s.kernel, os});
}
ALGP_INSTANTIATE(mll_grad_launch);

// ---------------------------------------------------------------------------------------------
// The relationship form's gathers from its table (algp_genotype_posterior's B, the per-site prior of the candidates).  Every
// product os_g G is rel_entry's (common.h).
// ---------------------------------------------------------------------------------------------
// B[q][i] = os_g G[q, g_i] for q < Q and train row i < N (g_i: the id in coordinate da of the row's pool site), zero in the
// padding up to Qpad x Npad: the right-hand sides of the genotype posterior.
template <typename T>
__global__ __launch_bounds__(256) void rel_gather_b_kernel(const T* G, int64_t Q, T os_g, const T* Xs, int DP, int da, const int64_t* aidx,
                                                           int64_t N, int64_t Qpad, int64_t Npad, T* B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t q = blockIdx.y;
    if (i >= Npad) return;
    T v = (T)0;
    if (q < Q && i < N) v = rel_entry<T>(G, Q, os_g, q, (int64_t)Xs[aidx[i] * DP + da]);
    B[q * Npad + i] = v;
}
template <typename T>
int rel_gather_b_launch(algp_ctx* c, const T* G, int64_t Q, T os_g, const T* Xs, int DP, int da, const int64_t* aidx, int64_t N,
                        int64_t Qpad, int64_t Npad, T* B) {
    if (Qpad <= 0 || Npad <= 0) return ALGP_OK;
    if (Qpad > 65535) return fail(c, ALGP_ERR_BAD_ARG, "genotype_posterior: at most 65408 genotypes");
    ProfScope ps(c, ALGP_PROF_ROWS, (double)Qpad * Npad, sizeof(T) * 2.0 * (double)Qpad * Npad);
    hipLaunchKernelGGL(rel_gather_b_kernel<T>, dim3((unsigned)((Npad + 255) / 256), (unsigned)Qpad), dim3(256), 0, c->cur, G, Q, os_g, Xs, DP,
                       da, aidx, N, Qpad, Npad, B);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(rel_gather_b_launch);

// prior[j] = os_a + os_g G[g_j, g_j] for every pool site j < n: K_jj under the relationship form, where the single forms have one
// scalar.  The value the matrix build gives the diagonal: kappa_a(0) = 1 exactly in all four forms (os_a * 1), then kval_rel's
// product and sum.
template <typename T>
__global__ __launch_bounds__(256) void rel_prior_kernel(const T* G, int64_t Q, T os_a, T os_g, const T* Xs, int DP, int da, int64_t n, T* prior) {
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t g = (int64_t)Xs[j * DP + da];
    const T vg = rel_entry<T>(G, Q, os_g, g, g);
    prior[j] = os_a + vg;
}
template <typename T>
int rel_prior_launch(algp_ctx* c, const T* G, int64_t Q, T os_a, T os_g, const T* Xs, int DP, int da, int64_t n, T* prior) {
    if (n <= 0) return ALGP_OK;
    hipLaunchKernelGGL(rel_prior_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->cur, G, Q, os_a, os_g, Xs, DP, da, n, prior);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(rel_prior_launch);

// cov[p][q] = cov[q][p] = os_g G[p, q] - WW[p][q] for q <= p < Q (WW: the lower tiles of W W^T, leading dimension ldw; null: no
// train rows, nothing is subtracted): the genotype posterior's covariance, both triangles from the one value -- identical bits.
template <typename T>
__global__ __launch_bounds__(256) void rel_cov_finish_kernel(const T* G, int64_t Q, T os_g, const T* WW, int64_t ldw, T* cov) {
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (q > p || p >= Q) return;
    const T pr = rel_entry<T>(G, Q, os_g, p, q);
    const T v = WW ? pr - WW[p * ldw + q] : pr;
    cov[p * Q + q] = v;
    cov[q * Q + p] = v;
}
template <typename T>
int rel_cov_finish_launch(algp_ctx* c, const T* G, int64_t Q, T os_g, const T* WW, int64_t ldw, T* cov) {
    if (Q <= 0) return ALGP_OK;
    if (Q > 65535) return fail(c, ALGP_ERR_BAD_ARG, "genotype_posterior: at most 65408 genotypes");
    ProfScope ps(c, ALGP_PROF_ROWS, (double)Q * Q, sizeof(T) * 2.5 * (double)Q * Q);
    hipLaunchKernelGGL(rel_cov_finish_kernel<T>, dim3((unsigned)((Q + 255) / 256), (unsigned)Q), dim3(256), 0, c->cur, G, Q, os_g, WW, ldw, cov);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(rel_cov_finish_launch);
// var[q] = os_g G[q, q] - ss[q], q < Q (ss: the squared row norms of W, or null)
template <typename T>
__global__ __launch_bounds__(256) void rel_var_finish_kernel(const T* G, int64_t Q, T os_g, const T* ss, T* var) {
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const T pr = rel_entry<T>(G, Q, os_g, q, q);
    var[q] = ss ? pr - ss[q] : pr;
}
template <typename T>
int rel_var_finish_launch(algp_ctx* c, const T* G, int64_t Q, T os_g, const T* ss, T* var) {
    if (Q <= 0) return ALGP_OK;
    hipLaunchKernelGGL(rel_var_finish_kernel<T>, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, c->cur, G, Q, os_g, ss, var);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(rel_var_finish_launch);

}  // namespace algp
