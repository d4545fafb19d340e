// fit_ai.hip -- the average-information matrix of the MLL (Gilmour, Thompson & Cullis 1995), the curvature AI-REML iterates on:
//
//   AI_ab = 1/2 alpha' dS/dtheta_a S^-1 dS/dtheta_b alpha = 1/2 (L^-1 u_a) . (L^-1 u_b),   u_a = dS/dtheta_a alpha
//
// with theta the log hyper-parameters in the gradient's order (fit.hip) and dS/dtheta per pair what fit.hip's header lists.  S
// and its derivatives are never formed: one pass over the N^2 pairs builds the P <= 11 vectors u_a as the rows of a P x Npad
// panel U (mll_ai_u_kernel), the blocked solve turns it into V = U L^-T against the resident factor (api_fit.hip), and the P x P
// Gram product of V's rows is the matrix (mll_ai_gram_kernel): N^2 P work beside the N^3 of the fit step.
// No floating-point atomics: a row's sum and a Gram entry's sum each have one order, so two calls return the same bits.
#include "common.h"

namespace algp {

// ---------------------------------------------------------------------------------------------
// What a kernel form says about one pair of rows (i, j) here: kv[q] = dS_ij/dlog os_q, dk[d] = the lengthscale factor of the part
// that owns coordinate d (dS_ij/dlog ls_d = dk[d] u2[d]), u2[d] = u_d^2.  The forms of the gradient kernel (GradSingle, GradAdd,
// GradRel in fit.hip) without the weight W_ij and with the same rounding rule per family: the single forms with contraction on
// (the squared distance a running fused sum), the two-part forms with it off (split_r2's and rel_r2's squares, each rounded on
// its own) -- the distances and kernel values are the ones the matrix build and the gradient see.
//   NOS          the number of outputscales
//   PAIR_FLOPS   the profile's accounting: flops per pair beyond 3 DP for the distances and 2 per sum
// ---------------------------------------------------------------------------------------------
template <typename T, int FAM>
struct AiSingle {
    static constexpr int NOS = 1;
    static constexpr double PAIR_FLOPS = 8.0;
    int kernel;
    T os;
    template <int DP>
    __device__ __forceinline__ void pair(const T (&xi)[DP], const T (&xj)[DP], T (&kv)[NOS], T (&dk)[DP], T (&u2)[DP]) const {
        T r2 = (T)0;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xi[d] - xj[d];
            u2[d] = df * df;
            r2 += u2[d];
        }
        T k1;                                                    // 0 at r = 0 for nu = 1/2
        kv[0] = kdk<T, FAM>(kernel, os, r2, k1);
#pragma unroll
        for (int d = 0; d < DP; ++d) dk[d] = k1;
    }
};

// The additive kernel: dS/dlog os_a = K_a, dS/dlog os_b = K_b, and coordinate d belongs to part a where d < da
template <typename T>
struct AiAdd {
    static constexpr int NOS = 2;
    static constexpr double PAIR_FLOPS = 16.0;
    int kernel_a;
    T os_a;
    int kernel_b;
    T os_b;
    int da;
    template <int DP>
    __device__ __forceinline__ void pair(const T (&xi)[DP], const T (&xj)[DP], T (&kv)[NOS], T (&dk)[DP], T (&u2)[DP]) const {
#pragma clang fp contract(off)
        T ra, rb, dka, dkb;
        split_r2<DP>(&xi[0], &xj[0], da, ra, rb);
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xi[d] - xj[d];
            u2[d] = df * df;                                     // the squares split_r2 has just summed
        }
        kv[0] = kdk<T>(kernel_a, os_a, ra, dka);
        kv[1] = kdk<T>(kernel_b, os_b, rb, dkb);
#pragma unroll
        for (int d = 0; d < DP; ++d) dk[d] = d < da ? dka : dkb;
    }
};

// The relationship kernel: dS/dlog os_a = K_a, dS/dlog os_g = os_g G[g_i, g_j] (rel_entry), and only the spatial coordinates
// d < da have a lengthscale: the id's coordinate and the padding get the factor 0 (their rows of U are not written at all)
template <typename T>
struct AiRel {
    static constexpr int NOS = 2;
    static constexpr double PAIR_FLOPS = 10.0;
    int kernel_a;
    T os_a;
    const T* G;
    int64_t Q;
    T os_g;
    int da;
    template <int DP>
    __device__ __forceinline__ void pair(const T (&xi)[DP], const T (&xj)[DP], T (&kv)[NOS], T (&dk)[DP], T (&u2)[DP]) const {
#pragma clang fp contract(off)
        T ra, dka;
        int64_t ia, ib;
        rel_r2<DP>(&xi[0], &xj[0], da, ra, ia, ib);
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xi[d] - xj[d];
            u2[d] = df * df;                                     // the squares rel_r2 has just summed
        }
        kv[0] = kdk<T>(kernel_a, os_a, ra, dka);
        kv[1] = rel_entry<T>(G, Q, os_g, ia, ib);
#pragma unroll
        for (int d = 0; d < DP; ++d) dk[d] = d < da ? dka : (T)0;
    }
};

// The separable kernel: GradSep's terms (fit.hip) without the weight -- dS/dlog os = os kappa_a kappa_b, dS/dlog os_g = os_g G where
// the genotype term is there (NOS_ = 2), the lengthscale factors os kappa_b dk_a | os kappa_a dk_b by the part that owns the
// coordinate, 0 for the id and the padding
template <typename T, int NOS_>
struct AiSep {
    static constexpr int NOS = NOS_;
    static constexpr double PAIR_FLOPS = 20.0;
    int kernel_a, kernel_b;
    T os;
    const T* G;
    int64_t Q;
    T os_g;
    int da, dg;
    template <int DP>
    __device__ __forceinline__ void pair(const T (&xi)[DP], const T (&xj)[DP], T (&kv)[NOS], T (&dk)[DP], T (&u2)[DP]) const {
#pragma clang fp contract(off)
        T ra, rb, dka, dkb;
        int64_t ia = 0, ib = 0;
        int sa = da, sg = dg;
        // The 2 DP tests of a coordinate against the split are uniform and invariant in the kernel's loop over columns: hoisted
        // out of it each holds an SGPR pair across it, and with the genotype term at DP = 8 the fp32 kernel spilled SGPRs to
        // scratch.  There they are formed where they are used instead, on the otherwise idle scalar unit (the column loop of
        // those two instantiations then stays rolled: the compiler says so).
        if constexpr (DP == 8 && NOS == 2) asm volatile("" : "+s"(sa), "+s"(sg));
        if constexpr (NOS == 2) sep_r2<DP>(&xi[0], &xj[0], sa, sg, ra, rb, ia, ib);
        else split_r2<DP>(&xi[0], &xj[0], sa, ra, rb);            // no id: sep_r2's sums with dg behind the last coordinate
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const T df = xi[d] - xj[d];
            u2[d] = df * df;                                     // the squares sep_r2 has just summed
        }
        const T fa = kdk<T>(kernel_a, (T)1, ra, dka);
        const T fb = kdk<T>(kernel_b, (T)1, rb, dkb);
        kv[0] = sep_prod<T>(os, fa, fb);
        if constexpr (NOS == 2) kv[1] = rel_entry<T>(G, Q, os_g, ia, ib);
        const T ga = sep_prod<T>(os, dka, fb), gb = sep_prod<T>(os, fa, dkb);
#pragma unroll
        for (int d = 0; d < DP; ++d) dk[d] = d < sa ? ga : ((NOS == 2 && d == sg) ? (T)0 : gb);   // (the padding's u2 is 0)
    }
};

// U[a][i] = sum_j (dS/dtheta_a)_ij alpha_j for the rows i of one 64-row group, a in the gradient's order: [0, nl) the
// lengthscales, [nl, nl + NOS) the outputscales, [nl + NOS] the noise (sigma_n^2 times the alpha of every row of i's pool site).
// One workgroup owns 64 rows: thread (lane, wave) holds row 64 b + lane's coordinates in registers and walks the columns in tiles
// of 64 staged in LDS (coordinates, alpha, pool index; coalesced loads by all 256 threads), wave w taking columns [16 w, 16 w + 16)
// of every tile -- every lane of a wave reads the same LDS address, a broadcast.  Each thread keeps NOS + 1 + DP running sums in
// double; the four waves' sums of a row are combined through LDS as (w0 + w1) + (w2 + w3).  Rows >= N are written as zeros
// (the grid covers [0, Npad)); the lengthscale slots d >= nl (padding, the relationship form's id) are not rows of U.
template <typename T, int DP, typename Form>
__global__ __launch_bounds__(256) void mll_ai_u_kernel(int64_t N, int64_t Npad, const T* Xs, const int64_t* aidx, const T* alpha, Form f,
                                                      int repeats /* a pool site occurs in more than one row */, int nl, T noise, T* U) {
    constexpr int NOS = Form::NOS, NQ = NOS + 1 + DP;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    __shared__ T s_x[64][DP];
    __shared__ T s_a[64];
    __shared__ int64_t s_p[64];
    __shared__ double s_red[3][NQ][64];
    T xi[DP];
    int64_t pi = -1;
#pragma unroll
    for (int d = 0; d < DP; ++d) xi[d] = (T)0;
    if (i < N) {
        pi = aidx[i];
#pragma unroll
        for (int d = 0; d < DP; ++d) xi[d] = Xs[pi * DP + d];
    }
    double a_os[NOS], a_n = 0, a_ls[DP];
#pragma unroll
    for (int q = 0; q < NOS; ++q) a_os[q] = 0;
#pragma unroll
    for (int d = 0; d < DP; ++d) a_ls[d] = 0;
    for (int64_t j0 = 0; j0 < N; j0 += 64) {
        __syncthreads();                                         // the tile before has been read by every wave
        for (int e = threadIdx.x; e < 64 * DP; e += 256) {
            const int cj = e / DP, d = e - cj * DP;
            const int64_t j = j0 + cj;
            s_x[cj][d] = j < N ? Xs[aidx[j] * DP + d] : (T)0;
        }
        if (threadIdx.x < 64) {
            const int64_t j = j0 + threadIdx.x;
            s_a[threadIdx.x] = j < N ? alpha[j] : (T)0;
            s_p[threadIdx.x] = j < N ? aidx[j] : (int64_t)-2;
        }
        __syncthreads();
#pragma unroll 4
        for (int jj = 0; jj < 16; ++jj) {
            const int lj = wv * 16 + jj;                         // the same column in every lane of the wave
            const int64_t j = j0 + lj;
            if (j >= N) break;
            T kv[NOS], dk[DP], u2[DP];
            f.template pair<DP>(xi, s_x[lj], kv, dk, u2);
            const T aj = s_a[lj];
#pragma unroll
            for (int q = 0; q < NOS; ++q) a_os[q] += (double)(kv[q] * aj);
            // the noise's E_ij: the same pool site (the gradient's g_tr rule); without repeats that is the row itself
            const bool same = repeats ? s_p[lj] == pi : j == i;
            a_n += same ? (double)aj : 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) a_ls[d] += (double)((dk[d] * u2[d]) * aj);
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int q = 0; q < NOS; ++q) s_red[wv - 1][q][lane] = a_os[q];
        s_red[wv - 1][NOS][lane] = a_n;
#pragma unroll
        for (int d = 0; d < DP; ++d) s_red[wv - 1][NOS + 1 + d][lane] = a_ls[d];
    }
    __syncthreads();
    if (wv > 0 || i >= Npad) return;
    const bool ok = i < N;
    auto total = [&](double own, int q) { return (own + s_red[0][q][lane]) + (s_red[1][q][lane] + s_red[2][q][lane]); };
#pragma unroll
    for (int q = 0; q < NOS; ++q) U[(int64_t)(nl + q) * Npad + i] = ok ? (T)total(a_os[q], q) : (T)0;
    U[(int64_t)(nl + NOS) * Npad + i] = ok ? noise * (T)total(a_n, NOS) : (T)0;
#pragma unroll
    for (int d = 0; d < DP; ++d)
        if (d < nl) U[(int64_t)d * Npad + i] = ok ? (T)total(a_ls[d], NOS + 1 + d) : (T)0;
}

// U (P x Npad, P = nl + nos + 1 rows in the gradient's order) for the form of `s` (a coordinate pool's source, make_src)
template <typename T>
int mll_ai_u_launch(algp_ctx* c, int64_t N, int64_t Npad, const int64_t* aidx, const T* alpha, const KmatSrc& s, int nl, T* U) {
    if (N <= 0 || Npad <= 0) return ALGP_OK;
    const int rp = c->train_has_repeats ? 1 : 0;
    dim3 grid((unsigned)(Npad / 64)), blk(256);
    auto launch = [&](auto f) -> int {
        using Form = decltype(f);
        const double nq = Form::NOS + 1 + s.DP;
        ProfScope ps(c, ALGP_PROF_KMAT, (double)N * N * (3.0 * s.DP + Form::PAIR_FLOPS + 2.0 * nq), sizeof(T) * (nq - 1.0) * (double)Npad);
        with_dp(s.DP, [&](auto dp) {
            hipLaunchKernelGGL((mll_ai_u_kernel<T, decltype(dp)::value, Form>), grid, blk, 0, c->cur, N, Npad, (const T*)s.Xs, aidx, alpha, f, rp,
                               nl, (T)s.noise, U);
        });
        ALGP_HIP(hipGetLastError());
        return ALGP_OK;
    };
    const T os = (T)s.outputscale;
    if (s.sepf()) {
        if (s.Q > 0) return launch(AiSep<T, 2>{s.kernel, s.kernel_b, os, (const T*)s.G, s.Q, (T)s.outputscale_g, s.da, s.dg});
        return launch(AiSep<T, 1>{s.kernel, s.kernel_b, os, nullptr, 0, (T)0, s.da, s.dg});
    }
    if (s.rel()) return launch(AiRel<T>{s.kernel, os, (const T*)s.G, s.Q, (T)s.outputscale_g, s.da});
    if (s.additive()) return launch(AiAdd<T>{s.kernel, os, s.kernel_b, (T)s.outputscale_b, s.da});
    if (kernel_family(s.kernel)) return launch(AiSingle<T, 1>{s.kernel, os});
    return launch(AiSingle<T, 0>{s.kernel, os});
}
ALGP_INSTANTIATE(mll_ai_u_launch);

// out[a P + b] = out[b P + a] = 1/2 sum_{i < N} V[a][i] V[b][i] for b <= a < P: one workgroup per pair, the products and the sum
// in double, thread-strided then a shuffle tree and the four waves in fixed order; both triangles from the one value
template <typename T>
__global__ __launch_bounds__(256) void mll_ai_gram_kernel(const T* V, int64_t ld, int64_t N, int P, double* out) {
    int a = 0, b = (int)blockIdx.x;
    while (b > a) {
        b -= a + 1;
        ++a;
    }
    const T* va = V + (int64_t)a * ld;
    const T* vb = V + (int64_t)b * ld;
    double v = 0;
    for (int64_t i = threadIdx.x; i < N; i += 256) v += (double)va[i] * (double)vb[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double r = 0.5 * ((part[0] + part[1]) + (part[2] + part[3]));
        out[a * P + b] = r;
        out[b * P + a] = r;
    }
}
template <typename T>
int mll_ai_gram_launch(algp_ctx* c, const T* V, int64_t ld, int64_t N, int P, double* out) {
    if (P <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_GEMM_OTHER, (double)P * (P + 1) * (double)N, sizeof(T) * (double)P * (P + 1) * (double)N);
    hipLaunchKernelGGL(mll_ai_gram_kernel<T>, dim3((unsigned)(P * (P + 1) / 2)), dim3(256), 0, c->cur, V, ld, N, P, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mll_ai_gram_launch);

}  // namespace algp
