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

// FAM: the family of `kernel` (kernel_family, common.h): one copy of the kernel per family
template <typename T, int DP, int FAM>
__global__ __launch_bounds__(256) void mll_grad_kernel(const T* Sinv, int64_t ld, int64_t N, const T* Xs,
                                                       const int64_t* aidx, const T* alpha, int kernel, T os,
                                                       int repeats /* a pool site occurs in more than one row */,
                                                       double* partial /* per workgroup: [0]=os, [1]=noise trace, [2..2+DP) = ls */) {
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
    double g_os = 0, g_tr = 0, g_ls[DP];
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
        T sv[16];                                                // this thread's 16 entries of S^-1, loaded up front
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int64_t i = (int64_t)bi * 64 + ty * 16 + rr;
            sv[rr] = (i < N && j <= i) ? Sinv[i * ld + j] : (T)0;
        }
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int li = ty * 16 + rr;
            const int64_t i = (int64_t)bi * 64 + li;
            if (i >= N || j > i) continue;
            T u2[DP], r2 = (T)0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const T df = s_x[li][d] - xj[d];
                u2[d] = df * df;
                r2 += u2[d];
            }
            const T w = s_a[li] * aj - sv[rr];
            const double m = (i == j) ? 1.0 : 2.0;               // symmetric: off-diagonal pairs count twice
            T dk;                                                // dk * u_d^2 = dK/dlog ls_d (kdk, common.h; 0 at r = 0 for nu = 1/2)
            const T kv = kdk<T, FAM>(kernel, os, r2, dk);
            g_os += m * (double)(w * kv);
            if (i == j) g_tr += (double)w;
            else if (repeats && s_p[li] == pj) g_tr += 2.0 * (double)w;   // a second row of the same site: S_ij holds sigma_n^2 too
#pragma unroll
            for (int d = 0; d < DP; ++d) g_ls[d] += m * (double)(w * dk * u2[d]);
        }
    }
    // block reduction: wave shuffles, LDS across the 4 waves, then one partial per block and quantity (summed in fixed
    // order by mll_grad_reduce_kernel: the gradient, and with it a whole fit trajectory, is the same in every run)
    auto wsum = [](double v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        return v;
    };
    __shared__ double s_red[4][2 + DP];
    g_os = wsum(g_os);
    g_tr = wsum(g_tr);
#pragma unroll
    for (int d = 0; d < DP; ++d) g_ls[d] = wsum(g_ls[d]);
    if (tx == 0) {
        s_red[ty][0] = g_os;
        s_red[ty][1] = g_tr;
#pragma unroll
        for (int d = 0; d < DP; ++d) s_red[ty][2 + d] = g_ls[d];
    }
    __syncthreads();
    if (threadIdx.x < 2 + DP)
        partial[(int64_t)blockIdx.x * (2 + DP) + threadIdx.x] =
            (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}

// The additive kernel (common.h: family 2), a kernel of its own beside the two copies above: S = os_a kappa_a(r_a) + os_b kappa_b(r_b)
// + ..., so dS/dlog os_a = K_a, dS/dlog os_b = K_b, and dS/dlog ls_d = dk_c u_d^2 with c the part that owns coordinate d (d < da: a).
// Two kdk values per pair, from the two squared distances of split_r2's rule (each square rounded on its own, added in
// coordinate order).  Per workgroup: [0] = os_a, [1] = os_b, [2] = noise trace, [3..3+DP) = ls -- 11 sums at most.  The same
// tiles, staging and fixed-order reduction as mll_grad_kernel.
template <typename T, int DP>
__global__ __launch_bounds__(256) void mll_grad_add_kernel(const T* Sinv, int64_t ld, int64_t N, const T* Xs, const int64_t* aidx,
                                                           const T* alpha, int kernel_a, T os_a, int kernel_b, T os_b, int da,
                                                           int repeats, double* partial) {
#pragma clang fp contract(off)
    int bi = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((int64_t)(bi + 1) * (bi + 2) / 2 <= (int64_t)blockIdx.x) ++bi;
    while ((int64_t)bi * (bi + 1) / 2 > (int64_t)blockIdx.x) --bi;
    const int bj = (int)(blockIdx.x - (int64_t)bi * (bi + 1) / 2);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
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
    double g_osa = 0, g_osb = 0, g_tr = 0, g_ls[DP];
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
        for (int rr = 0; rr < 16; ++rr) {
            const int li = ty * 16 + rr;
            const int64_t i = (int64_t)bi * 64 + li;
            if (i >= N || j > i) continue;
            T u2[DP], ra = (T)0, rb = (T)0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const T df = s_x[li][d] - xj[d];
                u2[d] = df * df;
                ra += d < da ? u2[d] : (T)0;
                rb += d < da ? (T)0 : u2[d];
            }
            const T w = s_a[li] * aj - Sinv[i * ld + j];
            const double m = (i == j) ? 1.0 : 2.0;
            T dka, dkb;
            const T ka = kdk<T>(kernel_a, os_a, ra, dka);
            const T kb = kdk<T>(kernel_b, os_b, rb, dkb);
            g_osa += m * (double)(w * ka);
            g_osb += m * (double)(w * kb);
            if (i == j) g_tr += (double)w;
            else if (repeats && s_p[li] == pj) g_tr += 2.0 * (double)w;
#pragma unroll
            for (int d = 0; d < DP; ++d) g_ls[d] += m * (double)(w * (d < da ? dka : dkb) * u2[d]);
        }
    }
    auto wsum = [](double v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        return v;
    };
    __shared__ double s_red[4][3 + DP];
    g_osa = wsum(g_osa);
    g_osb = wsum(g_osb);
    g_tr = wsum(g_tr);
#pragma unroll
    for (int d = 0; d < DP; ++d) g_ls[d] = wsum(g_ls[d]);
    if (tx == 0) {
        s_red[ty][0] = g_osa;
        s_red[ty][1] = g_osb;
        s_red[ty][2] = g_tr;
#pragma unroll
        for (int d = 0; d < DP; ++d) s_red[ty][3 + d] = g_ls[d];
    }
    __syncthreads();
    if (threadIdx.x < 3 + DP)
        partial[(int64_t)blockIdx.x * (3 + DP) + threadIdx.x] =
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

template <typename T>
int mll_grad_launch(algp_ctx* c, const T* Sinv, int64_t ld, int64_t N, const T* Xs, int DP, const int64_t* aidx,
                    const T* alpha, int kernel, T os, double* out_dev, double* partial) {
    if (N <= 0) return ALGP_OK;
    const int rp = c->train_has_repeats ? 1 : 0;
    const unsigned nb = (unsigned)((N + 63) / 64);
    ProfScope ps(c, ALGP_PROF_KMAT, 0.5 * (double)N * N * (3.0 * DP + 8.0), sizeof(T) * 0.5 * (double)N * N);
    dim3 grid(nb * (nb + 1) / 2), blk(256);
    auto launch = [&](auto fam) {
        constexpr int FAM = decltype(fam)::value;
        with_dp(DP, [&](auto dp) {
            hipLaunchKernelGGL((mll_grad_kernel<T, decltype(dp)::value, FAM>), grid, blk, 0, c->cur, Sinv, ld, N, Xs, aidx, alpha, kernel, os,
                               rp, partial);
        });
    };
    if (kernel_family(kernel)) launch(std::integral_constant<int, 1>{});
    else launch(std::integral_constant<int, 0>{});
    ALGP_HIP(hipGetLastError());
    hipLaunchKernelGGL(mll_grad_reduce_kernel, dim3(1), dim3(256), 0, c->cur, partial, (int64_t)grid.x, 2 + DP, out_dev);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mll_grad_launch);

// the additive kernel's: out_dev[0] = os_a, [1] = os_b, [2] = noise trace, [3..3+DP) = ls
template <typename T>
int mll_grad_add_launch(algp_ctx* c, const T* Sinv, int64_t ld, int64_t N, const T* Xs, int DP, const int64_t* aidx, const T* alpha,
                        int kernel_a, T os_a, int kernel_b, T os_b, int da, double* out_dev, double* partial) {
    if (N <= 0) return ALGP_OK;
    const int rp = c->train_has_repeats ? 1 : 0;
    const unsigned nb = (unsigned)((N + 63) / 64);
    ProfScope ps(c, ALGP_PROF_KMAT, 0.5 * (double)N * N * (3.0 * DP + 16.0), sizeof(T) * 0.5 * (double)N * N);
    dim3 grid(nb * (nb + 1) / 2), blk(256);
    with_dp(DP, [&](auto dp) {
        hipLaunchKernelGGL((mll_grad_add_kernel<T, decltype(dp)::value>), grid, blk, 0, c->cur, Sinv, ld, N, Xs, aidx, alpha, kernel_a, os_a,
                           kernel_b, os_b, da, rp, partial);
    });
    ALGP_HIP(hipGetLastError());
    hipLaunchKernelGGL(mll_grad_reduce_kernel, dim3(1), dim3(256), 0, c->cur, partial, (int64_t)grid.x, 3 + DP, out_dev);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mll_grad_add_launch);

// The relationship kernel (common.h: family 3), a third gradient kernel: S = os_a kappa_a(r_a) + os_g G[g_i, g_j] + ..., so
// dS/dlog os_a = K_a, dS/dlog os_g = os_g G[g_i, g_j] (the part's value as kval_rel rounds it), and dS/dlog ls_d = dk_a u_d^2 for
// the spatial coordinates d < da; the id's coordinate has no lengthscale (its sum stays 0 and is not returned).  r_a^2 by
// rel_r2's rule.  Per workgroup: [0] = os_a, [1] = os_g, [2] = noise trace, [3..3+DP) = ls.  The same tiles, staging and
// fixed-order reduction as mll_grad_kernel; the table entry is one gather per pair.
template <typename T, int DP>
__global__ __launch_bounds__(256) void mll_grad_rel_kernel(const T* Sinv, int64_t ld, int64_t N, const T* Xs, const int64_t* aidx,
                                                           const T* alpha, int kernel_a, T os_a, const T* G, int64_t Q, T os_g, int da,
                                                           int repeats, double* partial) {
#pragma clang fp contract(off)
    int bi = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((int64_t)(bi + 1) * (bi + 2) / 2 <= (int64_t)blockIdx.x) ++bi;
    while ((int64_t)bi * (bi + 1) / 2 > (int64_t)blockIdx.x) --bi;
    const int bj = (int)(blockIdx.x - (int64_t)bi * (bi + 1) / 2);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
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
    double g_osa = 0, g_osg = 0, g_tr = 0, g_ls[DP];
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
        for (int rr = 0; rr < 16; ++rr) {
            const int li = ty * 16 + rr;
            const int64_t i = (int64_t)bi * 64 + li;
            if (i >= N || j > i) continue;
            T u2[DP], ra = (T)0, gi = (T)0, gj = (T)0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const T xi = s_x[li][d];
                const T df = xi - xj[d];
                u2[d] = df * df;
                ra += d < da ? u2[d] : (T)0;
                gi = d == da ? xi : gi;
                gj = d == da ? xj[d] : gj;
            }
            const int64_t ia = (int64_t)gi, ib = (int64_t)gj;
            const T w = s_a[li] * aj - Sinv[i * ld + j];
            const double m = (i == j) ? 1.0 : 2.0;
            T dka;
            const T ka = kdk<T>(kernel_a, os_a, ra, dka);
            const T kg = os_g * (G ? G[ia * Q + ib] : (ia == ib ? (T)1 : (T)0));
            g_osa += m * (double)(w * ka);
            g_osg += m * (double)(w * kg);
            if (i == j) g_tr += (double)w;
            else if (repeats && s_p[li] == pj) g_tr += 2.0 * (double)w;
#pragma unroll
            for (int d = 0; d < DP; ++d) g_ls[d] += d < da ? m * (double)(w * dka * u2[d]) : 0.0;
        }
    }
    auto wsum = [](double v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        return v;
    };
    __shared__ double s_red[4][3 + DP];
    g_osa = wsum(g_osa);
    g_osg = wsum(g_osg);
    g_tr = wsum(g_tr);
#pragma unroll
    for (int d = 0; d < DP; ++d) g_ls[d] = wsum(g_ls[d]);
    if (tx == 0) {
        s_red[ty][0] = g_osa;
        s_red[ty][1] = g_osg;
        s_red[ty][2] = g_tr;
#pragma unroll
        for (int d = 0; d < DP; ++d) s_red[ty][3 + d] = g_ls[d];
    }
    __syncthreads();
    if (threadIdx.x < 3 + DP)
        partial[(int64_t)blockIdx.x * (3 + DP) + threadIdx.x] =
            (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}

// the relationship kernel's: out_dev[0] = os_a, [1] = os_g, [2] = noise trace, [3..3+DP) = ls (zero from the id's coordinate on)
template <typename T>
int mll_grad_rel_launch(algp_ctx* c, const T* Sinv, int64_t ld, int64_t N, const T* Xs, int DP, const int64_t* aidx, const T* alpha,
                        int kernel_a, T os_a, const T* G, int64_t Q, T os_g, int da, double* out_dev, double* partial) {
    if (N <= 0) return ALGP_OK;
    const int rp = c->train_has_repeats ? 1 : 0;
    const unsigned nb = (unsigned)((N + 63) / 64);
    ProfScope ps(c, ALGP_PROF_KMAT, 0.5 * (double)N * N * (3.0 * DP + 10.0), sizeof(T) * (double)N * N);
    dim3 grid(nb * (nb + 1) / 2), blk(256);
    with_dp(DP, [&](auto dp) {
        hipLaunchKernelGGL((mll_grad_rel_kernel<T, decltype(dp)::value>), grid, blk, 0, c->cur, Sinv, ld, N, Xs, aidx, alpha, kernel_a, os_a,
                           G, Q, os_g, da, rp, partial);
    });
    ALGP_HIP(hipGetLastError());
    hipLaunchKernelGGL(mll_grad_reduce_kernel, dim3(1), dim3(256), 0, c->cur, partial, (int64_t)grid.x, 3 + DP, out_dev);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mll_grad_rel_launch);

// ---------------------------------------------------------------------------------------------
// The relationship form's gathers from its table (algp_genotype_posterior's B, the per-site prior of the candidates).
// ---------------------------------------------------------------------------------------------
// B[q][i] = os_g G[q, g_i] for q < Q and train row i < N (g_i: the id in coordinate da of the row's pool site), zero in the
// padding up to Qpad x Npad: the right-hand sides of the genotype posterior.  The product rounds as kval_rel's does.
template <typename T>
__global__ __launch_bounds__(256) void rel_gather_b_kernel(const T* G, int64_t Q, T os_g, const T* Xs, int DP, int da, const int64_t* aidx,
                                                           int64_t N, int64_t Qpad, int64_t Npad, T* B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t q = blockIdx.y;
    if (i >= Npad) return;
    T v = (T)0;
    if (q < Q && i < N) {
        const int64_t gi = (int64_t)Xs[aidx[i] * DP + da];
        v = os_g * (G ? G[q * Q + gi] : (q == gi ? (T)1 : (T)0));
    }
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
    const T vg = os_g * (G ? G[g * Q + g] : (T)1);
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
// The product os_g G rounds as kval_rel's does.
template <typename T>
__global__ __launch_bounds__(256) void rel_cov_finish_kernel(const T* G, int64_t Q, T os_g, const T* WW, int64_t ldw, T* cov) {
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (q > p || p >= Q) return;
    const T pr = os_g * (G ? G[p * Q + q] : (p == q ? (T)1 : (T)0));
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
    const T pr = os_g * (G ? G[q * Q + q] : (T)1);
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
