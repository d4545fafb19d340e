// group.hip -- the kernels of algp_group_posterior (api_group.hip): sums over groups of candidate rows, the rows sorted by group
// on the host (GroupSegs, vecops.h).  Three segmented sums share one scheme: the sorted member list is cut into chunks of a
// fixed member count, a workgroup walks one chunk with a running sum that it flushes at every group boundary, and a group that
// lies in one chunk is written where it belongs while the pieces of a group that spans chunks go to a buffer of two slots per
// chunk and are added in chunk order by group_combine_kernel.  No atomics: every sum has one order, whatever the grid.
//   group_ksum_kernel    U[q][j] = sum_{l in q} a_l k(x_j, x_l): the kernel values are never stored (VALU-bound on the exponential)
//   group_rowsum_kernel  T[q][:] = sum_{l in q} a_l V[l][:]: one pass over the labelled rows of V^T, or of mu (HBM-bound)
//   group_colsum_kernel  cov[p][q] = sum_{l in q} a_l X[p][l] (- G[p][q]): the lower triangle, mirrored (HBM-bound; a row of X
//                        stays in the L2 while the groups gather from it)
#include "vecops.h"

namespace algp {

// where the piece of group g inside the chunk [m0, m1) of the member list goes: the group's own row of dst if all of it lies in
// the chunk; else slot 2 ch + 1 of the piece buffer if the group starts in this chunk (its first piece), slot 2 ch if it came
// in from the chunk before (a chunk holds at most one of each)
template <typename T>
__device__ __forceinline__ T* group_piece(const int64_t* off, int g, int64_t ch, int64_t m0, int64_t m1, T* dst, int64_t ld_dst, T* part,
                                          int64_t ld_part) {
    const int64_t b = off[g], e = off[g + 1];
    if (b >= m0 && e <= m1) return dst + (int64_t)g * ld_dst;
    return part + (2 * ch + (b >= m0 ? 1 : 0)) * ld_part;
}

// The pool covariance with the kernel's form a compile-time constant and no explicit covariance: pool_cov's tests of s.kernel
// and s.Cp fold away, and the two rows of a thread run as one straight line (with the form selected per evaluation the 10^10
// evaluations of DESIGN section 5 took 12.0 ms in fp64 instead of 8.7)
template <typename T, int KERNEL>
struct GroupCovSrc {
    static constexpr const T* Cp = nullptr;
    static constexpr int kernel = KERNEL;
    const T* Xs;
    int64_t n_pool;
    T os, noise;
};
// KERNEL = -1: the additive form -- the two forms, the split and part b's outputscale at run time (pool_cov's additive branch)
template <typename T>
struct GroupCovSrc<T, -1> {
    static constexpr const T* Cp = nullptr;
    const T* Xs;
    int64_t n_pool;
    T os, noise;
    int kernel, kernel_b, da, parts;
    T os_b;
};
// KERNEL = -2: the relationship form -- the spatial form, the table and the genotype part's outputscale at run time (pool_cov's
// relationship branch)
template <typename T>
struct GroupCovSrc<T, -2> {
    static constexpr const T* Cp = nullptr;
    const T* Xs;
    int64_t n_pool;
    T os, noise;
    int kernel;
    const T* G;
    int64_t Q;
    int da, parts;
    T os_g;
};
// KERNEL = -3: the separable form -- the two factors' forms, the split, and the genotype term's table and outputscale while
// sep_hasg, at run time (pool_cov's separable branch)
template <typename T>
struct GroupCovSrc<T, -3> {
    static constexpr const T* Cp = nullptr;
    const T* Xs;
    int64_t n_pool;
    T os, noise;
    int kernel;
    const T* sep_G;
    int64_t sep_Q;
    int sep_kb, sep_da, sep_dg, sep_hasg, sep_parts;
    T sep_osg;
};
template <typename F>
inline void with_kernel(int kernel, F&& f) {
    if (kernel == ALGP_KERNEL_RBF) f(std::integral_constant<int, ALGP_KERNEL_RBF>{});
    else if (kernel == ALGP_KERNEL_MATERN15) f(std::integral_constant<int, ALGP_KERNEL_MATERN15>{});
    else if (kernel == ALGP_KERNEL_MATERN05) f(std::integral_constant<int, ALGP_KERNEL_MATERN05>{});
    else f(std::integral_constant<int, ALGP_KERNEL_MATERN25>{});
}

template <typename T, int KERNEL>
struct GroupKsumArgs {
    GroupCovSrc<T, KERNEL> s;
    const int64_t* cidx;
    int64_t M, Mpad;
    GroupSegs<T> g;
    T* U;
    T* part;
};

// A workgroup owns GROUP_KROWS rows j (two per thread, their scaled coordinates in registers) and one chunk of GROUP_CHUNK
// members, staged through LDS in tiles of 256 (coordinates, coefficient, group): per member and row one pool_cov and one fused
// multiply-add; the LDS reads are broadcasts, shared by the thread's two rows.  Rows behind M are written as zeros (U is the C
// operand of a product).
constexpr int GROUP_KROWS = 512;
template <typename T, int DP, int KERNEL>
__global__ __launch_bounds__(256) void group_ksum_kernel(GroupKsumArgs<T, KERNEL> a) {
    constexpr int RPT = GROUP_KROWS / 256;
    __shared__ T sX[256][DP];
    __shared__ T sA[256];
    __shared__ int sG[256];
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * GROUP_KROWS + tid;
    const int64_t ch = blockIdx.y, m0 = ch * GROUP_CHUNK, m1 = m0 + GROUP_CHUNK < a.g.Lm ? m0 + GROUP_CHUNK : a.g.Lm;
    T x[RPT][DP], acc[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int64_t j = j0 + r * 256;
        const bool live = j < a.M;
        const int64_t pj = live ? a.cidx[j] : 0;
#pragma unroll
        for (int d = 0; d < DP; ++d) x[r][d] = live ? a.s.Xs[pj * DP + d] : (T)0;
        acc[r] = (T)0;
    }
    auto flush = [&](int g) {
        T* dst = group_piece(a.g.off, g, ch, m0, m1, a.U, a.Mpad, a.part, a.Mpad);
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int64_t j = j0 + r * 256;
            if (j < a.Mpad) dst[j] = j < a.M ? acc[r] : (T)0;
            acc[r] = (T)0;
        }
    };
    int cur = -1;
    for (int64_t t0 = m0; t0 < m1; t0 += 256) {
        __syncthreads();
        if (t0 + tid < m1) {
            const int64_t pl = a.cidx[a.g.perm[t0 + tid]];
#pragma unroll
            for (int d = 0; d < DP; ++d) sX[tid][d] = a.s.Xs[pl * DP + d];
            sA[tid] = a.g.coef[t0 + tid];
            sG[tid] = a.g.gid[t0 + tid];
        }
        __syncthreads();
        const int nt = (int)(m1 - t0 < 256 ? m1 - t0 : 256);
        for (int t = 0; t < nt; ++t) {
            const int g = __builtin_amdgcn_readfirstlane(sG[t]);   // the same member for every lane: a scalar branch
            if (g != cur) {
                if (cur >= 0) flush(cur);
                cur = g;
            }
            const T al = sA[t];
#pragma unroll
            for (int r = 0; r < RPT; ++r) acc[r] = kfma(al, pool_cov<DP, false>(a.s, 0, 0, x[r], sX[t]), acc[r]);
        }
    }
    if (cur >= 0) flush(cur);
}

// dst[g][i] = the pieces of a group g that spans chunks, added in chunk order (i < width); span: those groups
template <typename T>
__global__ __launch_bounds__(256) void group_combine_kernel(const int* span, const int64_t* off, int64_t chunk, const T* part, int64_t ld_part,
                                                            T* dst, int64_t ld_dst, int64_t width) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= width) return;
    const int g = span[blockIdx.y];
    const int64_t cf = off[g] / chunk, cl = (off[g + 1] - 1) / chunk;
    T s = part[(2 * cf + 1) * ld_part + i];
    for (int64_t ch = cf + 1; ch <= cl; ++ch) s += part[2 * ch * ld_part + i];
    dst[(int64_t)g * ld_dst + i] = s;
}

// the per-row term of the covariance: U[q(l)][l] += a_l extra_var_l, one entry per labelled row
template <typename T>
__global__ void group_diag_kernel(GroupSegs<T> g, const T* extra, T* U, int64_t ldu) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= g.Lm) return;
    const int64_t j = g.perm[m];
    U[(int64_t)g.gid[m] * ldu + j] += g.coef[m] * extra[j];
}

template <typename T>
int group_combine(algp_ctx* c, const GroupSegs<T>& g, const int* span, int nspan, int64_t chunk, const T* part, int64_t ld_part, T* dst,
                  int64_t ld_dst, int64_t width) {
    if (nspan <= 0 || width <= 0) return ALGP_OK;
    if (nspan > 65535) return fail(c, ALGP_ERR_BAD_ARG, "group sums: too many groups span member chunks");
    hipLaunchKernelGGL(group_combine_kernel<T>, dim3((unsigned)((width + 255) / 256), (unsigned)nspan), dim3(256), 0, c->cur, span, g.off,
                       chunk, part, ld_part, dst, ld_dst, width);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}

template <typename T>
int group_ksum_launch(algp_ctx* c, const KmatSrc& s, const int64_t* cidx, int64_t M, int64_t Mpad, const T* extra, const GroupSegs<T>& g,
                      const int* span, int nspan, T* U, T* part) {
    if (g.Lm <= 0 || Mpad <= 0) return ALGP_OK;
    const int64_t nch = (g.Lm + GROUP_CHUNK - 1) / GROUP_CHUNK;
    if (nch > 65535 || s.Cp) return fail(c, ALGP_ERR_BAD_ARG, "group_ksum: a coordinate pool and at most 65535 member chunks");
    {
        const double evals = (double)M * (double)g.Lm;
        ProfScope ps(c, ALGP_PROF_KMAT, evals * (3.0 * s.DP + 2.0), sizeof(T) * (double)Mpad * (double)(g.Q + 2 * nspan));
        const CovSrc<T> cs = cov_src<T>(s);
        const dim3 grid((unsigned)((Mpad + GROUP_KROWS - 1) / GROUP_KROWS), (unsigned)nch);
        if (s.sepf()) {
            GroupKsumArgs<T, -3> a = {{cs.Xs, cs.n_pool, cs.os, cs.noise, s.kernel, (const T*)s.G, s.Q, s.kernel_b, s.da, s.dg, s.Q > 0 ? 1 : 0, 3,
                                       (T)s.outputscale_g}, cidx, M, Mpad, g, U, part};
            with_dp(s.DP, [&](auto dp) {
                hipLaunchKernelGGL((group_ksum_kernel<T, decltype(dp)::value, -3>), grid, dim3(256), 0, c->cur, a);
            });
        } else if (s.rel()) {
            GroupKsumArgs<T, -2> a = {{cs.Xs, cs.n_pool, cs.os, cs.noise, s.kernel, (const T*)s.G, s.Q, s.da, 3, (T)s.outputscale_g}, cidx, M, Mpad, g, U, part};
            with_dp(s.DP, [&](auto dp) {
                hipLaunchKernelGGL((group_ksum_kernel<T, decltype(dp)::value, -2>), grid, dim3(256), 0, c->cur, a);
            });
        } else if (s.additive()) {
            GroupKsumArgs<T, -1> a = {{cs.Xs, cs.n_pool, cs.os, cs.noise, s.kernel, s.kernel_b, s.da, 3, (T)s.outputscale_b}, cidx, M, Mpad, g, U, part};
            with_dp(s.DP, [&](auto dp) {
                hipLaunchKernelGGL((group_ksum_kernel<T, decltype(dp)::value, -1>), grid, dim3(256), 0, c->cur, a);
            });
        } else with_kernel(s.kernel, [&](auto kn) {
            constexpr int KERNEL = decltype(kn)::value;
            GroupKsumArgs<T, KERNEL> a = {{cs.Xs, cs.n_pool, cs.os, cs.noise}, cidx, M, Mpad, g, U, part};
            with_dp(s.DP, [&](auto dp) {
                hipLaunchKernelGGL((group_ksum_kernel<T, decltype(dp)::value, KERNEL>), grid, dim3(256), 0, c->cur, a);
            });
        });
        ALGP_HIP(hipGetLastError());
    }
    if (nspan <= 0 && !extra) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_ROWS, (double)Mpad * 2.0 * nspan + 2.0 * g.Lm, sizeof(T) * ((double)Mpad * 3.0 * nspan + 3.0 * g.Lm));
    ALGP_TRY(group_combine<T>(c, g, span, nspan, GROUP_CHUNK, part, Mpad, U, Mpad, Mpad));
    if (extra) {
        hipLaunchKernelGGL(group_diag_kernel<T>, dim3((unsigned)((g.Lm + 255) / 256)), dim3(256), 0, c->cur, g, extra, U, Mpad);
        ALGP_HIP(hipGetLastError());
    }
    return ALGP_OK;
}
ALGP_INSTANTIATE(group_ksum_launch);

// A workgroup owns 256 VEC adjacent columns (VEC per thread: a 16-byte load, or one column) and one chunk of GROUP_ROWCHUNK
// members, whose rows of V it reads once each, coalesced; the member's row, coefficient and group are wave-uniform loads.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void group_rowsum_kernel(const T* V, int64_t ldv, int64_t ncols, GroupSegs<T> g, T* dst, int64_t ld_dst,
                                                           T* part, int64_t ld_part) {
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (c0 >= ncols) return;
    const int64_t ch = blockIdx.y, m0 = ch * GROUP_ROWCHUNK, m1 = m0 + GROUP_ROWCHUNK < g.Lm ? m0 + GROUP_ROWCHUNK : g.Lm;
    vec_t acc;
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = (T)0;
    auto flush = [&](int q) {
        T* d = group_piece(g.off, q, ch, m0, m1, dst, ld_dst, part, ld_part);
        *reinterpret_cast<vec_t*>(d + c0) = acc;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = (T)0;
    };
    int cur = -1;
    for (int64_t m = m0; m < m1; ++m) {
        const int q = g.gid[m];
        if (q != cur) {
            if (cur >= 0) flush(cur);
            cur = q;
        }
        const T al = g.coef[m];
        const vec_t v = *reinterpret_cast<const vec_t*>(V + (int64_t)g.perm[m] * ldv + c0);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = kfma(al, v[e], acc[e]);
    }
    if (cur >= 0) flush(cur);
}

template <typename T>
int group_rowsum_launch(algp_ctx* c, const T* V, int64_t ldv, int64_t ncols, const GroupSegs<T>& g, const int* span, int nspan, T* dst,
                        int64_t ld_dst, T* part, int64_t ld_part) {
    if (g.Lm <= 0 || ncols <= 0) return ALGP_OK;
    constexpr int VEC = 16 / sizeof(T);
    const bool wide = ncols % VEC == 0 && ldv % VEC == 0 && ld_dst % VEC == 0 && ld_part % VEC == 0;
    const int64_t nch = (g.Lm + GROUP_ROWCHUNK - 1) / GROUP_ROWCHUNK;
    if (nch > 65535) return fail(c, ALGP_ERR_BAD_ARG, "group_rowsum: more than 65535 member chunks");
    ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * (double)g.Lm * (double)ncols, sizeof(T) * (double)ncols * ((double)g.Lm + g.Q + 3.0 * nspan));
    const int64_t per = 256 * (wide ? VEC : 1);
    const dim3 grid((unsigned)((ncols + per - 1) / per), (unsigned)nch);
    if (wide) hipLaunchKernelGGL((group_rowsum_kernel<T, VEC>), grid, dim3(256), 0, c->cur, V, ldv, ncols, g, dst, ld_dst, part, ld_part);
    else hipLaunchKernelGGL((group_rowsum_kernel<T, 1>), grid, dim3(256), 0, c->cur, V, ldv, ncols, g, dst, ld_dst, part, ld_part);
    ALGP_HIP(hipGetLastError());
    return group_combine<T>(c, g, span, nspan, GROUP_ROWCHUNK, part, ld_part, dst, ld_dst, ncols);
}
ALGP_INSTANTIATE(group_rowsum_launch);

// One wave per entry (p, q) of the lower triangle: its lanes take the members of group q 64 apart, in ascending order, and
// fold with the shuffle tree -- one order per entry; lane 0 writes the entry and its mirror image, the same bits.
template <typename T>
__global__ __launch_bounds__(256) void group_colsum_kernel(const T* X, int64_t ldx, GroupSegs<T> g, const T* sub, int64_t lds, T* cov) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= g.Q) return;
    const int64_t b = g.off[q], e = g.off[q + 1];
    for (int64_t p = q + blockIdx.y; p < g.Q; p += gridDim.y) {
        const T* row = X + p * ldx;
        T s = (T)0;
        for (int64_t m = b + lane; m < e; m += 64) s = kfma(g.coef[m], row[g.perm[m]], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) {
            if (sub) s -= sub[p * lds + q];
            cov[p * g.Q + q] = s;
            cov[q * g.Q + p] = s;
        }
    }
}

template <typename T>
int group_colsum_launch(algp_ctx* c, const T* X, int64_t ldx, const GroupSegs<T>& g, const T* sub, int64_t lds, T* cov) {
    if (g.Q <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_ROWS, (double)g.Q * (double)g.Lm, sizeof(T) * 0.5 * ((double)g.Q * (double)g.Lm + 3.0 * g.Q * g.Q));
    const int64_t gy = g.Q < 4096 ? g.Q : 4096;
    hipLaunchKernelGGL(group_colsum_kernel<T>, dim3((unsigned)((g.Q + 3) / 4), (unsigned)gy), dim3(256), 0, c->cur, X, ldx, g, sub, lds, cov);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(group_colsum_launch);

}  // namespace algp
