// vecops.hip -- the HBM-bound tail of the path: row reductions over V^T (posterior variance and
// mean, greedy rank-1 updates), candidate scoring, argmax, and the fused kernel-GEMV for the
// mean-only posterior.  Replaces utils.py:301, 308 and the per-candidate slogdet loop of
// agent.py:317-347 (whose M fresh factorizations collapse to one pass over V^T per pick).
#include "common.h"
#include "vecops.h"
#include <algorithm>

namespace algp {

// ---------------------------------------------------------------------------------------------
// rows_reduce: one wave per row of V^T; 16-byte loads; ss[j] = sum v^2, dot[j] = sum v*w.
// ---------------------------------------------------------------------------------------------
// one wave, one row: lane-strided 16-byte loads, then a shuffle tree; lane 0 holds the sums.  Shared by the
// full-pass kernel and the lazy greedy refresh so that both produce bit-identical values.
template <typename T, bool HAS_W, bool HAS_SS>
__device__ __forceinline__ void wave_row_reduce(const T* row, const T* w, int64_t ncols, int lane, T& s2, T& sd) {
    constexpr int VEC = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const int64_t nvec = ncols / VEC;           // full vectors; the tail (ncols % VEC) is handled scalar
    s2 = (T)0;
    sd = (T)0;
    for (int64_t v = lane; v < nvec; v += 64) {
        const vec_t x = *reinterpret_cast<const vec_t*>(row + v * VEC);
        if (HAS_W) {
            const vec_t y = *reinterpret_cast<const vec_t*>(w + v * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) sd += x[e] * y[e];
        }
        if (HAS_SS) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) s2 += x[e] * x[e];
        }
    }
    const int64_t t = nvec * VEC + lane;
    if (t < ncols) {
        const T x = row[t];
        if (HAS_W) sd += x * w[t];
        if (HAS_SS) s2 += x * x;
    }
    for (int o = 32; o > 0; o >>= 1) {
        if (HAS_SS) s2 += __shfl_down(s2, o, 64);
        if (HAS_W) sd += __shfl_down(sd, o, 64);
    }
}

// tri_c0 >= 0: Vt is UPPER triangular by 128-tiles (row j is zero -- or holds something else: the MI criterion keeps a
// factor's strictly-lower tiles there -- left of column 128 (j / 128)): row j is walked from max(128 (j / 128), tri_c0) on
template <typename T, bool HAS_W, bool HAS_SS>
__global__ __launch_bounds__(256) void rows_reduce_kernel(const T* Vt, int64_t rows, int64_t ldv, int64_t ncols,
                                                          const T* w, T* ss, T* dot, int64_t tri_c0) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t j = wave; j < rows; j += nw) {
        T s2, sd;
        const int64_t c0 = tri_c0 < 0 ? 0 : (j / 128 * 128 > tri_c0 ? j / 128 * 128 : tri_c0);
        wave_row_reduce<T, HAS_W, HAS_SS>(Vt + j * ldv + c0, HAS_W ? w + c0 : w, ncols - c0, lane, s2, sd);
        if (lane == 0) {
            if (HAS_SS) ss[j] = s2;
            if (HAS_W) dot[j] = sd;
        }
    }
}

// Dot product of a row with w in an order that sixteen waves together or one wave alone can follow, bit for bit: vector v
// (16 bytes) belongs to virtual lane v mod 1024, a virtual lane adds its vectors in ascending order (fused multiply-adds,
// element by element), each of the sixteen virtual waves folds its 64 lanes with the shuffle tree, and the sixteen partial
// sums are added left to right.  The lazy refresh of ONE row (the pick's own row, the best stale row: latency-bound, 117 us
// for a row of 50 000 with one wave) runs the sixteen virtual waves on sixteen real ones; the sweeps over many rows keep a
// wave per row with sixteen accumulators.  The elements behind the last full vector go to virtual wave 0.
template <typename T>
__device__ __forceinline__ void dot_vec(T& acc, const T* row, const T* w, int64_t v) {
    constexpr int VEC = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const vec_t x = *reinterpret_cast<const vec_t*>(row + v * VEC);
    const vec_t y = *reinterpret_cast<const vec_t*>(w + v * VEC);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc = __builtin_fma(x[e], y[e], acc);
}
template <typename T>
__device__ __forceinline__ T dot_tree(T s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    return s;
}
// virtual wave vw's partial sum (valid in lane 0)
template <typename T>
__device__ __forceinline__ T row_dot_virtual_wave(const T* row, const T* w, int64_t ncols, int lane, int vw) {
    constexpr int VEC = 16 / sizeof(T);
    const int64_t nvec = ncols / VEC;
    T s = (T)0;
    for (int64_t v = vw * 64 + lane; v < nvec; v += 1024) dot_vec<T>(s, row, w, v);
    const int64_t t = nvec * VEC + lane;
    if (vw == 0 && t < ncols) s = __builtin_fma(row[t], w[t], s);
    return dot_tree<T>(s);
}
// the whole dot product by one wave (valid in lane 0)
template <typename T>
__device__ __forceinline__ T row_dot_one_wave(const T* row, const T* w, int64_t ncols, int lane) {
    constexpr int VEC = 16 / sizeof(T);
    const int64_t nvec = ncols / VEC;
    T acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = (T)0;
    for (int64_t base = 0; base < nvec; base += 1024) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t v = base + k * 64 + lane;
            if (v < nvec) dot_vec<T>(acc[k], row, w, v);
        }
    }
    const int64_t t = nvec * VEC + lane;
    if (t < ncols) acc[0] = __builtin_fma(row[t], w[t], acc[0]);
    T s = dot_tree<T>(acc[0]);
#pragma unroll
    for (int k = 1; k < 16; ++k) s += dot_tree<T>(acc[k]);
    return s;
}

// Column window [c0, c1) (multiples of 128) of every row: sum v^2, sum v u, sum v w; accumulate != 0 adds to the
// outputs.  Used by the incremental candidate solve: the sums over the kept columns of V^T are carried from
// step to step and only the new columns are read (the posterior mean needs V.z with z = u - ybar w).
template <typename T>
__global__ __launch_bounds__(256) void rows_reduce3_kernel(const T* Vt, int64_t rows, int64_t ldv, int64_t c0, int64_t c1,
                                                           const T* u, const T* w, T* oss, T* odu, T* odw, int accumulate) {
    constexpr int VEC = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t j = wave; j < rows; j += nw) {
        const T* row = Vt + j * ldv;
        T s2 = (T)0, su = (T)0, sw = (T)0;
        for (int64_t v = c0 / VEC + lane; v < c1 / VEC; v += 64) {
            const vec_t x = *reinterpret_cast<const vec_t*>(row + v * VEC);
            const vec_t a = *reinterpret_cast<const vec_t*>(u + v * VEC);
            const vec_t b = *reinterpret_cast<const vec_t*>(w + v * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                s2 += x[e] * x[e];
                su += x[e] * a[e];
                sw += x[e] * b[e];
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            s2 += __shfl_down(s2, o, 64);
            su += __shfl_down(su, o, 64);
            sw += __shfl_down(sw, o, 64);
        }
        if (lane == 0) {
            if (accumulate) {
                oss[j] += s2;
                odu[j] += su;
                odw[j] += sw;
            } else {
                oss[j] = s2;
                odu[j] = su;
                odw[j] = sw;
            }
        }
    }
}

// ss = a_ss + t_ss ; dot = (a_du + t_du) - ybar (a_dw + t_dw)
template <typename T>
__global__ void combine3_kernel(int64_t M, const T* acc, const T* tmp, int64_t stride, T ybar, T* ss, T* dot) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    ss[j] = acc[j] + tmp[j];
    dot[j] = (acc[stride + j] + tmp[stride + j]) - ybar * (acc[2 * stride + j] + tmp[2 * stride + j]);
}

template <typename T>
int rows_reduce3_launch(algp_ctx* c, const T* Vt, int64_t rows, int64_t ldv, int64_t c0, int64_t c1, const T* u, const T* w,
                        T* out3, int64_t stride, int accumulate) {
    if (rows <= 0) return ALGP_OK;
    int64_t g = (rows + 3) / 4;
    if (g > 8192) g = 8192;
    ProfScope ps(c, ALGP_PROF_ROWS, 6.0 * rows * (double)(c1 - c0), sizeof(T) * (double)rows * (double)(c1 - c0));
    hipLaunchKernelGGL(rows_reduce3_kernel<T>, dim3((unsigned)g), dim3(256), 0, c->cur, Vt, rows, ldv, c0, c1, u, w, out3,
                       out3 + stride, out3 + 2 * stride, accumulate);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
template <typename T>
int combine3_launch(algp_ctx* c, int64_t M, const T* acc, const T* tmp, int64_t stride, T ybar, T* ss, T* dot) {
    if (M <= 0) return ALGP_OK;
    hipLaunchKernelGGL(combine3_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->cur, M, acc, tmp, stride, ybar,
                       ss, dot);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(rows_reduce3_launch);
ALGP_INSTANTIATE(combine3_launch);

template <typename T>
int rows_reduce_launch(algp_ctx* c, const T* Vt, int64_t rows, int64_t ldv, int64_t ncols, const T* w, T* ss,
                       T* dot, int64_t tri_c0) {
    if (rows <= 0) return ALGP_OK;
    int64_t g = (rows + 3) / 4;
    if (g > 8192) g = 8192;
    const double share = tri_c0 < 0 ? 1.0 : 0.5;                   // an upper triangle is half the bytes
    ProfScope ps(c, ALGP_PROF_ROWS, share * 2.0 * rows * ncols * ((w ? 1 : 0) + (ss ? 1 : 0)), share * sizeof(T) * (double)rows * ncols);
    dim3 grid((unsigned)g), blk(256);
    if (w && ss) hipLaunchKernelGGL((rows_reduce_kernel<T, true, true>), grid, blk, 0, c->cur, Vt, rows, ldv, ncols, w, ss, dot, tri_c0);
    else if (w) hipLaunchKernelGGL((rows_reduce_kernel<T, true, false>), grid, blk, 0, c->cur, Vt, rows, ldv, ncols, w, ss, dot, tri_c0);
    else if (ss) hipLaunchKernelGGL((rows_reduce_kernel<T, false, true>), grid, blk, 0, c->cur, Vt, rows, ldv, ncols, w, ss, dot, tri_c0);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(rows_reduce_launch);

// The row statistics the candidate solve left per column tile (gemm.hip, STATS: stat[(2 t + 0 / 1) * ld + row]) summed over
// the tiles in ascending order: ss = sum v^2, dot = sum v z of every row, without a second pass over V^T.
template <typename T>
__global__ __launch_bounds__(256) void rowstat_combine_kernel(const T* stat, int64_t ld, int ntiles, int64_t rows, T* ss, T* dot) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int q = blockIdx.y;                                  // 0: sum v^2, 1: sum v z
    if (j >= rows) return;
    const T* p = stat + (int64_t)q * ld + j;
    T s = (T)0;
    int t = 0;
    for (; t + 8 <= ntiles; t += 8) {                          // eight loads in flight, added in tile order
        T v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p[(int64_t)(2 * (t + e)) * ld];
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[e];
    }
    for (; t < ntiles; ++t) s += p[(int64_t)(2 * t) * ld];
    (q == 0 ? ss : dot)[j] = s;
}
template <typename T>
int rowstat_combine_launch(algp_ctx* c, const T* stat, int64_t ld, int ntiles, int64_t rows, T* ss, T* dot) {
    if (rows <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * rows * ntiles, sizeof(T) * 2.0 * (double)rows * ntiles);
    hipLaunchKernelGGL(rowstat_combine_kernel<T>, dim3((unsigned)((rows + 255) / 256), 2), dim3(256), 0, c->cur, stat, ld, ntiles, rows, ss, dot);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(rowstat_combine_launch);

// ---------------------------------------------------------------------------------------------
// candidate finalize: dstat = prior - ss (ordinary) | ss (unit row: [S^-1]_jj); mu = ybar + dot
// prior of pool site p: Cp[p * n_pool + p] where Cp is given (the diagonal of an explicit covariance; with n_pool = 0 a vector of
// per-site priors, the relationship form's), else prior_const
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void cand_finalize_kernel(int64_t M, const int* ckind, const int64_t* cidx, const T* Cp, int64_t n_pool,
                                     T prior_const, const T* extra, const T* ss, const T* dot, T ybar, T* dstat,
                                     T* mu, unsigned char* alive) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const bool unit = ckind && ckind[j] >= 0;
    T prior = Cp ? Cp[cidx[j] * n_pool + cidx[j]] : prior_const;
    if (extra) prior += extra[j];
    dstat[j] = unit ? ss[j] : prior - ss[j];
    mu[j] = ybar + dot[j];
    alive[j] = 1;
}

template <typename T>
int cand_finalize_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* Cp, int64_t n_pool,
                         T prior_const, const T* extra, const T* ss, const T* dot, T ybar, T* dstat, T* mu,
                         unsigned char* alive) {
    if (M <= 0) return ALGP_OK;
    hipLaunchKernelGGL(cand_finalize_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->cur, M, ckind,
                       cidx, Cp, n_pool, prior_const, extra, ss, dot, ybar, dstat, mu, alive);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(cand_finalize_launch);

// ---------------------------------------------------------------------------------------------
// scores (entropy gain per candidate, agent.py:341 after telescoping)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double entropy_utility(double d, bool unit, double ss, double delta) {
    return unit ? 0.5 * log1p(delta * d) : ENT_CONST + 0.5 * log(d + ss);
}

template <typename T>
__global__ void score_kernel(int64_t M, const int* ckind, const unsigned char* alive, const T* dstat, double ss,
                             double delta, const double* extra, double* out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    double u;
    if (!alive[j]) {
        u = -INFINITY;
    } else {
        u = entropy_utility((double)dstat[j], ckind[j] >= 0, ss, delta);
        if (extra) u += extra[j];
    }
    out[j] = u;
}

template <typename T>
int score_launch(algp_ctx* c, int64_t M, const int* ckind, const unsigned char* alive, const T* dstat, double ss,
                 double delta, const double* extra, double* out) {
    if (M <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_SCORE, 4.0 * M, (sizeof(T) + 13.0) * M);
    hipLaunchKernelGGL(score_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->cur, M, ckind, alive,
                       dstat, ss, delta, extra, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(score_launch);

// ---------------------------------------------------------------------------------------------
// Variance-reduction criterion (include/algp_hip.h; state and driver: api_vr.hip).  w_c = sum over the targets j of E_jc^2
// comes from the fused product of gemm.hip as one partial sum per column tile; everything below is its HBM-bound rest.
// Every reduction runs in a fixed order: the same bits in every run.
// ---------------------------------------------------------------------------------------------
// w[c] (+)= the partial sums of `ntiles` column tiles, in tile order (the sibling of rowstat_combine_kernel)
template <typename T>
__global__ __launch_bounds__(256) void vr_combine_kernel(const T* part, int64_t ld, int ntiles, int64_t rows, int accumulate, T* w) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rows) return;
    T s = accumulate ? w[j] : (T)0;
    int t = 0;
    for (; t + 8 <= ntiles; t += 8) {                          // eight loads in flight, added in tile order
        T v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = part[(int64_t)(t + e) * ld + j];
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[e];
    }
    for (; t < ntiles; ++t) s += part[(int64_t)t * ld + j];
    w[j] = s;
}
template <typename T>
int vr_combine_launch(algp_ctx* c, const T* part, int64_t ld, int ntiles, int64_t rows, int accumulate, T* w) {
    if (rows <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_ROWS, (double)rows * ntiles, sizeof(T) * (double)rows * ntiles);
    hipLaunchKernelGGL(vr_combine_kernel<T>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->cur, part, ld, ntiles, rows, accumulate, w);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(vr_combine_launch);

// u_c = w_c / (pv_c + ss) (ordinary row) | -delta w_c / (1 + delta s_cc) (unit row); -inf where the row is not selectable
template <typename T>
__global__ void vr_score_kernel(int64_t M, const int* ckind, const unsigned char* alive, const T* dstat, const T* w, double ss,
                                double delta, double* out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    double u = -INFINITY;
    if (alive[j]) {
        const double d = (double)dstat[j], wj = (double)w[j];
        u = ckind[j] >= 0 ? -delta * wj / (1.0 + delta * d) : wj / (d + ss);
    }
    out[j] = u;
}
template <typename T>
int vr_score_launch(algp_ctx* c, int64_t M, const int* ckind, const unsigned char* alive, const T* dstat, const T* w, double ss,
                    double delta, double* out) {
    if (M <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_SCORE, 4.0 * M, (2.0 * sizeof(T) + 13.0) * M);
    hipLaunchKernelGGL(vr_score_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->cur, M, ckind, alive, dstat, w, ss,
                       delta, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(vr_score_launch);

// a committed pick's column `col` of V^T: r[c] of every row, rt[c] = omega_c r[c] on the targets (ordinary rows; omega = tw at
// the row's pool site, 1 without weights) and 0 elsewhere, and *nrm = sum_T omega_j r_j^2 (one workgroup: a thread adds its
// rows in ascending order, then the shuffle tree, then the waves left to right)
template <typename T>
__global__ __launch_bounds__(1024) void vr_pick_col_kernel(int64_t M, const int* ckind, const int64_t* cidx, const T* tw, const T* Vt,
                                                           int64_t ldv, int64_t col, T* r, T* rt, T* nrm) {
    __shared__ T red[16];
    T s = (T)0;
    for (int64_t j = threadIdx.x; j < M; j += 1024) {
        const T v = Vt[j * ldv + col];
        const T vt = ckind[j] < 0 ? v : (T)0;
        const T wv = tw ? tw[cidx[j]] * vt : vt;               // omega = 1: vt itself, the sum below the bits of vt vt
        r[j] = v;
        rt[j] = wv;
        s = __builtin_fma(wv, vt, s);
    }
    s = dot_tree<T>(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        T t = red[0];
        for (int k = 1; k < 16; ++k) t += red[k];
        *nrm = t;
    }
}
// t = V_T^T rt over the first ncols columns: row block b (rows_per rows) leaves its share at tp[b * ld + k] (a thread per
// column, rows in ascending order, rows outside the targets skipped); vr_tsum_kernel adds the blocks in order
template <typename T>
__global__ __launch_bounds__(256) void vr_tpart_kernel(int64_t M, int64_t rows_per, const T* Vt, int64_t ldv, int64_t ncols, const T* rt,
                                                       T* tp, int64_t ld) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ncols) return;
    const int64_t j0 = (int64_t)blockIdx.y * rows_per, j1 = j0 + rows_per < M ? j0 + rows_per : M;
    T s = (T)0;
    for (int64_t j = j0; j < j1; ++j) {
        const T rj = rt[j];
        if (rj != (T)0) s = __builtin_fma(Vt[j * ldv + k], rj, s);
    }
    tp[(int64_t)blockIdx.y * ld + k] = s;
}
template <typename T>
__global__ __launch_bounds__(256) void vr_tsum_kernel(int nblocks, const T* tp, int64_t ld, int64_t ncols, T* t) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ncols) return;
    T s = (T)0;
    for (int b = 0; b < nblocks; ++b) s += tp[(int64_t)b * ld + k];
    t[k] = s;
}
// the rank-1 fold of one pick: y_c = kappa_c (y1_c + noise rt_c) - y2_c, w_c <- w_c - 2 r_c y_c + r_c^2 nrm
// (y1: the kernel-GEMV over the targets, kgemv_launch, which leaves the source's noise term out; noise: CovSrc::noise)
template <typename T>
__global__ void vr_fold_kernel(int64_t M, const int* ckind, const T* r, const T* rt, const T* y1, const T* y2, const T* nrm, T noise,
                               T* w) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const T rj = r[j];
    const T y = (ckind[j] < 0 ? y1[j] + noise * rt[j] : (T)0) - y2[j];
    w[j] = w[j] - (T)2 * rj * y + rj * rj * *nrm;
}

// The fold in two halves, cut at its sums over the targets.  The first is local: the pick's column (r, rt, *nrm) and
// t = V_T^T rt over the columns left of it.  The second takes the targets as a list of (pool index, rt) pairs -- this context's
// own rows on one GPU, every rank's gathered pairs over a communicator, with t and *nrm summed over the ranks in between
// (vr_fold_gathered_kernel) -- and updates w.
template <typename T>
int vr_fold_local_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* Vt, int64_t ldv, int64_t col, const T* tw,
                         T* r, T* rt, T* nrm, T* tp, T* t) {
    if (M <= 0) return ALGP_OK;
    {
        ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * M, sizeof(T) * 3.0 * M);
        hipLaunchKernelGGL(vr_pick_col_kernel<T>, dim3(1), dim3(1024), 0, c->cur, M, ckind, cidx, tw, Vt, ldv, col, r, rt, nrm);
        ALGP_HIP(hipGetLastError());
    }
    const int nblocks = (int)std::min<int64_t>(VR_TBLOCKS, (M + 63) / 64);
    const int64_t rows_per = (M + nblocks - 1) / nblocks;
    {
        ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * M * col, sizeof(T) * (double)M * col);
        hipLaunchKernelGGL(vr_tpart_kernel<T>, dim3((unsigned)((col + 255) / 256), (unsigned)nblocks), dim3(256), 0, c->cur, M, rows_per, Vt,
                           ldv, col, (const T*)rt, tp, ldv);
        ALGP_HIP(hipGetLastError());
    }
    {
        ProfScope ps(c, ALGP_PROF_ROWS, (double)nblocks * col, sizeof(T) * (double)(nblocks + 1) * col);
        hipLaunchKernelGGL(vr_tsum_kernel<T>, dim3((unsigned)((col + 255) / 256)), dim3(256), 0, c->cur, nblocks, (const T*)tp, ldv, col, t);
        ALGP_HIP(hipGetLastError());
    }
    return ALGP_OK;
}
ALGP_INSTANTIATE(vr_fold_local_launch);

template <typename T>
int vr_fold_apply_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* Vt, int64_t ldv, int64_t col,
                         const KmatSrc& s, int64_t N, const int64_t* tidx, const T* tval, const T* r, const T* rt, const T* nrm,
                         const T* t, T* y1, T* y2, T* w) {
    if (M <= 0) return ALGP_OK;
    ALGP_TRY(rows_reduce_launch<T>(c, Vt, M, ldv, col, t, (T*)nullptr, y2));
    ALGP_TRY(kgemv_launch<T>(c, M, cidx, s, N, tidx, tval, (T)0, y1));
    ProfScope ps(c, ALGP_PROF_SCORE, 6.0 * M, sizeof(T) * 6.0 * M);
    hipLaunchKernelGGL(vr_fold_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->cur, M, ckind, r, rt, (const T*)y1,
                       (const T*)y2, nrm, cov_src<T>(s).noise, w);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(vr_fold_apply_launch);

// one GPU: the targets are this context's own ordinary rows (rt is zero on the others)
template <typename T>
int vr_fold_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* Vt, int64_t ldv, int64_t col, const KmatSrc& s,
                   const T* tw, T* r, T* rt, T* nrm, T* tp, T* t, T* y1, T* y2, T* w) {
    ALGP_TRY(vr_fold_local_launch<T>(c, M, ckind, cidx, Vt, ldv, col, tw, r, rt, nrm, tp, t));
    return vr_fold_apply_launch<T>(c, M, ckind, cidx, Vt, ldv, col, s, M, cidx, (const T*)rt, (const T*)r, (const T*)rt, (const T*)nrm,
                                   (const T*)t, y1, y2, w);
}
ALGP_INSTANTIATE(vr_fold_launch);

// ---- the criterion over the ranks of a communicator (api_vr.hip: vr_shard_build, vr_shard_fold) --------------------------
// A round's contribution of this rank: rows [row0, row0 + B) of V^T over K columns behind one header entry per row: its pool
// index p where the row is a target; -2 - p where it is a unit row (no target: the product reads any negative entry so, but the
// disjointness check below still learns the site); -1 behind M.  Rows that are no targets travel as zeros.  Columns from
// kvalid on (the part of the picks' block no pick has written) are zeros.  16-byte loads and stores.
template <typename T>
__global__ __launch_bounds__(256) void vr_pack_rows_kernel(int64_t M, int64_t row0, int64_t B, const int* ckind, const int64_t* cidx,
                                                           const T* Vt, int64_t ldv, int64_t K, int64_t kvalid, int64_t* head, T* rows) {
    constexpr int EPV = 16 / (int)sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(EPV)));
    const int64_t pieces = K / EPV;
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < B) {
        const int64_t src = row0 + id;
        head[id] = src < M ? (ckind[src] < 0 ? cidx[src] : -2 - cidx[src]) : (int64_t)-1;
    }
    if (id >= B * pieces) return;
    const int64_t row = id / pieces, col = (id - row * pieces) * EPV;
    const int64_t src = row0 + row;
    vec_t v;
#pragma unroll
    for (int e = 0; e < EPV; ++e) v[e] = (T)0;
    if (src < M && ckind[src] < 0) {
        v = *reinterpret_cast<const vec_t*>(Vt + src * ldv + col);
#pragma unroll
        for (int e = 0; e < EPV; ++e)
            if (col + e >= kvalid) v[e] = (T)0;
    }
    *reinterpret_cast<vec_t*>(rows + row * K + col) = v;
}
template <typename T>
int vr_pack_rows_launch(algp_ctx* c, int64_t M, int64_t row0, int64_t B, const int* ckind, const int64_t* cidx, const T* Vt, int64_t ldv,
                        int64_t K, int64_t kvalid, int64_t* head, T* rows) {
    const int64_t n = B * (K / (16 / (int64_t)sizeof(T)));
    ProfScope ps(c, ALGP_PROF_ROWS, 0.0, sizeof(T) * 2.0 * (double)B * K);
    hipLaunchKernelGGL(vr_pack_rows_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->cur, M, row0, B, ckind, cidx, Vt, ldv, K,
                       kvalid, head, rows);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(vr_pack_rows_launch);

// The shards must be disjoint: mark[pool site] = 1 for this rank's candidates, and a gathered row of ANOTHER rank, target or
// unit row, whose site lands on a mark (or outside the pool) raises mark[n_pool], which the build reads back before its last
// exchange
__global__ void vr_mark_kernel(int64_t M, const int64_t* cidx, int* mark) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < M) mark[cidx[j]] = 1;
}
__global__ void vr_overlap_kernel(const char* gathered, int64_t slice_bytes, int nranks, int self, int64_t B, int64_t n_pool, int* mark) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)nranks * B) return;
    const int r = (int)(id / B);
    if (r == self) return;
    const int64_t h = reinterpret_cast<const int64_t*>(gathered + (int64_t)r * slice_bytes)[id - (int64_t)r * B];
    if (h == -1) return;                                          // padding
    const int64_t p = h >= 0 ? h : -2 - h;
    if (p >= n_pool || mark[p]) mark[n_pool] = 1;
}
int vr_mark_launch(algp_ctx* c, int64_t M, const int64_t* cidx, int64_t n_pool, int* mark) {
    ALGP_HIP(hipMemsetAsync(mark, 0, sizeof(int) * (size_t)(n_pool + 1), c->cur));
    if (M <= 0) return ALGP_OK;
    hipLaunchKernelGGL(vr_mark_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->cur, M, cidx, mark);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
int vr_overlap_launch(algp_ctx* c, const char* gathered_heads, int64_t slice_bytes, int nranks, int self, int64_t B, int64_t n_pool,
                      int* mark) {
    const int64_t n = (int64_t)nranks * B;
    hipLaunchKernelGGL(vr_overlap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->cur, gathered_heads, slice_bytes, nranks, self,
                       B, n_pool, mark);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}

// A fold's pairs of this rank, padded to the largest shard: (pool index, rt) of its targets, (-1, 0) elsewhere
template <typename T>
__global__ void vr_pairs_kernel(int64_t M, int64_t cap, const int* ckind, const int64_t* cidx, const T* rt, int64_t* idx, T* val) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cap) return;
    const bool target = j < M && ckind[j] < 0;
    idx[j] = target ? cidx[j] : (int64_t)-1;
    val[j] = target ? rt[j] : (T)0;
}
template <typename T>
int vr_pairs_launch(algp_ctx* c, int64_t M, int64_t cap, const int* ckind, const int64_t* cidx, const T* rt, int64_t* idx, T* val) {
    if (cap <= 0) return ALGP_OK;
    hipLaunchKernelGGL(vr_pairs_kernel<T>, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, c->cur, M, cap, ckind, cidx, rt, idx, val);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(vr_pairs_launch);

// After a fold's gather (per rank: *nrm at off_nrm, t over ncols columns at off_t, cap pool indices at off_idx, cap values at
// off_val of its `stride` bytes): t and *nrm summed in rank order, the pairs in one list (padding: site 0 with value 0)
template <typename T>
__global__ void vr_fold_gathered_kernel(const char* gathered, int64_t stride, int nranks, int64_t ncols, int64_t cap, int64_t off_nrm,
                                        int64_t off_t, int64_t off_idx, int64_t off_val, T* t, T* nrm, int64_t* tidx, T* tval) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id < ncols) {
        T s = (T)0;
        for (int r = 0; r < nranks; ++r) s += reinterpret_cast<const T*>(gathered + (int64_t)r * stride + off_t)[id];
        t[id] = s;
    }
    if (id == 0) {
        T s = (T)0;
        for (int r = 0; r < nranks; ++r) s += *reinterpret_cast<const T*>(gathered + (int64_t)r * stride + off_nrm);
        *nrm = s;
    }
    if (id < (int64_t)nranks * cap) {
        const int64_t r = id / cap, j = id - r * cap;
        const int64_t p = reinterpret_cast<const int64_t*>(gathered + r * stride + off_idx)[j];
        tidx[id] = p >= 0 ? p : 0;
        tval[id] = p >= 0 ? reinterpret_cast<const T*>(gathered + r * stride + off_val)[j] : (T)0;
    }
}
template <typename T>
int vr_fold_gathered_launch(algp_ctx* c, const char* gathered, int64_t stride, int nranks, int64_t ncols, int64_t cap, int64_t off_nrm,
                            int64_t off_t, int64_t off_idx, int64_t off_val, T* t, T* nrm, int64_t* tidx, T* tval) {
    const int64_t n = std::max<int64_t>(std::max<int64_t>(ncols, (int64_t)nranks * cap), 1);
    ProfScope ps(c, ALGP_PROF_ROWS, (double)nranks * ncols, (sizeof(T) * (double)ncols + (sizeof(T) + 8.0) * cap) * nranks);
    hipLaunchKernelGGL(vr_fold_gathered_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->cur, gathered, stride, nranks, ncols,
                       cap, off_nrm, off_t, off_idx, off_val, t, nrm, tidx, tval);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(vr_fold_gathered_launch);

// the criterion's objective: *out = sum over the targets j (ordinary rows) of omega_j dstat_j in double (one workgroup, the
// order of vr_pick_col_kernel: a thread adds its rows in ascending order, then the shuffle tree, then the waves left to right)
template <typename T>
__global__ __launch_bounds__(1024) void vr_target_sum_kernel(int64_t M, const int* ckind, const int64_t* cidx, const T* dstat, const T* tw,
                                                             double* out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < M; j += 1024)
        if (ckind[j] < 0) {
            const double wj = tw ? (double)tw[cidx[j]] : 1.0;
            s = __builtin_fma(wj, (double)dstat[j], s);
        }
    s = dot_tree<double>(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
        for (int k = 1; k < 16; ++k) t += red[k];
        *out = t;
    }
}
template <typename T>
int vr_target_sum_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* dstat, const T* tw, double* out) {
    ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * M, (sizeof(T) * 2.0 + 12.0) * M);
    hipLaunchKernelGGL(vr_target_sum_kernel<T>, dim3(1), dim3(1024), 0, c->cur, M, ckind, cidx, dstat, tw, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(vr_target_sum_launch);

// first maximum (np.argmax semantics, agent.py:349): larger value wins, ties go to the smaller index
__global__ __launch_bounds__(1024) void argmax_kernel(const double* s, int64_t M, double* out_val, int64_t* out_idx) {
    __shared__ double sv[16];
    __shared__ int64_t si[16];
    double bv = -INFINITY;
    int64_t bi = -1;
    for (int64_t j = threadIdx.x; j < M; j += 1024) {
        const double v = s[j];
        if (bi < 0 || v > bv) {     // j ascending per thread: strict > keeps the first maximum
            if (!(v != v)) { bv = v; bi = j; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(bv, o, 64);
        const int64_t oi = __shfl_down(bi, o, 64);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w)
            if (si[w] >= 0 && (bi < 0 || sv[w] > bv || (sv[w] == bv && si[w] < bi))) { bv = sv[w]; bi = si[w]; }
        *out_val = bv;
        *out_idx = bi;
    }
}

// The same in two launches for long score vectors: ARGMAX_G workgroups leave their first maxima (value, index), one wave
// folds them with the same rule -- which does not depend on how the entries were grouped.  (One workgroup walking config
// 5's 100 000 utilities: 25-45 us, twice per pick.)
constexpr int ARGMAX_G = 64;
__global__ __launch_bounds__(256) void argmax_part_kernel(const double* s, int64_t M, double* pv, int64_t* pi) {
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    double bv = -INFINITY;
    int64_t bi = -1;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < M; j += 256 * ARGMAX_G) {
        const double v = s[j];
        if (bi < 0 || v > bv) {     // j ascending per thread: strict > keeps the first maximum
            if (!(v != v)) { bv = v; bi = j; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(bv, o, 64);
        const int64_t oi = __shfl_down(bi, o, 64);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (si[w] >= 0 && (bi < 0 || sv[w] > bv || (sv[w] == bv && si[w] < bi))) { bv = sv[w]; bi = si[w]; }
        pv[blockIdx.x] = bv;
        pi[blockIdx.x] = bi;
    }
}
__global__ __launch_bounds__(64) void argmax_final_kernel(const double* pv, const int64_t* pi, double* out_val, int64_t* out_idx) {
    double bv = pv[threadIdx.x];
    int64_t bi = pi[threadIdx.x];
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(bv, o, 64);
        const int64_t oi = __shfl_down(bi, o, 64);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (threadIdx.x == 0) {
        *out_val = bv;
        *out_idx = bi;
    }
}

int argmax_launch(algp_ctx* c, const double* s, int64_t M, double* out_val, int64_t* out_idx) {
    ProfScope ps(c, ALGP_PROF_SCORE, (double)M, 8.0 * M);
    static_assert(ARGMAX_G == 64, "argmax_final_kernel folds the partial maxima with one wave");
    if (M >= 32768) {
        ALGP_TRY(ensure(c, c->amax, 16 * ARGMAX_G));
        double* pv = (double*)c->amax.p;
        int64_t* pi = (int64_t*)(pv + ARGMAX_G);
        hipLaunchKernelGGL(argmax_part_kernel, dim3(ARGMAX_G), dim3(256), 0, c->cur, s, M, pv, pi);
        hipLaunchKernelGGL(argmax_final_kernel, dim3(1), dim3(64), 0, c->cur, (const double*)pv, (const int64_t*)pi, out_val, out_idx);
    } else {
        hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, c->cur, s, M, out_val, out_idx);
    }
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}

// ---------------------------------------------------------------------------------------------
// greedy commit, per row j: r_j = (b'_j - V_j . l) * scale ; dstat_j -= r^2 (ordinary) / += r^2 (unit row);
// V^T[j][ncols] = r_j.   b'_j = C(pick, j) when the pick is a new site and row j is ordinary.
// ---------------------------------------------------------------------------------------------
// b'_j = C(pick, j) when the pick is a new site and row j is ordinary, else 0
template <typename T, int DP, typename S>
__device__ __forceinline__ T pick_bprime(bool unit, int64_t pj, const S& src, int64_t pick_pool, int pick_in_train) {
    return (!pick_in_train && !unit) ? pool_cov<DP>(src, pick_pool, pj) : (T)0;
}

// z = u - ybar w ; rhs initialisation for the resumed substitutions: u[i] = y[i], w[i] = (i < n) for i >= k
template <typename T>
__global__ void uw_init_kernel(T* u, T* w, const T* y, int64_t k, int64_t n, int64_t npad) {
    const int64_t i = k + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    u[i] = y[i];
    w[i] = i < n ? (T)1 : (T)0;
}
template <typename T>
__global__ void uw_combine_kernel(T* z, const T* u, const T* w, T ybar, int64_t npad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npad) z[i] = u[i] - ybar * w[i];
}
template <typename T>
int uw_init_launch(algp_ctx* c, T* u, T* w, const T* y, int64_t k, int64_t n, int64_t npad) {
    if (npad <= k) return ALGP_OK;
    hipLaunchKernelGGL(uw_init_kernel<T>, dim3((unsigned)((npad - k + 255) / 256)), dim3(256), 0, c->cur, u, w, y, k, n, npad);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
template <typename T>
int uw_combine_launch(algp_ctx* c, T* z, const T* u, const T* w, T ybar, int64_t npad) {
    hipLaunchKernelGGL(uw_combine_kernel<T>, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, c->cur, z, u, w, ybar, npad);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(uw_init_launch);
ALGP_INSTANTIATE(uw_combine_launch);

// dst[r][0:ncols] = src[src_row[r]][0:ncols], or zeros where src_row[r] < 0 (one workgroup per row and 2048 columns: the
// row exchange of the sharded loop packs a handful of rows of 50 000).
// With lrow: rows with lrow[r] >= 0 are  Lb[lrow[r]][0:ncols] - lscale[r] * src[src_row[r]][0:ncols]
// (a second measurement of a site that already is train row lrow[r], see vt_rows_for_new_sites in api.hip).
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T* src, int64_t lds, const int64_t* src_row, T* dst,
                                                          int64_t ldd, int64_t ncols, const int64_t* lrow, const T* lscale,
                                                          const T* Lb, int64_t ldl) {
    const int64_t r = blockIdx.x, sr = src_row[r];
    T* d = dst + r * ldd;
    const int64_t k0 = (int64_t)blockIdx.y * 2048 + threadIdx.x;
    ncols = ncols < ((int64_t)blockIdx.y + 1) * 2048 ? ncols : ((int64_t)blockIdx.y + 1) * 2048;
    if (sr < 0) {
        for (int64_t k = k0; k < ncols; k += 256) d[k] = (T)0;
    } else if (lrow && lrow[r] >= 0) {
        const T* sp = src + sr * lds;
        const int64_t lr = lrow[r];
        const T* lp = Lb + lr * ldl;
        const T sc = lscale[r];
        // row lr of L ends at its diagonal (the strict upper part of a diagonal block is scratch)
        for (int64_t k = k0; k < ncols; k += 256) d[k] = (k <= lr ? lp[k] : (T)0) - sc * sp[k];
    } else {
        const T* sp = src + sr * lds;
        for (int64_t k = k0; k < ncols; k += 256) d[k] = sp[k];
    }
}

template <typename T>
int gather_rows_launch(algp_ctx* c, const T* src, int64_t lds, const int64_t* src_row, T* dst, int64_t ldd, int64_t nrows,
                       int64_t ncols, const int64_t* lrow, const T* lscale, const T* Lb, int64_t ldl) {
    if (nrows <= 0 || ncols <= 0) return ALGP_OK;
    hipLaunchKernelGGL(gather_rows_kernel<T>, dim3((unsigned)nrows, (unsigned)((ncols + 2047) / 2048)), dim3(256), 0, c->cur, src, lds, src_row, dst, ldd, ncols,
                       lrow, lscale, Lb, ldl);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(gather_rows_launch);

// ---------------------------------------------------------------------------------------------
// Lazy greedy (entropy criterion).  The gain of a candidate never grows when more sites are sampled
// (information gain is submodular), so a utility computed before the last picks is an upper bound.  After
// a pick only the rows that can still win are brought up to date: the best stale row first (its fresh
// utility becomes the threshold), then every stale row whose bound reaches the threshold.  A refresh
// applies the missing picks in order with exactly the arithmetic of the full pass (row_dot_* +
// pick_bprime), so picks and values equal the full pass bit for bit; it costs one row of V^T per pick
// instead of a sweep over all M rows.
//   mode 0: row `pos` only (grid = 1 block)   mode 1: alive stale rows with scores >= scores[pos]
//   mode 2: every stale row (flush before anything reads the full state)
// pos_dev != null: the row is the one an argmax kernel has just left on the device (*pos_dev; < 0 = no row, nothing to
// do), so that argmax -> refresh -> refresh -> argmax is one stream-ordered chain without a host round trip.
// ---------------------------------------------------------------------------------------------
// S: the source's type -- CovSrc<T>, or CovSrcAdd<T> (the additive form's own instantiations; with_src, common.h)
template <typename T, int DP, bool COOP, typename S>
__global__ __launch_bounds__(COOP ? 1024 : 256) void lazy_refresh_kernel(int64_t M, int mode, int64_t pos, const int64_t* pos_dev,
                                                           const LazyPick* picks,
                                                           int npicks, const int* ckind, const int64_t* cidx,
                                                           S src, const T* prevrows, int64_t ldv, T* Vt, T* dstat,
                                                           int* fresh, const unsigned char* alive, double* scores,
                                                           double ss, double delta) {
    const int lane = threadIdx.x & 63;
    if (pos_dev) {
        pos = *pos_dev;
        if (pos < 0 && mode != 2) return;
    }
    if (COOP) {
        // one row (mode 0: row pos; mode 2 with M = 1: row 0), sixteen waves: wave w is virtual wave w of the dot product
        __shared__ T red[16];
        const int wv = threadIdx.x >> 6;
        const int64_t j = (mode == 0) ? pos : 0;
        const int f = fresh[j];
        if (f >= npicks) return;
        const bool unit = ckind[j] >= 0;
        const int64_t pj = cidx[j];
        T* row = Vt + j * ldv;
        T d = dstat[j];
        for (int q = f; q < npicks; ++q) {
            const LazyPick pk = picks[q];
            const T part = row_dot_virtual_wave<T>(row, prevrows + (int64_t)q * ldv, pk.ncols, lane, wv);
            if (lane == 0) red[wv] = part;
            __syncthreads();
            T sd = red[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) sd += red[k];
            const T bp = pick_bprime<T, DP>(unit, pj, src, pk.pool_idx, (int)pk.in_train);
            const T r = (bp - sd) * (T)pk.scale;
            d += unit ? r * r : -(r * r);
            if (threadIdx.x == 0) row[pk.ncols] = r;
            __threadfence();                                   // the next pick's dot product reads this entry
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            dstat[j] = d;
            fresh[j] = npicks;
            scores[j] = alive[j] ? entropy_utility((double)d, unit, ss, delta) : -INFINITY;
        }
        return;
    }
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;
    const double thr = (mode == 1) ? scores[pos] : 0.0;        // row pos is up to date in mode 1: never rewritten here
    for (int64_t j = wave; j < M; j += nw) {
        const int f = fresh[j];
        if (f >= npicks) continue;
        if (mode == 1 && (!alive[j] || !(scores[j] >= thr))) continue;
        const bool unit = ckind[j] >= 0;
        const int64_t pj = cidx[j];
        T* row = Vt + j * ldv;
        T d = dstat[j];
        for (int q = f; q < npicks; ++q) {
            const LazyPick pk = picks[q];
            T sd = row_dot_one_wave<T>(row, prevrows + (int64_t)q * ldv, pk.ncols, lane);
            sd = __shfl(sd, 0, 64);
            const T bp = pick_bprime<T, DP>(unit, pj, src, pk.pool_idx, (int)pk.in_train);
            const T r = (bp - sd) * (T)pk.scale;
            d += unit ? r * r : -(r * r);
            if (lane == 0) row[pk.ncols] = r;
            __threadfence();                                   // the next pick's dot product reads this entry
        }
        if (lane == 0) {
            dstat[j] = d;
            fresh[j] = npicks;
            scores[j] = alive[j] ? entropy_utility((double)d, unit, ss, delta) : -INFINITY;
        }
    }
}

template <typename T>
int lazy_refresh_launch(algp_ctx* c, int64_t M, int mode, int64_t pos, const LazyPick* picks, int npicks, const int* ckind,
                        const int64_t* cidx, const KmatSrc& s, const T* prevrows, int64_t ldv, T* Vt, T* dstat, int* fresh,
                        const unsigned char* alive, double* scores, double ss, double delta, const int64_t* pos_dev) {
    if (M <= 0 || npicks <= 0) return ALGP_OK;
    const bool coop = (mode == 0 || (mode == 2 && M == 1));      // one row: sixteen waves share its dot products
    int64_t g = coop ? 1 : (M + 3) / 4;
    if (g > 65536) g = 65536;
    ProfScope ps(c, ALGP_PROF_ROWS, 0.0, 13.0 * M);
    dim3 grid((unsigned)g), blk(coop ? 1024 : 256);
    with_src<T>(s, [&](auto src) {
        auto launch = [&](auto dp, auto co) {
            hipLaunchKernelGGL((lazy_refresh_kernel<T, decltype(dp)::value, decltype(co)::value, decltype(src)>), grid, blk, 0, c->cur, M, mode,
                               pos, pos_dev, picks, npicks, ckind, cidx, src, prevrows, ldv, Vt, dstat, fresh, alive, scores, ss, delta);
        };
        with_dp(s.DP, [&](auto dp) {
            if (coop) launch(dp, std::true_type{});
            else launch(dp, std::false_type{});
        });
    });
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(lazy_refresh_launch);

// ---------------------------------------------------------------------------------------------
// greedy commit bookkeeping on the device (one thread): from the winner's statistic d_c (posterior variance, or
// [S^-1]_cc for a train site) the scale of the appended row, the pick record the lazy refresh reads, the winner's
// local row retired, and (d_c, scale) for the host's single read-back.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void commit_finalize_kernel(const T* dsrc, int in_train, double ss, double delta, LazyPick* lp_out,
                                       int64_t pool_idx, int64_t ncols, unsigned char* alive_local, double* score_local,
                                       double* out2) {
    const double dc = (double)*dsrc;
    const double scale = in_train ? sqrt(-(delta / (1.0 + delta * dc))) : 1.0 / sqrt(dc + ss);
    LazyPick lp;
    lp.pool_idx = pool_idx;
    lp.ncols = ncols;
    lp.scale = scale;
    lp.in_train = in_train;
    lp.d = dc;
    *lp_out = lp;
    // the winner retires -- unless its scale is not finite (a non-positive variance under the square root): the caller
    // of algp_commit_pick then takes the pick back, and the site must stay selectable
    if (alive_local && scale == scale && !isinf(scale)) {
        *alive_local = 0;
        *score_local = -INFINITY;
    }
    out2[0] = dc;
    out2[1] = scale;
}
template <typename T>
int commit_finalize_launch(algp_ctx* c, const T* dsrc, int in_train, double ss, double delta, LazyPick* lp_out,
                           int64_t pool_idx, int64_t ncols, unsigned char* alive_local, double* score_local, double* out2) {
    hipLaunchKernelGGL(commit_finalize_kernel<T>, dim3(1), dim3(1), 0, c->cur, dsrc, in_train, ss, delta, lp_out, pool_idx,
                       ncols, alive_local, score_local, out2);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(commit_finalize_launch);

// ---------------------------------------------------------------------------------------------
// MI criterion (agent.py:330-339).  Besides the entropy gain, the utility of candidate i needs H(Abar \ i) and H(all_i):
//   H(Abar \ i) = H(Abar) - CONST + 1/2 log [C_AbarAbar^-1]_ii                 (i not sampled)
//   H(all_i)    = H(all)  + 1/2 log(1 + d_i [(C + D_all)^-1]_ii),  d_i = ss (new site) | v_fused - sm (mobile-sampled)
// i.e. the DIAGONALS of two pool-wide inverses, P = C_AbarAbar^-1 and Q = (C + D_all)^-1.  Both are kept as their
// triangular factors' inverses X (P = X X^T), computed once per candidate solve; a committed pick c is a rank-1 change
//   removal of site c from Abar:   P <- P - p p^T / P_cc,                 p = P[:, c]
//   noise change d at site c:      Q <- Q - g q q^T,  g = d/(1 + d Q_cc),  q = Q[:, c]
// so each pick costs one pass over X (column c of X X^T = X times row c of X, rows_reduce_kernel) plus this kernel,
// which removes the earlier picks' rank-1 terms from that column, appends the new term u (sign sg) to the list and
// updates the diagonal and the entropy: O(n^2) per pick instead of two O(n^3) factorisations.
//   mode 0 (removal): u = p / sqrt(P_cc), sg = +1, H += -CONST + 1/2 log P_cc
//   mode 1 (noise):   u = q sqrt|g|,      sg = sign g, H += 1/2 log(1 + d Q_cc); also H_A += the pick's own entropy gain,
//                     read off the scale of its appended row (LazyPick): new site CONST - log scale, mobile-sampled
//                     1/2 log(-d) - log scale
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mi_rank1_kernel(int64_t m, const T* col0, T* U, int64_t ldu, double* sgn, int q, int64_t cpos,
                                                       int mode, double dlt, T* diag, double* H, double* H_A, const LazyPick* pick) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double pc = (double)col0[cpos];
    for (int r = 0; r < q; ++r) {
        const double uc = (double)U[(int64_t)r * ldu + cpos];
        pc -= sgn[r] * uc * uc;
    }
    double fac, sg;
    if (mode == 0) { fac = 1.0 / sqrt(pc); sg = 1.0; }
    else {
        const double g = dlt / (1.0 + dlt * pc);
        fac = sqrt(fabs(g));
        sg = g >= 0.0 ? 1.0 : -1.0;
    }
    if (j < m) {
        double cj = (double)col0[j];
        for (int r = 0; r < q; ++r) cj -= sgn[r] * (double)U[(int64_t)r * ldu + j] * (double)U[(int64_t)r * ldu + cpos];
        const double u = cj * fac;
        U[(int64_t)q * ldu + j] = (T)u;
        diag[j] = (T)((double)diag[j] - sg * u * u);
    }
    if (j == 0) {
        // every thread read sgn[0..q) and H before this block's thread 0 writes slot q / H: other blocks may still be
        // reading sgn[r < q] (untouched here); slot q and H are written once per launch
        sgn[q] = sg;
        *H += mode == 0 ? -ENT_CONST + 0.5 * log(pc) : 0.5 * log1p(dlt * pc);
        if (H_A) *H_A += (pick->in_train ? 0.5 * log(-dlt) : ENT_CONST) - log(pick->scale);
    }
}
template <typename T>
int mi_rank1_launch(algp_ctx* c, int64_t m, const T* col0, T* U, int64_t ldu, double* sgn, int q, int64_t cpos, int mode,
                    double dlt, T* diag, double* H, double* H_A, const LazyPick* pick) {
    hipLaunchKernelGGL(mi_rank1_kernel<T>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->cur, m, col0, U, ldu, sgn, q, cpos,
                       mode, dlt, diag, H, H_A, pick);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mi_rank1_launch);

// MI utility of every candidate from the device-resident terms: entropy gain + H(A) + H(Abar \ i) - H(all_i)
// Hs = (H(A), H(Abar), H(all)); posbar: pool index -> row of the complement matrix
template <typename T>
__global__ void mi_score_kernel(int64_t M, const int* ckind, const int64_t* cidx, const unsigned char* alive, const T* dstat,
                                double ss, double delta, const int64_t* posbar, const T* dP, const T* dQ, const double* Hs,
                                double* out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    double u = -INFINITY;
    if (alive[j]) {
        const bool unit = ckind[j] >= 0;
        const int64_t pj = cidx[j];
        u = entropy_utility((double)dstat[j], unit, ss, delta) + Hs[0];
        if (unit) u += Hs[1] - (Hs[2] + 0.5 * log1p(delta * (double)dQ[pj]));
        else u += (Hs[1] - ENT_CONST + 0.5 * log((double)dP[posbar[pj]])) - (Hs[2] + 0.5 * log1p(ss * (double)dQ[pj]));
    }
    out[j] = u;
}
template <typename T>
int mi_score_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const unsigned char* alive, const T* dstat,
                    double ss, double delta, const int64_t* posbar, const T* dP, const T* dQ, const double* Hs, double* out) {
    if (M <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_SCORE, 12.0 * M, (3.0 * sizeof(T) + 21.0) * M);
    hipLaunchKernelGGL(mi_score_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->cur, M, ckind, cidx, alive, dstat,
                       ss, delta, posbar, dP, dQ, Hs, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mi_score_launch);

// out[0] = fresh[*idx] (as a double; -1 when *idx < 0): rides with the argmax read-back of the lazy greedy
__global__ void fresh_at_kernel(const int* fresh, const int64_t* idx, double* out) {
    const int64_t i = *idx;
    *out = i >= 0 ? (double)fresh[i] : -1.0;
}
int fresh_at_launch(algp_ctx* c, const int* fresh, const int64_t* idx, double* out) {
    hipLaunchKernelGGL(fresh_at_kernel, dim3(1), dim3(1), 0, c->cur, fresh, idx, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}

// ---------------------------------------------------------------------------------------------
// best_path block scoring (agent.py:358-403, entropy criterion): the gain of a whole path of mobile readings,
//   dH = H(A u P) - H(A) = |P| CONST + 1/2 log det G,   G = C_PP + sigma_m^2 I - V_P^T V_P   (|P| <= 64),
// from the rows of V^T the candidate solve left resident -- one workgroup per path, no factor update, no host round
// trip per path.  A path entry is a local candidate position; entries with lpos >= 0 are sites that already are
// train row lpos (a second, mobile reading of a statically sampled site): their column is C[A, j] = S e_lpos - d e_lpos,
// so V_j = L[lpos, :]^T - d_lpos u with u = the candidate's unit row.  Accumulation in fp64 for either dtype.
// ---------------------------------------------------------------------------------------------
constexpr int PATH_SITES = 64;
template <typename T, int DP, typename S>
__global__ __launch_bounds__(256) void path_score_kernel(const int64_t* cpos, const int64_t* lpos, int maxlen, const int64_t* cidx,
                                                         const T* Vt, int64_t ldv, int64_t ncols, const T* L, int64_t ldl,
                                                         const T* varA, S src, double sm, double* out) {
    __shared__ double G[PATH_SITES][PATH_SITES + 1];
    __shared__ double R[PATH_SITES][33];
    __shared__ int64_t s_c[PATH_SITES], s_l[PATH_SITES];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int64_t* pc = cpos + (int64_t)blockIdx.x * maxlen;
    const int64_t* pl = lpos + (int64_t)blockIdx.x * maxlen;
    if (tid == 0) {
        int n = 0;
        for (int a = 0; a < maxlen && n < PATH_SITES; ++a)
            if (pc[a] >= 0) { s_c[n] = pc[a]; s_l[n] = pl[a]; ++n; }
        s_n = n;
    }
    __syncthreads();
    const int P = s_n;
    if (P == 0) {
        if (tid == 0) out[blockIdx.x] = 0.0;
        return;
    }
    // Gram matrix of the path's rows of V^T, 32 columns at a time; thread (ty, tx) owns G[ty + 16 i][tx + 16 j]
    const int ty = tid >> 4, tx = tid & 15;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int64_t k0 = 0; k0 < ncols; k0 += 32) {
        for (int e = tid; e < P * 32; e += 256) {
            const int a = e >> 5, k = e & 31;
            const int64_t kk = k0 + k;
            double v = 0.0;
            if (kk < ncols) {
                v = (double)Vt[s_c[a] * ldv + kk];
                const int64_t lp = s_l[a];
                if (lp >= 0) v = (kk <= lp ? (double)L[lp * ldl + kk] : 0.0) - (double)varA[lp] * v;
            }
            R[a][k] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = ty + 16 * i;
            if (a >= P) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = tx + 16 * j;
                if (b > a) continue;                            // lower triangle
                double s2 = 0.0;
#pragma unroll 8
                for (int k = 0; k < 32; ++k) s2 += R[a][k] * R[b][k];
                acc[i][j] += s2;
            }
        }
        __syncthreads();
    }
    // G = C_PP + sigma_m^2 I - Gram
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = ty + 16 * i;
        if (a >= P) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = tx + 16 * j;
            if (b > a) continue;
            G[a][b] = pool_cov<DP>(src, cidx[s_c[a]], cidx[s_c[b]]) + (a == b ? sm : 0.0) - acc[i][j];
        }
    }
    __syncthreads();
    // Cholesky of the P x P block in LDS, column by column; log det = 2 sum log diag
    double logdet = 0.0;
    for (int j = 0; j < P; ++j) {
        const double d = G[j][j];
        if (!(d > 0.0)) { logdet = NAN; break; }                   // wave-uniform: every thread reads the same G[j][j]
        const double rs = 1.0 / sqrt(d);
        logdet += log(d);
        __syncthreads();
        for (int i = j + 1 + tid; i < P; i += 256) G[i][j] *= rs;
        __syncthreads();
        for (int e = tid; e < (P - j - 1) * (P - j - 1); e += 256) {
            const int i = j + 1 + e / (P - j - 1), c2 = j + 1 + e % (P - j - 1);
            if (c2 <= i) G[i][c2] -= G[i][j] * G[c2][j];
        }
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = (double)P * ENT_CONST + 0.5 * logdet;
}

template <typename T>
int path_score_launch(algp_ctx* c, const int64_t* cpos, const int64_t* lpos, int npaths, int maxlen, const int64_t* cidx,
                      const T* Vt, int64_t ldv, int64_t ncols, const T* L, int64_t ldl, const T* varA, const KmatSrc& s, double sm,
                      double* out) {
    if (npaths <= 0) return ALGP_OK;
    with_src<T, double>(s, [&](auto src) {
        with_dp(s.DP, [&](auto dp) {
            hipLaunchKernelGGL((path_score_kernel<T, decltype(dp)::value, decltype(src)>), dim3((unsigned)npaths), dim3(256), 0, c->cur, cpos,
                               lpos, maxlen, cidx, Vt, ldv, ncols, L, ldl, varA, src, sm, out);
        });
    });
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(path_score_launch);

// ---- paths of 65 .. 256 sites (config 5's field rows: up to ~250 sites on a 250 x 200 field, env.py:197-310) -------------
// The path's posterior block no longer fits LDS: its rows of V^T are gathered into a scratch (gather_rows_kernel, the
// second-reading transform included), the Gram matrices of a batch of paths are ONE batched MFMA product (gemm.hip), this
// kernel turns each into G = C_PP + sigma_m^2 I - Gram (identity on the padding) in place, and the blocks are factored
// as 2 x 2 tiles of 128 by the diagonal-block kernel + two batched tile products (api.hip: score_paths_big).
template <typename T, int DP, typename S>
__global__ __launch_bounds__(256) void path_assemble_kernel(const int64_t* cpos, int ppad, const int64_t* cidx, S src,
                                                            double sm, T* G) {
    __shared__ int64_t s_p[256];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int64_t* pc = cpos + (int64_t)blockIdx.x * ppad;
    if (tid == 0) {
        int n = 0;
        while (n < ppad && pc[n] >= 0) ++n;                        // the host packs a path's sites to the front
        s_n = n;
    }
    if (tid < ppad) s_p[tid] = pc[tid] >= 0 ? cidx[pc[tid]] : -1;
    __syncthreads();
    const int P = s_n;
    T* Gp = G + (int64_t)blockIdx.x * ppad * ppad;
    for (int e = tid; e < ppad * ppad; e += 256) {
        const int a = e / ppad, b = e - a * ppad;
        if ((a >> 7) < (b >> 7)) continue;                         // tiles above the diagonal are never read
        T v;
        if (a < P && b < P) {
            v = (T)(pool_cov<DP>(src, s_p[a], s_p[b]) + (a == b ? sm : 0.0) - (double)Gp[e]);
        } else {
            v = a == b ? (T)1 : (T)0;
        }
        Gp[e] = v;
    }
}
template <typename T>
int path_assemble_launch(algp_ctx* c, const int64_t* cpos, int batch, int ppad, const int64_t* cidx, const KmatSrc& s, double sm, T* G) {
    if (batch <= 0) return ALGP_OK;
    with_src<T, double>(s, [&](auto src) {
        with_dp(s.DP, [&](auto dp) {
            hipLaunchKernelGGL((path_assemble_kernel<T, decltype(dp)::value, decltype(src)>), dim3((unsigned)batch), dim3(256), 0, c->cur, cpos,
                               ppad, cidx, src, sm, G);
        });
    });
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(path_assemble_launch);
// out[p] = P CONST + 1/2 log det (NaN where a pivot was not positive)
__global__ void path_finish_kernel(const int64_t* cpos, int ppad, int batch, const double* logdet, const int* info, double* out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= batch) return;
    int n = 0;
    const int64_t* pc = cpos + (int64_t)p * ppad;
    while (n < ppad && pc[n] >= 0) ++n;
    out[p] = info[p] != 0 ? NAN : (double)n * ENT_CONST + 0.5 * logdet[p];
}
int path_finish_launch(algp_ctx* c, const int64_t* cpos, int ppad, int batch, const double* logdet, const int* info, double* out) {
    if (batch <= 0) return ALGP_OK;
    hipLaunchKernelGGL(path_finish_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, c->cur, cpos, ppad, batch, logdet, info, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}

// ---------------------------------------------------------------------------------------------
// Variance reduction of whole paths (api_paths_vr.hip): u_p = tr((Gamma_SS + sm I)^-1 Phi_SS) over the path's sites S, from
// the two matrices the host has built over the union U of a group of paths: Gamma = C(U, U) - R_U R_U^T (the posterior
// covariance of the union sites) and Phi = E E^T (E: their cross covariances with the targets).  A path is its sites'
// positions in the union (upos: stride entries per path, packed to the front, -1 behind them) and the slot of the
// caller's output it writes (pid).  Only the lower tiles of Gamma and Phi are valid: every read goes to [max][min].
// ---------------------------------------------------------------------------------------------
// Gamma = C(U, U) - Gram in place, on and below the diagonal (one workgroup per row; sm is added per path)
template <typename T, int DP, typename S>
__global__ __launch_bounds__(256) void pvr_assemble_kernel(const int64_t* uidx, int64_t U, int64_t ld, S src, T* G) {
    const int64_t a = blockIdx.x;
    const int64_t pa = uidx[a];
    double xa[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) xa[d] = src.Cp ? 0.0 : (double)src.Xs[pa * DP + d];
    for (int64_t b = threadIdx.x; b <= a; b += 256) G[a * ld + b] = (T)(pool_cov<DP>(src, pa, uidx[b], xa) - (double)G[a * ld + b]);
}
template <typename T>
int pvr_assemble_launch(algp_ctx* c, const int64_t* uidx, int64_t U, int64_t ld, const KmatSrc& s, T* G) {
    if (U <= 0) return ALGP_OK;
    with_src<T, double>(s, [&](auto src) {
        with_dp(s.DP, [&](auto dp) {
            hipLaunchKernelGGL((pvr_assemble_kernel<T, decltype(dp)::value, decltype(src)>), dim3((unsigned)U), dim3(256), 0, c->cur, uidx, U,
                               ld, src, G);
        });
    });
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(pvr_assemble_launch);

// Paths of at most 64 sites, one workgroup per path, fp64 in LDS for either dtype like path_score_kernel: both k x k blocks
// gathered by union position, sm on Gamma's diagonal, the column Cholesky L L^T = Gamma_SS + sm I, W = L^-1 Phi_SS (a thread
// per column), then from the other side Y = W L^-T (a thread per row, up to its diagonal entry: the trace needs no more)
// and u = sum_r Y_rr in index order.  A pivot that is not positive: NaN.
template <typename T>
__global__ __launch_bounds__(256) void pvr_small_kernel(const int* upos, int stride, const int* pid, const T* Gam, const T* Phi, int64_t ld,
                                                        double sm, double* out) {
    __shared__ double G[PATH_SITES][PATH_SITES + 1];
    __shared__ double W[PATH_SITES][PATH_SITES + 1];
    __shared__ int s_u[PATH_SITES];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int* pu = upos + (int64_t)blockIdx.x * stride;
    if (tid == 0) {
        int n = 0;
        while (n < stride && n < PATH_SITES && pu[n] >= 0) { s_u[n] = pu[n]; ++n; }
        s_n = n;
    }
    __syncthreads();
    const int P = s_n;
    for (int e = tid; e < P * P; e += 256) {
        const int a = e / P, b = e - a * P;
        const int64_t ua = s_u[a], ub = s_u[b];
        const int64_t at = ua >= ub ? ua * ld + ub : ub * ld + ua;
        G[a][b] = (double)Gam[at] + (a == b ? sm : 0.0);
        W[a][b] = (double)Phi[at];
    }
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < P; ++j) {
        const double d = G[j][j];
        if (!(d > 0.0)) { bad = true; break; }                     // wave-uniform: every thread reads the same G[j][j]
        const double rs = 1.0 / sqrt(d);
        __syncthreads();
        for (int i = j + tid; i < P; i += 256) G[i][j] *= rs;      // the diagonal entry becomes sqrt(d)
        __syncthreads();
        for (int e = tid; e < (P - j - 1) * (P - j - 1); e += 256) {
            const int i = j + 1 + e / (P - j - 1), c2 = j + 1 + e % (P - j - 1);
            if (c2 <= i) G[i][c2] -= G[i][j] * G[c2][j];
        }
        __syncthreads();
    }
    if (bad) {
        if (tid == 0) out[pid[blockIdx.x]] = NAN;
        return;
    }
    if (tid < P) {
        for (int i = 0; i < P; ++i) {
            double s = W[i][tid];
            for (int m = 0; m < i; ++m) s -= G[i][m] * W[m][tid];
            W[i][tid] = s / G[i][i];
        }
    }
    __syncthreads();
    if (tid < P) {
        for (int j = 0; j <= tid; ++j) {
            double s = W[tid][j];
            for (int m = 0; m < j; ++m) s -= G[j][m] * W[tid][m];
            W[tid][j] = s / G[j][j];
        }
    }
    __syncthreads();
    if (tid == 0) {
        double u = 0.0;
        for (int r = 0; r < P; ++r) u += W[r][r];
        out[pid[blockIdx.x]] = u;
    }
}
template <typename T>
int pvr_small_launch(algp_ctx* c, const int* upos, int stride, const int* pid, int npaths, const T* Gam, const T* Phi, int64_t ld,
                     double sm, double* out) {
    if (npaths <= 0) return ALGP_OK;
    hipLaunchKernelGGL(pvr_small_kernel<T>, dim3((unsigned)npaths), dim3(256), 0, c->cur, upos, stride, pid, Gam, Phi, ld, sm, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(pvr_small_launch);

// Paths of 65 .. 256 sites, a batch of ppad x ppad blocks (ppad = 128 or 256).  Gather: G = Gamma_SS + sm I on its lower
// tiles, the identity behind the path's sites; F = Phi_SS in both triangles, zero behind them.
template <typename T>
__global__ __launch_bounds__(256) void pvr_gather_kernel(const int* upos, int ppad, const T* Gam, const T* Phi, int64_t ld, double sm, T* G,
                                                         T* F) {
    __shared__ int s_u[256];
    const int tid = threadIdx.x;
    if (tid < ppad) s_u[tid] = upos[(int64_t)blockIdx.x * ppad + tid];
    __syncthreads();
    T* Gp = G + (int64_t)blockIdx.x * ppad * ppad;
    T* Fp = F + (int64_t)blockIdx.x * ppad * ppad;
    for (int e = tid; e < ppad * ppad; e += 256) {
        const int a = e / ppad, b = e - a * ppad;
        const int64_t ua = s_u[a], ub = s_u[b];
        T g = a == b ? (T)1 : (T)0, f = (T)0;
        if (ua >= 0 && ub >= 0) {
            const int64_t at = ua >= ub ? ua * ld + ub : ub * ld + ua;
            g = (T)((double)Gam[at] + (a == b ? sm : 0.0));
            f = Phi[at];
        }
        if ((a >> 7) >= (b >> 7)) Gp[e] = g;                       // tiles above the diagonal are never read
        Fp[e] = f;
    }
}
template <typename T>
int pvr_gather_launch(algp_ctx* c, const int* upos, int ppad, int batch, const T* Gam, const T* Phi, int64_t ld, double sm, T* G, T* F) {
    if (batch <= 0) return ALGP_OK;
    if (ppad != NB && ppad != 2 * NB) return fail(c, ALGP_ERR_BAD_ARG, "pvr_gather: ppad must be 128 or 256");
    hipLaunchKernelGGL(pvr_gather_kernel<T>, dim3((unsigned)batch), dim3(256), 0, c->cur, upos, ppad, Gam, Phi, ld, sm, G, F);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(pvr_gather_launch);

// The block's L^-1 from its 2 x 2 tiled factor: the two inverse tiles (inv: [inv(L11) | inv(L22)], zeros above their
// diagonals) go to the diagonal tiles of Li, zeros above them; ppad = 256: tr = [L21^T | inv(L11)^T] are the transposed
// operands of the two products that fill the tile below, -inv(L22) L21 inv(L11).  64 x 64 pieces through LDS.
template <typename T>
__global__ __launch_bounds__(256) void pvr_linv_kernel(const T* inv, const T* L21, int ppad, T* Li, T* tr) {
    __shared__ T tile[64][65];
    const int64_t b_ = blockIdx.z;
    const int ta = blockIdx.x & 1, tb = blockIdx.x >> 1;           // a 64 x 64 piece of a 128 x 128 tile
    const int which = blockIdx.y;                                  // 0, 1: the inverse tiles; 2: L21^T; 3: inv(L11)^T
    const int tid = threadIdx.x;
    const T* iv = inv + b_ * 2 * NB * NB;
    T* Lo = Li + b_ * ppad * ppad;
    if (which < 2) {
        if (which == 1 && ppad == NB) return;
        for (int e = tid; e < 64 * 64; e += 256) {
            const int a = ta * 64 + (e >> 6), b = tb * 64 + (e & 63);
            Lo[(int64_t)(which * NB + a) * ppad + which * NB + b] = iv[which * NB * NB + a * NB + b];
            if (which == 0 && ppad > NB) Lo[(int64_t)a * ppad + NB + b] = (T)0;
        }
        return;
    }
    if (ppad == NB) return;
    const T* src = which == 2 ? L21 + b_ * NB * NB : iv;
    T* dst = tr + (b_ * 2 + (which - 2)) * NB * NB;
    for (int e = tid; e < 64 * 64; e += 256) {
        const int bb = e >> 6, aa = e & 63;
        tile[bb][aa] = src[(tb * 64 + bb) * NB + ta * 64 + aa];
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
        const int aa = e >> 6, bb = e & 63;
        dst[(ta * 64 + aa) * NB + tb * 64 + bb] = tile[bb][aa];
    }
}
template <typename T>
int pvr_linv_launch(algp_ctx* c, const T* inv, const T* L21, int ppad, int batch, T* Li, T* tr) {
    if (batch <= 0) return ALGP_OK;
    if (ppad != NB && ppad != 2 * NB) return fail(c, ALGP_ERR_BAD_ARG, "pvr_linv: ppad must be 128 or 256");
    hipLaunchKernelGGL(pvr_linv_kernel<T>, dim3(4, 4, (unsigned)batch), dim3(256), 0, c->cur, inv, L21, ppad, Li, tr);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(pvr_linv_launch);

// u = sum over the lower triangle of W_ij (L^-1)_ij = tr(L^-1 Phi_SS L^-T), W = L^-1 Phi_SS; fp64 sums in a fixed order (a
// thread's strided share, then a tree over the 256 threads); NaN where the factorisation met a bad pivot
template <typename T>
__global__ __launch_bounds__(256) void pvr_trace_kernel(const T* W, const T* Li, int ppad, const int* info, const int* pid, double* out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const T* Wp = W + (int64_t)blockIdx.x * ppad * ppad;
    const T* Lp = Li + (int64_t)blockIdx.x * ppad * ppad;
    double s = 0.0;
    for (int e = tid; e < ppad * ppad; e += 256) {
        const int a = e / ppad, b = e - a * ppad;
        if (b <= a) s += (double)Wp[e] * (double)Lp[e];
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[pid[blockIdx.x]] = info[blockIdx.x] != 0 ? NAN : red[0];
}
template <typename T>
int pvr_trace_launch(algp_ctx* c, const T* W, const T* Li, int ppad, int batch, const int* info, const int* pid, double* out) {
    if (batch <= 0) return ALGP_OK;
    hipLaunchKernelGGL(pvr_trace_kernel<T>, dim3((unsigned)batch), dim3(256), 0, c->cur, W, Li, ppad, info, pid, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(pvr_trace_launch);

// ---------------------------------------------------------------------------------------------
// fused kernel-GEMV: mu_j = ybar + sum_a C(q_j, a) alpha_a WITHOUT the noise term of coinciding sites, the matrix never
// materialised (utils.py:301; for an explicit covariance a gather of its entries).
// One wave per output; lanes stride over the train set (coordinates and alpha are L2 resident).
// ---------------------------------------------------------------------------------------------
template <typename T, int DP, typename S>
__global__ __launch_bounds__(256) void kgemv_kernel(int64_t M, const int64_t* qidx, S src, int64_t N, const int64_t* aidx,
                                                    const T* alpha, T ybar, T* mu) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t j = wave; j < M; j += nw) {
        const int64_t pj = qidx[j];
        T xj[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) xj[d] = src.Cp ? (T)0 : src.Xs[pj * DP + d];
        T s = (T)0;
        for (int64_t a = lane; a < N; a += 64) s += pool_cov<DP, false>(src, pj, aidx[a], xj) * alpha[a];
        s = dot_tree<T>(s);
        if (lane == 0) mu[j] = ybar + s;
    }
}

template <typename T>
int kgemv_launch(algp_ctx* c, int64_t M, const int64_t* qidx, const KmatSrc& s, int64_t N, const int64_t* aidx, const T* alpha, T ybar,
                 T* mu) {
    if (M <= 0) return ALGP_OK;
    int64_t g = (M + 3) / 4;
    if (g > 8192) g = 8192;
    ProfScope ps(c, ALGP_PROF_KMAT, (double)M * N * (s.Cp ? 2.0 : 3.0 * s.DP + 4.0),
                 sizeof(T) * (s.Cp ? (double)M * N : (double)(M + N) * (s.DP + 1)));
    with_src<T>(s, [&](auto src) {
        with_dp(s.DP, [&](auto dp) {
            hipLaunchKernelGGL((kgemv_kernel<T, decltype(dp)::value, decltype(src)>), dim3((unsigned)g), dim3(256), 0, c->cur, M, qidx, src, N,
                               aidx, alpha, ybar, mu);
        });
    });
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(kgemv_launch);

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void pad_identity_kernel(T* A, int64_t n, int64_t npad, int64_t ld) {
    // rows/cols >= n of an npad x npad matrix become identity (the interior is left alone)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= npad * npad) return;
    const int64_t i = e / npad, j = e - i * npad;
    if (i >= n || j >= n) A[i * ld + j] = (i == j) ? (T)1 : (T)0;
}
template <typename T>
int pad_identity_launch(algp_ctx* c, T* A, int64_t n, int64_t npad, int64_t ld) {
    const int64_t tot = npad * npad;
    hipLaunchKernelGGL(pad_identity_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->cur, A, n, npad, ld);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(pad_identity_launch);

// A[i][i] += v for i < n
template <typename T>
__global__ void add_diag_kernel(T* A, int64_t n, int64_t ld, T v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) A[i * ld + i] += v;
}
template <typename T>
int add_diag_launch(algp_ctx* c, T* A, int64_t n, int64_t ld, T v) {
    if (n <= 0) return ALGP_OK;
    hipLaunchKernelGGL(add_diag_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->cur, A, n, ld, v);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(add_diag_launch);

template <typename T>
__global__ void set_identity_kernel(T* A, int64_t npad, int64_t ld) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= npad * npad) return;
    const int64_t i = e / npad, j = e - i * npad;
    A[i * ld + j] = (i == j) ? (T)1 : (T)0;
}
template <typename T>
int set_identity_launch(algp_ctx* c, T* A, int64_t npad, int64_t ld) {
    const int64_t tot = npad * npad;
    hipLaunchKernelGGL(set_identity_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->cur, A, npad, ld);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(set_identity_launch);

// sum_i log L[i][i] for i < n, accumulated into *out (double)
// out[i] = sum_{k >= 128 (i / 128)} X[i][k] z[k] for an upper-triangular X (zero tiles left of the diagonal tile are never read):
// alpha = L^-T z from the X = L^-T a fit iteration's launch leaves behind.  A workgroup per row, the waves' quarters added in
// wave order (the same bits in every run).
template <typename T>
__global__ __launch_bounds__(256) void upper_gemv_kernel(const T* X, int64_t ld, int64_t n, const T* z, T* out) {
    constexpr int VEC = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    __shared__ T red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = blockIdx.x, k0 = i / 128 * 128;
    const T* row = X + i * ld;
    const int64_t nv = (n - k0) / VEC, per = (nv + 3) / 4;
    const int64_t v0 = wave * per, v1 = v0 + per < nv ? v0 + per : nv;
    T s = (T)0;
    for (int64_t v = v0 + lane; v < v1; v += 64) {
        const vec_t x = *reinterpret_cast<const vec_t*>(row + k0 + v * VEC);
        const vec_t a = *reinterpret_cast<const vec_t*>(z + k0 + v * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s += x[e] * a[e];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[i] = (red[0] + red[1]) + (red[2] + red[3]);
}
template <typename T>
int upper_gemv_launch(algp_ctx* c, const T* X, int64_t ld, int64_t n, const T* z, T* out) {
    if (n <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_TRSV, (double)n * n, sizeof(T) * (double)n * n / 2.0);
    hipLaunchKernelGGL(upper_gemv_kernel<T>, dim3((unsigned)n), dim3(256), 0, c->cur, X, ld, n, z, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(upper_gemv_launch);

// acc3[q * stride + rows[e]] = 0 for q < 3: the carried row sums of candidates whose kept columns were zeroed
template <typename T>
__global__ void zero_rows3_kernel(T* acc3, int64_t stride, const int64_t* rows, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < 3 * n) acc3[(e / n) * stride + rows[e % n]] = (T)0;
}
template <typename T>
int zero_rows3_launch(algp_ctx* c, T* acc3, int64_t stride, const int64_t* rows, int64_t n) {
    if (n <= 0) return ALGP_OK;
    hipLaunchKernelGGL(zero_rows3_kernel<T>, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, c->cur, acc3, stride, rows, n);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(zero_rows3_launch);

// X[rows[r]][0:ncols] = 0 for n listed rows (a workgroup per row and 2048 columns): the candidates that became train sites
// in an incremental step restart as unit rows (one memset per row before: ~30 per step of config 5's loop, 0.2 ms in all).
template <typename T>
__global__ __launch_bounds__(256) void zero_listed_rows_kernel(T* X, int64_t ldx, const int64_t* rows, int64_t ncols) {
    T* d = X + rows[blockIdx.x] * ldx;
    const int64_t end = ncols < ((int64_t)blockIdx.y + 1) * 2048 ? ncols : ((int64_t)blockIdx.y + 1) * 2048;
    for (int64_t k = (int64_t)blockIdx.y * 2048 + threadIdx.x; k < end; k += 256) d[k] = (T)0;
}
template <typename T>
int zero_listed_rows_launch(algp_ctx* c, T* X, int64_t ldx, const int64_t* rows, int64_t n, int64_t ncols) {
    if (n <= 0 || ncols <= 0) return ALGP_OK;
    hipLaunchKernelGGL(zero_listed_rows_kernel<T>, dim3((unsigned)n, (unsigned)((ncols + 2047) / 2048)), dim3(256), 0, c->cur, X, ldx, rows, ncols);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(zero_listed_rows_launch);

// Fixed assignment and fixed summation order: the log-determinant of an updated factor is the same number in every run.
// Workgroup b takes entries i = 256 (b + G q) + thread; its 4 wave sums go to part[4 b ..]; logdiag_sum_kernel adds the 4 G
// partials in index order.  (One workgroup walked the 50 000 diagonal entries of config 5's factor -- one cache line each --
// in 157 us of every planning step; 64 take 12.)
constexpr int LOGDIAG_G = 64;
template <typename T>
__global__ __launch_bounds__(256) void logdiag_kernel(const T* L, int64_t ld, int64_t n, double* part) {
    double v = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += 256 * LOGDIAG_G) v += log((double)L[i * ld + i]);
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[4 * blockIdx.x + (threadIdx.x >> 6)] = v;
}
__global__ void logdiag_sum_kernel(const double* part, double* out) {
    double s = 0;
    for (int q = 0; q < 4 * LOGDIAG_G; ++q) s += part[q];
    *out += s;
}
template <typename T>
int logdiag_launch(algp_ctx* c, const T* L, int64_t ld, int64_t n, double* out) {
    if (n <= 0) return ALGP_OK;
    ALGP_TRY(ensure(c, c->ldpart, sizeof(double) * 4 * LOGDIAG_G));
    hipLaunchKernelGGL(logdiag_kernel<T>, dim3(LOGDIAG_G), dim3(256), 0, c->cur, L, ld, n, (double*)c->ldpart.p);
    ALGP_HIP(hipGetLastError());
    hipLaunchKernelGGL(logdiag_sum_kernel, dim3(1), dim3(1), 0, c->cur, (const double*)c->ldpart.p, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(logdiag_launch);

template <typename T>
__global__ void add_doubles_kernel(double* dst, const T* src, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) dst[e] = (double)src[e];
}
template <typename T>
int to_double_launch(algp_ctx* c, double* dst, const T* src, int64_t n) {
    if (n <= 0) return ALGP_OK;
    hipLaunchKernelGGL(add_doubles_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->cur, dst, src, n);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(to_double_launch);

}  // namespace algp
