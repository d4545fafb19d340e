// fixed.hip -- fixed effects (a linear mean h(x)' beta beside the constant): the kernels behind algp_get_gls and
// algp_get_posterior_fixed (api_fixed.hip).  With H_A the basis rows of the train sites, S = L L^T and z = L^-1 (y - ybar):
//
//   F = L^-1 H_A (N x p)     A = F^T F     b = F^T z     beta = A^-1 b     A^-1 = C C^T (C = R^-1 upper, A = R^T R)
//   candidates (resident V^T = B^T L^-T):  R_j = h_j - V_j F,  mu_j += R_j beta,  var_j += |C^T R_j|^2,  proj_j = R_j C
//
// fixed_gather_kernel   F^T's right-hand sides: row a of a 16 x Npad panel = column a of H at the train sites (zero behind N, zero
//                       rows behind p); the blocked triangular solve turns the panel into F^T in place
// fixed_gram_kernel     A, b and z'z: the (p + 1) x (p + 1) Gram product of F^T's rows and z in double, one order per entry
// fixed_gls_kernel      the p x p work in double by one thread: A scaled to a unit diagonal, its Cholesky factor, C, beta, C C^T
// fixed_post_kernel     one pass over V^T: sixteen dot products per row on the 16x16x4 MFMA (16 candidate rows x 16 basis columns
//                       per instruction) and the epilogue above
// and for the restricted likelihood l_R = -1/2 [(N - p) log 2 pi + log|S| + log|A| + z'z - b' beta] as a fit objective, with
// P = S^-1 - G G^T, G = L^-T F C, alpha_R = L^-T (z - F beta):
// fixed_fc_kernel       the rows of (F C)^T (G^T is their product with X = L^-T, gemm_nt_launch)
// fixed_resid_kernel    z - F beta (alpha_R is its backward substitution)
// fixed_downdate_kernel S^-1 -> P on the lower-triangle entries mll_grad_kernel reads: the gradient is that kernel on (P, alpha_R)
// fixed_gram2_kernel    the average information's products v_a . v_b and F^T v_a (v_a: mll_ai_u_kernel's rows from alpha_R, solved)
// and for the read-outs that carry the estimated effects (the genotype effects, the mean at pool sites):
// fixed_fold_kernel     out (+)= P Qm^T for two panels of p columns: the covariance's term for beta's uncertainty, streamed
// fixed_trend_kernel    h_j' beta at pool sites
// (the pass over a row panel other than V^T -- W = B L^-T -- is fixed_post_kernel itself with a zero basis row: R = -W F)
// No atomics; the sum along a row of V^T has one order whatever the grid, so two calls return the same bits.
#include "common.h"
#include "mfma.h"
#include "vecops.h"

namespace algp {

template <typename T>
__global__ __launch_bounds__(256) void fixed_gather_kernel(const T* H, const int64_t* aidx, int64_t N, int64_t Npad, T* Pn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Npad) return;
    const T* h = i < N ? H + aidx[i] * FX_P : nullptr;
#pragma unroll
    for (int a = 0; a < FX_P; ++a) Pn[(int64_t)a * Npad + i] = h ? h[a] : (T)0;
}
template <typename T>
int fixed_gather_launch(algp_ctx* c, const T* H, const int64_t* aidx, int64_t N, int64_t Npad, T* Pn) {
    if (Npad <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_ROWS, 0.0, sizeof(T) * 2.0 * FX_P * (double)Npad);
    hipLaunchKernelGGL(fixed_gather_kernel<T>, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, c->cur, H, aidx, N, Npad, Pn);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_gather_launch);

// out[a (p + 1) + b] = out[b (p + 1) + a] = sum_{i < N} r_a[i] r_b[i] for b <= a <= p, r_a = row a of Ft for a < p and z for a = p:
// mll_ai_gram_kernel's summation order (thread-strided, a shuffle tree, the four waves left to right) without its factor 1/2
template <typename T>
__global__ __launch_bounds__(256) void fixed_gram_kernel(const T* Ft, int64_t ld, const T* z, int64_t N, int p, double* out) {
    int a = 0, b = (int)blockIdx.x;
    while (b > a) {
        b -= a + 1;
        ++a;
    }
    const T* va = a < p ? Ft + (int64_t)a * ld : z;
    const T* vb = b < p ? Ft + (int64_t)b * ld : z;
    double v = 0;
    for (int64_t i = threadIdx.x; i < N; i += 256) v += (double)va[i] * (double)vb[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double r = (part[0] + part[1]) + (part[2] + part[3]);
        out[a * (p + 1) + b] = r;
        out[b * (p + 1) + a] = r;
    }
}
template <typename T>
int fixed_gram_launch(algp_ctx* c, const T* Ft, int64_t ld, const T* z, int64_t N, int p, double* out) {
    const int q = p + 1;
    ProfScope ps(c, ALGP_PROF_GEMM_OTHER, (double)q * (q + 1) * (double)N, sizeof(T) * (double)q * (q + 1) * (double)N);
    hipLaunchKernelGGL(fixed_gram_kernel<T>, dim3((unsigned)(q * (q + 1) / 2)), dim3(256), 0, c->cur, Ft, ld, z, N, p, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_gram_launch);

// The p x p work, in double: As = D A D with D = diag(A)^-1/2 (a unit diagonal: the columns of H may differ by orders of
// magnitude), As = Ls Ls^T, C = D Ls^-T (upper: A^-1 = C C^T, C the inverse of A's upper Cholesky factor), beta = C C^T b.
// A pivot of the scaled matrix at or below tol says that column is in the span of the ones before it at the precision F was
// computed in: info = its 1-based number, nothing else is written.  g: the Gram product above, (p + 1) x (p + 1).
__host__ __device__ inline void fixed_gls_small(const double* g, int p, double tol, double* out) {
    const int q = p + 1;
    double d[FX_P], Ls[FX_P][FX_P], Li[FX_P][FX_P];
    out[FX_INFO] = 0.0;
    for (int a = 0; a < p; ++a) {
        const double gaa = g[a * q + a];
        if (!(gaa > 0.0)) { out[FX_INFO] = (double)(a + 1); return; }
        d[a] = 1.0 / sqrt(gaa);
    }
    for (int a = 0; a < p; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = (g[a * q + b] * d[a]) * d[b];
            for (int k = 0; k < b; ++k) s -= Ls[a][k] * Ls[b][k];
            if (a == b) {
                if (!(s > tol)) { out[FX_INFO] = (double)(a + 1); return; }
                Ls[a][a] = sqrt(s);
            } else {
                Ls[a][b] = s / Ls[b][b];
            }
        }
    // Li = Ls^-1 (lower), column by column
    for (int b = 0; b < p; ++b)
        for (int a = 0; a < p; ++a) {
            if (a < b) { Li[a][b] = 0.0; continue; }
            double s = a == b ? 1.0 : 0.0;
            for (int k = b; k < a; ++k) s -= Ls[a][k] * Li[k][b];
            Li[a][b] = s / Ls[a][a];
        }
    // C[a][b] = d_a Li[b][a] (upper)
    double* C = out + FX_C;
    for (int a = 0; a < FX_P; ++a)
        for (int b = 0; b < FX_P; ++b) C[a * FX_P + b] = (a < p && b < p && a <= b) ? d[a] * Li[b][a] : 0.0;
    double t[FX_P];                                              // C^T b
    for (int b = 0; b < p; ++b) {
        double s = 0.0;
        for (int a = 0; a <= b; ++a) s += C[a * FX_P + b] * g[a * q + p];
        t[b] = s;
    }
    double quad = 0.0, ld = 0.0;
    for (int a = 0; a < FX_P; ++a) {
        double s = 0.0;
        for (int b = a; b < p; ++b) s += C[a * FX_P + b] * t[b];
        out[FX_BETA + a] = a < p ? s : 0.0;
    }
    for (int b = 0; b < p; ++b) quad += t[b] * t[b];             // b' beta = |C^T b|^2
    for (int a = 0; a < p; ++a) ld += 2.0 * (log(Ls[a][a]) - log(d[a]));
    for (int a = 0; a < p; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = 0.0;
            for (int k = a; k < p; ++k) s += C[a * FX_P + k] * C[b * FX_P + k];
            out[FX_COV + a * p + b] = s;
            out[FX_COV + b * p + a] = s;
        }
    out[FX_LOGDET_A] = ld;
    out[FX_QUAD] = quad;
    out[FX_ZZ] = g[p * q + p];
}
__global__ void fixed_gls_kernel(const double* g, int p, double tol, double* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) fixed_gls_small(g, p, tol, out);
}
int fixed_gls_launch(algp_ctx* c, const double* g, int p, double tol, double* out) {
    ProfScope ps(c, ALGP_PROF_GEMM_OTHER, (double)p * p * p, 8.0 * FX_OUT);
    hipLaunchKernelGGL(fixed_gls_kernel, dim3(1), dim3(64), 0, c->cur, g, p, tol, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}

// ---- the restricted likelihood's gradient and average information --------------------------------------------------------
// FCt[b][k] = sum_{a <= b} C[a][b] Ft[a][k] for b < FX_P, k < npad: the rows of (F C)^T, products and sums in double
template <typename T>
__global__ __launch_bounds__(256) void fixed_fc_kernel(const T* Ft, int64_t npad, const double* gls, T* FCt) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= npad) return;
    double f[FX_P];
#pragma unroll
    for (int a = 0; a < FX_P; ++a) f[a] = (double)Ft[(int64_t)a * npad + k];
#pragma unroll
    for (int b = 0; b < FX_P; ++b) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a <= b; ++a) s = __builtin_fma(gls[FX_C + a * FX_P + b], f[a], s);
        FCt[(int64_t)b * npad + k] = (T)s;
    }
}
template <typename T>
int fixed_fc_launch(algp_ctx* c, const T* Ft, int64_t npad, const double* gls, T* FCt) {
    ProfScope ps(c, ALGP_PROF_ROWS, (double)FX_P * FX_P * (double)npad, sizeof(T) * 2.0 * FX_P * (double)npad);
    hipLaunchKernelGGL(fixed_fc_kernel<T>, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, c->cur, Ft, npad, gls, FCt);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_fc_launch);

// w[i] = z[i] - sum_a Ft[a][i] beta[a] for i < N, 0 behind: alpha_R = L^-T w is the projected alpha P (y - ybar)
template <typename T>
__global__ __launch_bounds__(256) void fixed_resid_kernel(const T* Ft, int64_t npad, int64_t N, const T* z, const double* gls, T* w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    double s = 0.0;
    if (i < N) {
        s = (double)z[i];
#pragma unroll
        for (int a = 0; a < FX_P; ++a) s = __builtin_fma(-(double)Ft[(int64_t)a * npad + i], gls[FX_BETA + a], s);
    }
    w[i] = (T)s;
}
template <typename T>
int fixed_resid_launch(algp_ctx* c, const T* Ft, int64_t npad, int64_t N, const T* z, const double* gls, T* w) {
    ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * FX_P * (double)npad, sizeof(T) * (FX_P + 2.0) * (double)npad);
    hipLaunchKernelGGL(fixed_resid_kernel<T>, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, c->cur, Ft, npad, N, z, gls, w);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_resid_launch);

// The rank-p downdate S^-1 -> P = S^-1 - G G^T on the entries the gradient's kernel reads: j <= i < N, by 64 x 64 tiles of the
// lower triangle (mll_grad_kernel's grid).  Gt is G^T (FX_P x ldg); the tile's two 64 x FX_P slabs of G are staged in LDS; every
// entry takes p fused multiply-adds in ascending order of the basis column.  No atomics: an entry has one writer.
template <typename T>
__global__ __launch_bounds__(256) void fixed_downdate_kernel(T* Sinv, int64_t ld, int64_t N, const T* Gt, int64_t ldg, int p) {
    int bi = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((int64_t)(bi + 1) * (bi + 2) / 2 <= (int64_t)blockIdx.x) ++bi;
    while ((int64_t)bi * (bi + 1) / 2 > (int64_t)blockIdx.x) --bi;
    const int bj = (int)(blockIdx.x - (int64_t)bi * (bi + 1) / 2);
    __shared__ T gi[FX_P][64], gj[FX_P][64];
    for (int e = threadIdx.x; e < FX_P * 64; e += 256) {
        const int a = e >> 6, l = e & 63;
        const int64_t ri = (int64_t)bi * 64 + l, rj = (int64_t)bj * 64 + l;
        gi[a][l] = (a < p && ri < N) ? Gt[(int64_t)a * ldg + ri] : (T)0;
        gj[a][l] = (a < p && rj < N) ? Gt[(int64_t)a * ldg + rj] : (T)0;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t j = (int64_t)bj * 64 + tx;
    if (j >= N) return;
#pragma unroll 4
    for (int rr = 0; rr < 16; ++rr) {
        const int li = ty * 16 + rr;
        const int64_t i = (int64_t)bi * 64 + li;
        if (i >= N || j > i) continue;
        T s = Sinv[i * ld + j];
        for (int a = 0; a < p; ++a) s = __builtin_fma(-gi[a][li], gj[a][tx], s);
        Sinv[i * ld + j] = s;
    }
}
template <typename T>
int fixed_downdate_launch(algp_ctx* c, T* Sinv, int64_t ld, int64_t N, const T* Gt, int64_t ldg, int p) {
    if (N <= 0) return ALGP_OK;
    const unsigned nb = (unsigned)((N + 63) / 64);
    ProfScope ps(c, ALGP_PROF_ROWS, (double)p * (double)N * N, sizeof(T) * (double)N * N);
    hipLaunchKernelGGL(fixed_downdate_kernel<T>, dim3(nb * (nb + 1) / 2), dim3(256), 0, c->cur, Sinv, ld, N, Gt, ldg, p);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_downdate_launch);

// out[r (P + p) + s] = sum_{i < N} V[r][i] W_s[i] for r < P, s < P + p, W_s = V's row s for s < P, Ft's row s - P behind: the
// average information's products v_a . v_b and F^T v_a.  One workgroup per entry, fixed_gram_kernel's order; entry (r, s) and
// (s, r) of the V V^T block add the same products in the same order: symmetric bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void fixed_gram2_kernel(const T* V, const T* Ft, int64_t ld, int64_t N, int P, int p, double* out) {
    const int r = (int)blockIdx.x / (P + p), s = (int)blockIdx.x % (P + p);
    const T* va = V + (int64_t)r * ld;
    const T* vb = s < P ? V + (int64_t)s * ld : Ft + (int64_t)(s - P) * ld;
    double v = 0;
    for (int64_t i = threadIdx.x; i < N; i += 256) v += (double)va[i] * (double)vb[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
template <typename T>
int fixed_gram2_launch(algp_ctx* c, const T* V, const T* Ft, int64_t ld, int64_t N, int P, int p, double* out) {
    ProfScope ps(c, ALGP_PROF_GEMM_OTHER, 2.0 * P * (P + p) * (double)N, sizeof(T) * 2.0 * P * (P + p) * (double)N);
    hipLaunchKernelGGL(fixed_gram2_kernel<T>, dim3((unsigned)(P * (P + p))), dim3(256), 0, c->cur, V, Ft, ld, N, P, p, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_gram2_launch);

// The posterior pass.  One wave owns 64 rows of V^T as four groups of 16 and walks the columns KT at a time: lane (r, g) = (lane
// & 15, lane >> 4) loads 16 bytes of row r of each group and of row r of F^T at columns k0 + 4 E u + E g (E elements per 16
// bytes, u < 4), and element s of that chunk is the lane's operand of MFMA (u, s): the instruction's k index is g, so both
// operands name column k0 + 4 E u + E g + s.  Four lanes cover 64 contiguous bytes of a row per u, 256 per step.  The four groups'
// accumulators are independent chains; F^T (16 x ncols, from L2) is read once per 64 rows.  A row's sum runs over (k0, u, s, g)
// in that order whatever the grid.  Columns in [N, ncols) are zero in both operands (the solve's padding), rows >= M of the last
// group are computed and dropped.  Epilogue: the 64 x 16 products through LDS, then lane l finishes row 64 b + l in double with
// beta and C (gls: fixed_gls_small's output) in ascending order of the basis column.
template <typename T>
__global__ __launch_bounds__(64) void fixed_post_kernel(const T* Vt, int64_t ldv, int64_t M, int64_t ncols, const T* Ft, int64_t ldf,
                                                        const T* H, const int64_t* cidx, const double* gls, int p, const T* mu_in,
                                                        const T* var_in, T* mu_out, T* var_out, T* proj_out) {
    using MFT = MF<T>;
    using chunk_t = typename MFT::chunk_t;
    using acc_t = typename MFT::acc_t;
    constexpr int E = MFT::EPC, U = 4, RG = 4, KT = 4 * E * U;
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    __shared__ double sR[64][FX_P + 1];
    if (gls[FX_INFO] != 0.0) return;                              // a rank-deficient basis: the host reports it
    acc_t acc[RG];
#pragma unroll
    for (int q = 0; q < RG; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q][e] = (T)0;
    const T* fb = Ft + (int64_t)r * ldf + E * g;
    const T* va = Vt + (row0 + r) * ldv + E * g;
    for (int64_t k0 = 0; k0 < ncols; k0 += KT) {
        chunk_t bf[U], af[RG][U];
#pragma unroll
        for (int u = 0; u < U; ++u) bf[u] = *reinterpret_cast<const chunk_t*>(fb + k0 + 4 * E * u);
#pragma unroll
        for (int q = 0; q < RG; ++q)
#pragma unroll
            for (int u = 0; u < U; ++u) af[q][u] = *reinterpret_cast<const chunk_t*>(va + (int64_t)(16 * q) * ldv + k0 + 4 * E * u);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int s = 0; s < E; ++s)
#pragma unroll
                for (int q = 0; q < RG; ++q) acc[q] = MFT::mfma(af[q][u][s], bf[u][s], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < RG; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) sR[16 * q + MFT::row_of(lane, e)][r] = (double)acc[q][e];
    __syncthreads();
    const int64_t j = row0 + lane;
    if (j >= M) return;
    const T* h = H + cidx[j] * FX_P;
    double R[FX_P];
#pragma unroll
    for (int a = 0; a < FX_P; ++a) R[a] = a < p ? (double)h[a] - sR[lane][a] : 0.0;
    double m = 0.0, v = 0.0;
#pragma unroll
    for (int a = 0; a < FX_P; ++a) m = __builtin_fma(R[a], gls[FX_BETA + a], m);
    for (int b = 0; b < p; ++b) {
        double t = 0.0;
        for (int a = 0; a <= b; ++a) t = __builtin_fma(R[a], gls[FX_C + a * FX_P + b], t);
        v = __builtin_fma(t, t, v);
        if (proj_out) proj_out[j * p + b] = (T)t;
    }
    if (mu_out) mu_out[j] = (T)((double)mu_in[j] + m);
    if (var_out) var_out[j] = (T)((double)var_in[j] + v);
}
template <typename T>
int fixed_post_launch(algp_ctx* c, const T* Vt, int64_t ldv, int64_t M, int64_t ncols, const T* Ft, int64_t ldf, const T* H,
                      const int64_t* cidx, const double* gls, int p, const T* mu_in, const T* var_in, T* mu_out, T* var_out, T* proj_out) {
    if (M <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * FX_P * (double)M * (double)ncols, sizeof(T) * (double)M * (double)ncols);
    hipLaunchKernelGGL(fixed_post_kernel<T>, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, c->cur, Vt, ldv, M, ncols, Ft, ldf, H, cidx, gls,
                       p, mu_in, var_in, mu_out, var_out, proj_out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_post_launch);

// ---- the read-outs with the estimated effects (algp_genotype_posterior_fixed, algp_group_posterior_fixed,
// algp_posterior_mean_fixed, algp_sample_posterior_fixed) ------------------------------------------------------------------------
// The rank-p fold: out[i][j] += sign sum_{a < p} P[i][a] Qm[j][a] for i < rows, j < cols -- the term (R C)(R' C)^T that beta's
// uncertainty adds to a covariance (the genotype effects', the groups' Q x Q and Q x M) and, with sign = -1, R_j beta_s in a tile of
// draws.  A streaming pass over out: a workgroup owns FOLD_ROWS rows x 256 chunks of 16 bytes; the rows
// of P are staged in LDS (zero behind p and behind the last row), a lane keeps Qm's rows of its chunk's columns in registers (zero
// behind p) and walks down the rows with one 16-byte load and store per row where the leading dimension allows, element by element
// where it does not (an odd packed Q x Q).  Every entry takes FX_P fused multiply-adds in ascending order of the basis column from
// 0 (the padding adds exact zeros), then one addition onto (sign = 1) or subtraction from (sign = -1) what is there: one writer per
// entry, no atomics, and with P = Qm the entries (i, j) and (j, i) get the same bits (a product commutes; out's own are equal).
constexpr int FOLD_ROWS = 64;
template <typename T>
__global__ __launch_bounds__(256) void fixed_fold_kernel(T* out, int64_t ldo, int64_t rows, int64_t cols, const T* P, int64_t ldp, const T* Qm,
                                                         int64_t ldq, int p, int sign) {
    constexpr int E = 16 / (int)sizeof(T);
    struct alignas(16) chunk_t { T v[E]; };
    __shared__ T sP[FOLD_ROWS][FX_P];
    const int64_t i0 = (int64_t)blockIdx.y * FOLD_ROWS;
    for (int e = threadIdx.x; e < FOLD_ROWS * FX_P; e += 256) {
        const int li = e / FX_P, a = e % FX_P;
        sP[li][a] = (a < p && i0 + li < rows) ? P[(i0 + li) * ldp + a] : (T)0;
    }
    __syncthreads();
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * E;
    if (j0 >= cols) return;
    T q[E][FX_P];
#pragma unroll
    for (int s = 0; s < E; ++s)
#pragma unroll
        for (int a = 0; a < FX_P; ++a) q[s][a] = (a < p && j0 + s < cols) ? Qm[(j0 + s) * ldq + a] : (T)0;
    const bool whole = ldo % E == 0 && j0 + E <= cols;
    const int nr = (int)(rows - i0 < FOLD_ROWS ? rows - i0 : FOLD_ROWS);
    auto update = [&](int li, chunk_t& c) {
#pragma unroll
        for (int s = 0; s < E; ++s) {
            T t = (T)0;
#pragma unroll
            for (int a = 0; a < FX_P; ++a) t = __builtin_fma(sP[li][a], q[s][a], t);
            c.v[s] = sign > 0 ? c.v[s] + t : c.v[s] - t;
        }
    };
    if (whole) {
        // FOLD_AHEAD rows' loads are issued before the first of them is used: a lane keeps that many 16-byte reads in flight
        constexpr int FOLD_AHEAD = 4;
        for (int l0 = 0; l0 < nr; l0 += FOLD_AHEAD) {
            chunk_t c[FOLD_AHEAD];
#pragma unroll
            for (int u = 0; u < FOLD_AHEAD; ++u)
                if (l0 + u < nr) c[u] = *reinterpret_cast<const chunk_t*>(out + (i0 + l0 + u) * ldo + j0);
#pragma unroll
            for (int u = 0; u < FOLD_AHEAD; ++u)
                if (l0 + u < nr) {
                    update(l0 + u, c[u]);
                    *reinterpret_cast<chunk_t*>(out + (i0 + l0 + u) * ldo + j0) = c[u];
                }
        }
        return;
    }
    for (int li = 0; li < nr; ++li) {
        T* o = out + (i0 + li) * ldo + j0;
        chunk_t c;
#pragma unroll
        for (int s = 0; s < E; ++s) c.v[s] = j0 + s < cols ? o[s] : (T)0;
        update(li, c);
#pragma unroll
        for (int s = 0; s < E; ++s)
            if (j0 + s < cols) o[s] = c.v[s];
    }
}
template <typename T>
int fixed_fold_launch(algp_ctx* c, T* out, int64_t ldo, int64_t rows, int64_t cols, const T* P, int64_t ldp, const T* Qm, int64_t ldq, int p,
                      int sign) {
    if (rows <= 0 || cols <= 0) return ALGP_OK;
    constexpr int E = 16 / (int)sizeof(T);
    const int64_t gx = (cols + 256 * E - 1) / (256 * E), gy = (rows + FOLD_ROWS - 1) / FOLD_ROWS;
    if (gy > 65535 || gx > INT32_MAX) return fail(c, ALGP_ERR_BAD_ARG, "fixed_fold: the matrix is too large for one launch");
    if ((uintptr_t)out % 16 != 0) return fail(c, ALGP_ERR_BAD_ARG, "fixed_fold: the matrix is not aligned to 16 bytes");
    if (sign != 1 && sign != -1) return fail(c, ALGP_ERR_BAD_ARG, "fixed_fold: sign is 1 or -1");
    ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * FX_P * (double)rows * (double)cols, sizeof(T) * 2.0 * (double)rows * (double)cols);
    hipLaunchKernelGGL(fixed_fold_kernel<T>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, c->cur, out, ldo, rows, cols, P, ldp, Qm, ldq, p,
                       sign);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_fold_launch);

// out[j] (+)= sum_{a < p} H[idx[j]][a] beta[a] for j < M, in double in ascending order of the basis column: the trend's share
// h_j' beta of the mean at pool sites (idx: pool indices on the device)
template <typename T>
__global__ __launch_bounds__(256) void fixed_trend_kernel(const T* H, const int64_t* idx, int64_t M, const double* gls, int p, int add, T* out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const T* h = H + idx[j] * FX_P;
    double m = 0.0;
    for (int a = 0; a < p; ++a) m = __builtin_fma((double)h[a], gls[FX_BETA + a], m);
    out[j] = (T)(add ? (double)out[j] + m : m);
}
template <typename T>
int fixed_trend_launch(algp_ctx* c, const T* H, const int64_t* idx, int64_t M, const double* gls, int p, bool add, T* out) {
    if (M <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_ROWS, 2.0 * p * (double)M, sizeof(T) * (FX_P + 2.0) * (double)M);
    hipLaunchKernelGGL(fixed_trend_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->cur, H, idx, M, gls, p, add ? 1 : 0, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_trend_launch);

// out[j][a] = H[idx[j]][a] for j < M, a < FX_P: the basis rows of listed pool sites, packed (the operand of the sums by group)
template <typename T>
__global__ __launch_bounds__(256) void fixed_rows_kernel(const T* H, const int64_t* idx, int64_t M, T* out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * FX_P) return;
    out[e] = H[idx[e / FX_P] * FX_P + e % FX_P];
}
template <typename T>
int fixed_rows_launch(algp_ctx* c, const T* H, const int64_t* idx, int64_t M, T* out) {
    if (M <= 0) return ALGP_OK;
    ProfScope ps(c, ALGP_PROF_ROWS, 0.0, sizeof(T) * 2.0 * FX_P * (double)M);
    hipLaunchKernelGGL(fixed_rows_kernel<T>, dim3((unsigned)((M * FX_P + 255) / 256)), dim3(256), 0, c->cur, H, idx, M, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(fixed_rows_launch);

// Timing on device-resident zeroed operands, no host traffic (algp_bench_fixed_fold, algp_bench_fixed_panel): the average ms per
// launch of the fold on a rows x cols matrix beside a device-to-device copy of that matrix, and of the posterior pass over a
// rows x ncols panel with a zero basis row (how W, T and a sample tile Z^T go through it).
template <typename T>
int bench_fixed(algp_ctx* c, int64_t rows, int64_t cols, int p, int reps, double* fold_ms, double* copy_ms, double* panel_ms) {
    constexpr int E = 16 / (int)sizeof(T);
    const int64_t ld = (cols + E - 1) / E * E, rpad = (rows + 63) / 64 * 64;
    DevBuf a, b, sm;
    const size_t small = sizeof(T) * (size_t)(rows + cols + rpad + 2) * FX_P + sizeof(int64_t) * (size_t)rpad + sizeof(double) * FX_OUT +
                         sizeof(T) * 2 * (size_t)rpad + 4096;
    int rc = ensure(c, a, sizeof(T) * (size_t)rpad * (size_t)ld);
    if (rc == ALGP_OK) rc = ensure(c, b, fold_ms ? sizeof(T) * (size_t)rows * (size_t)ld : 16);
    if (rc == ALGP_OK) rc = ensure(c, sm, small);
    auto done = [&](int r) {
        hipFree(a.p); hipFree(b.p); hipFree(sm.p);
        c->dev_bytes -= (int64_t)(a.cap + b.cap + sm.cap);
        return r;
    };
    if (rc != ALGP_OK) return done(rc);
    hipMemsetAsync(a.p, 0, sizeof(T) * (size_t)rpad * (size_t)ld, c->cur);
    hipMemsetAsync(sm.p, 0, small, c->cur);
    // carved from sm, 256 bytes apart at least: gls | idx | P | Qm | h0 | mu, var | proj | Ft
    char* q = (char*)sm.p;
    auto take = [&](size_t bytes) { char* o = q; q += (bytes + 255) / 256 * 256; return o; };
    double* gls = (double*)take(sizeof(double) * FX_OUT);
    int64_t* idx = (int64_t*)take(sizeof(int64_t) * (size_t)rpad);
    T* P = (T*)take(sizeof(T) * (size_t)rows * FX_P);
    T* Qm = (T*)take(sizeof(T) * (size_t)cols * FX_P);
    T* h0 = (T*)take(sizeof(T) * FX_P);
    T* mu = (T*)take(sizeof(T) * 2 * (size_t)rpad);
    T* proj = (T*)take(sizeof(T) * (size_t)rpad * FX_P);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    auto timed = [&](auto&& one, double* out) {
        for (int w = 0; w < 2 && rc == ALGP_OK; ++w) rc = one();
        hipEventRecord(e0, c->cur);
        for (int r = 0; r < reps && rc == ALGP_OK; ++r) rc = one();
        hipEventRecord(e1, c->cur);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        *out = ms / reps;
    };
    if (fold_ms) {
        timed([&] { return fixed_fold_launch<T>(c, (T*)a.p, ld, rows, cols, P, p, Qm, p, p, 1); }, fold_ms);
        timed([&] { return hipMemcpyAsync(b.p, a.p, sizeof(T) * (size_t)rows * (size_t)ld, hipMemcpyDeviceToDevice, c->cur) == hipSuccess
                               ? ALGP_OK : ALGP_ERR_HIP; }, copy_ms);
    }
    if (panel_ms) {
        DevBuf ft;                                                // F^T: FX_P x cols
        rc = ensure(c, ft, sizeof(T) * FX_P * (size_t)ld);
        if (rc == ALGP_OK) {
            hipMemsetAsync(ft.p, 0, sizeof(T) * FX_P * (size_t)ld, c->cur);
            timed([&] { return fixed_post_launch<T>(c, (const T*)a.p, ld, rows, cols, (const T*)ft.p, ld, h0, idx, gls, p, mu, mu + rpad, mu,
                                                    mu + rpad, proj); }, panel_ms);
        }
        hipFree(ft.p);
        c->dev_bytes -= (int64_t)ft.cap;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return done(rc);
}
ALGP_INSTANTIATE(bench_fixed);

}  // namespace algp
