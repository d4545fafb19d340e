// paths_mi.hip -- best_path under the mutual-information criterion (agent.py:374-400): the device pieces that turn each
// path's two pool-wide log-determinants into small blocks of the resident inverses P = C_AbarAbar^-1 and Q = (C + D)^-1
// (api_paths.hip: score_paths_mi).  Both inverses are kept as X = L^-T on and above the diagonal tiles of their buffer
// (api_mi.hip: mi_build), so a block P_SS (Q_SS) is the Gram matrix of |S| rows of X:
//   mi_tri_gather_kernel   the rows of X, zero left of each row's own diagonal tile (the buffer holds L there)
//   mi_pad_diag_kernel     ones on the diagonal behind a path's sites (padding of the ppad x ppad block)
//   mi_transpose_kernel    from the factor G of Q_SS (2 x 2 tiles of 128: L11, L22 in the block, L21 apart) the two
//                          operands of I + G^T D G = I + Lt (Lt D)^T, D = diag(delta) of the path's noise changes
// The Gram products and the factorisations are the batched launchers of gemm.hip / potrf.hip.
#include "common.h"
#include "vecops.h"

namespace algp {

// dst[r][k] = X[src_row[r]][k] for k >= 128 (src_row[r] / 128), else 0 (and a zero row where src_row[r] < 0);
// one workgroup per row and 2048 columns
template <typename T>
__global__ __launch_bounds__(256) void mi_tri_gather_kernel(const T* X, int64_t ldx, const int64_t* src_row, T* dst, int64_t ldd,
                                                            int64_t ncols) {
    const int64_t r = blockIdx.x, sr = src_row[r];
    T* d = dst + r * ldd;
    const int64_t k0 = (int64_t)blockIdx.y * 2048 + threadIdx.x;
    const int64_t k1 = ncols < ((int64_t)blockIdx.y + 1) * 2048 ? ncols : ((int64_t)blockIdx.y + 1) * 2048;
    if (sr < 0) {
        for (int64_t k = k0; k < k1; k += 256) d[k] = (T)0;
        return;
    }
    const T* sp = X + sr * ldx;
    const int64_t c0 = sr / 128 * 128;
    for (int64_t k = k0; k < k1; k += 256) d[k] = k >= c0 ? sp[k] : (T)0;
}

template <typename T>
int mi_tri_gather_launch(algp_ctx* c, const T* X, int64_t ldx, const int64_t* src_row, T* dst, int64_t ldd, int64_t nrows,
                         int64_t ncols) {
    if (nrows <= 0 || ncols <= 0) return ALGP_OK;
    // a row operation (class ROWS, so that GEMM_OTHER's rate stays the products'); bytes: a triangle row is half a row on
    // average, plus the full row written
    ProfScope ps(c, ALGP_PROF_ROWS, 0.0, sizeof(T) * 1.5 * (double)nrows * ncols);
    hipLaunchKernelGGL(mi_tri_gather_kernel<T>, dim3((unsigned)nrows, (unsigned)((ncols + 2047) / 2048)), dim3(256), 0, c->cur, X, ldx,
                       src_row, dst, ldd, ncols);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mi_tri_gather_launch);

// G[b][a][a] = 1 for cnt[b] <= a < ppad (the Gram of the zero rows behind a path's sites is exactly 0 there)
template <typename T>
__global__ __launch_bounds__(256) void mi_pad_diag_kernel(T* G, int ppad, const int* cnt) {
    const int b = blockIdx.x, a = threadIdx.x;
    if (a < ppad && a >= cnt[b]) G[(int64_t)b * ppad * ppad + (int64_t)a * ppad + a] = (T)1;
}

template <typename T>
int mi_pad_diag_launch(algp_ctx* c, T* G, int ppad, const int* cnt, int batch) {
    if (batch <= 0) return ALGP_OK;
    if (ppad > 256) return fail(c, ALGP_ERR_BAD_ARG, "mi_pad_diag: blocks of at most 256");
    ProfScope ps(c, ALGP_PROF_GEMM_OTHER, 0.0, sizeof(T) * (double)batch * ppad);
    hipLaunchKernelGGL(mi_pad_diag_kernel<T>, dim3((unsigned)batch), dim3(256), 0, c->cur, G, ppad, cnt);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mi_pad_diag_launch);

// Lt[a][b] = G[b][a] (b >= a, else 0) and LtD[a][b] = G[b][a] delta[b], per ppad x ppad block of the batch.  G is the
// factor of the 2 x 2 tiled block: L11 and L22 in the block's diagonal tiles (their strict upper parts are not read),
// L21 in its own NB x NB buffer per path.  64 x 64 tiles through LDS: reads along a, writes along b.
template <typename T>
__global__ __launch_bounds__(256) void mi_transpose_kernel(const T* G, const T* L21, const T* delta, int ppad, T* Lt, T* LtD) {
    __shared__ T tile[64][65];
    const int b_ = blockIdx.z;
    const int tpr = ppad / 64;
    const int ta = blockIdx.x % tpr, tb = blockIdx.x / tpr;            // output tile: rows a in ta, columns b in tb
    const int tid = threadIdx.x;
    const T* Gp = G + (int64_t)b_ * ppad * ppad;
    const T* Lp = L21 + (int64_t)b_ * NB * NB;
    // load source rows b (tile tb), columns a (tile ta): tile[bb][aa] = G[b][a] when b >= a
    for (int e = tid; e < 64 * 64; e += 256) {
        const int bb = e >> 6, aa = e & 63;
        const int b = tb * 64 + bb, a = ta * 64 + aa;
        T v = (T)0;
        if (b >= a) {
            if (b >= NB && a < NB) v = Lp[(int64_t)(b - NB) * NB + a];
            else v = Gp[(int64_t)b * ppad + a];
        }
        tile[bb][aa] = v;
    }
    __syncthreads();
    const T* dl = delta + (int64_t)b_ * ppad;
    T* Lo = Lt + (int64_t)b_ * ppad * ppad;
    T* Do = LtD + (int64_t)b_ * ppad * ppad;
    for (int e = tid; e < 64 * 64; e += 256) {
        const int aa = e >> 6, bb = e & 63;
        const int a = ta * 64 + aa, b = tb * 64 + bb;
        const T v = tile[bb][aa];
        Lo[(int64_t)a * ppad + b] = v;
        Do[(int64_t)a * ppad + b] = v * dl[b];
    }
}

template <typename T>
int mi_transpose_launch(algp_ctx* c, const T* G, const T* L21, const T* delta, int ppad, T* Lt, T* LtD, int batch) {
    if (batch <= 0) return ALGP_OK;
    if (ppad % 64 || ppad > 2 * NB) return fail(c, ALGP_ERR_BAD_ARG, "mi_transpose: ppad must be 128 or 256");
    ProfScope ps(c, ALGP_PROF_GEMM_OTHER, (double)batch * ppad * ppad, sizeof(T) * 3.0 * batch * ppad * ppad);
    const int tpr = ppad / 64;
    hipLaunchKernelGGL(mi_transpose_kernel<T>, dim3((unsigned)(tpr * tpr), 1, (unsigned)batch), dim3(256), 0, c->cur, G, L21, delta,
                       ppad, Lt, LtD);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mi_transpose_launch);

}  // namespace algp
