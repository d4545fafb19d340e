// mi_shard.hip -- the device side of the MI criterion dealt over ranks (api_mi.hip): a rank holds the 128-row blocks
// b = member, member + g, member + 2g, ... of X = L^-T for one pool-wide matrix (g ranks share it), computes them from the
// factor on the MFMA GEMM path, and per committed pick turns its rows into its entries of the pick's column of P = X X^T.
// Every rank then rebuilds the whole column from the gathered pieces and folds it with mi_rank1_kernel (vecops.hip).
#include "common.h"
#include "vecops.h"
#include <algorithm>

namespace algp {

// local row tile t <-> global row block t g + member (the deal of rows over the g ranks of a group)
__host__ __device__ inline int64_t mi_local_block(int64_t t, int g, int member) { return t * g + member; }

// X (nloc x 128 rows, ldx) <- zero, then the identity tile of every local row tile at its global block's columns
template <typename T>
__global__ __launch_bounds__(128) void mi_rows_ident_kernel(T* X, int64_t ldx, int g, int member) {
    const int64_t t = blockIdx.x;
    const int r = threadIdx.x;
    X[(t * NB + r) * ldx + mi_local_block(t, g, member) * NB + r] = (T)1;
}

// local row tiles whose global block is <= kb: a prefix of the local rows (the blocks ascend with t)
static int64_t mi_tiles_upto(int64_t kb, int64_t nloc, int g, int member) {
    if (kb < member) return 0;
    return std::min<int64_t>(nloc, (kb - member) / g + 1);
}

// A rank's rows of X = L^-T: the rows solve X L^T = E, E the identity rows of their blocks.  Row tile t is zero left of its
// global block, so column tile k0 involves only the local tiles whose block is <= k0 / 128 -- a prefix of the local rows --
// and the push of a finished column block into the trailing columns only the tiles left of its end: trinv_upper's sweep with
// `rows = k0 + 128` replaced by that prefix.  Cost: sum over the rank's blocks b of 128 (n - 128 b)^2 multiply-adds
// (~ n^3 / (3 g) flop); the tiles that would only ever see zeros are never launched.  op: X the rank's nloc x 128 rows (mpad unused).
template <typename T>
int mi_trinv_rows(algp_ctx* c, const TrsmOp<T>& op, int64_t nloc, int g, int member) {
    const auto& [klass, X, mpad, ldx, L, npad, ldl, invD] = op;
    if (nloc <= 0) return ALGP_OK;
    if (nloc > 65535) return fail(c, ALGP_ERR_BAD_ARG, "mi_trinv_rows: too many row blocks");
    if (mi_local_block(nloc - 1, g, member) * NB >= npad) return fail(c, ALGP_ERR_BAD_ARG, "mi_trinv_rows: a row block outside the matrix");
    ALGP_HIP(hipMemsetAsync(X, 0, sizeof(T) * (size_t)nloc * NB * ldx, c->cur));
    hipLaunchKernelGGL(mi_rows_ident_kernel<T>, dim3((unsigned)nloc), dim3(NB), 0, c->cur, X, ldx, g, member);
    ALGP_HIP(hipGetLastError());
    for (int64_t j0 = 0; j0 < npad; j0 += WB) {
        const int64_t w = std::min<int64_t>(WB, npad - j0), j1 = j0 + w;
        ALGP_TRY(block_solve_right<T>(c, op, j0, j1, [&](int64_t k0) { return mi_tiles_upto(k0 / NB, nloc, g, member) * NB; }));
        if (j1 >= npad) break;
        const int64_t rows = mi_tiles_upto(j1 / NB - 1, nloc, g, member) * NB;
        if (rows > 0)
            ALGP_TRY(gemm_nt_launch<T>(c, klass, rows, npad - j1, w, (T)-1, X + j0, ldx, L + j1 * ldl + j0, ldl, (T)1, X + j1, ldx, X + j1, ldx, 0));
    }
    return ALGP_OK;
}
ALGP_INSTANTIATE(mi_trinv_rows);

// The local form of mi_rank1_kernel's first half: raw[t] = (X X_c^T) at local row t (rows_reduce_kernel) -> the entry of the
// pick's column at that row's global index with the earlier picks' rank-1 terms removed, into this rank's piece `out`
// (zero for the padding rows of the last block).  U (q terms, full length, ldu) and sgn are replicated on every rank.
template <typename T>
__global__ __launch_bounds__(256) void mi_cols_local_kernel(int64_t rows, int g, int member, int64_t m, const T* raw, const T* U,
                                                            int64_t ldu, const double* sgn, int q, int64_t cpos, T* out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows) return;
    const int64_t gj = mi_local_block(t / NB, g, member) * NB + t % NB;
    double cj = 0.0;
    if (gj < m) {
        cj = (double)raw[t];
        for (int r = 0; r < q; ++r) cj -= sgn[r] * (double)U[(int64_t)r * ldu + gj] * (double)U[(int64_t)r * ldu + cpos];
    }
    out[t] = (T)cj;
}
template <typename T>
int mi_cols_local_launch(algp_ctx* c, int64_t rows, int g, int member, int64_t m, const T* raw, const T* U, int64_t ldu,
                         const double* sgn, int q, int64_t cpos, T* out) {
    if (rows <= 0) return ALGP_OK;
    hipLaunchKernelGGL(mi_cols_local_kernel<T>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->cur, rows, g, member, m, raw, U,
                       ldu, sgn, q, cpos, out);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mi_cols_local_launch);

// dst[j] (j < m) <- the piece of the rank that owns global row j: rank first + (j / 128) mod g, its local row
// (j / 128) / g * 128 + j mod 128, in its payload at gathered + rank * stride + off bytes
template <typename T>
__global__ __launch_bounds__(256) void mi_assemble_kernel(int64_t m, int g, int first, const char* gathered, int64_t stride, int64_t off,
                                                          T* dst) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int64_t b = j / NB;
    const T* piece = (const T*)(gathered + (int64_t)(first + (int)(b % g)) * stride + off);
    dst[j] = piece[b / g * NB + j % NB];
}
template <typename T>
int mi_assemble_launch(algp_ctx* c, int64_t m, int g, int first, const char* gathered, int64_t stride, int64_t off, T* dst) {
    if (m <= 0) return ALGP_OK;
    hipLaunchKernelGGL(mi_assemble_kernel<T>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->cur, m, g, first, gathered, stride,
                       off, dst);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(mi_assemble_launch);

}  // namespace algp
