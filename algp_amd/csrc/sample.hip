// sample.hip -- the kernels of algp_sample_posterior (api_sample.hip): the prior draw of a pathwise-conditioned sample at a
// list of pool sites, by random Fourier features on the matrix cores or gathered from values the caller supplies, with the
// two epilogues of common.h (SampleEpi); the conversion of the call's host doubles.
#include "common.h"
#include "mfma.h"

namespace algp {

__device__ __forceinline__ float kcos(float x) { return cosf(x); }
__device__ __forceinline__ double kcos(double x) { return cos(x); }
__device__ __forceinline__ float ksqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double ksqrt(double x) { return sqrt(x); }

// one entry of the result from the prior draw g of (row, s): see SampleEpi
template <typename T>
__device__ __forceinline__ void sample_store(const SampleEpi<T>& e, int64_t row, int s, T g) {
    T v = (T)0;
    if (row < e.nrows) {
        if (!e.y0) v = e.ybar + g;
        else if (s < e.slive) v = e.y0[row] - g - ksqrt(e.var[row] + e.noise) * e.eps[(int64_t)s * e.ld + row];
    }
    e.out[(int64_t)s * e.ld + row] = v;
}

template <typename T>
struct FeatArgs {
    const T* Xs;
    const int64_t* idx;
    const T* Wt;
    const T* om;
    const T* ph;
    int64_t Fpad;
    T scale;
    SampleEpi<T> e;
};

// The feature product: 128 rows x 128 samples per workgroup, K = Fpad.  Four waves of 32 rows each (two 16-row blocks) against
// the tile's eight 16-sample blocks: per k-step of 4 features a lane computes the two cosines of its A fragments -- A[i = lane & 15]
// [k = lane >> 4] is one scalar per lane, so the lane that feeds the instruction forms it from its rows' coordinates (registers)
// and that k's frequency and phase (LDS) -- and reuses each across the eight blocks: 16 MFMAs per 2 cosines.  Only the weights
// are staged (KT x 128 per k-tile, row stride 144: the four feature rows of a B fragment fall on disjoint banks in both widths);
// no feature matrix exists in memory or in LDS.  Accumulators: 2 x 8 fragments = 64 values per lane, in arch VGPRs.
constexpr int SAMPLE_WLD = SAMPLE_TILE + 16;
template <typename T, int DP>
__global__ __launch_bounds__(256, 2) void sample_features_kernel(FeatArgs<T> a) {
    using M = MF<T>;
    using acc_t = typename M::acc_t;
    constexpr int KT = SAMPLE_KT;
    __shared__ T sW[KT][SAMPLE_WLD];
    __shared__ T sOm[KT][DP];
    __shared__ T sPh[KT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * 128 + wave * 32;
    T x[2][DP];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int64_t r = row0 + rb * 16 + (lane & 15);
        const bool live = r < a.e.nrows;
        const int64_t q = live ? a.idx[r] : 0;
#pragma unroll
        for (int d = 0; d < DP; ++d) x[rb][d] = live ? a.Xs[q * DP + d] : (T)0;
    }
    acc_t acc[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int jb = 0; jb < 8; ++jb)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[rb][jb][r] = (T)0;
    for (int64_t f0 = 0; f0 < a.Fpad; f0 += KT) {
        __syncthreads();
        for (int e = tid; e < KT * SAMPLE_TILE; e += 256) sW[e >> 7][e & 127] = a.Wt[(f0 + (e >> 7)) * SAMPLE_TILE + (e & 127)];
        if (tid < KT * DP) sOm[tid / DP][tid % DP] = a.om[f0 * DP + tid];
        if (tid < KT) sPh[tid] = a.ph[f0 + tid];
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < KT; kk += 4) {
            const int f = kk + (lane >> 4);
            T av[2];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                T arg = sPh[f];
#pragma unroll
                for (int d = 0; d < DP; ++d) arg = kfma(x[rb][d], sOm[f][d], arg);
                av[rb] = kcos(arg);
            }
#pragma unroll
            for (int jb = 0; jb < 8; ++jb) {
                const T b = sW[f][jb * 16 + (lane & 15)];
                acc[0][jb] = M::mfma(av[0], b, acc[0][jb]);
                acc[1][jb] = M::mfma(av[1], b, acc[1][jb]);
            }
        }
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int jb = 0; jb < 8; ++jb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                sample_store(a.e, row0 + rb * 16 + M::row_of(lane, r), jb * 16 + (lane & 15), a.scale * acc[rb][jb][r]);
}

template <typename T>
int sample_features_launch(algp_ctx* c, const T* Xs, int DP, const int64_t* idx, const T* Wt, const T* om, const T* ph,
                           int64_t Fpad, int64_t flop_f, T scale, const SampleEpi<T>& e) {
    if (e.ld <= 0) return ALGP_OK;
    if (e.ld % 128 || Fpad % SAMPLE_KT) return fail(c, ALGP_ERR_BAD_ARG, "sample_features: operands must be padded");
    FeatArgs<T> a = {Xs, idx, Wt, om, ph, Fpad, scale, e};
    ProfScope ps(c, ALGP_PROF_GEMM_OTHER, 2.0 * (double)e.nrows * (double)e.slive * (double)flop_f,
                 sizeof(T) * ((double)e.ld * SAMPLE_TILE * (e.y0 ? 2.0 : 1.0) + (double)Fpad * SAMPLE_TILE));
    with_dp(DP, [&](auto dp) {
        hipLaunchKernelGGL((sample_features_kernel<T, decltype(dp)::value>), dim3((unsigned)(e.ld / 128)), dim3(256), 0, c->cur, a);
    });
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(sample_features_launch);

template <typename T>
__global__ void sample_values_kernel(const T* prior, int64_t n_pool, const int64_t* idx, SampleEpi<T> e) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (row >= e.ld) return;
    sample_store(e, row, s, row < e.nrows ? prior[(int64_t)s * n_pool + idx[row]] : (T)0);
}
template <typename T>
int sample_values_launch(algp_ctx* c, const T* prior, int64_t n_pool, const int64_t* idx, const SampleEpi<T>& e) {
    if (e.ld <= 0) return ALGP_OK;
    hipLaunchKernelGGL(sample_values_kernel<T>, dim3((unsigned)((e.ld + 255) / 256), SAMPLE_TILE), dim3(256), 0, c->cur, prior, n_pool,
                       idx, e);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(sample_values_launch);

template <typename T>
__global__ void sample_convert_kernel(const double* src, int64_t rows, int64_t cols, T* dst, int64_t rows_pad, int64_t cols_pad,
                                      int64_t ldd, int transposed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows_pad * cols_pad) return;
    // the fast index runs along dst's rows in either orientation
    const int64_t r = transposed ? e % rows_pad : e / cols_pad, q = transposed ? e / rows_pad : e % cols_pad;
    const T v = (r < rows && q < cols) ? (T)src[r * cols + q] : (T)0;
    dst[transposed ? q * ldd + r : r * ldd + q] = v;
}
template <typename T>
int sample_convert_launch(algp_ctx* c, const double* src, int64_t rows, int64_t cols, T* dst, int64_t rows_pad, int64_t cols_pad,
                          int64_t ldd, int transposed) {
    const int64_t tot = rows_pad * cols_pad;
    if (tot <= 0) return ALGP_OK;
    hipLaunchKernelGGL(sample_convert_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->cur, src, rows, cols, dst,
                       rows_pad, cols_pad, ldd, transposed);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(sample_convert_launch);

}  // namespace algp
