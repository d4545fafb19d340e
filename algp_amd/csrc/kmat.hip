// kmat.hip -- kernel-matrix build: ScaleKernel(RBF-ARD) / ScaleKernel(Matern-1.5) values, the
// per-point white-noise diagonal and the likelihood-noise diagonal in one pass.
//
// Replaces GPR.cov_mat (reference models.py:161-181): gpytorch materialises an n1 x n2 x D
// difference tensor, then np.diag(var) and np.eye(n) allocate two more dense n x n arrays just to
// add a diagonal (models.py:175-180).  Here every output element is produced once, in registers,
// and stored once: the kernel is HBM-write bound (s * n1 * n2 bytes; 4.6 TB/s of stores at the bench's sizes since
// round 4: 4 KiB-contiguous rows per workgroup, the rows' coordinates staged in LDS, the short fp64 exp of common.h --
// 2.5 -> 2.0 ms per step; non-temporal stores and deeper unrolling: no further change).
//
// Layout: coordinates are pre-scaled by 1/lengthscale and zero padded to DP in {2,4,8} columns
// (scale_coords), so the distance loop is fully unrolled.  A 256-thread workgroup produces a
// 32-row x (256*VEC)-column tile: each lane owns VEC = 16 B / sizeof(T) adjacent columns (its
// column coordinates stay in registers), the four waves sit side by side and walk the same 32 rows
// (coordinates are wave-uniform loads): every row of the tile is written as 4 KiB contiguous.
#include "common.h"

namespace algp {

template <typename T>
struct Vec16;
template <>
struct Vec16<double> {
    typedef double type __attribute__((ext_vector_type(2)));
    static constexpr int N = 2;
};
template <>
struct Vec16<float> {
    typedef float type __attribute__((ext_vector_type(4)));
    static constexpr int N = 4;
};

template <typename T>
struct KmatArgs {
    const T* X1;            // scaled coords of the row side   (n x DP)
    const T* X2;            // scaled coords of the column side
    const T* Cp;            // explicit pool covariance or null
    int64_t n_pool;
    const int64_t* ridx;    // row -> pool index (null: identity)
    const int64_t* cidx;    // col -> pool index (null: identity)
    int64_t rows, rows_pad, cols, cols_pad;
    int64_t row_base;       // first row handled by this launch (gridDim.y is limited to 65535)
    const T* diag_add;      // per-row value added where pool indices coincide (null: none)
    T noise_on_equal;       // added where pool indices coincide
    int same_pool;          // row and column indices address the same pool (equality is meaningful)
    const int* unit;        // unit[r] >= 0: row r is the unit vector e_{unit[r]} (null: none)
    int identity_pad;
    int64_t ident_shift;    // identity padding sits at column r + ident_shift (row windows of a larger matrix)
    int64_t col_shift;      // global column of local column 0 (unit rows compare global columns)
    int kernel;
    T outputscale;
    T* out;
    int64_t ldo;
    // the additive form (FAM = 2; kernel_b < 0: a single form): part b, and the coordinates [0, da) that are part a's.  Behind
    // everything else: the single forms' kernels read their arguments where they always were
    int kernel_b, da;
    T outputscale_b;
    // the relationship form (FAM = 3; Q = 0: another form): the table (null: the identity), its order, the genotype part's
    // outputscale; da is then the coordinate that holds the id
    const T* G;
    int64_t Q;
    T outputscale_g;
    // the separable form (FAM = 4; sep = 0: another form): kernel / kernel_b are the two factors', outputscale the product's, da
    // the split and dg the end of factor b's coordinates -- the id's coordinate while Q > 0 (the genotype term, the table's fields
    // above), the padded width else
    int sep, dg;
};

// (the kernel value itself: kval / kmat_value in common.h, shared with the product epilogue that generates B^T, gemm.hip)

// EQ: entries whose row and column address the same pool site receive a diagonal term (the symmetric builds); without it
// (the candidates' B^T, cross matrices) the index comparisons are not even compiled in -- they and the other per-element
// bookkeeping were half of the kernel's VALU instructions, and the kernel is VALU-issue bound (profiles/r04_valu_by_kernel.json).
// FAM: the family of a.kernel (kernel_family, common.h): one copy of the kernel per family, the form selected inside it; 2: the
// additive form (kmat_value_add), any two of the four forms; 3: the relationship form (kmat_value_rel) -- the ids ride along as the
// last coordinate of the row (LDS) and the column (registers), the table entry is one gather per output element; 4: the separable
// form (kmat_value_sep), with the genotype term while a.Q > 0 (uniform over the launch)
template <typename T, int DP, bool EQ, int FAM>
__global__ __launch_bounds__(256) void kmat_kernel(KmatArgs<T> a) {
    constexpr int VEC = Vec16<T>::N;
    using vec_t = typename Vec16<T>::type;
    // the four waves of a workgroup sit side by side on the same 32 rows: every row of the tile is 4 KiB contiguous
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c0 = (((int64_t)blockIdx.x * 4 + wave) * 64 + lane) * VEC;
    const int64_t r0 = a.row_base + (int64_t)blockIdx.y * 32;

    T xc[VEC][DP];
    int64_t pc[VEC];
    bool live[VEC];                                                // column inside the matrix (not padding): per lane, per launch
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const int64_t c = c0 + v;
        pc[v] = -1;
        live[v] = c < a.cols;
        if (live[v]) {
            pc[v] = a.cidx ? a.cidx[c] : c;
            if (!a.Cp) {
#pragma unroll
                for (int d = 0; d < DP; ++d) xc[v][d] = a.X2[pc[v] * DP + d];
            }
        } else {
#pragma unroll
            for (int d = 0; d < DP; ++d) xc[v][d] = (T)0;
        }
    }
    // the 32 rows' unit flags, pool indices and coordinates once per workgroup into LDS: the row loop then has no
    // dependent global loads (unit -> pool index -> coordinates were three serial scalar loads per row and wave)
    __shared__ int s_u[32];
    __shared__ int64_t s_p[32];
    __shared__ T s_x[32][DP];
    if (threadIdx.x < 32) {
        const int64_t r = r0 + threadIdx.x;
        int u = -1;
        int64_t pr = 0;
        if (r < a.rows) {
            u = a.unit ? a.unit[r] : -1;
            pr = a.ridx ? a.ridx[r] : r;
        }
        s_u[threadIdx.x] = u;
        s_p[threadIdx.x] = pr;
#pragma unroll
        for (int d = 0; d < DP; ++d) s_x[threadIdx.x][d] = (r < a.rows && u < 0 && !a.Cp) ? a.X1[pr * DP + d] : (T)0;
    }
    __syncthreads();
    if (c0 >= a.cols_pad) return;
    const int64_t cend = c0 + VEC;                                 // this lane's columns are [c0, cend)
#pragma unroll 2
    for (int rr = 0; rr < 32; ++rr) {
        const int64_t r = r0 + rr;
        if (r >= a.rows_pad) break;
        vec_t o;
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = (T)0;
        // the row's facts are wave-uniform: told so to the compiler, its branches become scalar branches
        const int u = __builtin_amdgcn_readfirstlane(s_u[rr]);
        if (r < a.rows && u < 0) {
            const int64_t pr = s_p[rr];
            if (a.Cp) {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (live[v]) o[v] = a.Cp[pr * a.n_pool + pc[v]];
            } else {
                T xr[DP];
#pragma unroll
                for (int d = 0; d < DP; ++d) xr[d] = s_x[rr][d];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    T val;
                    if constexpr (FAM == 4) val = kmat_value_sep<T, DP>(a.kernel, a.kernel_b, a.outputscale, a.da, a.dg, a.Q > 0, a.G, a.Q, a.outputscale_g, xr, xc[v]);
                    else if constexpr (FAM == 3) val = kmat_value_rel<T, DP>(a.kernel, a.outputscale, a.G, a.Q, a.outputscale_g, a.da, xr, xc[v]);
                    else if constexpr (FAM == 2) val = kmat_value_add<T, DP>(a.kernel, a.outputscale, a.kernel_b, a.outputscale_b, a.da, xr, xc[v]);
                    else val = kmat_value<T, DP, FAM>(a.kernel, a.outputscale, xr, xc[v]);
                    o[v] = live[v] ? val : (T)0;
                }
            }
            if (EQ) {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (live[v] && a.same_pool && pr == pc[v]) {
                        o[v] += a.noise_on_equal;
                        // the per-row term only on the row's own diagonal entry: two train rows may address the
                        // same site (independent measurements), and their cross entry is C(i,i) without it
                        if (a.diag_add && c0 + v == r + a.ident_shift) o[v] += a.diag_add[r];
                    }
            }
        } else if (r < a.rows) {
            // a unit row e_u (a candidate that is a train site): one 1 in global column u
            const int64_t cu = (int64_t)u - a.col_shift;
            if (cu >= c0 && cu < cend && cu < a.cols) o[(int)(cu - c0)] = (T)1;
        }
        if (a.identity_pad) {
            // the padded diagonal: (r, r + shift) for rows and columns beyond the matrix
            const int64_t cd = r + a.ident_shift;
            if (cd >= c0 && cd < cend && (cd >= a.cols || r >= a.rows)) o[(int)(cd - c0)] = (T)1;
        }
        if (cend <= a.cols_pad) {
            *reinterpret_cast<vec_t*>(a.out + r * a.ldo + c0) = o;
        } else {                                                   // a column count that is no multiple of VEC (a window that starts
#pragma unroll                                                     // at an arbitrary column of V^T): never store beyond it
            for (int v = 0; v < VEC; ++v)
                if (c0 + v < a.cols_pad) a.out[r * a.ldo + c0 + v] = o[v];
        }
    }
}

template <typename T>
static int kmat_dispatch(algp_ctx* c, const KmatArgs<T>& a, int DP) {
    constexpr int VEC = Vec16<T>::N;
    if (a.rows_pad <= 0 || a.cols_pad <= 0) return ALGP_OK;
    const int64_t gx = (a.cols_pad + 256 * VEC - 1) / (256 * VEC);
    const int64_t gy = (a.rows_pad + 31) / 32;
    const double elems = (double)a.rows_pad * (double)a.cols_pad;
    ProfScope ps(c, ALGP_PROF_KMAT, elems * (3.0 * DP + 2.0), sizeof(T) * elems);
    const int64_t ymax = 65535;
    for (int64_t y0 = 0; y0 < gy; y0 += ymax) {
        KmatArgs<T> b = a;
        const int64_t ny = (gy - y0 < ymax) ? gy - y0 : ymax;
        b.row_base = y0 * 32;
        dim3 grid((unsigned)gx, (unsigned)ny);
        const bool eq = a.same_pool && (a.noise_on_equal != (T)0 || a.diag_add != nullptr);
        auto launch = [&](auto fam) {
            constexpr int FAM = decltype(fam)::value;
            with_dp(DP, [&](auto dp) {
                if (eq) hipLaunchKernelGGL((kmat_kernel<T, decltype(dp)::value, true, FAM>), grid, dim3(256), 0, c->cur, b);
                else hipLaunchKernelGGL((kmat_kernel<T, decltype(dp)::value, false, FAM>), grid, dim3(256), 0, c->cur, b);
            });
        };
        if (a.sep && !a.Cp) launch(std::integral_constant<int, 4>{});
        else if (a.Q > 0 && !a.Cp) launch(std::integral_constant<int, 3>{});
        else if (a.kernel_b >= 0 && !a.Cp) launch(std::integral_constant<int, 2>{});
        else if (kernel_family(a.kernel)) launch(std::integral_constant<int, 1>{});
        else launch(std::integral_constant<int, 0>{});
    }
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}

template <typename T>
int kmat_launch(algp_ctx* c, const KmatSrc& s, const int64_t* ridx, int64_t rows, int64_t rows_pad,
                const int64_t* cidx, int64_t cols, int64_t cols_pad, const T* diag_add, int add_noise_on_equal,
                const int* unit, int identity_pad, T* out, int64_t ldo, int64_t ident_shift, int64_t col_shift) {
    KmatArgs<T> a;
    a.X1 = (const T*)s.Xs;
    a.X2 = (const T*)s.Xs;
    a.Cp = (const T*)s.Cp;
    a.n_pool = s.n_pool;
    a.ridx = ridx;
    a.cidx = cidx;
    a.rows = rows; a.rows_pad = rows_pad; a.cols = cols; a.cols_pad = cols_pad;
    a.diag_add = diag_add;
    a.noise_on_equal = (T)(add_noise_on_equal ? s.noise : 0.0);
    a.same_pool = 1;
    a.unit = unit;
    a.identity_pad = identity_pad;
    a.ident_shift = ident_shift;
    a.col_shift = col_shift;
    a.kernel = s.kernel;
    a.outputscale = (T)s.outputscale;
    a.kernel_b = s.kernel_b; a.da = s.da; a.outputscale_b = (T)s.outputscale_b;
    a.G = (const T*)s.G; a.Q = s.Q; a.outputscale_g = (T)s.outputscale_g;
    a.sep = s.sep ? 1 : 0; a.dg = s.dg;
    a.out = out;
    a.ldo = ldo;
    return kmat_dispatch<T>(c, a, s.DP);
}
ALGP_INSTANTIATE(kmat_launch);

template <typename T>
int kmat_xy_launch(algp_ctx* c, const T* xs1, int64_t n1, const T* xs2, int64_t n2, int symmetric,
                   const T* diag_add, double add_noise, T* out, int64_t ldo) {
    KmatArgs<T> a;
    a.X1 = xs1;
    a.X2 = symmetric ? xs1 : xs2;
    a.Cp = nullptr;
    a.n_pool = 0;
    a.ridx = nullptr;
    a.cidx = nullptr;
    a.rows = n1; a.rows_pad = n1; a.cols = n2; a.cols_pad = round_up(n2, Vec16<T>::N);
    a.diag_add = symmetric ? diag_add : nullptr;
    a.noise_on_equal = (T)(symmetric ? add_noise : 0.0);
    a.same_pool = symmetric;
    a.unit = nullptr;
    a.identity_pad = 0;
    a.ident_shift = 0;
    a.col_shift = 0;
    a.kernel = c->hyp.kernel;
    a.outputscale = (T)c->hyp.outputscale;
    a.kernel_b = (c->hyp.additive || c->hyp.sep) ? c->hyp.kernel_b : -1; a.da = c->hyp.Da; a.outputscale_b = (T)c->hyp.outputscale_b;
    a.G = c->hyp.has_ids() && c->hyp.has_table ? (const T*)c->Gtab.p : nullptr; a.Q = c->hyp.has_ids() ? c->hyp.Q : 0;
    a.sep = c->hyp.sep ? 1 : 0; a.dg = c->hyp.sep && c->hyp.Q > 0 ? c->hyp.idc() : c->hyp.DP;
    a.outputscale_g = (T)c->hyp.outputscale_g;
    a.out = out;
    a.ldo = ldo;
    return kmat_dispatch<T>(c, a, c->hyp.DP);
}
ALGP_INSTANTIATE(kmat_xy_launch);

// The candidates' right-hand sides as a generator (RhsGen, common.h): the coordinates of the candidate rows and of the train
// columns gathered into two contiguous arrays, once per solve, so that the product epilogue that forms B^T entries has no
// index -> coordinate dependent loads; and the rows' kinds (-1 ordinary, >= 0 a unit row's column, -2 padding).
template <typename T>
__global__ void rhs_gather_kernel(const T* Xs, int DP, const int64_t* ridx, int64_t rows, int64_t rows_pad, const int* unit,
                                  const int64_t* cidx, int64_t cols, int64_t cols_pad, T* rx, T* cx, int* rk) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows_pad) {
        const bool live = i < rows;
        const int u = live ? (unit ? unit[i] : -1) : -2;
        rk[i] = u < -1 ? -2 : u;
        const int64_t p = live ? ridx[i] : 0;
        for (int d = 0; d < DP; ++d) rx[i * DP + d] = (live && u < 0) ? Xs[p * DP + d] : (T)0;
    } else if (i - rows_pad < cols_pad) {
        const int64_t j = i - rows_pad;
        const bool live = j < cols;
        const int64_t p = live ? cidx[j] : 0;
        for (int d = 0; d < DP; ++d) cx[j * DP + d] = live ? Xs[p * DP + d] : (T)0;
    }
}
template <typename T>
int rhs_gather_launch(algp_ctx* c, const T* Xs, int DP, const int64_t* ridx, int64_t rows, int64_t rows_pad, const int* unit,
                      const int64_t* cidx, int64_t cols, int64_t cols_pad, T* rx, T* cx, int* rk) {
    const int64_t tot = rows_pad + cols_pad;
    if (tot <= 0) return ALGP_OK;
    hipLaunchKernelGGL(rhs_gather_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->cur, Xs, DP, ridx, rows, rows_pad, unit,
                       cidx, cols, cols_pad, rx, cx, rk);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(rhs_gather_launch);

// xs[i][d] = x[i][d] / lengthscale_d for d < D, 0 for D <= d < DP
struct InvLs {
    double v[MAXD];
};

template <typename T>
__global__ void scale_coords_kernel(const T* x, int64_t n, int D, int DP, InvLs inv_ls8, T* xs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * DP) return;
    const int64_t p = i / DP;
    const int d = (int)(i - p * DP);
    xs[i] = d < D ? x[p * D + d] * (T)inv_ls8.v[d] : (T)0;
}

template <typename T>
int scale_coords_launch(algp_ctx* c, const T* x, int64_t n, T* xs) {
    if (n <= 0) return ALGP_OK;
    InvLs il;
    for (int d = 0; d < MAXD; ++d) il.v[d] = c->hyp.inv_ls[d];
    const int64_t tot = n * c->hyp.DP;
    hipLaunchKernelGGL(scale_coords_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->cur, x, n,
                       c->hyp.D, c->hyp.DP, il, xs);
    ALGP_HIP(hipGetLastError());
    return ALGP_OK;
}
ALGP_INSTANTIATE(scale_coords_launch);

}  // namespace algp
