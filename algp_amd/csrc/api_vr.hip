// api_vr.hip -- the variance-reduction (ALC) criterion: the utility of a candidate is how much its static reading lowers
// the summed predictive variance of the targets T (the ordinary rows of the candidate set, fixed by the solve), see
// include/algp_hip.h.  With the signed cross term E_jc = [c ordinary] C(j, c) - (V V^T)_jc, the target weights omega (one per
// pool site, algp_set_target_weights; 1 where none are attached) and w_c = sum_{j in T} omega_j E_jc^2,
//   u_c = w_c / (pv_c + ss) (ordinary c)        u_c = -delta w_c / (1 + delta s_cc) (unit c),
// so the state is the vector w (VrState, common.h); new weights drop it.
//   First scoring after a solve (vr_product): w is the row sums of the squared M x M matrix E over its target columns -- one
//     fused product V^T V on the matrix cores whose epilogue forms E in registers and leaves one partial sum per row and
//     128-column tile (gemm.hip: gemm_nt_launch_vr); neither E nor a kernel-matrix block is written.  The column tiles go in
//     chunks of VR_CHUNK so that the partial sums stay small, and are added in tile order (vr_combine_kernel).
//   Every later pick (vr_fold): its appended column r of V^T gives E' = E - r_T r_c^T, hence
//     w'_c = w_c - 2 r_c y_c + r_c^2 sum_T omega_j r_j^2 with rt = (omega r)_T and
//     y = E^T rt = kappa_c sum_{j in T} C(j, c) rt_j - V_c . (V_T^T rt):
//     a fused kernel-GEMV (or a row gather of an explicit covariance) and two passes over V^T instead of the product.
//   $ALGP_VR_RANK1=0 (cross-check): the full product at every scoring.
#include "api_impl.h"

using namespace algp;

namespace algp {

constexpr int VR_CHUNK = 64;             // column tiles per launch of the product: 64 x Mpad partial sums

void release(algp_ctx* c, VrState& vr) {
    for (DevBuf* b : {&vr.W, &vr.Part, &vr.R, &vr.Tp, &vr.Tv, &vr.Y, &vr.Nrm, &vr.Obj}) release(c, *b);
    vr.drop();
}

static bool lists_site_twice(const algp_ctx* c) {
    std::vector<int64_t> sorted(c->cand_idx);
    std::sort(sorted.begin(), sorted.end());
    return std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
}

// w for the current state of V^T (all committed picks included), from scratch
template <typename T>
int Impl<T>::vr_product(algp_ctx* c) {
    VrState& vr = c->vr;
    vr.drop();
    const int64_t M = c->M, Mpad = c->Mpad, Npad = c->Npad, ldv = c->ldv;
    const int64_t q = (int64_t)c->picks.size();
    int64_t K = Npad;
    if (q > 0) {
        // the picks' columns [Npad, Npad + q) ride along as one more 128-column k block: whatever else that block holds
        // (columns no pick has written yet; the padding rows behind M, which never get a pick's entry) is zeroed first
        K = Npad + NB;
        if (q < NB)
            ALGP_HIP(hipMemset2DAsync(p(c->Vt) + Npad + q, sizeof(T) * ldv, 0, sizeof(T) * (NB - q), Mpad, c->stream));
        if (Mpad > M)
            ALGP_HIP(hipMemset2DAsync(p(c->Vt) + M * ldv + Npad, sizeof(T) * ldv, 0, sizeof(T) * NB, Mpad - M, c->stream));
    }
    const int tiles = (int)(Mpad / NB);
    const int chunk = std::min(tiles, VR_CHUNK);
    ALGP_TRY(ensure(c, vr.W, sizeof(T) * Mpad));
    ALGP_TRY(ensure(c, vr.Part, sizeof(T) * (size_t)chunk * Mpad));
    const KmatSrc s = make_src(c);
    for (int t0 = 0; t0 < tiles; t0 += chunk) {
        const int nt = std::min(chunk, tiles - t0);
        ALGP_TRY(gemm_nt_launch_vr<T>(c, ALGP_PROF_GEMM_OTHER, Mpad, (int64_t)nt * NB, K, p(c->Vt), ldv, (int64_t)t0 * NB, s,
                                      (const int64_t*)c->Cidx.p, (const int*)c->ckind.p, M, c->has_tw ? (const T*)c->tw.p : nullptr,
                                      p(vr.Part), Mpad));
        ALGP_TRY(vr_combine_launch<T>(c, p(vr.Part), Mpad, nt, M, t0 > 0, p(vr.W)));
    }
    vr.npicks = q;
    vr.valid = true;
    return ALGP_OK;
}

// fold pick number q (0-based; its column of V^T is Npad + q, and E before it reads the columns left of that) into w
template <typename T>
int Impl<T>::vr_fold(algp_ctx* c, int64_t q) {
    VrState& vr = c->vr;
    const int64_t M = c->M, Mpad = c->Mpad, ldv = c->ldv;
    ALGP_TRY(ensure(c, vr.R, sizeof(T) * 2 * Mpad));
    ALGP_TRY(ensure(c, vr.Y, sizeof(T) * 2 * Mpad));
    ALGP_TRY(ensure(c, vr.Tp, sizeof(T) * (size_t)VR_TBLOCKS * ldv));
    ALGP_TRY(ensure(c, vr.Tv, sizeof(T) * ldv));
    ALGP_TRY(ensure(c, vr.Nrm, sizeof(T)));
    return vr_fold_launch<T>(c, M, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, p(c->Vt), ldv, c->Npad + q, (const T*)c->Xs.p,
                             c->pool_is_cov ? (const T*)c->Cp.p : nullptr, c->n_pool, c->hyp.DP, c->hyp.kernel,
                             (T)c->hyp.outputscale, (T)c->hyp.noise, c->has_tw ? (const T*)c->tw.p : nullptr, p(vr.R), p(vr.R) + Mpad,
                             p(vr.Nrm), p(vr.Tp), p(vr.Tv), p(vr.Y), p(vr.Y) + Mpad, p(vr.W));
}

// utilities of every row into dst (device), stream-ordered; the rows are flushed (scores_enqueue)
template <typename T>
int Impl<T>::vr_scores_enqueue(algp_ctx* c, double ss, double delta, double* dst) {
    if (c->cextra.p)
        return fail(c, ALGP_ERR_STATE, "variance_reduction: candidates with an extra variance of their own are not supported");
    const bool rank1 = env_switch("ALGP_VR_RANK1", true);       // read per call: the tests flip it
    VrState& vr = c->vr;
    const int64_t q = (int64_t)c->picks.size();
    if (c->M > 0) {
        if (!vr.valid || !rank1 || vr.npicks > q) {
            // a pool site listed twice would be two targets with sigma_n^2 between them, which only the product sees (the fold
            // adds sigma_n^2 on a row's own entry alone): refused rather than scored two ways
            if (lists_site_twice(c))
                return fail(c, ALGP_ERR_STATE, "variance_reduction: the candidate set lists a pool site more than once");
            ALGP_TRY(vr_product(c));
        } else {
            while (vr.npicks < q) {
                const int rc = vr_fold(c, vr.npicks);
                if (rc != ALGP_OK) { vr.drop(); return rc; }
                ++vr.npicks;
            }
        }
    }
    return vr_score_launch<T>(c, c->M, (const int*)c->ckind.p, (const unsigned char*)c->alive.p, (const T*)c->dstat.p,
                              (const T*)vr.W.p, ss, delta, dst);
}

// the pool's target weights (host doubles, checked by the caller; null: detach) to the device in the context's dtype
template <typename T>
int Impl<T>::set_target_weights(algp_ctx* c, const double* w) {
    if (w) {
        std::vector<T> h((size_t)c->n_pool);
        for (int64_t q = 0; q < c->n_pool; ++q) h[(size_t)q] = (T)w[q];
        ALGP_TRY(sync(c));                                      // nothing enqueued still reads the old weights
        ALGP_TRY(ensure(c, c->tw, sizeof(T) * (size_t)c->n_pool));
        ALGP_HIP(hipMemcpyAsync(c->tw.p, h.data(), sizeof(T) * (size_t)c->n_pool, hipMemcpyHostToDevice, c->stream));
        ALGP_TRY(sync(c));
    }
    c->has_tw = w != nullptr;
    c->vr.drop();                                               // the next scoring is the full product, picks included
    return ALGP_OK;
}

// sum_{j in T} omega_j pv_j under the current state (committed picks included): one workgroup, a fixed order
template <typename T>
int Impl<T>::target_variance(algp_ctx* c, double* sum) {
    if (!c->solved) return fail(c, ALGP_ERR_STATE, "get_target_variance: call algp_solve_candidates first");
    if (c->cextra.p)
        return fail(c, ALGP_ERR_STATE, "get_target_variance: candidates with an extra variance of their own are not supported");
    if (lists_site_twice(c))
        return fail(c, ALGP_ERR_STATE, "get_target_variance: the candidate set lists a pool site more than once");
    ALGP_TRY(flush_lazy(c));
    ALGP_TRY(ensure(c, c->vr.Obj, sizeof(double)));
    ALGP_TRY(vr_target_sum_launch<T>(c, c->M, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, (const T*)c->dstat.p,
                                     c->has_tw ? (const T*)c->tw.p : nullptr, (double*)c->vr.Obj.p));
    ALGP_HIP(hipMemcpyAsync(sum, c->vr.Obj.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_set_target_weights(algp_ctx* c, const double* w, int64_t n_pool) {
    CHECK_CTX(c);
    if (c->n_pool <= 0) return fail(c, ALGP_ERR_STATE, "set_target_weights: set a pool first");
    if (w) {
        if (n_pool != c->n_pool)
            return fail(c, ALGP_ERR_BAD_ARG, "set_target_weights: " + std::to_string(n_pool) + " weights for a pool of " +
                                                 std::to_string(c->n_pool) + " sites");
        for (int64_t q = 0; q < n_pool; ++q)
            if (!(std::isfinite(w[q]) && w[q] >= 0.0))
                return fail(c, ALGP_ERR_BAD_ARG, "set_target_weights: weight " + std::to_string(q) + " is not finite and >= 0");
    }
    FINISH(c, DISPATCH(c, set_target_weights(c, w)));
}

int algp_get_target_variance(algp_ctx* c, double* sum) {
    CHECK_CTX(c);
    if (!sum) return fail(c, ALGP_ERR_BAD_ARG, "get_target_variance: bad arguments");
    FINISH(c, DISPATCH(c, target_variance(c, sum)));
}

}  // extern "C"
