// api_fit.hip -- one iteration of GPR.fit (models.py:145-158): MLL and its gradient w.r.t. the log hyper-parameters; the
// average-information matrix of the MLL in the same parameters (algp_get_mll_ai).
#include "api_impl.h"

using namespace algp;

namespace algp {


// have_X: c->auxW already holds X = L^-T (it rode along with the factorisation as an identity panel); inv_enqueued: and
// S^-1 = X X^T is already running on the helper stream (event 21 marks its end)
template <typename T>
int Impl<T>::mll_grad(algp_ctx* c, double* grad_out, bool have_X, bool inv_enqueued) {
    if (!c->factored || c->train_dirty) return fail(c, ALGP_ERR_STATE, "get_mll_grad: call algp_factorize first");
    if (c->pool_is_cov) return fail(c, ALGP_ERR_BAD_ARG, "get_mll_grad needs a coordinate pool");
    const int64_t N = c->N, Npad = c->Npad;
    if (have_X && !c->alpha_valid) {
        // alpha = L^-T z = X z with the X the launch left in auxW: one pass over its upper triangle (0.4 GB at N = 10 000)
        // instead of the backward substitution's chain of 79 hand-offs
        ALGP_TRY(upper_gemv_launch<T>(c, p(c->auxW), Npad, Npad, (const T*)c->z.p, p(c->alpha)));
        c->alpha_valid = true;
    }
    ALGP_TRY(need_alpha(c));
    ALGP_TRY(ensure(c, c->auxA, sizeof(T) * Npad * Npad));
    // X = I L^-T = L^-T ;  S^-1 = X X^T (lower tiles)
    if (!have_X) {
        ALGP_TRY(ensure(c, c->auxW, sizeof(T) * Npad * Npad));
        ALGP_TRY(set_identity_launch<T>(c, p(c->auxW), Npad, Npad));
        ALGP_TRY(trinv_upper<T>(c, ALGP_PROF_GEMM_OTHER, p(c->auxW), Npad, Npad, p(c->L), c->Lld, p(c->invD)));
    }
    if (inv_enqueued) ALGP_HIP(hipStreamWaitEvent(c->stream, sync_event(c, EV_INV_DONE), 0));
    else ALGP_TRY(syrk_upper<T>(c, ALGP_PROF_GEMM_OTHER, p(c->auxW), Npad, Npad, p(c->auxA), Npad));
    // slots 16..27: [0, nos) the outputscale sums (two under the additive and the relationship form: os_a, then os_b or os_g),
    // [nos] the noise trace, [nos + 1, nos + 1 + DP) the lengthscale sums
    double* sc = (double*)c->scal.p + SC_GRAD;
    ALGP_HIP(hipMemsetAsync(sc, 0, sizeof(double) * 12, c->stream));
    ALGP_TRY(mll_grad_launch<T>(c, p(c->auxA), Npad, N, (const int64_t*)c->Aidx.p, (const T*)c->alpha.p, make_src(c), sc,
                                (double*)c->auxW.p /* X = L^-T is spent: room for the per-workgroup partials */));
    double h[12];
    ALGP_HIP(hipMemcpyAsync(h, sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    {
        const int rc = sync_checked(c, "get_mll_grad");
        if (rc != ALGP_OK) { c->alpha_valid = false; return rc; }
    }
    // [log ls | the log outputscales | log sigma_n^2]; under the relationship form the id has no lengthscale
    const int nos = c->hyp.n_os(), nl = c->hyp.n_ls();
    for (int d = 0; d < nl; ++d) grad_out[d] = 0.5 * h[nos + 1 + d];
    for (int q = 0; q < nos; ++q) grad_out[nl + q] = 0.5 * h[q];
    grad_out[nl + nos] = 0.5 * c->hyp.noise * h[nos];
    return ALGP_OK;
}


// The average-information matrix AI_ab = 1/2 alpha' dS/dtheta_a S^-1 dS/dtheta_b alpha in the gradient's parameter order (fit_ai.hip):
//   U (128 x Npad, P live rows)    u_a = dS/dtheta_a alpha, one pass over the N^2 pairs              mll_ai_u_launch
//   V = U L^-T, in place           the blocked triangular solve through its plan                    trsm_blocked
//   AI = 1/2 V V^T (P x P)         a fixed-order reduction in double, both triangles from one value  mll_ai_gram_launch
// Beyond bringing alpha up to date nothing of the resident state is written, and nothing is expected in auxA / auxW; the scratch
// is one buffer of the context (algp_ctx::ai), counted by algp_device_bytes and freed by algp_destroy.  One synchronisation.
template <typename T>
int Impl<T>::mll_ai(algp_ctx* c, double* ai_out) {
    if (!c->factored || c->train_dirty) return fail(c, ALGP_ERR_STATE, "get_mll_ai: call algp_factorize first");
    if (c->pool_is_cov) return fail(c, ALGP_ERR_BAD_ARG, "get_mll_ai needs a coordinate pool");
    const int64_t N = c->N, Npad = c->Npad;
    // [log ls | the log outputscales | log sigma_n^2]; under the relationship form the id has no lengthscale
    const int nos = c->hyp.n_os(), nl = c->hyp.n_ls(), P = nl + nos + 1;
    if (N <= 0) {
        for (int e = 0; e < P * P; ++e) ai_out[e] = 0.0;
        return ALGP_OK;
    }
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t o = total; total += (bytes + 255) / 256 * 256; return o; };
    const size_t o_U = take(sizeof(T) * (size_t)NB * (size_t)Npad);
    const size_t o_out = take(sizeof(double) * (size_t)P * (size_t)P);
    if (total > c->ai.cap) {
        size_t free_b = 0, total_b = 0;
        ALGP_HIP(hipMemGetInfo(&free_b, &total_b));
        if (total > c->ai.cap + free_b)
            return fail(c, ALGP_ERR_OOM, "get_mll_ai: the scratch of " + std::to_string(N) + " train rows takes " + std::to_string(total) +
                                             " bytes, " + std::to_string(c->ai.cap + free_b) + " available");
    }
    ALGP_TRY(ensure(c, c->ai, total));
    ALGP_TRY(need_alpha(c));
    T* U = (T*)((char*)c->ai.p + o_U);
    double* out = (double*)((char*)c->ai.p + o_out);
    // the rows behind the P live ones ride through the solve as zeros (the panel is one 128-row tile)
    ALGP_HIP(hipMemsetAsync(U + (int64_t)P * Npad, 0, sizeof(T) * (size_t)(NB - P) * (size_t)Npad, c->stream));
    ALGP_TRY(mll_ai_u_launch<T>(c, N, Npad, (const int64_t*)c->Aidx.p, (const T*)c->alpha.p, make_src(c), nl, U));
    ALGP_TRY(trsm_blocked<T>(c, {.klass = ALGP_PROF_GEMM_TRSM, .X = U, .mpad = NB, .ldx = Npad, .L = p(c->L), .npad = Npad, .ldl = c->Lld,
                                 .invD = p(c->invD)}));
    ALGP_TRY(mll_ai_gram_launch<T>(c, U, Npad, N, P, out));
    ALGP_HIP(hipMemcpyAsync(ai_out, out, sizeof(double) * (size_t)P * (size_t)P, hipMemcpyDeviceToHost, c->stream));
    const int rc = sync_checked(c, "get_mll_ai");
    if (rc != ALGP_OK) c->alpha_valid = false;
    return rc;
}


// f2: the device work of ONE iteration of GPR.fit (models.py:145-158: loss = -mll(model(train_x), train_y); backward) in
// one ABI call: S, its factor AND X = L^-T out of the same task-list launch (the identity rides along as a panel
// whose zero tiles are never touched), alpha by the two one-launch substitutions, S^-1 = X X^T as one
// triangular-aware launch, the pairwise gradient reduction.  Same values as algp_factorize + algp_get_mll +
// algp_get_mll_grad (tested); N^3 flop in all (N^3/3 each for the factor, the inverse of the factor and the product).
template <typename T>
int Impl<T>::fit_step(algp_ctx* c, double* mll_out, double* grad_out, bool reml) {
    if (c->pool_is_cov) return fail(c, ALGP_ERR_BAD_ARG, reml ? "reml_step needs a coordinate pool" : "fit_step needs a coordinate pool");
    const int64_t Npad = c->Npad;
    bool inv_enq = false;
    // Round 5: z rides along too (a dense tile row behind the identity that carries y - ybar), and alpha = X z is one pass
    // over the X the launch leaves -- no substitution chain runs beside S^-1 = X X^T any more (the two took 5.5 ms there,
    // starved by the GEMM).  (X X^T as tasks of the same launch as well was built
    // and measured in round 5 -- the launch grew by what the separate 5.1-ms GEMM launch costs, 12.9 -> 18.9 ms at N = 10 000
    // fp64: the list leaves nothing idle to fill -- and removed again: EXPERIMENTS.md.)
    const int64_t prow = grad_out ? Npad + NB : Npad;
    const bool have_X = c->N > 0 && panel_fits(Npad, prow);          // the identity rides along: X = L^-T in auxW
    if (have_X) {
        ALGP_TRY(ensure(c, c->auxW, sizeof(T) * prow * Npad));
        ALGP_TRY(ensure(c, c->auxA, sizeof(T) * Npad * Npad));
        ALGP_TRY(set_identity_launch<T>(c, p(c->auxW), Npad, Npad));
        Panel pn{p(c->auxW), Npad, prow, 2};
        pn.inv_out = grad_out ? p(c->auxA) : nullptr;
        if (prow > Npad) {
            ALGP_HIP(hipMemsetAsync(p(c->auxW) + Npad * Npad, 0, sizeof(T) * NB * Npad, c->stream));
            ALGP_HIP(hipMemcpyAsync(p(c->auxW) + Npad * Npad, c->y0.p, sizeof(T) * Npad, hipMemcpyDeviceToDevice, c->stream));
            pn.z_row = Npad;
        }
        const int frc = factorize(c, 0, &pn);
        if (pn.inv_enqueued && (frc != ALGP_OK || !grad_out)) hipStreamSynchronize(c->stream2);   // nothing outlives the call
        ALGP_TRY(frc);
        inv_enq = pn.inv_enqueued;
    } else {
        ALGP_TRY(factorize(c, 0));
    }
    if (reml && !grad_out) {                                     // the value alone: the GLS read-out on the new factor
        double beta[FX_P];
        return mll_out ? get_gls(c, beta, nullptr, mll_out) : ALGP_OK;
    }
    if (mll_out && !reml) *mll_out = -0.5 * c->yalpha - 0.5 * c->logdet - 0.5 * (double)c->N * 1.8378770664093453;
    if (!grad_out) return ALGP_OK;
    // algp_reml_step: the same launch, then the restricted likelihood's tail (api_fixed.hip) on the X and S^-1 it leaves
    const int grc = reml ? reml_grad(c, grad_out, mll_out, have_X, inv_enq) : mll_grad(c, grad_out, have_X, inv_enq);
    if (grc != ALGP_OK && inv_enq) hipStreamSynchronize(c->stream2);
    return grc;
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_get_mll_grad(algp_ctx* c, double* grad) {
    CHECK_CTX(c);
    if (!grad) return fail(c, ALGP_ERR_BAD_ARG, "get_mll_grad: bad arguments");
    FINISH(c, DISPATCH(c, mll_grad(c, grad)));
}

int algp_get_mll_ai(algp_ctx* c, double* ai) {
    CHECK_CTX(c);
    if (!ai) return fail(c, ALGP_ERR_BAD_ARG, "get_mll_ai: bad arguments");
    FINISH(c, DISPATCH(c, mll_ai(c, ai)));
}

int algp_fit_step(algp_ctx* c, double* mll, double* grad) {
    CHECK_CTX(c);
    NEED_HYPERS(c);
    if (c->n_pool <= 0) return fail(c, ALGP_ERR_STATE, "fit_step: set a pool first");
    if (!c->y0.p || (int64_t)c->pos_in_train.size() != c->n_pool) return fail(c, ALGP_ERR_STATE, "fit_step: call algp_set_train first");
    FINISH(c, DISPATCH(c, fit_step(c, mll, grad)));
}

}  // extern "C"
