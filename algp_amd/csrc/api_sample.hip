// api_sample.hip -- algp_sample_posterior: joint draws of the latent field at the candidates by pathwise conditioning
// (Matheron's rule) on the resident candidate solve.  With V^T = B^T L^-T on the device a prior draw g becomes a posterior draw,
//     f_s(j) = ybar + g_s(j) + V_j . L^-1 (y - ybar - g_s(A) - sqrt(v) o eps_s),      v_i = var_i + sigma_n^2,
// by one triangular solve of the S right-hand sides and one product against V^T.  The prior draw is either a random-Fourier-
// feature sum (sample.hip: an M x S x F product whose A operand is generated in registers) or values the caller supplies.  The
// library draws nothing: frequencies, phases, weights and the noise draws are arguments.  Samples go through in tiles of 128:
//   R^T (128 x Npad)  = the train rows' epilogue of the prior draw                 sample_features_launch / sample_values_launch
//   Z^T               = R^T L^-T, in place                                          trsm_blocked
//   out (128 x Mpad)  = ybar + G_X + Z^T (V^T)^T                                    gemm_nt_launch, beta = 1 on the prior draw
// algp_sample_posterior_fixed: draws of ybar + h' beta + f with beta's uncertainty in them, the same rule on the universal-kriging
// predictor: beta_s = C C^T F^T z_s per sample and f_s(j) += R_j beta_s = (R_j C) . (C^T F^T z_s).  The pass over the tile Z^T in
// place of V^T with a zero basis row gives -(Z^T F) C (fixed.hip), so per tile
//   out -= (Z^T F C) proj^T                          the rank-p fold, proj the candidates' rows R_j C   fixed_post_launch, fixed_fold_launch
// The mean over draws is algp_get_posterior_fixed's mu, their covariance posterior_cov + proj proj^T.
// Nothing of the resident state is written; the scratch is one buffer of the context (algp_ctx::smp).
#include "api_impl.h"

using namespace algp;

namespace algp {

template <typename T>
int Impl<T>::sample_posterior(algp_ctx* c, int S, int F, const double* omega, const double* phase, const double* weights,
                              const double* prior, const double* eps, void* out, bool fixed) {
    const std::string who = fixed ? "sample_posterior_fixed" : "sample_posterior";
    if (fixed && c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, who + ": no fixed effects are attached (algp_set_fixed_effects)");
    if (!c->solved) return fail(c, ALGP_ERR_STATE, who + ": call algp_solve_candidates first");
    const int64_t N = c->N, Npad = c->Npad, M = c->M, Mpad = c->Mpad, n_pool = c->n_pool;
    // the two states algp_get_posterior_cov refuses, for its reasons: V_j . z is the conditional update only for ordinary rows
    // solved against the train set alone
    if (c->prior_noise)
        for (int64_t j = 0; j < M; ++j)
            if (c->vt_kind[j] >= 0)
                return fail(c, ALGP_ERR_STATE,
                            who + ": candidate " + std::to_string(j) + " (pool index " + std::to_string(c->cand_idx[j]) +
                                ") is a train site and was solved as a unit row (prior_includes_noise = 1): set the "
                                "candidates with prior_includes_noise = 0");
    if (!c->picks.empty())
        return fail(c, ALGP_ERR_STATE, who + ": " + std::to_string(c->picks.size()) +
                                           " pick(s) were committed since the candidate solve, which the draws would not "
                                           "include: solve the candidates again");
    // rows of one site share its sigma_n^2 term (algp_set_train): independent eps cannot describe their noise
    if (c->train_has_repeats)
        return fail(c, ALGP_ERR_STATE, who + ": the train set lists a pool site in more than one row");
    if (fixed) {                                                  // algp_get_posterior_fixed's
        if (c->train_dirty || c->vt_hyp_stamp != c->hyp_stamp || c->vt_fact_idx != c->fact_idx || c->vt_fact_var != c->fact_var)
            return fail(c, ALGP_ERR_STATE, who + ": the candidate solve is not the current factor's: solve the candidates again");
        if (c->ldv % 4 != 0) return fail(c, ALGP_ERR_STATE, who + ": the row stride of V^T is not a multiple of 4");
    }
    if (F > 0 && c->pool_is_cov) return fail(c, ALGP_ERR_BAD_ARG, who + ": random features need a coordinate pool (pass prior values)");
    if (F > 0 && c->hyp.has_ids() && !c->pool_is_cov)
        return fail(c, ALGP_ERR_BAD_ARG, who + ": under the relationship kernel the genotype part has no spectral density, so "
                                         "random features cannot draw it (pass prior values, F == 0)");
    if (N > 0 && !eps) return fail(c, ALGP_ERR_BAD_ARG, who + ": eps is NULL");
    if (M > 0 && !out) return fail(c, ALGP_ERR_BAD_ARG, who + ": out is NULL");
    if (M == 0) return ALGP_OK;

    // (An explicit covariance takes prior_includes_noise = 1 only, so a train site among its candidates is a unit row and was
    // refused above: every row that arrives here was solved from K_Aj, on either pool kind.)
    const int DP = c->hyp.DP, D = c->hyp.D;
    const int64_t Fpad = round_up(F, SAMPLE_KT);
    // the scratch, carved out of one allocation
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t off = total; total += (bytes + 255) / 256 * 256; return off; };
    const size_t o_stA = take(sizeof(double) * (size_t)SAMPLE_TILE * (size_t)(F > 0 ? F : n_pool));   // weights / prior values
    const size_t o_stB = take(sizeof(double) * (size_t)SAMPLE_TILE * (size_t)N);                      // eps
    const size_t o_stC = take(sizeof(double) * (size_t)F * (size_t)(D + 1));                          // omega, phase
    const size_t o_G = take(sizeof(T) * (size_t)SAMPLE_TILE * (size_t)(F > 0 ? Fpad : n_pool));       // W^T (Fpad x 128) / prior (128 x n_pool)
    const size_t o_om = take(sizeof(T) * (size_t)Fpad * DP);
    const size_t o_ph = take(sizeof(T) * (size_t)Fpad);
    const size_t o_E = take(sizeof(T) * (size_t)SAMPLE_TILE * (size_t)Npad);
    const size_t o_R = take(sizeof(T) * (size_t)SAMPLE_TILE * (size_t)Npad);
    const size_t o_O = take(sizeof(T) * (size_t)SAMPLE_TILE * (size_t)Mpad);
    // fixed: the tile's rows -(Z^T F) C; one zero basis row and row 0 as every row's index
    const size_t o_pZ = take(fixed ? sizeof(T) * (size_t)SAMPLE_TILE * FX_P : 0);
    const size_t o_h0 = take(fixed ? sizeof(int64_t) * (size_t)SAMPLE_TILE + sizeof(T) * FX_P : 0);
    if (total > c->smp.cap) {
        size_t free_b = 0, total_b = 0;
        ALGP_HIP(hipMemGetInfo(&free_b, &total_b));
        if (total > c->smp.cap + free_b)
            return fail(c, ALGP_ERR_OOM, who + ": the scratch of one tile of 128 samples takes " + std::to_string(total) +
                                             " bytes, " + std::to_string(c->smp.cap + free_b) + " available");
    }
    ALGP_TRY(ensure(c, c->smp, total));
    char* base = (char*)c->smp.p;
    double *stA = (double*)(base + o_stA), *stB = (double*)(base + o_stB), *stC = (double*)(base + o_stC);
    T *G = (T*)(base + o_G), *om = (T*)(base + o_om), *ph = (T*)(base + o_ph), *E = (T*)(base + o_E), *R = (T*)(base + o_R);
    T* O = (T*)(base + o_O);
    T* pZ = (T*)(base + o_pZ);
    FixedPlan pl;
    double info = 0.0;
    const int fp = c->fx_p;
    if (fixed) {
        // F^T, the p x p work and the candidates' rows R_j C, once for every tile
        ALGP_TRY(fixed_enqueue(c, who.c_str(), {.post_rows = M, .proj = true}, pl));
        ALGP_TRY(fixed_post_launch<T>(c, p(c->Vt), c->ldv, M, Npad, pl.Ft, Npad, (const T*)c->fxH.p, (const int64_t*)c->Cidx.p, pl.gls, fp,
                                      (const T*)nullptr, (const T*)nullptr, (T*)nullptr, (T*)nullptr, pl.proj));
        ALGP_HIP(hipMemsetAsync(base + o_h0, 0, sizeof(int64_t) * (size_t)SAMPLE_TILE + sizeof(T) * FX_P, c->stream));
        // the rank flag before the first tile: on a dependent column proj is not written, and no tile is to be folded with it
        ALGP_HIP(hipMemcpyAsync(&info, pl.gls + FX_INFO, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        ALGP_TRY(sync_checked(c, who.c_str()));
        if (info != 0.0) return fixed_rank_error(c, who.c_str(), info);
    }

    if (F > 0) {
        ALGP_HIP(hipMemcpyAsync(stC, omega, sizeof(double) * (size_t)F * D, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(stC + (size_t)F * D, phase, sizeof(double) * (size_t)F, hipMemcpyHostToDevice, c->stream));
        ALGP_TRY(sample_convert_launch<T>(c, stC, F, D, om, Fpad, DP, DP, 0));
        ALGP_TRY(sample_convert_launch<T>(c, stC + (size_t)F * D, 1, F, ph, 1, Fpad, Fpad, 0));
    }
    const T scale = F > 0 ? (T)sqrt(2.0 * c->hyp.prior_var() / (double)F) : (T)1;
    for (int64_t s0 = 0; s0 < S; s0 += SAMPLE_TILE) {
        const int sl = (int)std::min<int64_t>(SAMPLE_TILE, S - s0);
        if (F > 0) {
            ALGP_HIP(hipMemcpyAsync(stA, weights + s0 * F, sizeof(double) * (size_t)sl * F, hipMemcpyHostToDevice, c->stream));
            ALGP_TRY(sample_convert_launch<T>(c, stA, sl, F, G, SAMPLE_TILE, Fpad, SAMPLE_TILE, 1));
        } else {
            ALGP_HIP(hipMemcpyAsync(stA, prior + s0 * n_pool, sizeof(double) * (size_t)sl * n_pool, hipMemcpyHostToDevice, c->stream));
            ALGP_TRY(sample_convert_launch<T>(c, stA, sl, n_pool, G, SAMPLE_TILE, n_pool, n_pool, 0));
        }
        auto draw = [&](const int64_t* idx, const SampleEpi<T>& e) {
            return F > 0 ? sample_features_launch<T>(c, (const T*)c->Xs.p, DP, idx, G, om, ph, Fpad, F, scale, e)
                         : sample_values_launch<T>(c, G, n_pool, idx, e);
        };
        if (N > 0) {
            ALGP_HIP(hipMemcpyAsync(stB, eps + s0 * N, sizeof(double) * (size_t)sl * N, hipMemcpyHostToDevice, c->stream));
            ALGP_TRY(sample_convert_launch<T>(c, stB, sl, N, E, SAMPLE_TILE, Npad, Npad, 0));
            ALGP_TRY(draw((const int64_t*)c->Aidx.p, {R, Npad, N, sl, (T)0, (const T*)c->y0.p, (const T*)c->varA.p, E, (T)c->hyp.noise}));
            ALGP_TRY(trsm_blocked<T>(c, {.klass = ALGP_PROF_GEMM_TRSM, .X = R, .mpad = SAMPLE_TILE, .ldx = Npad, .L = p(c->L), .npad = Npad, .ldl = c->Lld, .invD = p(c->invD)}));
        }
        ALGP_TRY(draw((const int64_t*)c->Cidx.p, {O, Mpad, M, sl, (T)c->ybar, nullptr, nullptr, nullptr, (T)0}));
        if (N > 0) {
            ALGP_TRY(gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, SAMPLE_TILE, Mpad, Npad, (T)1, R, Npad, p(c->Vt), c->ldv, (T)1, O, Mpad,
                                       O, Mpad, 0));
        }
        if (fixed) {
            ALGP_TRY(fixed_post_launch<T>(c, R, Npad, sl, Npad, pl.Ft, Npad, (const T*)(base + o_h0 + sizeof(int64_t) * (size_t)SAMPLE_TILE),
                                          (const int64_t*)(base + o_h0), pl.gls, fp, (const T*)nullptr, (const T*)nullptr, (T*)nullptr,
                                          (T*)nullptr, pZ));
            ALGP_TRY(fixed_fold_launch<T>(c, O, Mpad, sl, M, pZ, fp, pl.proj, fp, fp, -1));
        }
        ALGP_HIP(hipMemcpy2DAsync((T*)out + s0 * M, sizeof(T) * M, O, sizeof(T) * Mpad, sizeof(T) * M, (size_t)sl, hipMemcpyDeviceToHost,
                                  c->stream));
        ALGP_TRY(sync(c));                                           // the staging is reused by the next tile
    }
    return ALGP_OK;
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_sample_posterior(algp_ctx* c, int S, int F, const double* omega, const double* phase, const double* weights,
                          const double* prior, const double* eps, void* out) {
    CHECK_CTX(c);
    if (S < 1 || F < 0) return fail(c, ALGP_ERR_BAD_ARG, "sample_posterior: S >= 1 and F >= 0 required");
    if (F > 0 ? (!omega || !phase || !weights || prior) : (omega || phase || weights || !prior))
        return fail(c, ALGP_ERR_BAD_ARG, F > 0 ? "sample_posterior: F > 0 takes omega, phase and weights, and no prior values"
                                               : "sample_posterior: F == 0 takes prior values, and no omega, phase or weights");
    FINISH(c, DISPATCH(c, sample_posterior(c, S, F, omega, phase, weights, prior, eps, out)));
}

int algp_sample_posterior_fixed(algp_ctx* c, int S, int F, const double* omega, const double* phase, const double* weights,
                                const double* prior, const double* eps, void* out) {
    CHECK_CTX(c);
    if (S < 1 || F < 0) return fail(c, ALGP_ERR_BAD_ARG, "sample_posterior_fixed: S >= 1 and F >= 0 required");
    if (F > 0 ? (!omega || !phase || !weights || prior) : (omega || phase || weights || !prior))
        return fail(c, ALGP_ERR_BAD_ARG, F > 0 ? "sample_posterior_fixed: F > 0 takes omega, phase and weights, and no prior values"
                                               : "sample_posterior_fixed: F == 0 takes prior values, and no omega, phase or weights");
    FINISH(c, DISPATCH(c, sample_posterior(c, S, F, omega, phase, weights, prior, eps, out, true)));
}

}  // extern "C"
