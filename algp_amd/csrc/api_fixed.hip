// api_fixed.hip -- fixed effects: the mean ybar + h(x)' beta with beta estimated by generalised least squares.
//   algp_set_fixed_effects     the basis H (one row per pool site) to the device, zero-padded to FX_P columns
//   algp_get_gls               beta, its covariance A^-1 and the restricted log-likelihood
//   algp_get_posterior_fixed   the candidates' mean and variance with the estimated trend (universal kriging), the rows R_j C
//   algp_genotype_posterior_fixed   the genotype effects adjusted for the estimated effects, with beta's share of their variance
//   algp_posterior_mean_fixed       the mean at pool sites with the estimated trend, whole or by share, without a candidate solve
// (algp_group_posterior_fixed and algp_sample_posterior_fixed are branches of their siblings: api_group.hip, api_sample.hip)
// All read the resident factor (and candidate solve) and write none of it; their scratch is one buffer of the context
// (algp_ctx::fx), beside the sibling's own where a call has one (the genotype effects: algp_ctx::gen).  The kernels and the
// algebra: fixed.hip.
#include "api_impl.h"

using namespace algp;

namespace algp {

template <typename T>
int Impl<T>::set_fixed_effects(algp_ctx* c, const double* H, int p) {
    if (!H) {
        c->fx_p = 0;
        return ALGP_OK;
    }
    std::vector<T> h((size_t)c->n_pool * FX_P, (T)0);
    for (int64_t q = 0; q < c->n_pool; ++q)
        for (int a = 0; a < p; ++a) h[(size_t)q * FX_P + a] = (T)H[q * p + a];
    ALGP_TRY(sync(c));                                          // nothing enqueued still reads the old basis
    ALGP_TRY(ensure(c, c->fxH, sizeof(T) * h.size()));
    ALGP_HIP(hipMemcpyAsync(c->fxH.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, c->stream));
    ALGP_TRY(sync(c));
    c->fx_p = p;
    return ALGP_OK;
}

// What both read-outs share, enqueued on the main stream without a synchronisation: the panel [H_A^T] -> F^T through the blocked
// solve, the Gram product [A b; b' z'z] and the p x p work (pl.gls: the FX_* slots).  wants.post_rows > 0 reserves the posterior's
// outputs (mu, var; proj), wants.fit the fit's vectors and panels, in the same buffer.
template <typename T>
int Impl<T>::fixed_enqueue(algp_ctx* c, const char* who, const typename Impl<T>::FixedWants& wants, typename Impl<T>::FixedPlan& pl) {
    const int64_t post_rows = wants.post_rows;
    const bool want_proj = wants.proj;
    const std::string w(who);
    if (c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, w + ": no fixed effects are attached (algp_set_fixed_effects)");
    if (!c->factored || c->train_dirty) return fail(c, ALGP_ERR_STATE, w + ": call algp_factorize first");
    const int64_t N = c->N, Npad = c->Npad;
    const int p = c->fx_p;
    if (N <= p)
        return fail(c, ALGP_ERR_BAD_ARG, w + ": " + std::to_string(N) + " train rows do not determine " + std::to_string(p) + " fixed effects");
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t o = total; total += (bytes + 255) / 256 * 256; return o; };
    const size_t o_F = take(sizeof(T) * (size_t)NB * (size_t)Npad);
    const size_t o_gram = take(sizeof(double) * (FX_P + 1) * (FX_P + 1));
    const size_t o_gls = take(sizeof(double) * FX_OUT);
    const size_t o_mu = take(sizeof(T) * (size_t)post_rows);
    const size_t o_var = take(sizeof(T) * (size_t)post_rows);
    const size_t o_proj = take(want_proj ? sizeof(T) * (size_t)post_rows * FX_P : 0);
    const size_t o_aR = take(wants.fit || wants.resid ? sizeof(T) * (size_t)Npad : 0);
    const size_t o_panel = take(wants.fit ? sizeof(T) * (size_t)NB * (size_t)Npad : 0);
    const size_t o_Gt = take(wants.grad ? sizeof(T) * (size_t)NB * (size_t)Npad : 0);
    const size_t o_gram2 = take(wants.fit ? sizeof(double) * 12 * (12 + FX_P) : 0);
    if (total > c->fx.cap) {
        size_t free_b = 0, total_b = 0;
        ALGP_HIP(hipMemGetInfo(&free_b, &total_b));
        if (total > c->fx.cap + free_b)
            return fail(c, ALGP_ERR_OOM, w + ": " + std::to_string(total) + " bytes of scratch for " + std::to_string(N) + " train rows and " +
                                             std::to_string(post_rows) + " candidates, " + std::to_string(c->fx.cap + free_b) + " available");
    }
    ALGP_TRY(ensure(c, c->fx, total));
    char* base = (char*)c->fx.p;
    pl.Ft = (T*)(base + o_F);
    pl.gram = (double*)(base + o_gram);
    pl.gls = (double*)(base + o_gls);
    pl.mu = (T*)(base + o_mu);
    pl.var = (T*)(base + o_var);
    pl.proj = want_proj ? (T*)(base + o_proj) : nullptr;
    pl.aR = (T*)(base + o_aR);
    pl.panel = (T*)(base + o_panel);
    pl.Gt = (T*)(base + o_Gt);
    pl.gram2 = (double*)(base + o_gram2);
    // the rows behind the FX_P gathered ones ride through the solve as zeros (the panel is one 128-row tile)
    ALGP_HIP(hipMemsetAsync(pl.Ft + (int64_t)FX_P * Npad, 0, sizeof(T) * (size_t)(NB - FX_P) * (size_t)Npad, c->stream));
    ALGP_TRY(fixed_gather_launch<T>(c, (const T*)c->fxH.p, (const int64_t*)c->Aidx.p, N, Npad, pl.Ft));
    ALGP_TRY(trsm_blocked<T>(c, {.klass = ALGP_PROF_GEMM_TRSM, .X = pl.Ft, .mpad = NB, .ldx = Npad, .L = (T*)c->L.p, .npad = Npad, .ldl = c->Lld,
                                 .invD = (T*)c->invD.p}));
    ALGP_TRY(fixed_gram_launch<T>(c, pl.Ft, Npad, (const T*)c->z.p, N, p, pl.gram));
    // a scaled pivot at or below 64 eps: the column is in the span of the ones before it at the precision of F
    const double eps = sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-07;
    return fixed_gls_launch(c, pl.gram, p, 64.0 * eps, pl.gls);
}

// Harville's restricted likelihood from the p x p work's read-back h, without the constant 1/2 log|H'H|
static double fixed_reml(const algp_ctx* c, const double* h) {
    return -0.5 * ((double)(c->N - c->fx_p) * 1.8378770664093453 + c->logdet + h[FX_LOGDET_A] + h[FX_ZZ] - h[FX_QUAD]);
}

template <typename T>
int Impl<T>::get_gls(algp_ctx* c, double* beta_out, double* cov_out, double* reml_out) {
    FixedPlan pl;
    ALGP_TRY(fixed_enqueue(c, "get_gls", {}, pl));
    double h[FX_OUT];
    ALGP_HIP(hipMemcpyAsync(h, pl.gls, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    ALGP_TRY(sync_checked(c, "get_gls"));
    if (h[FX_INFO] != 0.0) return fixed_rank_error(c, "get_gls", h[FX_INFO]);
    const int p = c->fx_p;
    for (int a = 0; a < p; ++a) beta_out[a] = h[FX_BETA + a];
    if (cov_out) memcpy(cov_out, h + FX_COV, sizeof(double) * (size_t)p * (size_t)p);
    if (reml_out) *reml_out = fixed_reml(c, h);
    return ALGP_OK;
}

template <typename T>
int Impl<T>::get_posterior_fixed(algp_ctx* c, void* mu_out, void* var_out, void* proj_out) {
    if (c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, "get_posterior_fixed: no fixed effects are attached (algp_set_fixed_effects)");
    if (!c->solved) return fail(c, ALGP_ERR_STATE, "get_posterior_fixed: call algp_solve_candidates first");
    const int64_t M = c->M;
    // R_j = h_j - V_j F is the residual basis only for ordinary rows solved against the train set alone: algp_get_posterior_cov's
    // two refusals, for its reasons
    if (c->prior_noise)
        for (int64_t j = 0; j < M; ++j)
            if (c->vt_kind[j] >= 0)
                return fail(c, ALGP_ERR_STATE,
                            "get_posterior_fixed: candidate " + std::to_string(j) + " (pool index " + std::to_string(c->cand_idx[j]) +
                                ") is a train site and was solved as a unit row (prior_includes_noise = 1): set the "
                                "candidates with prior_includes_noise = 0");
    if (!c->picks.empty())
        return fail(c, ALGP_ERR_STATE, "get_posterior_fixed: " + std::to_string(c->picks.size()) +
                                           " pick(s) were committed since the candidate solve, which the covariance would "
                                           "not include: solve the candidates again");
    if (c->train_dirty || c->vt_hyp_stamp != c->hyp_stamp || c->vt_fact_idx != c->fact_idx || c->vt_fact_var != c->fact_var)
        return fail(c, ALGP_ERR_STATE, "get_posterior_fixed: the candidate solve is not the current factor's: solve the candidates again");
    if (c->ldv % 4 != 0) return fail(c, ALGP_ERR_STATE, "get_posterior_fixed: the row stride of V^T is not a multiple of 4");
    FixedPlan pl;
    ALGP_TRY(fixed_enqueue(c, "get_posterior_fixed", {.post_rows = std::max<int64_t>(M, 1), .proj = proj_out != nullptr}, pl));
    const int p = c->fx_p;
    ALGP_TRY(fixed_post_launch<T>(c, (const T*)c->Vt.p, c->ldv, M, c->Npad, pl.Ft, c->Npad, (const T*)c->fxH.p, (const int64_t*)c->Cidx.p, pl.gls, p,
                                  (const T*)c->mu.p, (const T*)c->dstat.p, pl.mu, pl.var, pl.proj));
    // one synchronisation: the outputs travel with the rank flag (a rank-deficient basis leaves them unspecified)
    double info = 0.0;
    ALGP_HIP(hipMemcpyAsync(&info, pl.gls + FX_INFO, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (M > 0) {
        if (mu_out) ALGP_HIP(hipMemcpyAsync(mu_out, pl.mu, sizeof(T) * M, hipMemcpyDeviceToHost, c->stream));
        if (var_out) ALGP_HIP(hipMemcpyAsync(var_out, pl.var, sizeof(T) * M, hipMemcpyDeviceToHost, c->stream));
        if (proj_out) ALGP_HIP(hipMemcpyAsync(proj_out, pl.proj, sizeof(T) * M * p, hipMemcpyDeviceToHost, c->stream));
    }
    ALGP_TRY(sync_checked(c, "get_posterior_fixed"));
    if (info != 0.0) return fixed_rank_error(c, "get_posterior_fixed", info);
    return ALGP_OK;
}

// alpha_R = P (y - ybar) = L^-T (z - F beta) into pl.aR: the residual of z on F, then the backward substitution alpha itself takes
template <typename T>
int Impl<T>::fixed_alpha_r(algp_ctx* c, typename Impl<T>::FixedPlan& pl) {
    ALGP_TRY(fixed_resid_launch<T>(c, pl.Ft, c->Npad, c->N, (const T*)c->z.p, pl.gls, pl.aR));
    return trsv_backward<T>(c, (const T*)c->L.p, c->Npad, c->Lld, (const T*)c->invD.p, pl.aR);
}

// The genotype effects with the estimated fixed effects: algp_genotype_posterior's W = B L^-T and then, with the effects' residual
// basis R_u = -W F (u has no trend share of its own),
//   mean = W z + R_u beta = B alpha_R       var_q = os_g G_qq - |W_q|^2 + |C' R_u,q|^2       cov = os_g G - W W^T + (R_u C)(R_u C)^T
// the prediction-error variances of the mixed-model equations, os_g G - B P B^T.  The sibling's launches in the sibling's order
// (its scratch, algp_ctx::gen), then the posterior pass over W in place of V^T with a zero basis row (fixed_post_launch: every row
// reads row 0 of a zeroed h) and the fold of (R_u C)(R_u C)^T onto the covariance.  Nothing resident is written; one
// synchronisation.
template <typename T>
int Impl<T>::genotype_posterior_fixed(algp_ctx* c, void* mean_out, void* var_out, void* cov_out) {
    const char* who = "genotype_posterior_fixed";
    if (!c->hyp.set || !c->hyp.has_ids())
        return fail(c, ALGP_ERR_STATE, "genotype_posterior_fixed: no kernel with a genotype term is in force (algp_set_hypers_relationship, "
                                       "algp_set_hypers_separable with Q >= 1)");
    if (c->pool_is_cov || c->n_pool <= 0) return fail(c, ALGP_ERR_STATE, "genotype_posterior_fixed needs a coordinate pool");
    if (c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, "genotype_posterior_fixed: no fixed effects are attached (algp_set_fixed_effects)");
    if (!c->factored || c->train_dirty) return fail(c, ALGP_ERR_STATE, "genotype_posterior_fixed: call algp_factorize first");
    if (c->solved && !c->picks.empty())
        return fail(c, ALGP_ERR_STATE, "genotype_posterior_fixed: " + std::to_string(c->picks.size()) +
                                           " pick(s) were committed since the factorisation, which the effects would not "
                                           "include: factorize again");
    const int64_t Q = c->hyp.Q, N = c->N, Npad = c->Npad, Qpad = round_up(Q, NB);
    const int p = c->fx_p;
    if (N <= p)
        return fail(c, ALGP_ERR_BAD_ARG, std::string(who) + ": " + std::to_string(N) + " train rows do not determine " + std::to_string(p) +
                                             " fixed effects");
    const T* G = c->hyp.has_table ? (const T*)c->Gtab.p : nullptr;
    const T osg = (T)c->hyp.outputscale_g;

    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t o = total; total += (bytes + 255) / 256 * 256; return o; };
    const size_t o_B = take(sizeof(T) * (size_t)Qpad * (size_t)Npad);
    const size_t o_ss = take(sizeof(T) * (size_t)Qpad);
    const size_t o_mean = take(sizeof(T) * (size_t)Qpad);
    const size_t o_var = take(sizeof(T) * (size_t)Qpad);
    const size_t o_h0 = take(sizeof(T) * FX_P + sizeof(int64_t) * (size_t)Qpad);   // the zero basis row, and row 0 as every row's index
    const size_t o_WW = take(cov_out ? sizeof(T) * (size_t)Qpad * (size_t)Qpad : 0);
    const size_t o_cov = take(cov_out ? sizeof(T) * (size_t)Q * (size_t)Q : 0);
    if (total > c->gen.cap) {
        size_t free_b = 0, total_b = 0;
        ALGP_HIP(hipMemGetInfo(&free_b, &total_b));
        if (total > c->gen.cap + free_b)
            return fail(c, ALGP_ERR_OOM, std::string(who) + ": the scratch of " + std::to_string(Q) + " genotypes takes " + std::to_string(total) +
                                             " bytes, " + std::to_string(c->gen.cap + free_b) + " available");
    }
    ALGP_TRY(ensure(c, c->gen, total));
    char* base = (char*)c->gen.p;
    T *B = (T*)(base + o_B), *ss = (T*)(base + o_ss), *meanD = (T*)(base + o_mean), *varD = (T*)(base + o_var);
    T *WW = (T*)(base + o_WW), *covD = (T*)(base + o_cov);
    const int64_t* idx0 = (const int64_t*)(base + o_h0);
    const T* h0 = (const T*)(base + o_h0 + sizeof(int64_t) * (size_t)Qpad);
    FixedPlan pl;
    ALGP_TRY(fixed_enqueue(c, who, {.post_rows = Qpad, .proj = cov_out != nullptr}, pl));

    ALGP_TRY(rel_gather_b_launch<T>(c, G, Q, osg, (const T*)c->Xs.p, c->hyp.DP, c->hyp.idc(), (const int64_t*)c->Aidx.p, N, Qpad, Npad, B));
    ALGP_TRY(trsm_blocked<T>(c, {.klass = ALGP_PROF_GEMM_TRSM, .X = B, .mpad = Qpad, .ldx = Npad, .L = (T*)c->L.p, .npad = Npad, .ldl = c->Lld,
                                 .invD = (T*)c->invD.p}));
    ALGP_TRY(rows_reduce_launch<T>(c, B, Qpad, Npad, Npad, (T*)c->z.p, ss, meanD));
    ALGP_TRY(rel_var_finish_launch<T>(c, G, Q, osg, ss, varD));
    ALGP_HIP(hipMemsetAsync(base + o_h0, 0, sizeof(T) * FX_P + sizeof(int64_t) * (size_t)Qpad, c->stream));
    ALGP_TRY(fixed_post_launch<T>(c, B, Npad, Q, Npad, pl.Ft, Npad, h0, idx0, pl.gls, p, meanD, varD, pl.mu, var_out ? pl.var : (T*)nullptr,
                                  pl.proj));
    double info = 0.0;
    ALGP_HIP(hipMemcpyAsync(&info, pl.gls + FX_INFO, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ALGP_HIP(hipMemcpyAsync(mean_out, pl.mu, sizeof(T) * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    if (var_out) ALGP_HIP(hipMemcpyAsync(var_out, pl.var, sizeof(T) * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    if (cov_out) {
        ALGP_TRY(gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, Qpad, Qpad, Npad, (T)1, B, Npad, B, Npad, (T)0, (const T*)nullptr, Qpad, WW, Qpad, 1));
        ALGP_TRY(rel_cov_finish_launch<T>(c, G, Q, osg, WW, Qpad, covD));
        ALGP_TRY(fixed_fold_launch<T>(c, covD, Q, Q, Q, pl.proj, p, pl.proj, p, p, 1));
        ALGP_HIP(hipMemcpyAsync(cov_out, covD, sizeof(T) * (size_t)Q * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    }
    ALGP_TRY(sync_checked(c, who));
    if (info != 0.0) return fixed_rank_error(c, who, info);
    return ALGP_OK;
}

// The mean at pool sites with the estimated trend and no candidate solve: the kernel-GEMV of algp_posterior_mean on alpha_R =
// P (y - ybar) in alpha's place, and the trend's share h_j' beta.  component -1: ybar + h_j' beta + k_j' alpha_R; 0, 1: that
// part's share k_c,j' alpha_R (algp_posterior_mean_component's rules); 2: h_j' beta.  Nothing resident is written (alpha is
// not needed); one synchronisation.
template <typename T>
int Impl<T>::posterior_mean_fixed(algp_ctx* c, int component, const int64_t* idx, int64_t M, void* mu_out) {
    const char* who = "posterior_mean_fixed";
    if (c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, "posterior_mean_fixed: no fixed effects are attached (algp_set_fixed_effects)");
    if (!c->factored || c->train_dirty) return fail(c, ALGP_ERR_STATE, "posterior_mean_fixed: call algp_factorize first");
    if (c->N <= c->fx_p)
        return fail(c, ALGP_ERR_BAD_ARG, std::string(who) + ": " + std::to_string(c->N) + " train rows do not determine " +
                                             std::to_string(c->fx_p) + " fixed effects");
    if (M == 0) return ALGP_OK;
    ALGP_TRY(ensure(c, c->auxIdx, sizeof(int64_t) * M));
    FixedPlan pl;
    ALGP_TRY(fixed_enqueue(c, who, {.post_rows = M, .resid = true}, pl));
    ALGP_HIP(hipMemcpyAsync(c->auxIdx.p, idx, sizeof(int64_t) * M, hipMemcpyHostToDevice, c->stream));
    const int64_t* didx = (const int64_t*)c->auxIdx.p;
    if (component != 2) {
        ALGP_TRY(fixed_alpha_r(c, pl));
        KmatSrc s = make_src(c);
        s.parts = component < 0 ? 3 : 1 << component;
        ALGP_TRY(kgemv_launch<T>(c, M, didx, s, c->N, (const int64_t*)c->Aidx.p, pl.aR, component < 0 ? (T)c->ybar : (T)0, pl.mu));
    }
    if (component < 0 || component == 2) ALGP_TRY(fixed_trend_launch<T>(c, (const T*)c->fxH.p, didx, M, pl.gls, c->fx_p, component < 0, pl.mu));
    double info = 0.0;
    ALGP_HIP(hipMemcpyAsync(&info, pl.gls + FX_INFO, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ALGP_HIP(hipMemcpyAsync(mu_out, pl.mu, sizeof(T) * M, hipMemcpyDeviceToHost, c->stream));
    ALGP_TRY(sync_checked(c, who));
    if (info != 0.0) return fixed_rank_error(c, who, info);
    return ALGP_OK;
}

// d l_R / d theta = 1/2 tr((alpha_R alpha_R' - P) dS/dtheta): the MLL gradient's kernel, unchanged, on the projected pair.
//   S^-1 (auxA, lower tiles) and X = L^-T (auxW) as algp_get_mll_grad forms them, or as fit_step's launch has left them
//   G^T = (F C)^T X^T          one product of the padded panel against X                        fixed_fc_launch, gemm_nt_launch
//   alpha_R = L^-T (z - F beta)                                                                 fixed_alpha_r
//   P = S^-1 - G G^T           on the lower-triangle entries the gradient reads, in auxA        fixed_downdate_launch
//   the pairwise reduction     mll_grad_launch(P, alpha_R); auxW (X is spent) holds its partials
// auxA / auxW are scratch here as there; alpha is brought up to date, nothing else resident is written.  One synchronisation.
template <typename T>
int Impl<T>::reml_grad(algp_ctx* c, double* grad_out, double* reml_out, bool have_X, bool inv_enqueued) {
    if (c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, "get_reml_grad: no fixed effects are attached (algp_set_fixed_effects)");
    if (!c->factored || c->train_dirty) return fail(c, ALGP_ERR_STATE, "get_reml_grad: call algp_factorize first");
    if (c->pool_is_cov) return fail(c, ALGP_ERR_BAD_ARG, "get_reml_grad needs a coordinate pool");
    const int64_t N = c->N, Npad = c->Npad;
    if (have_X && !c->alpha_valid) {
        ALGP_TRY(upper_gemv_launch<T>(c, p(c->auxW), Npad, Npad, (const T*)c->z.p, p(c->alpha)));
        c->alpha_valid = true;
    }
    ALGP_TRY(need_alpha(c));
    ALGP_TRY(ensure(c, c->auxA, sizeof(T) * Npad * Npad));
    if (!have_X) {
        ALGP_TRY(ensure(c, c->auxW, sizeof(T) * Npad * Npad));
        ALGP_TRY(set_identity_launch<T>(c, p(c->auxW), Npad, Npad));
        ALGP_TRY(trinv_upper<T>(c, ALGP_PROF_GEMM_OTHER, p(c->auxW), Npad, Npad, p(c->L), c->Lld, p(c->invD)));
    }
    // S^-1 is complete before the panel's solve starts: the blocked solve may use the helper stream S^-1 runs on
    if (inv_enqueued) ALGP_HIP(hipStreamWaitEvent(c->stream, sync_event(c, EV_INV_DONE), 0));
    else ALGP_TRY(syrk_upper<T>(c, ALGP_PROF_GEMM_OTHER, p(c->auxW), Npad, Npad, p(c->auxA), Npad));
    FixedPlan pl;
    ALGP_TRY(fixed_enqueue(c, "get_reml_grad", {.fit = true, .grad = true}, pl));
    const int fp = c->fx_p;
    ALGP_HIP(hipMemsetAsync(pl.panel + (int64_t)FX_P * Npad, 0, sizeof(T) * (size_t)(NB - FX_P) * (size_t)Npad, c->stream));
    ALGP_TRY(fixed_fc_launch<T>(c, pl.Ft, Npad, pl.gls, pl.panel));
    ALGP_TRY(gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, NB, Npad, Npad, (T)1, pl.panel, Npad, p(c->auxW), Npad, (T)0, pl.Gt, Npad, pl.Gt, Npad, 0));
    ALGP_TRY(fixed_alpha_r(c, pl));
    ALGP_TRY(fixed_downdate_launch<T>(c, p(c->auxA), Npad, N, pl.Gt, Npad, fp));
    double* sc = (double*)c->scal.p + SC_GRAD;
    ALGP_HIP(hipMemsetAsync(sc, 0, sizeof(double) * 12, c->stream));
    ALGP_TRY(mll_grad_launch<T>(c, p(c->auxA), Npad, N, (const int64_t*)c->Aidx.p, pl.aR, make_src(c), sc, (double*)c->auxW.p));
    double h[12], g[FX_OUT];
    ALGP_HIP(hipMemcpyAsync(h, sc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    ALGP_HIP(hipMemcpyAsync(g, pl.gls, sizeof(g), hipMemcpyDeviceToHost, c->stream));
    {
        const int rc = sync_checked(c, "get_reml_grad");
        if (rc != ALGP_OK) { c->alpha_valid = false; return rc; }
    }
    if (g[FX_INFO] != 0.0) return fixed_rank_error(c, "get_reml_grad", g[FX_INFO]);
    // [log ls | the log outputscales | log sigma_n^2], algp_get_mll_grad's order
    const int nos = c->hyp.n_os(), nl = c->hyp.n_ls();
    if (grad_out) {
        for (int d = 0; d < nl; ++d) grad_out[d] = 0.5 * h[nos + 1 + d];
        for (int q = 0; q < nos; ++q) grad_out[nl + q] = 0.5 * h[q];
        grad_out[nl + nos] = 0.5 * c->hyp.noise * h[nos];
    }
    if (reml_out) *reml_out = fixed_reml(c, g);
    return ALGP_OK;
}

// AI_R,ab = 1/2 alpha_R' dS_a P dS_b alpha_R = 1/2 [ v_a . v_b - (F' v_a)' A^-1 (F' v_b) ], v_a = L^-1 dS_a alpha_R: algp_get_mll_ai's
// pass with the projected alpha (mll_ai_u_launch takes the pointer) and p more rows in the Gram product; the p x p part on the
// host in double, w_a = C' F' v_a.  Writes nothing resident; one synchronisation; symmetric bit for bit.
template <typename T>
int Impl<T>::reml_ai(algp_ctx* c, double* ai_out) {
    if (c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, "get_reml_ai: no fixed effects are attached (algp_set_fixed_effects)");
    if (!c->factored || c->train_dirty) return fail(c, ALGP_ERR_STATE, "get_reml_ai: call algp_factorize first");
    if (c->pool_is_cov) return fail(c, ALGP_ERR_BAD_ARG, "get_reml_ai needs a coordinate pool");
    const int64_t N = c->N, Npad = c->Npad;
    const int nos = c->hyp.n_os(), nl = c->hyp.n_ls(), P = nl + nos + 1;
    const int fp = c->fx_p, W = P + fp;
    FixedPlan pl;
    ALGP_TRY(fixed_enqueue(c, "get_reml_ai", {.fit = true}, pl));
    ALGP_TRY(fixed_alpha_r(c, pl));
    ALGP_HIP(hipMemsetAsync(pl.panel + (int64_t)P * Npad, 0, sizeof(T) * (size_t)(NB - P) * (size_t)Npad, c->stream));
    ALGP_TRY(mll_ai_u_launch<T>(c, N, Npad, (const int64_t*)c->Aidx.p, pl.aR, make_src(c), nl, pl.panel));
    ALGP_TRY(trsm_blocked<T>(c, {.klass = ALGP_PROF_GEMM_TRSM, .X = pl.panel, .mpad = NB, .ldx = Npad, .L = (T*)c->L.p, .npad = Npad, .ldl = c->Lld,
                                 .invD = (T*)c->invD.p}));
    ALGP_TRY(fixed_gram2_launch<T>(c, pl.panel, pl.Ft, Npad, N, P, fp, pl.gram2));
    double g2[12 * (12 + FX_P)], g[FX_OUT];
    ALGP_HIP(hipMemcpyAsync(g2, pl.gram2, sizeof(double) * (size_t)P * (size_t)W, hipMemcpyDeviceToHost, c->stream));
    ALGP_HIP(hipMemcpyAsync(g, pl.gls, sizeof(g), hipMemcpyDeviceToHost, c->stream));
    ALGP_TRY(sync_checked(c, "get_reml_ai"));
    if (g[FX_INFO] != 0.0) return fixed_rank_error(c, "get_reml_ai", g[FX_INFO]);
    double w[12][FX_P];
    for (int a = 0; a < P; ++a)
        for (int b = 0; b < fp; ++b) {
            double s = 0.0;
            for (int k = 0; k <= b; ++k) s += g[FX_C + k * FX_P + b] * g2[a * W + P + k];
            w[a][b] = s;
        }
    for (int a = 0; a < P; ++a)
        for (int b = 0; b < P; ++b) {
            double s = 0.0;
            for (int k = 0; k < fp; ++k) s += w[a][k] * w[b][k];
            ai_out[a * P + b] = 0.5 * (g2[a * W + b] - s);
        }
    return ALGP_OK;
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_set_fixed_effects(algp_ctx* c, const double* H, int64_t n_pool, int p) {
    CHECK_CTX(c);
    if (!H || p == 0) FINISH(c, DISPATCH(c, set_fixed_effects(c, nullptr, 0)));
    if (c->n_pool <= 0) return fail(c, ALGP_ERR_STATE, "set_fixed_effects: set a pool first");
    if (p < 1 || p > FX_P) return fail(c, ALGP_ERR_BAD_ARG, "set_fixed_effects: 1 <= p <= 16 required");
    if (n_pool != c->n_pool)
        return fail(c, ALGP_ERR_BAD_ARG, "set_fixed_effects: " + std::to_string(n_pool) + " rows for a pool of " + std::to_string(c->n_pool) + " sites");
    for (int64_t e = 0; e < n_pool * p; ++e)
        if (!std::isfinite(H[e]))
            return fail(c, ALGP_ERR_BAD_ARG, "set_fixed_effects: H[" + std::to_string(e / p) + ", " + std::to_string(e % p) + "] is not finite");
    FINISH(c, DISPATCH(c, set_fixed_effects(c, H, p)));
}

int algp_get_gls(algp_ctx* c, double* beta, double* cov, double* reml) {
    CHECK_CTX(c);
    if (!beta) return fail(c, ALGP_ERR_BAD_ARG, "get_gls: bad arguments");
    FINISH(c, DISPATCH(c, get_gls(c, beta, cov, reml)));
}

int algp_get_reml_grad(algp_ctx* c, double* grad) {
    CHECK_CTX(c);
    if (!grad) return fail(c, ALGP_ERR_BAD_ARG, "get_reml_grad: bad arguments");
    FINISH(c, DISPATCH(c, reml_grad(c, grad, nullptr)));
}

int algp_get_reml_ai(algp_ctx* c, double* ai) {
    CHECK_CTX(c);
    if (!ai) return fail(c, ALGP_ERR_BAD_ARG, "get_reml_ai: bad arguments");
    FINISH(c, DISPATCH(c, reml_ai(c, ai)));
}

int algp_reml_step(algp_ctx* c, double* reml, double* grad) {
    CHECK_CTX(c);
    NEED_HYPERS(c);
    if (c->n_pool <= 0) return fail(c, ALGP_ERR_STATE, "reml_step: set a pool first");
    if (!c->y0.p || (int64_t)c->pos_in_train.size() != c->n_pool) return fail(c, ALGP_ERR_STATE, "reml_step: call algp_set_train first");
    if (c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, "reml_step: no fixed effects are attached (algp_set_fixed_effects)");
    FINISH(c, DISPATCH(c, fit_step(c, reml, grad, true)));
}

int algp_get_posterior_fixed(algp_ctx* c, void* mu, void* var, void* proj) {
    CHECK_CTX(c);
    FINISH(c, DISPATCH(c, get_posterior_fixed(c, mu, var, proj)));
}

int algp_genotype_posterior_fixed(algp_ctx* c, void* mean_out, void* var_out, void* cov_out) {
    CHECK_CTX(c);
    if (!mean_out) return fail(c, ALGP_ERR_BAD_ARG, "genotype_posterior_fixed: mean_out is NULL");
    FINISH(c, DISPATCH(c, genotype_posterior_fixed(c, mean_out, var_out, cov_out)));
}

int algp_bench_fixed_fold(algp_ctx* c, int64_t rows, int64_t cols, int p, int reps, double* fold_ms, double* copy_ms) {
    CHECK_CTX(c);
    if (!fold_ms || !copy_ms || rows <= 0 || cols <= 0 || p < 1 || p > FX_P || reps <= 0) return fail(c, ALGP_ERR_BAD_ARG, "bench_fixed_fold: bad arguments");
    const bool was = c->prof_on;
    c->prof_on = false;
    const int rc = c->dtype == ALGP_F64 ? bench_fixed<double>(c, rows, cols, p, reps, fold_ms, copy_ms, nullptr)
                                        : bench_fixed<float>(c, rows, cols, p, reps, fold_ms, copy_ms, nullptr);
    c->prof_on = was;
    return rc;
}

int algp_bench_fixed_panel(algp_ctx* c, int64_t rows, int64_t ncols, int p, int reps, double* ms) {
    CHECK_CTX(c);
    if (!ms || rows <= 0 || ncols <= 0 || ncols % NB != 0 || p < 1 || p > FX_P || reps <= 0)
        return fail(c, ALGP_ERR_BAD_ARG, "bench_fixed_panel: bad arguments (ncols a multiple of 128)");
    const bool was = c->prof_on;
    c->prof_on = false;
    const int rc = c->dtype == ALGP_F64 ? bench_fixed<double>(c, rows, ncols, p, reps, nullptr, nullptr, ms)
                                        : bench_fixed<float>(c, rows, ncols, p, reps, nullptr, nullptr, ms);
    c->prof_on = was;
    return rc;
}

int algp_posterior_mean_fixed(algp_ctx* c, int component, const int64_t* idx, int64_t M, void* mu) {
    CHECK_CTX(c);
    if (component < -1 || component > 2) return fail(c, ALGP_ERR_BAD_ARG, "posterior_mean_fixed: component must be -1, 0, 1 or 2");
    if (M < 0 || (M > 0 && (!idx || !mu))) return fail(c, ALGP_ERR_BAD_ARG, "posterior_mean_fixed: bad arguments");
    if (c->pool_is_cov) return fail(c, ALGP_ERR_BAD_ARG, "posterior_mean_fixed needs a coordinate pool");
    if ((component == 0 || component == 1) && (!c->hyp.set || !(c->hyp.additive || c->hyp.has_ids())))
        return fail(c, ALGP_ERR_STATE, c->hyp.sep ? "posterior_mean_fixed: a product has no additive shares (the separable kernel without a genotype term)"
                                                  : "posterior_mean_fixed: a single kernel is in force (algp_set_hypers_additive)");
    for (int64_t i = 0; i < M; ++i)
        if (idx[i] < 0 || idx[i] >= c->n_pool) return fail(c, ALGP_ERR_BAD_ARG, "posterior_mean_fixed: index outside the pool");
    FINISH(c, DISPATCH(c, posterior_mean_fixed(c, component, idx, M, mu)));
}

}  // extern "C"
