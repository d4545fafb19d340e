// api_group.hip -- algp_group_posterior: the joint posterior of linear functionals g_q = sum_{j in q} a_j f(x_j) of the latent
// field over groups of candidate rows (a genotype's plots, a field row), from the resident candidate solve.  With A the Q x M
// matrix of coefficients, mean = A mu and cov = A Sigma A^T for Sigma = K_xx + diag(extra_var) - V^T V, the matrix
// algp_get_posterior_cov defines -- without K_xx or Sigma ever existing: the labelled rows are sorted by group on the host and
//   U (Qpad x Mpad) = A (K_xx + diag(extra_var))       kernel values summed by group as they are formed      group_ksum_launch
//   T (Qpad x Npad) = A V^T                            a segmented sum over the rows of V^T                   group_rowsum_launch
//   cross wanted:  cross = U - T (V^T)^T               one product on the matrix cores, in place              gemm_nt_launch
//                  cov   = cross A^T                   a segmented sum along the rows of cross                group_colsum_launch
//   cov alone:     cov   = U A^T - T T^T               the big product is not launched; T T^T: lower tiles    gemm_nt_launch
// algp_group_posterior_fixed: the same functionals of the total signal ybar + h' beta + f with the attached fixed effects
// estimated.  With R_g = A H_C - T F (H_C: the candidates' basis rows; fixed.hip's pass over T in place of V^T):
//   mean  = A mu + R_g beta                                                                                fixed_post_launch
//   cov   = A Sigma A^T + (R_g C)(R_g C)^T             the rank-p fold onto the Q x Q result               fixed_fold_launch
//   cross = A Sigma + (R_g C) proj^T                   proj: the candidates' rows R_j C; cov = cross A^T as above
// Nothing of the resident state is written; the scratch is one buffer of the context (algp_ctx::grp).
#include <cmath>

#include "api_impl.h"

using namespace algp;

namespace algp {

template <typename T>
int Impl<T>::group_posterior(algp_ctx* c, const int32_t* group, const double* weight, int64_t Q, void* mean_out, void* cov_out,
                             void* cross_out, bool fixed) {
    const std::string who = fixed ? "group_posterior_fixed" : "group_posterior";
    if (fixed && c->fx_p <= 0) return fail(c, ALGP_ERR_STATE, who + ": no fixed effects are attached (algp_set_fixed_effects)");
    // the preconditions of algp_get_posterior_cov, for its reasons
    if (!c->solved) return fail(c, ALGP_ERR_STATE, who + ": call algp_solve_candidates first");
    if (c->pool_is_cov) return fail(c, ALGP_ERR_BAD_ARG, who + " needs a coordinate pool");
    const int64_t N = c->N, Npad = c->Npad, M = c->M, Mpad = c->Mpad;
    if (c->prior_noise)
        for (int64_t j = 0; j < M; ++j)
            if (c->vt_kind[j] >= 0)
                return fail(c, ALGP_ERR_STATE,
                            who + ": candidate " + std::to_string(j) + " (pool index " + std::to_string(c->cand_idx[j]) +
                                ") is a train site and was solved as a unit row (prior_includes_noise = 1): set the "
                                "candidates with prior_includes_noise = 0");
    if (!c->picks.empty())
        return fail(c, ALGP_ERR_STATE, who + ": " + std::to_string(c->picks.size()) +
                                           " pick(s) were committed since the candidate solve, which the aggregates would "
                                           "not include: solve the candidates again");
    if (fixed) {                                                  // and algp_get_posterior_fixed's
        if (c->train_dirty || c->vt_hyp_stamp != c->hyp_stamp || c->vt_fact_idx != c->fact_idx || c->vt_fact_var != c->fact_var)
            return fail(c, ALGP_ERR_STATE, who + ": the candidate solve is not the current factor's: solve the candidates again");
        if (c->ldv % 4 != 0) return fail(c, ALGP_ERR_STATE, who + ": the row stride of V^T is not a multiple of 4");
    }
    if (M > 0 && !group) return fail(c, ALGP_ERR_BAD_ARG, who + ": group is NULL");
    if (Q > INT_MAX) return fail(c, ALGP_ERR_BAD_ARG, who + ": Q is too large");
    for (int64_t j = 0; j < M; ++j) {
        if (group[j] < -1 || group[j] >= Q)
            return fail(c, ALGP_ERR_BAD_ARG, who + ": candidate " + std::to_string(j) + " carries the label " +
                                                 std::to_string(group[j]) + ", outside [-1, " + std::to_string(Q) + ")");
        if (weight && !std::isfinite(weight[j]))
            return fail(c, ALGP_ERR_BAD_ARG, who + ": the weight of candidate " + std::to_string(j) + " is not finite");
    }

    // the stable counting sort of the labelled rows by group: candidate order inside a group
    std::vector<int64_t> off((size_t)Q + 1, 0);
    for (int64_t j = 0; j < M; ++j)
        if (group[j] >= 0) ++off[(size_t)group[j] + 1];
    if (!weight)
        for (int64_t q = 0; q < Q; ++q)
            if (off[(size_t)q + 1] == 0)
                return fail(c, ALGP_ERR_BAD_ARG, who + ": group " + std::to_string(q) + " has no members (its mean is undefined; "
                                                 "pass explicit weights for a zero functional)");
    for (int64_t q = 0; q < Q; ++q) off[(size_t)q + 1] += off[(size_t)q];
    const int64_t Lm = off[(size_t)Q];
    std::vector<int> perm((size_t)Lm), gid((size_t)Lm);
    std::vector<T> coef((size_t)Lm);
    {
        std::vector<int64_t> next(off.begin(), off.end() - 1);
        for (int64_t j = 0; j < M; ++j) {
            const int q = group[j];
            if (q < 0) continue;
            const int64_t m = next[(size_t)q]++;
            perm[(size_t)m] = (int)j;
            gid[(size_t)m] = q;
            coef[(size_t)m] = (T)(weight ? weight[j] : 1.0 / (double)(off[(size_t)q + 1] - off[(size_t)q]));
        }
    }
    // the groups that span chunks of the member list, per chunk size
    auto spanning = [&](int64_t chunk) {
        std::vector<int> s;
        for (int64_t q = 0; q < Q; ++q)
            if (off[(size_t)q + 1] > off[(size_t)q] && off[(size_t)q] / chunk != (off[(size_t)q + 1] - 1) / chunk) s.push_back((int)q);
        return s;
    };
    const std::vector<int> spanK = spanning(GROUP_CHUNK), spanR = spanning(GROUP_ROWCHUNK);
    const bool want_mat = cov_out || cross_out;
    const int64_t Qpad = round_up(Q, NB);
    const int64_t nchK = (Lm + GROUP_CHUNK - 1) / GROUP_CHUNK, nchR = (Lm + GROUP_ROWCHUNK - 1) / GROUP_ROWCHUNK;

    // the scratch, carved out of one allocation; the sorted list goes up in one copy ([off | perm | gid | coef | spanK | spanR])
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t o = total; total += (bytes + 255) / 256 * 256; return o; };
    const size_t o_off = take(sizeof(int64_t) * ((size_t)Q + 1));
    const size_t o_perm = take(sizeof(int) * (size_t)Lm);
    const size_t o_gid = take(sizeof(int) * (size_t)Lm);
    const size_t o_coef = take(sizeof(T) * (size_t)Lm);
    const size_t o_spK = take(sizeof(int) * spanK.size());
    const size_t o_spR = take(sizeof(int) * spanR.size());
    const size_t o_iota = take(fixed ? sizeof(int64_t) * (size_t)Qpad : 0);         // fixed: row q of A H_C is row q's basis row
    const size_t up_bytes = total;
    const size_t o_mean = take(sizeof(T) * (size_t)Qpad);
    const size_t o_mpart = take(sizeof(T) * 2 * (size_t)nchR);
    const size_t o_U = take(want_mat ? sizeof(T) * (size_t)Qpad * (size_t)Mpad : 0);
    const size_t o_Upart = take(want_mat ? sizeof(T) * 2 * (size_t)nchK * (size_t)Mpad : 0);
    const size_t o_T = take(want_mat || fixed ? sizeof(T) * (size_t)Qpad * (size_t)Npad : 0);
    const size_t o_Tpart = take(want_mat || fixed ? sizeof(T) * 2 * (size_t)nchR * (size_t)Npad : 0);
    // fixed: H_C (the candidates' basis rows), A H_C and its chunk pieces, the mean with the trend, the rows R_g C
    const size_t o_HC = take(fixed ? sizeof(T) * (size_t)std::max<int64_t>(M, 1) * FX_P : 0);
    const size_t o_AH = take(fixed ? sizeof(T) * (size_t)Qpad * FX_P : 0);
    const size_t o_AHpart = take(fixed ? sizeof(T) * 2 * (size_t)nchR * FX_P : 0);
    const size_t o_meanF = take(fixed ? sizeof(T) * (size_t)Qpad : 0);
    const size_t o_projG = take(fixed ? sizeof(T) * (size_t)Qpad * FX_P : 0);
    const size_t o_G = take(cov_out && !cross_out ? sizeof(T) * (size_t)Qpad * (size_t)Qpad : 0);
    const size_t o_cov = take(cov_out ? sizeof(T) * (size_t)Q * (size_t)Q : 0);
    if (total > c->grp.cap) {
        size_t free_b = 0, total_b = 0;
        ALGP_HIP(hipMemGetInfo(&free_b, &total_b));
        if (total > c->grp.cap + free_b)
            return fail(c, ALGP_ERR_OOM, who + ": the scratch of " + std::to_string(Q) + " groups takes " + std::to_string(total) +
                                             " bytes, " + std::to_string(c->grp.cap + free_b) + " available");
    }
    ALGP_TRY(ensure(c, c->grp, total));
    char* base = (char*)c->grp.p;
    {
        std::vector<char> up(up_bytes, 0);
        memcpy(up.data() + o_off, off.data(), sizeof(int64_t) * off.size());
        if (Lm > 0) {
            memcpy(up.data() + o_perm, perm.data(), sizeof(int) * (size_t)Lm);
            memcpy(up.data() + o_gid, gid.data(), sizeof(int) * (size_t)Lm);
            memcpy(up.data() + o_coef, coef.data(), sizeof(T) * (size_t)Lm);
        }
        if (!spanK.empty()) memcpy(up.data() + o_spK, spanK.data(), sizeof(int) * spanK.size());
        if (!spanR.empty()) memcpy(up.data() + o_spR, spanR.data(), sizeof(int) * spanR.size());
        if (fixed)
            for (int64_t q = 0; q < Qpad; ++q) ((int64_t*)(up.data() + o_iota))[q] = q;
        ALGP_HIP(hipMemcpy(base, up.data(), up_bytes, hipMemcpyHostToDevice));   // complete on return: `up` goes out of scope
    }
    const GroupSegs<T> g = {(const int*)(base + o_perm), (const int*)(base + o_gid), (const T*)(base + o_coef),
                            (const int64_t*)(base + o_off), Lm, (int)Q};
    const int *spK = (const int*)(base + o_spK), *spR = (const int*)(base + o_spR);
    T *meanD = (T*)(base + o_mean), *mpart = (T*)(base + o_mpart), *U = (T*)(base + o_U), *Upart = (T*)(base + o_Upart);
    T *Tm = (T*)(base + o_T), *Tpart = (T*)(base + o_Tpart), *G = (T*)(base + o_G), *covD = (T*)(base + o_cov);

    // fixed: F^T and the p x p work; T = A V^T and A H_C first, the pass over T's rows gives R_g = A H_C - T F, R_g beta and R_g C
    FixedPlan pl;
    T *HC = (T*)(base + o_HC), *AH = (T*)(base + o_AH), *AHpart = (T*)(base + o_AHpart), *meanF = (T*)(base + o_meanF);
    T* projG = (T*)(base + o_projG);
    const int fp = c->fx_p;
    auto form_T = [&]() -> int {
        ALGP_HIP(hipMemsetAsync(Tm, 0, sizeof(T) * (size_t)Qpad * (size_t)Npad, c->stream));
        return group_rowsum_launch<T>(c, p(c->Vt), c->ldv, Npad, g, spR, (int)spanR.size(), Tm, Npad, Tpart, Npad);
    };
    if (fixed) {
        ALGP_TRY(fixed_enqueue(c, who.c_str(), {.post_rows = cross_out ? std::max<int64_t>(M, 1) : 1, .proj = cross_out != nullptr}, pl));
        if (M > 0) {
            ALGP_TRY(form_T());
            ALGP_TRY(fixed_rows_launch<T>(c, (const T*)c->fxH.p, (const int64_t*)c->Cidx.p, M, HC));
            ALGP_HIP(hipMemsetAsync(AH, 0, sizeof(T) * (size_t)Qpad * FX_P, c->stream));
            ALGP_TRY(group_rowsum_launch<T>(c, HC, FX_P, FX_P, g, spR, (int)spanR.size(), AH, FX_P, AHpart, FX_P));
        }
    }
    if (mean_out) {
        ALGP_HIP(hipMemsetAsync(meanD, 0, sizeof(T) * (size_t)Qpad, c->stream));                      // groups without members: 0
        ALGP_TRY(group_rowsum_launch<T>(c, p(c->mu), 1, 1, g, spR, (int)spanR.size(), meanD, 1, mpart, 1));
        if (!fixed) ALGP_HIP(hipMemcpyAsync(mean_out, meanD, sizeof(T) * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    }
    if (fixed) {
        if (M > 0)
            ALGP_TRY(fixed_post_launch<T>(c, Tm, Npad, Q, Npad, pl.Ft, Npad, AH, (const int64_t*)(base + o_iota), pl.gls, fp, meanD, (const T*)nullptr,
                                          mean_out ? meanF : (T*)nullptr, (T*)nullptr, projG));
        else
            ALGP_HIP(hipMemsetAsync(meanF, 0, sizeof(T) * (size_t)Qpad, c->stream));
        if (mean_out) ALGP_HIP(hipMemcpyAsync(mean_out, meanF, sizeof(T) * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    }
    if (want_mat && M == 0) {                                     // no candidates: every functional is zero
        if (cov_out) memset(cov_out, 0, sizeof(T) * (size_t)Q * (size_t)Q);
    } else if (want_mat) {
        // rows of groups without members and the padding rows stay zero: U is an operand of the products
        ALGP_HIP(hipMemsetAsync(U, 0, sizeof(T) * (size_t)Qpad * (size_t)Mpad, c->stream));
        ALGP_TRY(group_ksum_launch<T>(c, make_src(c), (const int64_t*)c->Cidx.p, M, Mpad, c->cextra.p ? (const T*)c->cextra.p : nullptr, g,
                                      spK, (int)spanK.size(), U, Upart));
        if (N > 0 && !fixed) ALGP_TRY(form_T());
        if (cross_out) {
            if (N > 0)
                ALGP_TRY(gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, Qpad, Mpad, Npad, (T)-1, Tm, Npad, p(c->Vt), c->ldv, (T)1, U, Mpad, U,
                                           Mpad, 0));
            if (fixed) {
                // cross += (R_g C) proj^T with proj the candidates' own rows R_j C; cov = cross A^T then carries (R_g C)(R_g C)^T
                ALGP_TRY(fixed_post_launch<T>(c, p(c->Vt), c->ldv, M, Npad, pl.Ft, Npad, (const T*)c->fxH.p, (const int64_t*)c->Cidx.p, pl.gls, fp,
                                              (const T*)nullptr, (const T*)nullptr, (T*)nullptr, (T*)nullptr, pl.proj));
                ALGP_TRY(fixed_fold_launch<T>(c, U, Mpad, Q, M, projG, fp, pl.proj, fp, fp, 1));
            }
            ALGP_HIP(hipMemcpy2DAsync(cross_out, sizeof(T) * M, U, sizeof(T) * Mpad, sizeof(T) * M, (size_t)Q, hipMemcpyDeviceToHost,
                                      c->stream));
            if (cov_out) ALGP_TRY(group_colsum_launch<T>(c, U, Mpad, g, (const T*)nullptr, 0, covD));
        } else {
            if (N > 0)
                ALGP_TRY(gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, Qpad, Qpad, Npad, (T)1, Tm, Npad, Tm, Npad, (T)0, (const T*)nullptr,
                                           Qpad, G, Qpad, 1));
            ALGP_TRY(group_colsum_launch<T>(c, U, Mpad, g, N > 0 ? G : (const T*)nullptr, Qpad, covD));
            if (fixed) ALGP_TRY(fixed_fold_launch<T>(c, covD, Q, Q, Q, projG, fp, projG, fp, fp, 1));
        }
        if (cov_out) ALGP_HIP(hipMemcpyAsync(cov_out, covD, sizeof(T) * (size_t)Q * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    }
    if (!fixed) return sync(c);
    double info = 0.0;
    ALGP_HIP(hipMemcpyAsync(&info, pl.gls + FX_INFO, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ALGP_TRY(sync_checked(c, who.c_str()));
    if (info != 0.0) return fixed_rank_error(c, who.c_str(), info);
    return ALGP_OK;
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_group_posterior(algp_ctx* c, const int32_t* group, const double* weight, int64_t Q, void* mean_out, void* cov_out,
                         void* cross_out) {
    CHECK_CTX(c);
    if (Q < 1) return fail(c, ALGP_ERR_BAD_ARG, "group_posterior: Q >= 1 required");
    FINISH(c, DISPATCH(c, group_posterior(c, group, weight, Q, mean_out, cov_out, cross_out)));
}

int algp_group_posterior_fixed(algp_ctx* c, const int32_t* group, const double* weight, int64_t Q, void* mean_out, void* cov_out,
                               void* cross_out) {
    CHECK_CTX(c);
    if (Q < 1) return fail(c, ALGP_ERR_BAD_ARG, "group_posterior_fixed: Q >= 1 required");
    FINISH(c, DISPATCH(c, group_posterior(c, group, weight, Q, mean_out, cov_out, cross_out, true)));
}

}  // extern "C"
