// api_paths.hip -- best_path (agent.py:358-403): the entropy gain of every enumerated path in one call.
#include "api_impl.h"

using namespace algp;

namespace algp {


// Paths of 65 .. 256 distinct sites (cpos / lpos: candidate row and train row per site, packed to the front of each path's
// maxlen entries).  Per batch of paths: the paths' rows of V^T gathered into a scratch (a site that is a train row
// already: L[lpos, :] - var_lpos * its unit row, as in the LDS kernel), the Gram matrices as ONE batched lower-tile MFMA
// product, G = C_PP + sigma_m^2 I - Gram, then the ppad x ppad blocks factored as 2 x 2 tiles of 128
// (factor_blocks_batched, api_impl.h) -- every step one launch for the whole batch.
template <typename T>
int Impl<T>::score_paths_big(algp_ctx* c, const std::vector<int64_t>& cpos, const std::vector<int64_t>& lpos, int npaths, int maxlen,
                               int maxused, double mobile_std, double* dH) {
    const int64_t Npad = c->Npad;
    const int ppad = maxused <= NB ? NB : 2 * NB;
    // rows scratch: batch * ppad * Npad elements, at most ~4 GB
    const int64_t per_path = (int64_t)ppad * Npad * (int64_t)sizeof(T);
    const int bmax = (int)std::max<int64_t>(1, std::min<int64_t>(npaths, (int64_t)4e9 / per_path));
    ALGP_TRY(ensure(c, c->auxW, (size_t)bmax * per_path));
    ALGP_TRY(ensure(c, c->auxA, sizeof(T) * (size_t)bmax * ppad * ppad));
    ALGP_TRY(ensure(c, c->auxInv, sizeof(T) * (size_t)bmax * 2 * NB * NB));
    ALGP_TRY(ensure(c, c->auxD, sizeof(T) * (size_t)bmax * NB * NB));
    ALGP_TRY(ensure(c, c->auxIdx, sizeof(int64_t) * 2 * (size_t)bmax * ppad));
    ALGP_TRY(ensure(c, c->auxVar, sizeof(T) * (size_t)bmax * ppad + 256));
    ALGP_TRY(ensure(c, c->hostStage, sizeof(double) * (size_t)(npaths + bmax) + sizeof(int) * (size_t)bmax + 64));
    double* d_out = (double*)c->hostStage.p;
    double* d_ld = d_out + npaths;
    int* d_info = (int*)(d_ld + bmax);
    T* rows = p(c->auxW);
    T* G = p(c->auxA);
    T* inv = p(c->auxInv);
    T* L21 = p(c->auxD);
    int64_t* d_src = (int64_t*)c->auxIdx.p;
    int64_t* d_lrow = d_src + (size_t)bmax * ppad;
    std::vector<int64_t> src((size_t)bmax * ppad), lr((size_t)bmax * ppad);
    std::vector<T> lsc((size_t)bmax * ppad);
    for (int p0 = 0; p0 < npaths; p0 += bmax) {
        const int B = std::min(bmax, npaths - p0);
        bool second = false;
        for (int b = 0; b < B; ++b)
            for (int a = 0; a < ppad; ++a) {
                const size_t e = (size_t)b * ppad + a;
                const int64_t cp = a < maxlen ? cpos[(size_t)(p0 + b) * maxlen + a] : -1;
                const int64_t lp = a < maxlen ? lpos[(size_t)(p0 + b) * maxlen + a] : -1;
                src[e] = cp;
                lr[e] = cp >= 0 ? lp : -1;
                lsc[e] = (cp >= 0 && lp >= 0) ? (T)c->train_var_host[(size_t)lp] : (T)0;
                second |= cp >= 0 && lp >= 0;
            }
        const size_t nrow = (size_t)B * ppad;
        ALGP_HIP(hipMemcpyAsync(d_src, src.data(), sizeof(int64_t) * nrow, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(d_lrow, lr.data(), sizeof(int64_t) * nrow, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(c->auxVar.p, lsc.data(), sizeof(T) * nrow, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemsetAsync(d_ld, 0, sizeof(double) * B, c->stream));
        ALGP_HIP(hipMemsetAsync(d_info, 0, sizeof(int) * B, c->stream));
        ALGP_TRY(gather_rows_launch<T>(c, p(c->Vt), c->ldv, d_src, rows, Npad, (int64_t)nrow, Npad, second ? d_lrow : nullptr,
                                       second ? (const T*)c->auxVar.p : nullptr, p(c->L), c->Lld));
        ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = ppad, .n = ppad, .k = Npad, .A = {rows, Npad, (int64_t)ppad * Npad},
                                .B = {rows, Npad, (int64_t)ppad * Npad}, .D = {G, ppad, (int64_t)ppad * ppad}, .batch = B, .lower_only = 1}));
        ALGP_TRY(path_assemble_launch<T>(c, d_src, B, ppad, (const int64_t*)c->Cidx.p, make_src(c), mobile_std * mobile_std, G));
        ALGP_TRY(factor_blocks_batched<T>(c, G, ppad, inv, L21, d_ld, d_info, B));
        ALGP_TRY(path_finish_launch(c, d_src, ppad, B, d_ld, d_info, d_out + p0));
        ALGP_TRY(sync(c));                                   // the index vectors are reused by the next batch
    }
    ALGP_HIP(hipMemcpyAsync(dH, d_out, sizeof(double) * npaths, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}


// a8 / f3: the entropy gain of every enumerated path (agent.py:374-400 computes one slogdet per path) from ONE
// resident factor and candidate solve: sites[p][a] are pool indices (-1 = none); a site that already is a train
// row receives a second (mobile) row, a new site a first one; dH[p] = H(A u path_p) - H(A)
template <typename T>
int Impl<T>::score_paths(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double mobile_std, double* dH) {
    if (!c->solved) return fail(c, ALGP_ERR_STATE, "score_paths: call algp_solve_candidates first");
    if (!c->prior_noise) return fail(c, ALGP_ERR_STATE, "score_paths: candidates were set with predictive semantics");
    if (!c->picks.empty()) return fail(c, ALGP_ERR_STATE, "score_paths: picks were committed since the candidate solve; solve again");
    const size_t tot = (size_t)npaths * maxlen;
    std::vector<int64_t> cpos(tot, -1), lpos(tot, -1);
    int maxused = 0;
    for (int pth = 0; pth < npaths; ++pth) {
        int used = 0;
        for (int a = 0; a < maxlen; ++a) {
            const int64_t j = sites[(size_t)pth * maxlen + a];
            if (j < 0) continue;
            if (j >= c->n_pool) return fail(c, ALGP_ERR_BAD_ARG, "score_paths: index outside the pool");
            const int64_t cp = c->cand_pos[j];
            if (cp < 0) return fail(c, ALGP_ERR_BAD_ARG, "score_paths: site " + std::to_string(j) + " is not a resident candidate");
            bool dup = false;
            for (int b = 0; b < used; ++b) dup |= cpos[(size_t)pth * maxlen + b] == cp;
            if (dup) continue;                                  // a site crossed twice is measured once (mobile mask)
            cpos[(size_t)pth * maxlen + used] = cp;
            lpos[(size_t)pth * maxlen + used] = c->pos_in_train[j];
            ++used;
        }
        if (used > 256) return fail(c, ALGP_ERR_BAD_ARG, "score_paths: more than 256 distinct sites in a path");
        maxused = std::max(maxused, used);
    }
    if (maxused > 64) return score_paths_big(c, cpos, lpos, npaths, maxlen, maxused, mobile_std, dH);
    ALGP_TRY(ensure(c, c->auxIdx, sizeof(int64_t) * 2 * tot));
    ALGP_TRY(ensure(c, c->hostStage, sizeof(double) * std::max<size_t>(npaths, 1)));
    int64_t* d_c = (int64_t*)c->auxIdx.p;
    int64_t* d_l = d_c + tot;
    ALGP_HIP(hipMemcpyAsync(d_c, cpos.data(), sizeof(int64_t) * tot, hipMemcpyHostToDevice, c->stream));
    ALGP_HIP(hipMemcpyAsync(d_l, lpos.data(), sizeof(int64_t) * tot, hipMemcpyHostToDevice, c->stream));
    ALGP_TRY(path_score_launch<T>(c, d_c, d_l, npaths, maxlen, (const int64_t*)c->Cidx.p, p(c->Vt), c->ldv, c->ncols, p(c->L),
                                  c->Lld, (const T*)c->varA.p, make_src(c), mobile_std * mobile_std, (double*)c->hostStage.p));
    ALGP_HIP(hipMemcpyAsync(dH, c->hostStage.p, sizeof(double) * npaths, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

// best_path under the MI criterion (agent.py:374-400: ent_a + ent_abar - ent_all per path, two of them pool-sized).  Relative
// to the base state (train set A0, complement Abar0, noise D0), path p changes S = S_new u S_rm: new sites join A with noise
// sm and leave Abar; re-measured train sites keep their place and their fused noise goes v_a -> v_a sm / (v_a + sm).
//   dH_A    = H(A0 u S_new, fused) - H(A0): score_paths' dH (a re-measured site as a second row) minus
//             sum over S_rm of CONST + 1/2 log(v_a + sm) (row form -> fused form)
//   dH_Abar = 1/2 log det P[S_new, S_new] - |S_new| CONST            (Jacobi: det C_{Abar0 \ S} = det C_Abar0 det (C^-1)_SS)
//   dH_all  = 1/2 log det (I + G^T D G), Q[S, S] = G G^T            (determinant lemma; D = diag(delta) < 0 on S_rm, so the
//             symmetric form sqrt(D) Q sqrt(D) does not exist -- I + G^T D G is congruent to the Schur complement of C + D_p)
// P and Q are the resident inverses of mi_build, built only when the MI state is not valid; per batch of paths their rows are
// gathered (masked left of the diagonal tile), the blocks are batched Gram products on MFMA, then 2 x 2 tiled factorisations.
template <typename T>
int Impl<T>::score_paths_mi(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double static_std, double mobile_std,
                            double* dMI, double* terms) {
    if (!c->solved) return fail(c, ALGP_ERR_STATE, "score_paths_mi: call algp_solve_candidates first");
    if (!c->prior_noise) return fail(c, ALGP_ERR_STATE, "score_paths_mi: candidates were set with predictive semantics");
    if (!c->picks.empty()) return fail(c, ALGP_ERR_STATE, "score_paths_mi: picks were committed since the candidate solve; solve again");
    const double ss = static_std * static_std, sm = mobile_std * mobile_std;
    // per path: its changing sites, new ones first (pool indices), and how many of them are new
    const size_t tot = (size_t)npaths * maxlen;
    std::vector<int64_t> packed(tot, -1);
    std::vector<int> knew(npaths, 0), kall(npaths, 0);
    int maxk = 0;
    for (int pth = 0; pth < npaths; ++pth) {
        std::vector<int64_t> nw, rm;
        for (int a = 0; a < maxlen; ++a) {
            const int64_t j = sites[(size_t)pth * maxlen + a];
            if (j < 0) continue;
            if (j >= c->n_pool) return fail(c, ALGP_ERR_BAD_ARG, "score_paths_mi: index outside the pool");
            if (c->cand_pos[j] < 0)
                return fail(c, ALGP_ERR_STATE, "score_paths_mi: site " + std::to_string(j) + " is not a resident candidate");
            auto& lst = c->pos_in_train[j] >= 0 ? rm : nw;
            if (std::find(lst.begin(), lst.end(), j) == lst.end()) lst.push_back(j);   // a site crossed twice counts once
        }
        const int k = (int)(nw.size() + rm.size());
        if (k > 256) return fail(c, ALGP_ERR_BAD_ARG, "score_paths_mi: more than 256 changing sites in a path");
        knew[pth] = (int)nw.size();
        kall[pth] = k;
        for (int a = 0; a < k; ++a) packed[(size_t)pth * maxlen + a] = a < knew[pth] ? nw[a] : rm[a - knew[pth]];
        maxk = std::max(maxk, k);
    }
    // the pool-wide inverses (their O(n^3) build, or ALGP_ERR_OOM up front) unless the one-GPU state is held (MiState::current)
    if (!c->mi.holds(0)) ALGP_TRY(mi_build(c, ss, sm));
    // dH_A: the entropy block scorer on the same sites (both of its regimes)
    std::vector<double> dHA(npaths);
    ALGP_TRY(score_paths(c, packed.data(), npaths, maxlen, mobile_std, dHA.data()));

    const int64_t npad = c->mi.npad, mb = c->mi.mb, mbpad = c->mi.mbpad;
    const int ppad = maxk <= NB ? NB : 2 * NB;
    const size_t mat = (size_t)ppad * ppad;
    // per path: its gathered rows (ppad x npad, P's narrower rows reuse them), four blocks, two inverse tiles, one L21 tile
    const double per_path = (double)sizeof(T) * ((double)ppad * npad + 4.0 * mat + 3.0 * NB * NB);
    const int bmax = (int)std::max<double>(1.0, std::min<double>({(double)npaths, 4e9 / per_path, 65535.0}));
    ALGP_TRY(ensure(c, c->auxW, sizeof(T) * (size_t)bmax * ppad * npad));
    ALGP_TRY(ensure(c, c->auxA, sizeof(T) * (4 * (size_t)bmax + 1) * mat));
    ALGP_TRY(ensure(c, c->auxInv, sizeof(T) * (size_t)bmax * 2 * NB * NB));
    ALGP_TRY(ensure(c, c->auxD, sizeof(T) * (size_t)bmax * NB * NB));
    ALGP_TRY(ensure(c, c->auxIdx, sizeof(int64_t) * 2 * (size_t)bmax * ppad));
    ALGP_TRY(ensure(c, c->auxVar, sizeof(T) * (size_t)bmax * ppad + sizeof(int) * 2 * (size_t)bmax + 256));
    ALGP_TRY(ensure(c, c->hostStage, sizeof(double) * 3 * (size_t)bmax + sizeof(int) * 3 * (size_t)bmax + 64));
    T* rows = p(c->auxW);
    T* GP = p(c->auxA);                                      // P_SS, then I + G^T D G
    T* GQ = GP + (size_t)bmax * mat;                         // Q_SS -> its factor G
    T* Lt = GQ + (size_t)bmax * mat;
    T* LtD = Lt + (size_t)bmax * mat;
    T* ident = LtD + (size_t)bmax * mat;
    T* inv = p(c->auxInv);
    T* L21 = p(c->auxD);
    int64_t* d_srcP = (int64_t*)c->auxIdx.p;
    int64_t* d_srcQ = d_srcP + (size_t)bmax * ppad;
    T* d_delta = p(c->auxVar);
    int* d_cntP = (int*)((char*)c->auxVar.p + sizeof(T) * (size_t)bmax * ppad);
    int* d_cntQ = d_cntP + bmax;
    double* d_ld = (double*)c->hostStage.p;                  // [log det P_SS | log det Q_SS | log det (I + G^T D G)]
    int* d_info = (int*)(d_ld + 3 * (size_t)bmax);
    ALGP_TRY(set_identity_launch<T>(c, ident, ppad, ppad));
    std::vector<int64_t> srcP((size_t)bmax * ppad), srcQ((size_t)bmax * ppad);
    std::vector<T> delta((size_t)bmax * ppad);
    std::vector<int> cnt(2 * (size_t)bmax);
    std::vector<double> ld(3 * (size_t)bmax), ldP(npaths), ldM(npaths);
    std::vector<int> info(3 * (size_t)bmax), bad(npaths);
    for (int p0 = 0; p0 < npaths; p0 += bmax) {
        const int B = std::min(bmax, npaths - p0);
        for (int b = 0; b < B; ++b) {
            const int pth = p0 + b;
            for (int a = 0; a < ppad; ++a) {
                const size_t e = (size_t)b * ppad + a;
                const int64_t j = a < kall[pth] ? packed[(size_t)pth * maxlen + a] : -1;
                srcP[e] = a < knew[pth] ? c->mi.posbar[j] : -1;
                srcQ[e] = j;
                double dl = 0.0;
                if (a < knew[pth]) dl = sm;
                else if (j >= 0) {
                    const double va = c->train_var_host[(size_t)c->pos_in_train[j]];
                    dl = va * sm / (va + sm) - va;
                }
                delta[e] = (T)dl;
            }
            cnt[b] = knew[pth];
            cnt[bmax + b] = kall[pth];
        }
        const size_t nrow = (size_t)B * ppad;
        ALGP_HIP(hipMemcpyAsync(d_srcP, srcP.data(), sizeof(int64_t) * nrow, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(d_srcQ, srcQ.data(), sizeof(int64_t) * nrow, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(d_delta, delta.data(), sizeof(T) * nrow, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(d_cntP, cnt.data(), sizeof(int) * 2 * (size_t)bmax, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemsetAsync(d_ld, 0, sizeof(double) * 3 * (size_t)bmax, c->stream));
        ALGP_HIP(hipMemsetAsync(d_info, 0, sizeof(int) * 3 * (size_t)bmax, c->stream));
        // P_SS over the new sites (nothing to do when every site is sampled: no path then has a new site)
        if (mb > 0) {
            ALGP_TRY(mi_tri_gather_launch<T>(c, p(c->mi.Xbar), mbpad, d_srcP, rows, mbpad, (int64_t)nrow, mbpad));
            ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = ppad, .n = ppad, .k = mbpad, .A = {rows, mbpad, (int64_t)ppad * mbpad},
                                    .B = {rows, mbpad, (int64_t)ppad * mbpad}, .D = {GP, ppad, (int64_t)mat}, .batch = B, .lower_only = 1}));
            ALGP_TRY(mi_pad_diag_launch<T>(c, GP, ppad, d_cntP, B));
            ALGP_TRY(factor_blocks_batched<T>(c, GP, ppad, inv, L21, d_ld, d_info, B));
        }
        // Q_SS over all changing sites -> G, then I + G^T D G = I + Lt LtD^T
        ALGP_TRY(mi_tri_gather_launch<T>(c, p(c->mi.Xall), npad, d_srcQ, rows, npad, (int64_t)nrow, npad));
        ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = ppad, .n = ppad, .k = npad, .A = {rows, npad, (int64_t)ppad * npad},
                                .B = {rows, npad, (int64_t)ppad * npad}, .D = {GQ, ppad, (int64_t)mat}, .batch = B, .lower_only = 1}));
        ALGP_TRY(mi_pad_diag_launch<T>(c, GQ, ppad, d_cntQ, B));
        ALGP_TRY(factor_blocks_batched<T>(c, GQ, ppad, inv, L21, d_ld + bmax, d_info + bmax, B));
        ALGP_TRY(mi_transpose_launch<T>(c, GQ, L21, d_delta, ppad, Lt, LtD, B));
        ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = ppad, .n = ppad, .k = ppad, .beta = (T)1, .A = {Lt, ppad, (int64_t)mat},
                                .B = {LtD, ppad, (int64_t)mat}, .C = {ident, ppad}, .D = {GP, ppad, (int64_t)mat}, .batch = B, .lower_only = 1}));
        ALGP_TRY(factor_blocks_batched<T>(c, GP, ppad, inv, L21, d_ld + 2 * bmax, d_info + 2 * bmax, B));
        ALGP_HIP(hipMemcpyAsync(ld.data(), d_ld, sizeof(double) * 3 * (size_t)bmax, hipMemcpyDeviceToHost, c->stream));
        ALGP_HIP(hipMemcpyAsync(info.data(), d_info, sizeof(int) * 3 * (size_t)bmax, hipMemcpyDeviceToHost, c->stream));
        ALGP_TRY(sync(c));                                   // the index vectors are reused by the next batch
        for (int b = 0; b < B; ++b) {
            ldP[p0 + b] = ld[b];
            ldM[p0 + b] = ld[2 * (size_t)bmax + b];
            bad[p0 + b] = info[b] != 0 || info[bmax + b] != 0 || info[2 * (size_t)bmax + b] != 0;
        }
    }
    for (int pth = 0; pth < npaths; ++pth) {
        double fuse = 0.0;                                   // row form -> fused form, per re-measured site
        for (int a = knew[pth]; a < kall[pth]; ++a) {
            const int64_t j = packed[(size_t)pth * maxlen + a];
            fuse += ENT_CONST + 0.5 * log(c->train_var_host[(size_t)c->pos_in_train[j]] + sm);
        }
        const double hA = dHA[pth] - fuse;
        const double hBar = bad[pth] ? NAN : 0.5 * ldP[pth] - (double)knew[pth] * ENT_CONST;
        const double hAll = bad[pth] ? NAN : 0.5 * ldM[pth];
        dMI[pth] = hA + hBar - hAll;
        if (terms) {
            terms[3 * (size_t)pth + 0] = hA;
            terms[3 * (size_t)pth + 1] = hBar;
            terms[3 * (size_t)pth + 2] = hAll;
        }
    }
    return ALGP_OK;
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_score_paths(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double mobile_std, double* dH_out) {
    CHECK_CTX(c);
    if (npaths < 0 || maxlen < 1 || (npaths > 0 && (!sites || !dH_out))) return fail(c, ALGP_ERR_BAD_ARG, "score_paths: bad arguments");
    if (npaths == 0) return ALGP_OK;
    FINISH(c, DISPATCH(c, score_paths(c, sites, npaths, maxlen, mobile_std, dH_out)));
}

int algp_score_paths_mi(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double static_std, double mobile_std, double* dMI_out,
                        double* terms_out) {
    CHECK_CTX(c);
    if (npaths < 0 || maxlen < 1 || (npaths > 0 && (!sites || !dMI_out)) || !(static_std > 0) || !(mobile_std > 0))
        return fail(c, ALGP_ERR_BAD_ARG, "score_paths_mi: bad arguments");
    if (npaths == 0) return ALGP_OK;
    FINISH(c, DISPATCH(c, score_paths_mi(c, sites, npaths, maxlen, static_std, mobile_std, dMI_out, terms_out)));
}

}  // extern "C"
