// api_paths_vr.hip -- the variance-reduction utility of whole paths (include/algp_hip.h: algp_score_paths_vr): how much the
// mobile readings along path p lower the summed predictive variance of the targets T (the ordinary rows of the candidate set),
//   u_p = sum_{j in T} var(j | A) - sum_{j in T} var(j | A u path_p) = tr((Gamma_SS + sm I)^-1 Phi_SS),   S = the path's sites,
//   Gamma_ss' = C(s, s') - R_s . R_s'      the posterior covariance of the sites (R_s: the site's row of V^T; a site that is train
//                                          row l already: L[l, :] - var_l * its unit row, as in score_paths)
//   E_sj      = C(s, j) - R_s . V_j        their cross covariance with the targets
//   Phi       = E Omega E^T                summed over the targets, Omega = diag of the pool's target weights (algp_set_target_weights;
//                                          the identity where none are attached): the E tile carries sqrt(omega_j) E_sj
// (with weights the first sum is over omega_j var(j | .) as well).
// Gamma and Phi depend on the sites, not on the path, and the paths of one planning step share most of their sites: both are
// built once over the union U of a group of consecutive paths, then every path gathers its two k x k blocks.
//   rows   R_U = the union's rows of V^T (gather_rows_launch, zero rows behind U up to a multiple of 128)
//   Gamma  one lower-only product R_U R_U^T, then C(U, U) - Gram in place (pvr_assemble_kernel)
//   Phi    the targets in chunks of columns: E_chunk = C(U, chunk) - R_U V_chunk^T as ONE product whose epilogue forms the kernel
//          term in registers, masks the columns that are not targets and writes the tile (gemm.hip: gemm_nt_launch_pvr), then
//          Phi += E_chunk E_chunk^T (lower-only), in chunk order: the same bits in every run
//   paths  up to 64 sites: one workgroup per path in LDS (pvr_small_kernel); 65 .. 256: batched 2 x 2 tiled factorisations
//          (factor_blocks_batched), L^-1 from the inverse tiles, W = L^-1 Phi_SS as one batched product, u = sum_{i >= j} W_ij (L^-1)_ij
#include "api_impl.h"

using namespace algp;

namespace algp {

constexpr int64_t PVR_CHUNK = 16384;     // target columns per E scratch (U x chunk)

template <typename T>
int Impl<T>::score_paths_vr(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double mobile_std, int64_t max_union, double* dV) {
    if (!c->solved) return fail(c, ALGP_ERR_STATE, "score_paths_vr: call algp_solve_candidates first");
    if (!c->prior_noise) return fail(c, ALGP_ERR_STATE, "score_paths_vr: candidates were set with predictive semantics");
    if (!c->picks.empty()) return fail(c, ALGP_ERR_STATE, "score_paths_vr: picks were committed since the candidate solve; solve again");
    if (c->cextra.p)
        return fail(c, ALGP_ERR_STATE, "score_paths_vr: candidates with an extra variance of their own are not supported");
    {
        // as for the criterion: a pool site listed twice would be two targets with sigma_n^2 between them
        std::vector<int64_t> sorted(c->cand_idx);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(c, ALGP_ERR_STATE, "score_paths_vr: the candidate set lists a pool site more than once");
    }
    if (max_union > 0 && max_union < 256) return fail(c, ALGP_ERR_BAD_ARG, "score_paths_vr: max_union below 256 (one path's sites)");
    const int64_t M = c->M, Mpad = c->Mpad, Npad = c->Npad;
    const double sm = mobile_std * mobile_std;
    // per path: the candidate rows of its distinct sites, packed to the front
    const size_t tot = (size_t)npaths * maxlen;
    std::vector<int64_t> cpos(tot, -1);
    std::vector<int> used(npaths, 0);
    for (int pth = 0; pth < npaths; ++pth) {
        int k = 0;
        for (int a = 0; a < maxlen; ++a) {
            const int64_t j = sites[(size_t)pth * maxlen + a];
            if (j < 0) continue;
            if (j >= c->n_pool) return fail(c, ALGP_ERR_BAD_ARG, "score_paths_vr: index outside the pool");
            const int64_t cp = c->cand_pos[j];
            if (cp < 0) return fail(c, ALGP_ERR_BAD_ARG, "score_paths_vr: site " + std::to_string(j) + " is not a resident candidate");
            bool dup = false;
            for (int b = 0; b < k; ++b) dup |= cpos[(size_t)pth * maxlen + b] == cp;
            if (dup) continue;                                  // a site crossed twice is measured once
            cpos[(size_t)pth * maxlen + k++] = cp;
        }
        if (k > 256) return fail(c, ALGP_ERR_BAD_ARG, "score_paths_vr: more than 256 distinct sites in a path");
        used[pth] = k;
    }
    // groups of consecutive paths whose union holds at most ucap sites; by default the largest union whose rows (U x Npad) and
    // whose two U x U matrices each stay within ~4 GB: a site shared by paths of two groups is paid for in both
    const int64_t by_rows = (int64_t)4e9 / (std::max<int64_t>(Npad, NB) * (int64_t)sizeof(T));
    const int64_t by_mats = (int64_t)sqrt(4e9 / (2.0 * sizeof(T)));
    const int64_t ucap = max_union > 0 ? max_union : std::max<int64_t>(256, std::min(by_rows, by_mats) / NB * NB);
    struct Group {
        int p0, p1;
        std::vector<int64_t> urow;                              // candidate row of every union site, in order of first use
        std::vector<int> upos;                                  // per path and site: its position in urow (maxlen apart)
    };
    std::vector<Group> groups;
    {
        std::vector<int> where((size_t)M, -1);
        Group g{0, 0, {}, {}};
        for (int pth = 0; pth < npaths; ++pth) {
            int fresh = 0;
            for (int a = 0; a < used[pth]; ++a) fresh += where[(size_t)cpos[(size_t)pth * maxlen + a]] < 0;
            if (pth > g.p0 && (int64_t)g.urow.size() + fresh > ucap) {
                g.p1 = pth;
                for (int64_t r : g.urow) where[(size_t)r] = -1;
                groups.push_back(std::move(g));
                g = Group{pth, pth, {}, {}};
            }
            for (int a = 0; a < maxlen; ++a) {
                int u = -1;
                if (a < used[pth]) {
                    const int64_t cp = cpos[(size_t)pth * maxlen + a];
                    if (where[(size_t)cp] < 0) {
                        where[(size_t)cp] = (int)g.urow.size();
                        g.urow.push_back(cp);
                    }
                    u = where[(size_t)cp];
                }
                g.upos.push_back(u);
            }
        }
        g.p1 = npaths;
        groups.push_back(std::move(g));
    }
    // scratch, sized once for the largest group (ensure() does not keep a buffer's contents)
    int64_t Upad_max = NB;
    int nbig_max = 0, np_max = 0, ppad_max = NB;
    for (const Group& g : groups) {
        Upad_max = std::max<int64_t>(Upad_max, ((int64_t)g.urow.size() + NB - 1) / NB * NB);
        int nbig = 0;
        for (int pth = g.p0; pth < g.p1; ++pth) {
            nbig += used[pth] > 64;
            if (used[pth] > NB) ppad_max = 2 * NB;
        }
        nbig_max = std::max(nbig_max, nbig);
        np_max = std::max(np_max, g.p1 - g.p0);
    }
    const int64_t chunk = std::min<int64_t>({Mpad, PVR_CHUNK, std::max<int64_t>(NB, (int64_t)4e9 / (Upad_max * (int64_t)sizeof(T)) / NB * NB)});
    const size_t mat_max = (size_t)ppad_max * ppad_max;
    const int bmax = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nbig_max, (int64_t)1e9 / (int64_t)(4 * mat_max * sizeof(T)), 65535}));
    ALGP_TRY(ensure(c, c->auxW, sizeof(T) * std::max<size_t>((size_t)Upad_max * Npad, nbig_max ? 4 * mat_max * bmax : 0)));
    ALGP_TRY(ensure(c, c->auxA, sizeof(T) * 2 * (size_t)Upad_max * Upad_max));
    ALGP_TRY(ensure(c, c->auxD, sizeof(T) * (size_t)Upad_max * chunk));
    ALGP_TRY(ensure(c, c->auxInv, sizeof(T) * (size_t)bmax * 6 * NB * NB));
    ALGP_TRY(ensure(c, c->auxIdx, sizeof(int64_t) * 3 * (size_t)Upad_max + sizeof(int) * (size_t)np_max * (2 * NB + 1) + 64));
    ALGP_TRY(ensure(c, c->auxVar, sizeof(T) * (size_t)Upad_max + 256));
    ALGP_TRY(ensure(c, c->hostStage, sizeof(double) * (size_t)(npaths + bmax) + sizeof(int) * (size_t)bmax + 64));
    double* d_out = (double*)c->hostStage.p;
    double* d_ld = d_out + npaths;
    int* d_info = (int*)(d_ld + bmax);
    T* R = p(c->auxW);
    T* Gam = p(c->auxA);
    T* Es = p(c->auxD);
    T* inv = p(c->auxInv);
    T* L21 = inv + (size_t)bmax * 2 * NB * NB;
    T* tr = L21 + (size_t)bmax * NB * NB;
    T* X = tr + (size_t)bmax * 2 * NB * NB;
    int64_t* d_src = (int64_t*)c->auxIdx.p;
    int64_t* d_lrow = d_src + Upad_max;
    int64_t* d_uidx = d_lrow + Upad_max;
    int* d_upos = (int*)(d_uidx + Upad_max);
    int* d_pid = d_upos + (size_t)np_max * 2 * NB;
    const KmatSrc s = make_src(c);
    ALGP_HIP(hipMemsetAsync(d_out, 0, sizeof(double) * npaths, c->stream));      // an empty path scores 0
    for (const Group& g : groups) {
        const int64_t U = (int64_t)g.urow.size();
        if (U == 0) continue;
        const int64_t Upad = (U + NB - 1) / NB * NB;
        T* Phi = Gam + (size_t)Upad * Upad;
        std::vector<int64_t> src((size_t)Upad, -1), lr((size_t)Upad, -1), uidx((size_t)Upad, 0);
        std::vector<T> lsc((size_t)Upad, (T)0);
        bool second = false;
        for (int64_t u = 0; u < U; ++u) {
            const int64_t pool = c->cand_idx[(size_t)g.urow[(size_t)u]];
            const int64_t lp = c->pos_in_train[(size_t)pool];
            src[(size_t)u] = g.urow[(size_t)u];
            uidx[(size_t)u] = pool;
            if (lp >= 0) {
                lr[(size_t)u] = lp;
                lsc[(size_t)u] = (T)c->train_var_host[(size_t)lp];
                second = true;
            }
        }
        ALGP_HIP(hipMemcpyAsync(d_src, src.data(), sizeof(int64_t) * Upad, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(d_lrow, lr.data(), sizeof(int64_t) * Upad, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(d_uidx, uidx.data(), sizeof(int64_t) * Upad, hipMemcpyHostToDevice, c->stream));
        ALGP_HIP(hipMemcpyAsync(c->auxVar.p, lsc.data(), sizeof(T) * Upad, hipMemcpyHostToDevice, c->stream));
        ALGP_TRY(gather_rows_launch<T>(c, p(c->Vt), c->ldv, d_src, R, Npad, Upad, Npad, second ? d_lrow : nullptr,
                                       second ? (const T*)c->auxVar.p : nullptr, p(c->L), c->Lld));
        ALGP_TRY(gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, Upad, Upad, Npad, (T)1, R, Npad, R, Npad, (T)0, nullptr, 0, Gam, Upad, 1));
        ALGP_TRY(pvr_assemble_launch<T>(c, d_uidx, U, Upad, s, Gam));
        for (int64_t n0 = 0; n0 < Mpad; n0 += chunk) {
            const int64_t nc = std::min(chunk, Mpad - n0);
            ALGP_TRY(gemm_nt_launch_pvr<T>(c, ALGP_PROF_GEMM_OTHER, Upad, nc, Npad, R, Npad, p(c->Vt), c->ldv, n0, s, d_uidx, U,
                                           (const int64_t*)c->Cidx.p, (const int*)c->ckind.p, M, c->has_tw ? (const T*)c->tw.p : nullptr,
                                           Es, chunk));
            ALGP_TRY(gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, Upad, Upad, nc, (T)1, Es, chunk, Es, chunk, n0 > 0 ? (T)1 : (T)0, Phi, Upad,
                                       Phi, Upad, 1));
        }
        // the paths by length: up to 64 sites in LDS, the longer ones batched at one ppad
        std::vector<int> small_pos, small_pid, big_pid;
        int bigk = 0;
        for (int pth = g.p0; pth < g.p1; ++pth) {
            if (used[pth] == 0) continue;
            if (used[pth] > 64) { big_pid.push_back(pth); bigk = std::max(bigk, used[pth]); continue; }
            small_pid.push_back(pth);
            for (int a = 0; a < 64; ++a) small_pos.push_back(a < maxlen ? g.upos[(size_t)(pth - g.p0) * maxlen + a] : -1);
        }
        if (!small_pid.empty()) {
            const int ns = (int)small_pid.size();
            ALGP_HIP(hipMemcpyAsync(d_upos, small_pos.data(), sizeof(int) * small_pos.size(), hipMemcpyHostToDevice, c->stream));
            ALGP_HIP(hipMemcpyAsync(d_pid, small_pid.data(), sizeof(int) * ns, hipMemcpyHostToDevice, c->stream));
            ALGP_TRY(pvr_small_launch<T>(c, d_upos, 64, d_pid, ns, Gam, Phi, Upad, sm, d_out));
        }
        if (!big_pid.empty()) {
            // the rows scratch becomes the blocks (stream order: every product that reads the rows is enqueued)
            const int ppad = bigk <= NB ? NB : 2 * NB;
            const size_t mat = (size_t)ppad * ppad;
            T* G = p(c->auxW);
            T* F = G + (size_t)bmax * mat;
            T* Li = F + (size_t)bmax * mat;
            T* Wm = Li + (size_t)bmax * mat;
            std::vector<int> big_pos;
            for (int p0 = 0; p0 < (int)big_pid.size(); p0 += bmax) {
                const int B = std::min(bmax, (int)big_pid.size() - p0);
                big_pos.clear();
                for (int b = 0; b < B; ++b)
                    for (int a = 0; a < ppad; ++a)
                        big_pos.push_back(a < maxlen ? g.upos[(size_t)(big_pid[p0 + b] - g.p0) * maxlen + a] : -1);
                ALGP_HIP(hipMemcpyAsync(d_upos, big_pos.data(), sizeof(int) * big_pos.size(), hipMemcpyHostToDevice, c->stream));
                ALGP_HIP(hipMemcpyAsync(d_pid, big_pid.data() + p0, sizeof(int) * B, hipMemcpyHostToDevice, c->stream));
                ALGP_HIP(hipMemsetAsync(d_ld, 0, sizeof(double) * B, c->stream));
                ALGP_HIP(hipMemsetAsync(d_info, 0, sizeof(int) * B, c->stream));
                ALGP_TRY(pvr_gather_launch<T>(c, d_upos, ppad, B, Gam, Phi, Upad, sm, G, F));
                ALGP_TRY(factor_blocks_batched<T>(c, G, ppad, inv, L21, d_ld, d_info, B));
                ALGP_TRY(pvr_linv_launch<T>(c, inv, L21, ppad, B, Li, tr));
                if (ppad > NB) {
                    // the lower left tile of L^-1: -inv(L22) L21 inv(L11), two products against the transposed operands
                    ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = NB, .n = NB, .k = NB, .A = {inv + NB * NB, NB, 2 * NB * NB},
                                            .B = {tr, NB, 2 * NB * NB}, .D = {X, NB, NB * NB}, .batch = B}));
                    ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = NB, .n = NB, .k = NB, .alpha = (T)-1, .A = {X, NB, NB * NB},
                                            .B = {tr + NB * NB, NB, 2 * NB * NB}, .D = {Li + (size_t)NB * ppad, ppad, (int64_t)mat}, .batch = B}));
                }
                // W = L^-1 Phi_SS (Phi_SS is symmetric: the NT product's second operand as it is)
                ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = ppad, .n = ppad, .k = ppad, .A = {Li, ppad, (int64_t)mat},
                                        .B = {F, ppad, (int64_t)mat}, .D = {Wm, ppad, (int64_t)mat}, .batch = B}));
                ALGP_TRY(pvr_trace_launch<T>(c, Wm, Li, ppad, B, d_info, d_pid, d_out));
                ALGP_TRY(sync(c));                              // the index vectors are reused by the next batch
            }
        } else {
            ALGP_TRY(sync(c));                                  // the index vectors are reused by the next group
        }
    }
    ALGP_HIP(hipMemcpyAsync(dV, d_out, sizeof(double) * npaths, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_score_paths_vr(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double mobile_std, int64_t max_union, double* dV_out) {
    CHECK_CTX(c);
    if (npaths < 0 || maxlen < 1 || (npaths > 0 && (!sites || !dV_out)) || !(mobile_std > 0))
        return fail(c, ALGP_ERR_BAD_ARG, "score_paths_vr: bad arguments");
    if (vr_over_ranks(c))
        return fail(c, ALGP_ERR_STATE, "score_paths_vr: this context scores the variance-reduction criterion over the ranks of its "
                                       "communicator, and a path's targets here would be this rank's own only; not sharded");
    if (npaths == 0) return ALGP_OK;
    FINISH(c, DISPATCH(c, score_paths_vr(c, sites, npaths, maxlen, mobile_std, max_union, dV_out)));
}

}  // extern "C"
