// api_genotype.hip -- algp_genotype_posterior: the posterior of the genotype effects u (Q of them, prior N(0, os_g G)) under the
// relationship form k = os_a kappa_a + os_g G[g, g'] (or the separable form with its genotype term), from the resident factor of S = K_AA + diag(var) + sigma_n^2 I.
// cov(u, y_A) = B with B[q][i] = os_g G[q, g_i] (g_i: the id of train row i), so with W = B L^-T and z = L^-1 (y - ybar):
//   B (Qpad x Npad)                a gather from the table (or from the identity)                  rel_gather_b_launch
//   W = B L^-T, in place           the blocked triangular solve through its plan                    trsm_blocked
//   mean = W z, ss_q = |W_q|^2     one pass over W                                                  rows_reduce_launch
//   var_q = os_g G_qq - ss_q                                                                        rel_var_finish_launch
//   cov = os_g G - W W^T           the lower tiles of the product on the matrix cores, then both     gemm_nt_launch,
//                                  triangles written from the one value                             rel_cov_finish_launch
// A genotype without a train row has a row of B like any other: it is predicted through its relatives (under the identity its
// row is zero: mean 0, variance os_g).  Nothing of the resident state is written; the scratch is one buffer of the context
// (algp_ctx::gen), counted by algp_device_bytes and freed by algp_destroy.
#include "api_impl.h"

using namespace algp;

namespace algp {

template <typename T>
int Impl<T>::genotype_posterior(algp_ctx* c, void* mean_out, void* var_out, void* cov_out) {
    if (!c->hyp.set || !c->hyp.has_ids())
        return fail(c, ALGP_ERR_STATE, "genotype_posterior: no kernel with a genotype term is in force (algp_set_hypers_relationship, "
                                       "algp_set_hypers_separable with Q >= 1)");
    if (c->pool_is_cov || c->n_pool <= 0) return fail(c, ALGP_ERR_STATE, "genotype_posterior needs a coordinate pool");
    if (!c->factored || c->train_dirty) return fail(c, ALGP_ERR_STATE, "genotype_posterior: call algp_factorize first");
    if (c->solved && !c->picks.empty())                 // (a new factorisation invalidates the candidate solve and its picks with it)
        return fail(c, ALGP_ERR_STATE, "genotype_posterior: " + std::to_string(c->picks.size()) +
                                           " pick(s) were committed since the factorisation, which the effects would not "
                                           "include: factorize again");
    const int64_t Q = c->hyp.Q, N = c->N, Npad = c->Npad, Qpad = round_up(Q, NB);
    const T* G = c->hyp.has_table ? (const T*)c->Gtab.p : nullptr;
    const T osg = (T)c->hyp.outputscale_g;

    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t o = total; total += (bytes + 255) / 256 * 256; return o; };
    const size_t o_B = take(N > 0 ? sizeof(T) * (size_t)Qpad * (size_t)Npad : 0);
    const size_t o_ss = take(sizeof(T) * (size_t)Qpad);
    const size_t o_mean = take(sizeof(T) * (size_t)Qpad);
    const size_t o_var = take(sizeof(T) * (size_t)Qpad);
    const size_t o_WW = take(cov_out && N > 0 ? sizeof(T) * (size_t)Qpad * (size_t)Qpad : 0);
    const size_t o_cov = take(cov_out ? sizeof(T) * (size_t)Q * (size_t)Q : 0);
    if (total > c->gen.cap) {
        size_t free_b = 0, total_b = 0;
        ALGP_HIP(hipMemGetInfo(&free_b, &total_b));
        if (total > c->gen.cap + free_b)
            return fail(c, ALGP_ERR_OOM, "genotype_posterior: the scratch of " + std::to_string(Q) + " genotypes takes " + std::to_string(total) +
                                             " bytes, " + std::to_string(c->gen.cap + free_b) + " available");
    }
    ALGP_TRY(ensure(c, c->gen, total));
    char* base = (char*)c->gen.p;
    T *B = (T*)(base + o_B), *ss = (T*)(base + o_ss), *meanD = (T*)(base + o_mean), *varD = (T*)(base + o_var);
    T *WW = (T*)(base + o_WW), *covD = (T*)(base + o_cov);

    if (N > 0) {
        ALGP_TRY(rel_gather_b_launch<T>(c, G, Q, osg, (const T*)c->Xs.p, c->hyp.DP, c->hyp.idc(), (const int64_t*)c->Aidx.p, N, Qpad, Npad, B));
        ALGP_TRY(trsm_blocked<T>(c, {.klass = ALGP_PROF_GEMM_TRSM, .X = B, .mpad = Qpad, .ldx = Npad, .L = p(c->L), .npad = Npad, .ldl = c->Lld,
                                     .invD = p(c->invD)}));
        ALGP_TRY(rows_reduce_launch<T>(c, B, Qpad, Npad, Npad, p(c->z), ss, meanD));
    } else {
        ALGP_HIP(hipMemsetAsync(meanD, 0, sizeof(T) * (size_t)Qpad, c->stream));
    }
    if (mean_out) ALGP_HIP(hipMemcpyAsync(mean_out, meanD, sizeof(T) * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    if (var_out) {
        ALGP_TRY(rel_var_finish_launch<T>(c, G, Q, osg, N > 0 ? ss : (const T*)nullptr, varD));
        ALGP_HIP(hipMemcpyAsync(var_out, varD, sizeof(T) * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    }
    if (cov_out) {
        if (N > 0)
            ALGP_TRY(gemm_nt_launch<T>(c, ALGP_PROF_GEMM_OTHER, Qpad, Qpad, Npad, (T)1, B, Npad, B, Npad, (T)0, (const T*)nullptr, Qpad, WW,
                                       Qpad, 1));
        ALGP_TRY(rel_cov_finish_launch<T>(c, G, Q, osg, N > 0 ? WW : (const T*)nullptr, Qpad, covD));
        ALGP_HIP(hipMemcpyAsync(cov_out, covD, sizeof(T) * (size_t)Q * (size_t)Q, hipMemcpyDeviceToHost, c->stream));
    }
    return sync_checked(c, "genotype_posterior");
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_genotype_posterior(algp_ctx* c, void* mean_out, void* var_out, void* cov_out) {
    CHECK_CTX(c);
    if (!mean_out) return fail(c, ALGP_ERR_BAD_ARG, "genotype_posterior: mean_out is NULL");
    FINISH(c, DISPATCH(c, genotype_posterior(c, mean_out, var_out, cov_out)));
}

}  // extern "C"
