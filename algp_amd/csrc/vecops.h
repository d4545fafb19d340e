// launchers defined in vecops.hip (the sums over groups of candidate rows at the end: group.hip).  A launcher whose kernel
// evaluates the pool covariance takes the source as a KmatSrc (make_src(c) at the call site) and hands its kernel the typed
// device view (cov_src -> CovSrc, common.h); every entry C(pa, pb) is pool_cov (common.h), whatever the kernel holds the two
// sites' coordinates in.
#pragma once
#include "common.h"
namespace algp {
template <typename T>
int cand_finalize_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* Cp, int64_t n_pool,
                         T prior_const, const T* extra, const T* ss, const T* dot, T ybar, T* dstat, T* mu,
                         unsigned char* alive);
template <typename T>
int score_launch(algp_ctx* c, int64_t M, const int* ckind, const unsigned char* alive, const T* dstat, double ss,
                 double delta, const double* extra, double* out);
// variance-reduction criterion (vecops.hip): the product's partial sums per column tile added in tile order; the utilities from
// w; and one pick's rank-1 fold w_c <- w_c - 2 r_c y_c + r_c^2 sum_T omega_j r_j^2 (col: the pick's column of V^T; r, rt, y1, y2:
// one entry per row; tp: VR_TBLOCKS x ldv; t: ldv; nrm: one entry; tw: the target weight of every pool site, or null); and the
// weighted sum of the target rows' variances, sum_{j in T} omega_j dstat_j, into *out (device)
constexpr int VR_TBLOCKS = 128;
template <typename T>
int vr_combine_launch(algp_ctx* c, const T* part, int64_t ld, int ntiles, int64_t rows, int accumulate, T* w);
template <typename T>
int vr_score_launch(algp_ctx* c, int64_t M, const int* ckind, const unsigned char* alive, const T* dstat, const T* w, double ss,
                    double delta, double* out);
template <typename T>
int vr_fold_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* Vt, int64_t ldv, int64_t col, const KmatSrc& s,
                   const T* tw, T* r, T* rt, T* nrm, T* tp, T* t, T* y1, T* y2, T* w);
// the same fold cut at its sums over the targets (local half; then the update from a list of N (pool index, rt) target pairs),
// and the pieces of the criterion over the ranks of a communicator: a round's packed rows, the disjointness marks, a fold's
// pairs, and its gathered sums and pair list (vecops.hip)
template <typename T>
int vr_fold_local_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* Vt, int64_t ldv, int64_t col, const T* tw,
                         T* r, T* rt, T* nrm, T* tp, T* t);
template <typename T>
int vr_fold_apply_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* Vt, int64_t ldv, int64_t col,
                         const KmatSrc& s, int64_t N, const int64_t* tidx, const T* tval, const T* r, const T* rt, const T* nrm,
                         const T* t, T* y1, T* y2, T* w);
template <typename T>
int vr_pack_rows_launch(algp_ctx* c, int64_t M, int64_t row0, int64_t B, const int* ckind, const int64_t* cidx, const T* Vt, int64_t ldv,
                        int64_t K, int64_t kvalid, int64_t* head, T* rows);
int vr_mark_launch(algp_ctx* c, int64_t M, const int64_t* cidx, int64_t n_pool, int* mark);
int vr_overlap_launch(algp_ctx* c, const char* gathered_heads, int64_t slice_bytes, int nranks, int self, int64_t B, int64_t n_pool,
                      int* mark);
template <typename T>
int vr_pairs_launch(algp_ctx* c, int64_t M, int64_t cap, const int* ckind, const int64_t* cidx, const T* rt, int64_t* idx, T* val);
template <typename T>
int vr_fold_gathered_launch(algp_ctx* c, const char* gathered, int64_t stride, int nranks, int64_t ncols, int64_t cap, int64_t off_nrm,
                            int64_t off_t, int64_t off_idx, int64_t off_val, T* t, T* nrm, int64_t* tidx, T* tval);
template <typename T>
int vr_target_sum_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const T* dstat, const T* tw, double* out);
int argmax_launch(algp_ctx* c, const double* s, int64_t M, double* out_val, int64_t* out_idx);
template <typename T>
int rows_reduce3_launch(algp_ctx* c, const T* Vt, int64_t rows, int64_t ldv, int64_t c0, int64_t c1, const T* u, const T* w,
                        T* out3, int64_t stride, int accumulate);
template <typename T>
int combine3_launch(algp_ctx* c, int64_t M, const T* acc, const T* tmp, int64_t stride, T ybar, T* ss, T* dot);
template <typename T>
int upper_gemv_launch(algp_ctx* c, const T* X, int64_t ld, int64_t n, const T* z, T* out);
template <typename T>
int zero_rows3_launch(algp_ctx* c, T* acc3, int64_t stride, const int64_t* rows, int64_t n);
template <typename T>
int zero_listed_rows_launch(algp_ctx* c, T* X, int64_t ldx, const int64_t* rows, int64_t n, int64_t ncols);
template <typename T>
int rowstat_combine_launch(algp_ctx* c, const T* stat, int64_t ld, int ntiles, int64_t rows, T* ss, T* dot);
template <typename T>
int uw_init_launch(algp_ctx* c, T* u, T* w, const T* y, int64_t k, int64_t n, int64_t npad);
template <typename T>
int uw_combine_launch(algp_ctx* c, T* z, const T* u, const T* w, T ybar, int64_t npad);
template <typename T>
int gather_rows_launch(algp_ctx* c, const T* src, int64_t lds, const int64_t* src_row, T* dst, int64_t ldd, int64_t nrows,
                       int64_t ncols, const int64_t* lrow = nullptr, const T* lscale = nullptr, const T* Lb = nullptr,
                       int64_t ldl = 0);
// lazy greedy refresh (vecops.hip): mode 0 = row pos, 1 = stale rows whose bound reaches scores[pos], 2 = all stale;
// pos_dev != null: the row index is read from the device (what an argmax kernel left there; < 0 = nothing to do)
template <typename T>
int lazy_refresh_launch(algp_ctx* c, int64_t M, int mode, int64_t pos, const LazyPick* picks, int npicks, const int* ckind,
                        const int64_t* cidx, const KmatSrc& s, const T* prevrows, int64_t ldv, T* Vt, T* dstat, int* fresh,
                        const unsigned char* alive, double* scores, double ss, double delta, const int64_t* pos_dev = nullptr);
// best_path block scoring: dH of every path from the resident rows of V^T (one workgroup per path, <= 64 sites each)
template <typename T>
int path_score_launch(algp_ctx* c, const int64_t* cpos, const int64_t* lpos, int npaths, int maxlen, const int64_t* cidx,
                      const T* Vt, int64_t ldv, int64_t ncols, const T* L, int64_t ldl, const T* varA, const KmatSrc& s, double sm,
                      double* out);
// paths of 65 .. 256 sites: G = C_PP + sigma_m^2 I - Gram in place for a batch of ppad x ppad blocks (sites packed to the front
// of each path's ppad entries of cpos, -1 behind them); out[p] = P CONST + 1/2 logdet[p] (NaN where info[p] != 0)
template <typename T>
int path_assemble_launch(algp_ctx* c, const int64_t* cpos, int batch, int ppad, const int64_t* cidx, const KmatSrc& s, double sm, T* G);
int path_finish_launch(algp_ctx* c, const int64_t* cpos, int ppad, int batch, const double* logdet, const int* info, double* out);
// variance reduction of whole paths (api_paths_vr.hip), over Gamma and Phi of a group's union sites (ld apart, lower tiles
// valid): Gamma = C(U, U) - Gram in place; the paths of at most 64 sites, one workgroup each (upos: stride union positions per
// path, packed to the front, -1 behind; pid: the slot of out each writes); for a batch of longer paths the gathered blocks
// G = Gamma_SS + sm I (identity on the padding) and F = Phi_SS (both triangles), the block's L^-1 (Li) from the tiled factor's
// inverse tiles and, at ppad = 256, tr = [L21^T | inv(L11)^T] per block for the products of its lower left tile; and
// out[pid[b]] = sum over the lower triangle of W_ij Li_ij (NaN where info[b] != 0)
template <typename T>
int pvr_assemble_launch(algp_ctx* c, const int64_t* uidx, int64_t U, int64_t ld, const KmatSrc& s, T* G);
template <typename T>
int pvr_small_launch(algp_ctx* c, const int* upos, int stride, const int* pid, int npaths, const T* Gam, const T* Phi, int64_t ld,
                     double sm, double* out);
template <typename T>
int pvr_gather_launch(algp_ctx* c, const int* upos, int ppad, int batch, const T* Gam, const T* Phi, int64_t ld, double sm, T* G, T* F);
template <typename T>
int pvr_linv_launch(algp_ctx* c, const T* inv, const T* L21, int ppad, int batch, T* Li, T* tr);
template <typename T>
int pvr_trace_launch(algp_ctx* c, const T* W, const T* Li, int ppad, int batch, const int* info, const int* pid, double* out);
// best_path under the MI criterion (paths_mi.hip): rows of a resident triangular inverse X = L^-T, zero left of each row's
// diagonal tile (-1: a zero row); ones on the diagonal behind each path's cnt[b] sites; the operands Lt = G^T, LtD = G^T diag(delta)
// of I + G^T diag(delta) G from the 2 x 2 tiled factor G of a batch of ppad x ppad blocks (L21 in its own NB x NB buffer per block)
template <typename T>
int mi_tri_gather_launch(algp_ctx* c, const T* X, int64_t ldx, const int64_t* src_row, T* dst, int64_t ldd, int64_t nrows,
                         int64_t ncols);
template <typename T>
int mi_pad_diag_launch(algp_ctx* c, T* G, int ppad, const int* cnt, int batch);
template <typename T>
int mi_transpose_launch(algp_ctx* c, const T* G, const T* L21, const T* delta, int ppad, T* Lt, T* LtD, int batch);
// greedy commit bookkeeping on the device: scale of the appended row, pick record, winner retired, (d_c, scale) out
template <typename T>
int commit_finalize_launch(algp_ctx* c, const T* dsrc, int in_train, double ss, double delta, LazyPick* lp_out,
                           int64_t pool_idx, int64_t ncols, unsigned char* alive_local, double* score_local, double* out2);
int fresh_at_launch(algp_ctx* c, const int* fresh, const int64_t* idx, double* out);
// MI criterion: fold one committed pick into a resident inverse (its diagonal, its rank-1 list, its entropy), and score
template <typename T>
int mi_rank1_launch(algp_ctx* c, int64_t m, const T* col0, T* U, int64_t ldu, double* sgn, int q, int64_t cpos, int mode,
                    double dlt, T* diag, double* H, double* H_A, const LazyPick* pick);
template <typename T>
int mi_score_launch(algp_ctx* c, int64_t M, const int* ckind, const int64_t* cidx, const unsigned char* alive, const T* dstat,
                    double ss, double delta, const int64_t* posbar, const T* dP, const T* dQ, const double* Hs, double* out);
// MI criterion dealt over ranks (mi_shard.hip): a rank's row blocks t g + member of X = L^-T (nloc of them, X zeroed here),
// its pieces of a pick's column with the earlier picks' terms removed, and a whole vector put together from gathered pieces
template <typename T>
int mi_trinv_rows(algp_ctx* c, const TrsmOp<T>& op, int64_t nloc, int g, int member);
template <typename T>
int mi_cols_local_launch(algp_ctx* c, int64_t rows, int g, int member, int64_t m, const T* raw, const T* U, int64_t ldu,
                         const double* sgn, int q, int64_t cpos, T* out);
template <typename T>
int mi_assemble_launch(algp_ctx* c, int64_t m, int g, int first, const char* gathered, int64_t stride, int64_t off, T* dst);
// mu[j] = ybar + sum_a C(qidx[j], aidx[a]) alpha[a] over N listed sites, sigma_n^2 of coinciding sites left out (the mean-only
// posterior; the variance-reduction fold's sum over its targets, for either pool kind)
template <typename T>
int kgemv_launch(algp_ctx* c, int64_t M, const int64_t* qidx, const KmatSrc& s, int64_t N, const int64_t* aidx, const T* alpha, T ybar,
                 T* mu);
// ---- sums over groups of candidate rows (group.hip; algp_group_posterior, api_group.hip) ----
// The labelled rows sorted by group on the host (a stable counting sort): slot m of the sorted list holds candidate row perm[m]
// of group gid[m] with coefficient coef[m]; group q owns the slots [off[q], off[q + 1]).  All on the device.
template <typename T>
struct GroupSegs {
    const int* perm;
    const int* gid;
    const T* coef;
    const int64_t* off;
    int64_t Lm;          // labelled rows
    int Q;
};
// members per chunk of the sorted list: a launch's workgroups each walk one chunk; the pieces of a group that spans chunks go to
// a buffer of two slots per chunk (part) and are added in chunk order.  span / nspan: the groups that span chunks of that size
constexpr int GROUP_CHUNK = 1024;      // group_ksum_launch
constexpr int GROUP_ROWCHUNK = 256;    // group_rowsum_launch
// U[q][j] = sum_{l in q} coef_l (k(x_j, x_l) + [j = l] extra_j) for j < M, 0 for M <= j < Mpad (leading dimension Mpad), K never
// stored; the rows of U of groups without members are not written; part: 2 ceil(Lm / GROUP_CHUNK) x Mpad
template <typename T>
int group_ksum_launch(algp_ctx* c, const KmatSrc& s, const int64_t* cidx, int64_t M, int64_t Mpad, const T* extra, const GroupSegs<T>& g,
                      const int* span, int nspan, T* U, T* part);
// dst[q][c] = sum_{l in q} coef_l V[perm_l][c] for c < ncols; part: 2 ceil(Lm / GROUP_ROWCHUNK) x ld_part.  16-byte loads where
// ncols and the leading dimensions allow, else a column per thread (the mean: V = mu, one column)
template <typename T>
int group_rowsum_launch(algp_ctx* c, const T* V, int64_t ldv, int64_t ncols, const GroupSegs<T>& g, const int* span, int nspan, T* dst,
                        int64_t ld_dst, T* part, int64_t ld_part);
// cov[p][q] = cov[q][p] = sum_{l in q} coef_l X[p][perm_l] (- sub[p][q], sub or null) for q <= p < Q; cov: Q x Q, packed
template <typename T>
int group_colsum_launch(algp_ctx* c, const T* X, int64_t ldx, const GroupSegs<T>& g, const T* sub, int64_t lds, T* cov);

template <typename T>
int pad_identity_launch(algp_ctx* c, T* A, int64_t n, int64_t npad, int64_t ld);
template <typename T>
int set_identity_launch(algp_ctx* c, T* A, int64_t npad, int64_t ld);
template <typename T>
int add_diag_launch(algp_ctx* c, T* A, int64_t n, int64_t ld, T v);
template <typename T>
int logdiag_launch(algp_ctx* c, const T* L, int64_t ld, int64_t n, double* out);
template <typename T>
int to_double_launch(algp_ctx* c, double* dst, const T* src, int64_t n);
// inverse of the NB x NB lower-triangular diagonal block at A (no factorisation)
template <typename T>
int trinv_diag_launch(algp_ctx* c, const T* A, int64_t lda, T* inv_out);
// the MLL gradient's sums (fit.hip), nos = 2 under the additive and the relationship form, else 1: out_dev[0, nos) += the
// outputscale sums, [nos] the noise trace, [nos + 1, nos + 1 + DP) the lengthscale sums
template <typename T>
int mll_grad_launch(algp_ctx* c, const T* Sinv, int64_t ld, int64_t N, const int64_t* aidx, const T* alpha, const KmatSrc& s,
                    double* out_dev, double* partial);
// the average-information matrix's two kernels (fit_ai.hip): U[a][i] = (dS/dtheta_a alpha)_i as a P x Npad panel in the gradient's
// parameter order (nl lengthscale rows, the outputscales, the noise; rows >= N zero), and out[a P + b] = out[b P + a] =
// 1/2 sum_{i < N} V[a][i] V[b][i] in double, both in fixed order
template <typename T>
int mll_ai_u_launch(algp_ctx* c, int64_t N, int64_t Npad, const int64_t* aidx, const T* alpha, const KmatSrc& s, int nl, T* U);
template <typename T>
int mll_ai_gram_launch(algp_ctx* c, const T* V, int64_t ld, int64_t N, int P, double* out);
// fixed effects (fixed.hip): the 16 x Npad panel of F^T's right-hand sides (column a of H at the train sites); the (p + 1)^2 Gram
// product of F^T's rows and z in double; the p x p work by one thread (out: the FX_* slots of common.h); the posterior pass over V^T
template <typename T>
int fixed_gather_launch(algp_ctx* c, const T* H, const int64_t* aidx, int64_t N, int64_t Npad, T* Pn);
template <typename T>
int fixed_gram_launch(algp_ctx* c, const T* Ft, int64_t ld, const T* z, int64_t N, int p, double* out);
int fixed_gls_launch(algp_ctx* c, const double* g, int p, double tol, double* out);
template <typename T>
int fixed_post_launch(algp_ctx* c, const T* Vt, int64_t ldv, int64_t M, int64_t ncols, const T* Ft, int64_t ldf, const T* H,
                      const int64_t* cidx, const double* gls, int p, const T* mu_in, const T* var_in, T* mu_out, T* var_out, T* proj_out);
// the restricted likelihood's gradient and average information (fixed.hip): the rows of (F C)^T; w = z - F beta (alpha_R =
// L^-T w); S^-1 -> P = S^-1 - G G^T on the entries j <= i < N mll_grad_launch reads (Gt = G^T, FX_P x ldg); out[r (P + p) + s] =
// V's row r . (V's row s | Ft's row s - P)
template <typename T>
int fixed_fc_launch(algp_ctx* c, const T* Ft, int64_t npad, const double* gls, T* FCt);
template <typename T>
int fixed_resid_launch(algp_ctx* c, const T* Ft, int64_t npad, int64_t N, const T* z, const double* gls, T* w);
template <typename T>
int fixed_downdate_launch(algp_ctx* c, T* Sinv, int64_t ld, int64_t N, const T* Gt, int64_t ldg, int p);
template <typename T>
int fixed_gram2_launch(algp_ctx* c, const T* V, const T* Ft, int64_t ld, int64_t N, int P, int p, double* out);
// the read-outs with the estimated effects (fixed.hip): out[i][j] += sign sum_{a < p} P[i][a] Qm[j][a] for i < rows, j < cols, sign = 1
// or -1 (out aligned to 16 bytes; one writer per entry, with P = Qm symmetric bit for bit); out[j] (+)= H[idx[j]] . beta for j < M
template <typename T>
int fixed_fold_launch(algp_ctx* c, T* out, int64_t ldo, int64_t rows, int64_t cols, const T* P, int64_t ldp, const T* Qm, int64_t ldq, int p,
                      int sign);
template <typename T>
int fixed_trend_launch(algp_ctx* c, const T* H, const int64_t* idx, int64_t M, const double* gls, int p, bool add, T* out);
// out[j][a] = H[idx[j]][a], j < M, a < FX_P
template <typename T>
int fixed_rows_launch(algp_ctx* c, const T* H, const int64_t* idx, int64_t M, T* out);
// the relationship form's gathers from its table (fit.hip): B[q][i] = os_g G[q, g_i] (Qpad x Npad, zero padded), the prior
// variance os_a + os_g G[g_j, g_j] of every pool site, and the two last steps of algp_genotype_posterior
template <typename T>
int rel_gather_b_launch(algp_ctx* c, const T* G, int64_t Q, T os_g, const T* Xs, int DP, int da, const int64_t* aidx, int64_t N,
                        int64_t Qpad, int64_t Npad, T* B);
template <typename T>
int rel_prior_launch(algp_ctx* c, const T* G, int64_t Q, T os_a, T os_g, const T* Xs, int DP, int da, int64_t n, T* prior);
template <typename T>
int rel_cov_finish_launch(algp_ctx* c, const T* G, int64_t Q, T os_g, const T* WW, int64_t ldw, T* cov);
template <typename T>
int rel_var_finish_launch(algp_ctx* c, const T* G, int64_t Q, T os_g, const T* ss, T* var);
}  // namespace algp
