// api_impl.h -- the typed host-side implementation behind the C ABI (include/algp_hip.h), declared once and defined by
// concern: api.hip (context, hyper-parameters, pool, train set, the stand-alone matrix entry points), api_factor.hip (the
// factor of the train set and its updates), api_candidates.hip (candidate solve and posterior), api_greedy.hip (scoring,
// picks, the sharded exchange), api_mi.hip (the MI criterion's state, on one GPU and over the ranks), api_vr.hip (the
// variance-reduction criterion), api_paths.hip (best_path block scoring), api_paths_vr.hip (the variance-reduction utility of
// whole paths), api_fit.hip (MLL gradient, one fit iteration, the average-information matrix), api_sample.hip (joint posterior draws),
// api_group.hip (the joint posterior of group aggregates), api_genotype.hip (the genotype effects under the relationship form),
// api_fixed.hip (fixed effects: the GLS estimates and the posterior with an estimated trend).
// Every file defines its members of Impl<T> and instantiates Impl<float> / Impl<double> for them.
#pragma once
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <stdlib.h>

#include "common.h"
#include "vecops.h"

namespace algp {

void release(algp_ctx* c, DevBuf& b);
void release(algp_ctx* c, MiState& mi);   // every MI buffer (api_mi.hip)
void release(algp_ctx* c, VrState& vr);   // every buffer of the variance-reduction criterion (api_vr.hip)
KmatSrc make_src(algp_ctx* c);
template <typename T>
int rel_check_ids(algp_ctx* c, const T* x, int64_t n, int D, int64_t Q, const char* what);
int sync(algp_ctx* c);
int sync_checked(algp_ctx* c, const char* what);
// the variance-reduction criterion is scored over the ranks of the communicator: a layout is attached (algp_comm_set_vr_exchange)
// and there is more than one rank (a world of one keeps the one-GPU state, as under the MI criterion)
inline bool vr_over_ranks(const algp_ctx* c) { return c->vr.xrows != 0 && c->comm_nranks > 1; }
// the fixed effects' rank failure, from the p x p work's flag (FX_INFO: the 1-based column): ALGP_ERR_NOT_PD with that pivot
inline int fixed_rank_error(algp_ctx* c, const char* who, double info) {
    c->pivot = (int64_t)info;
    return fail(c, ALGP_ERR_NOT_PD, std::string(who) + ": column " + std::to_string((int64_t)info) +
                                        " of the basis at the train sites is in the span of the columns before it (H_A' S^-1 H_A is singular)");
}

// how the candidate solve runs (Impl::SolvePlan): the new columns only (tail.hip), one task-list launch (chol_dag.hip),
// the sweep (trsm_blocked, potrf.hip), or folded into the factorisation's own launch (fit_and_solve)
enum class SolveRoute { Segments, TaskList, Sweep, Folded };

template <typename T>
struct Impl {
    static T* p(DevBuf& b) { return (T*)b.p; }
    static int rescale_pool(algp_ctx* c);
    static int kernel_matrix(algp_ctx* c, const void* x1, int64_t n1, const void* x2, int64_t n2, const void* diag_add,
                             int add_lik, void* out);
    static int set_pool(algp_ctx* c, const void* x, int64_t n);
    // the relationship form (api.hip): the resident pool's ids against Q; the table to the device; (api_candidates.hip) the prior
    // variance of the candidates as cand_finalize_launch takes it; (api_genotype.hip) the genotype effects' posterior
    static int rel_check_pool(algp_ctx* c, int D, int64_t Q, const char* what = "set_hypers_relationship: the resident pool");
    static int rel_upload_table(algp_ctx* c, const double* G, int64_t Q, DevBuf& dst);
    struct SitePrior { const T* tab; int64_t stride; T scalar; };
    static int site_prior(algp_ctx* c, SitePrior& pr);
    static int genotype_posterior(algp_ctx* c, void* mean_out, void* var_out, void* cov_out);
    static uint64_t train_sites_hash(const algp_ctx* c, const std::vector<int64_t>& idx);
    static int set_pool_cov(algp_ctx* c, const void* cov, int64_t n);
    static int set_train(algp_ctx* c, const int64_t* idx, int64_t N, const void* y, const void* var);

    // Rows that ride along with a factorisation as extra block rows of its task list (chol_dag.hip): P <- P L^-T comes out
    // of the same launch.  Only a from-scratch factorisation takes a panel, and only one that panel_fits (its caller checks).
    struct Panel {
        T* P;
        int64_t ldp, mpad;
        int mode;                  // 1: dense rows (the candidates' B^T), 2: the identity (-> L^-T)
        T* inv_out = nullptr;      // mode 2: S^-1 = P P^T (lower tiles, ld = mpad) is enqueued on the helper stream right behind
        bool inv_enqueued = false; // the launch, beside the substitutions and read-backs that follow on the main stream
        int64_t z_row = -1;        // this row of P holds y - ybar (mode 1: a padding row; mode 2: a dense tile row behind the identity):
                                   // z^T = (y - ybar)^T L^-T comes out of the launch too
        int64_t short_rows = 0;    // mode 1: the first short_rows rows (a multiple of 128) leave their last column tile to the caller
                                   // (SolvePlan::short_rows)
    };
    static bool panel_fits(int64_t npad, int64_t mpad);
    static int factor_resident(algp_ctx* c, T* A, int64_t n, int64_t npad, T* invD, int slot_logdet, int slot_info,
                               double* logdet, int64_t ld = 0, int64_t pivot_offset = 0, Panel* panel = nullptr);
    static int reserve_factor(algp_ctx* c, int64_t npad_need, int64_t keep_rows, int64_t keep_height = 0,
                              bool headroom = false);
    static bool vt_rows_for_new_sites(algp_ctx* c, int64_t Nb, int64_t p0, std::vector<int64_t>& src_row,
                                      std::vector<int64_t>& lrow, std::vector<T>& lscale, bool& any_second);
    static int exchange_new_rows(algp_ctx* c, int64_t Nb, int64_t p0, int* placed, int st_in = 0);
    static int factorize(algp_ctx* c, int incremental, Panel* panel = nullptr);
    static int finish_factor(algp_ctx* c, int64_t keep, int64_t p0, double ld_total, T* z_src = nullptr);
    static int factorize_from(algp_ctx* c, algp_ctx* src);
    static int need_alpha(algp_ctx* c);
    static int set_candidates(algp_ctx* c, const int64_t* idx, int64_t M, int prior_noise, const void* extra);

    // V^T = B^T L^-T for the candidate list, then pv / s / mu.  With `incremental`, the columns that
    // were solved against rows of the factor that are unchanged (same leading train rows, same
    // hyper-parameters, same candidate list) are kept and only the trailing column blocks are solved.
    // `alive` (M bytes, may be null) disables candidates (sites that became static-sampled).
    // plan_route decides the whole route once per call; then solve_prepare (buffers, candidate kinds' upload, B^T), the
    // solve itself (solve_run, or the factorisation's launch on the folded route: fit_and_solve), solve_finish (row
    // statistics, bookkeeping).
    struct SolvePlan {
        SolveRoute route = SolveRoute::Sweep;
        int64_t keep = 0;                    // leading columns of V^T that stay
        std::vector<int> kind;               // per candidate: its train row (a unit right-hand side) or -1
        std::vector<int64_t> became_unit;
        bool carried_sums = false;           // solve_finish will carry the rows' sums from step to step (u, w form of z)
        int nseg = 0;                        // Segments: only the new columns are solved (tail.hip), as 1-2 ranges [seg_c0, seg_c0 + seg_w)
        int64_t seg_c0[2] = {0, 0};
        int seg_w[2] = {0, 0};
        bool seg_window = false;             // the one range straddles two 128-column blocks of the factor
        int narrow_r = 0;                    // > 0: the last column tile holds only narrow_r columns: the route solves the first
        int64_t short_rows = 0;              // short_rows rows without that tile, the tail kernel its columns (solve_narrow_tile)
        bool row_stats = false;              // Sweep: ask its launches for the rows' sums per column tile
        bool rowstat_done = false;           // solve_run's launches left the rows' sums per column tile in c->rowstat
        bool rhs_fused = false;              // Sweep: B^T is not written to V^T; the scheduled sweep's update products generate it (gen)
        int64_t sweep_end = 0;               // Sweep: the columns [0, sweep_end) are the sweep's, the rest the narrow tile's and padding
        int split_tiles = 0;                 // Sweep, fit_and_solve: the last split_tiles tile rows (the one that carries z among them) ride
        int64_t sweep_rows = 0;              // the factorisation's launch as its panel; the sweep solves rows [0, sweep_rows) only
        RhsGen gen;
    };
    // The split is taken for up to this many leftover row panels of the sweep: the largest measured p that still pays.  Measured
    // on an MI355X at N = 10 000, fp64, from today's routes for the two halves (profiles/split_solve_parts.txt, medians of 5):
    // predicted gain per step +0.06 / +1.35 / +1.02 / -0.60 / -2.01 ms for p = 8 / 14 / 16 / 24 / 32 folded tile rows against
    // the 1.2 ms asked of it (three times the headline's run-to-run spread); the step itself, p = 14: -1.3 ms of 153.3.
    static constexpr int SPLIT_P_MAX = 14;
    // columns [c0, c0 + w) of the candidates' B^T by the kernel-matrix build, to out (leading dimension ldo): RhsGen::window
    static int rhs_window(algp_ctx* c, int64_t c0, int64_t w, void* out, int64_t ldo);
    static void plan_route(algp_ctx* c, int incremental, bool allow_fold, SolvePlan& pl);
    static int solve_prepare(algp_ctx* c, int incremental, SolvePlan& pl);
    static int solve_run(algp_ctx* c, SolvePlan& pl);
    static int solve_narrow_tile(algp_ctx* c, const SolvePlan& pl);
    static int solve_finish(algp_ctx* c, int incremental, const unsigned char* alive_host, const SolvePlan& pl);
    static int solve_candidates(algp_ctx* c, int incremental, const unsigned char* alive_host);
    static int fit_and_solve(algp_ctx* c);
    static int get_posterior(algp_ctx* c, void* mu, void* var);
    static int get_posterior_cov(algp_ctx* c, void* cov_out, double* mi_out);
    // parts: KmatSrc::parts -- 3: the posterior mean; 1, 2: one part's share of it under the additive kernel, without ybar
    static int posterior_mean(algp_ctx* c, const int64_t* idx, int64_t M, void* mu_out, int parts = 3);
    // joint draws of the latent field at the candidates by pathwise conditioning (api_sample.hip)
    // fixed: of ybar + h' beta + f with the attached fixed effects' uncertainty in the draws (algp_sample_posterior_fixed)
    static int sample_posterior(algp_ctx* c, int S, int F, const double* omega, const double* phase, const double* weights,
                                const double* prior, const double* eps, void* out, bool fixed = false);
    // the joint posterior of sums over groups of candidate rows (api_group.hip)
    // fixed: of the total signal ybar + h' beta + f with the attached fixed effects estimated (algp_group_posterior_fixed)
    static int group_posterior(algp_ctx* c, const int32_t* group, const double* weight, int64_t Q, void* mean_out, void* cov_out,
                               void* cross_out, bool fixed = false);
    static int build_set_matrix(algp_ctx* c, const int64_t* idx, int64_t m, const void* var, int64_t* mpad_out, T* dst = nullptr);
    static int set_entropy(algp_ctx* c, const int64_t* idx, int64_t m, const void* var, double* H);
    static int inverse_diag_resident(algp_ctx* c, int64_t m, int64_t mpad, void* diag_out);
    static int set_inverse_diag(algp_ctx* c, const int64_t* idx, int64_t m, const void* var, void* diag_out, double* H);
    static int upload_padded(algp_ctx* c, DevBuf& b, const void* A, int64_t rows, int64_t cols, int64_t rpad,
                             int64_t cpad);
    static int entropy_from_cov(algp_ctx* c, const void* cov, int64_t k, double* H, void* L_out, double* logdet);
    static int gemm_host(algp_ctx* c, int64_t m, int64_t n, int64_t k, double alpha, const void* A, const void* B,
                         double beta, const void* C, void* D);
    static int trsm_host(algp_ctx* c, const void* L, int64_t n, const void* B, int64_t m, void* X);
    // the MI criterion's state (api_mi.hip).  A build: mi_sets (host), the form's own factorisations, mi_install.
    struct MiPlan {
        std::vector<int64_t> A, Abar, all, posbar;   // sampled sites, the others, every site; pool index -> row in Abar (-1)
        std::vector<T> vA, vall;                     // the noise of A's sites, of every site (0 where unsampled)
        int64_t mb = 0, mbpad = 0, npad = 0;
        size_t rbytes = 0, cbytes = 0;               // form 1: bytes per rank of a pick's row gather and of a column gather
    };
    static int mi_sets(algp_ctx* c, double ss, double sm, MiPlan& pl);
    static int mi_vectors(algp_ctx* c, const MiPlan& pl, int64_t col);
    static int mi_install(algp_ctx* c, MiPlan& pl, const double* Hs, int form, double ss, double sm);
    static int mi_build(algp_ctx* c, double ss, double sm);
    static int mi_apply_pick(algp_ctx* c, int64_t q, double ss, double sm);
    // form 1, dealt over the ranks: collectives, every rank calls them with its status st
    static int mi_shard_plan(algp_ctx* c, double ss, double sm, MiPlan& pl);
    static int mi_shard_build(algp_ctx* c, MiPlan& pl, double* H3);
    static int mi_shard_fold(algp_ctx* c, int st);
    static int mi_shard_step(algp_ctx* c, double ss, double sm, int st, bool first_of_call);
    static int mi_scores_enqueue(algp_ctx* c, double ss, double sm, double delta, double* dst);
    // the variance-reduction criterion's column sums (api_vr.hip): the fused product, one pick's rank-1 fold, the utilities
    static int vr_product(algp_ctx* c);
    static int vr_fold(algp_ctx* c, int64_t q);
    static int vr_scores_enqueue(algp_ctx* c, double ss, double delta, double* dst);
    // over the ranks of a communicator (algp_comm_set_vr_exchange): collectives, every rank calls them with its status st
    static int vr_zero_picks_block(algp_ctx* c, int64_t q);
    static int vr_shard_build(algp_ctx* c, int64_t max_rows, int st = 0);
    static int vr_shard_fold(algp_ctx* c, int st);
    static int vr_shard_step(algp_ctx* c, int st, bool first_of_call);
    static int set_target_weights(algp_ctx* c, const double* w);
    static int target_variance(algp_ctx* c, double* sum);
    static int scores_enqueue(algp_ctx* c, int criterion, double static_std, double mobile_std, double* dst);
    static int scores(algp_ctx* c, int criterion, double static_std, double mobile_std, void* out, int out_is_device);
    static int argmax(algp_ctx* c, int64_t* local_pos, int64_t* pool_idx, double* value);

    // Row of V^T for a pool index that is not a local candidate (sharded scoring: the global winner lives on another
    // rank), entirely on the device: kernel-matrix row, forward substitution against the replicated factor, then the
    // entries appended by earlier picks through the SAME kernels a local row goes through (rows_reduce +
    // cand_finalize for the statistic, lazy_refresh for the picks), so the row and its statistic equal the owner's bit
    // for bit.  The statistic stays on the device (c->remote); nothing is read back here.
    struct RemoteSlots {            // one-row stand-ins for the per-candidate arrays, 64 bytes apart in c->remote
        int64_t* cidx;
        int* ckind;
        T *ss, *dot, *dstat, *mu;
        unsigned char* alive;
        int* fresh;
        double* score;
    };
    static RemoteSlots remote_slots(algp_ctx* c);
    static int remote_row(algp_ctx* c, int64_t pool_idx, int in_train);
    static int commit_enqueue(algp_ctx* c, int64_t pool_idx, double ss, double delta, const char* winner_payload = nullptr);
    static int commit_pick(algp_ctx* c, int64_t pool_idx, double static_std, double mobile_std);
    static int lazy_launch(algp_ctx* c, int mode, int64_t pos, double ss, double delta, const int64_t* pos_dev = nullptr);
    static int reset_lazy(algp_ctx* c);
    static int flush_lazy(algp_ctx* c);
    static int enqueue_local_best(algp_ctx* c, double ss, double delta);
    static int ensure_bounds(algp_ctx* c, int criterion, double static_std, double mobile_std, double ss, double delta);
    static int best_candidate(algp_ctx* c, int criterion, double static_std, double mobile_std, int64_t* local_pos,
                              int64_t* pool_idx, double* value);
    static int greedy_picks(algp_ctx* c, int criterion, double static_std, double mobile_std, int k, int64_t* picks_out, double* ut_out);
    static int greedy(algp_ctx* c, int criterion, double static_std, double mobile_std, int k, const int64_t* forced,
                      int64_t* picks_out, double* ut_out);
    static int score_paths_big(algp_ctx* c, const std::vector<int64_t>& cpos, const std::vector<int64_t>& lpos, int npaths, int maxlen,
                               int maxused, double mobile_std, double* dH);
    static int score_paths(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double mobile_std, double* dH);
    static int score_paths_mi(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double static_std, double mobile_std,
                              double* dMI, double* terms);
    static int score_paths_vr(algp_ctx* c, const int64_t* sites, int npaths, int maxlen, double mobile_std, int64_t max_union, double* dV);
    static int mll_grad(algp_ctx* c, double* grad_out, bool have_X = false, bool inv_enqueued = false);
    static int mll_ai(algp_ctx* c, double* ai_out);
    static int fit_step(algp_ctx* c, double* mll_out, double* grad_out, bool reml = false);   // reml: the restricted likelihood's (algp_reml_step)
    // fixed effects (api_fixed.hip): the basis to the device; F^T, its Gram product and the p x p work (enqueued, no sync);
    // the GLS estimates; the candidates' posterior with the estimated trend
    static int set_fixed_effects(algp_ctx* c, const double* H, int p);
    struct FixedPlan {
        T* Ft; double* gram; double* gls; T* mu; T* var; T* proj;
        T* aR;                       // fit: alpha_R (Npad)
        T* panel;                    // fit: a second 128 x Npad panel ((F C)^T, then the AI's U -> V)
        T* Gt;                       // fit, with the gradient: G^T (128 x Npad)
        double* gram2;               // fit: the AI's products
    };
    // what a call needs of the scratch beyond F^T, the Gram product and the p x p work
    // (resid: alpha_R alone of the fit's vectors)
    struct FixedWants { int64_t post_rows = 0; bool proj = false, fit = false, grad = false, resid = false; };
    static int fixed_enqueue(algp_ctx* c, const char* who, const FixedWants& w, FixedPlan& pl);
    static int fixed_alpha_r(algp_ctx* c, FixedPlan& pl);
    static int get_gls(algp_ctx* c, double* beta_out, double* cov_out, double* reml_out);
    static int get_posterior_fixed(algp_ctx* c, void* mu_out, void* var_out, void* proj_out);
    // the read-outs that carry the estimated effects: the genotype effects (mean B alpha_R, covariance os_g G - B P B^T); the
    // mean at pool sites without a candidate solve (component -1: all of it; 0, 1: a kernel part's share; 2: the trend's)
    static int genotype_posterior_fixed(algp_ctx* c, void* mean_out, void* var_out, void* cov_out);
    static int posterior_mean_fixed(algp_ctx* c, int component, const int64_t* idx, int64_t M, void* mu_out);
    // the restricted likelihood's gradient (have_X / inv_enqueued: mll_grad's), its value with it; its average information
    static int reml_grad(algp_ctx* c, double* grad_out, double* reml_out, bool have_X = false, bool inv_enqueued = false);
    static int reml_ai(algp_ctx* c, double* ai_out);
    static int get_alpha(algp_ctx* c, void* out);
    static int get_factor(algp_ctx* c, void* out);
    static int selftest(algp_ctx* c, int* mism);
};

// Factor a batch of ppad x ppad blocks (ppad = 128 or 256, lower tiles) as 2 x 2 tiles of 128, every step one launch for the
// whole batch: L11 and L22 in place, L21 = G21 inv(L11)^T into L21 (NB x NB per block), log det added to logdet[b], first bad
// pivot to info[b]
template <typename T>
int factor_blocks_batched(algp_ctx* c, T* G, int ppad, T* inv, T* L21, double* logdet, int* info, int B) {
    ALGP_TRY(potrf_diag_batched_launch<T>(c, G, (int64_t)ppad * ppad, ppad, inv, 2 * NB * NB, logdet, info, B));
    if (ppad > NB) {
        T* G21 = G + (int64_t)NB * ppad;
        T* G22 = G21 + NB;
        ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = NB, .n = NB, .k = NB, .A = {G21, ppad, (int64_t)ppad * ppad},
                                .B = {inv, NB, 2 * NB * NB}, .D = {L21, NB, NB * NB}, .batch = B}));
        ALGP_TRY(gemm_nt<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .m = NB, .n = NB, .k = NB, .alpha = (T)-1, .beta = (T)1, .A = {L21, NB, NB * NB},
                                .B = {L21, NB, NB * NB}, .D = {G22, ppad, (int64_t)ppad * ppad}, .batch = B}));
        ALGP_TRY(potrf_diag_batched_launch<T>(c, G22, (int64_t)ppad * ppad, ppad, inv + NB * NB, 2 * NB * NB, logdet, info, B));
    }
    return ALGP_OK;
}

}  // namespace algp

#define DISPATCH(c, call) ((c)->dtype == ALGP_F64 ? Impl<double>::call : Impl<float>::call)
#define CHECK_CTX(c) do { if (!(c)) return ALGP_ERR_BAD_ARG; (c)->err.clear(); hipSetDevice((c)->device); } while (0)
#define NEED_HYPERS(c) do { if (!(c)->hyp.set) return fail(c, ALGP_ERR_STATE, "call algp_set_hypers first"); } while (0)
#define FINISH(c, expr) do { int rc__ = (expr); if ((c)->prof_on) prof_collect(c); return rc__; } while (0)

