/*
 * algp_hip.h -- C ABI of libalgp_hip.so: the MI355X (gfx950) GP-inference hot path of sumitsk/algp.
 *
 * The reference has NO native/FFI layer (it is 8 Python files); its seam for this path is the
 * duck-typed Python surface
 *     GPR.cov_mat / GPR.set_train_data            (reference models.py:126-135, 161-181)
 *     predictive_distribution / entropy_from_cov  (reference utils.py:188-194, 293-319)
 *     Agent._post_update / greedy / best_path     (reference agent.py:89-90, 295-403)
 * plus NumPy inv / slogdet / dot / argmax.  This header is the boundary a maintainer would bind
 * (ctypes) to route those calls onto the GPU.  Each entry point cites the
 * reference code it replaces.
 *
 * Conventions
 *  - one opaque context per GPU; NOT thread-safe (one caller thread per ctx); every call is
 *    synchronous at the ABI (stream-ordered inside, stream synchronised before return);
 *  - all matrices row-major, contiguous; element type = the ctx dtype (ALGP_F32 / ALGP_F64),
 *    passed as void*; indices int64_t; utilities / entropies / log-dets are always double;
 *  - caller owns every host buffer; the library owns device memory inside the ctx;
 *  - return value: 0 = ALGP_OK, otherwise an ALGP_ERR_* code; algp_last_error() gives text.
 *    A non-positive pivot (reference: LinAlgError from inv, utils.py:300, or a silently wrong
 *    slogdet, utils.py:193) returns ALGP_ERR_NOT_PD and algp_last_pivot() the 1-based index.
 *  - the "pool" is the set of n field locations (reference env.X); train set and candidates are
 *    index lists into it, exactly like Agent's static_data/mobile_data bookkeeping.
 */
#ifndef ALGP_HIP_H
#define ALGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct algp_ctx algp_ctx;

enum { ALGP_F32 = 0, ALGP_F64 = 1 };
enum { ALGP_KERNEL_RBF = 0, ALGP_KERNEL_MATERN15 = 1, ALGP_KERNEL_MATERN05 = 2, ALGP_KERNEL_MATERN25 = 3 };  /* models.py:217-222 */
enum { ALGP_CRIT_ENTROPY = 0, ALGP_CRIT_MUTUAL_INFORMATION = 1, ALGP_CRIT_VARIANCE_REDUCTION = 2 };  /* agent.py:128; 2: below */
enum {
    ALGP_OK = 0,
    ALGP_ERR_BAD_ARG = 1,
    ALGP_ERR_HIP = 2,
    ALGP_ERR_NOT_PD = 3,
    ALGP_ERR_OOM = 4,
    ALGP_ERR_STATE = 5,
    ALGP_ERR_NO_DEVICE = 6
};

/* profiling classes for algp_prof_get (HIP-event timed, see DESIGN.md "measurement") */
enum {
    ALGP_PROF_KMAT = 0,        /* kernel-matrix build (HBM-bound)                  */
    ALGP_PROF_GEMM_CHOL = 1,   /* MFMA GEMM launches inside the Cholesky            */
    ALGP_PROF_GEMM_TRSM = 2,   /* MFMA GEMM launches inside the candidate TRSM      */
    ALGP_PROF_POTRF_DIAG = 3,  /* 128x128 diagonal-block factor + inverse           */
    ALGP_PROF_TRSV = 4,        /* vector triangular solves                           */
    ALGP_PROF_ROWS = 5,        /* row reductions over V^T (variance, mean, updates) */
    ALGP_PROF_SCORE = 6,       /* score + argmax                                    */
    ALGP_PROF_GEMM_OTHER = 7,
    ALGP_PROF_CHOLESKY = 8,    /* wall time of whole train-set factorisations (kernel build + factor + z)  */
    ALGP_PROF_TRSM = 9,        /* wall time of whole candidate solves (row chunks overlap on 3 streams) */
    ALGP_PROF_GEMM_CHOL_UPDATE = 10, /* the Cholesky's K=512 trailing (rank-512) updates, a subset of GEMM_CHOL's work
                                      * counted here instead: the "dense panel update" of the blocked factorisation */
    ALGP_PROF_CHOL_DAG = 11,   /* the Cholesky as one dependency-driven launch (chol_dag.hip): the whole factorisation */
    ALGP_PROF_DAG_PANEL = 12,  /* the same launch carrying a row panel: factorisation + candidate solve (or + L^-T), or the solve alone */
    ALGP_PROF_TAIL_COLS = 13,  /* tail_cols_kernel: the new columns of V^T after an append (HBM-bound: s * M * N_old bytes) */
    ALGP_PROF_COUNT = 14
};

/* ---- lifecycle ------------------------------------------------------------------------- */
int algp_version(void);
int algp_device_count(void);
int algp_create(int device_id, int dtype, algp_ctx** out);
void algp_destroy(algp_ctx* ctx);
const char* algp_last_error(const algp_ctx* ctx);
int64_t algp_last_pivot(const algp_ctx* ctx);
/* Diagonal jitter the last algp_get_posterior_cov had to add to cov_xx and cov before the two log-determinants of its
 * MI term existed (0: none).  utils.py:314 takes slogdet of the noise-free K_xx, which is singular to working precision
 * on dense grids; the reference returns rounding noise there (sign dropped, utils.py:193), this library a regularised
 * value plus the jitter it used.  Factorisations of the TRAIN matrix never use a jitter: they fail with ALGP_ERR_NOT_PD. */
double algp_last_jitter(const algp_ctx* ctx);
int algp_dtype(const algp_ctx* ctx);

/* ---- hyper-parameters: ExactGPModel's D+2 scalars (models.py:206-254; names run.py:35-37) ---
 * With os = exp(log_outputscale), r^2 = sum_d ((x_d-x'_d)/exp(log_lengthscale[d]))^2 and r = sqrt(r^2), k(x,x') is
 *   ALGP_KERNEL_RBF       os exp(-r^2 / 2)
 *   ALGP_KERNEL_MATERN05  os exp(-r)                                    (nu = 1/2, the exponential kernel)
 *   ALGP_KERNEL_MATERN15  os (1 + a) exp(-a),           a = sqrt(3) r   (nu = 3/2)
 *   ALGP_KERNEL_MATERN25  os (1 + a + a^2 / 3) exp(-a), a = sqrt(5) r   (nu = 5/2)
 * (gpytorch's ScaleKernel(RBFKernel | MaternKernel(nu), ard_num_dims = D)); any other id is ALGP_ERR_BAD_ARG.
 * sigma_n^2 = exp(log_noise) (models.py:180).                                                  */
int algp_set_hypers(algp_ctx* ctx, int kernel, int D, const double* log_lengthscale,
                    double log_outputscale, double log_noise);
/* The additive kernel over two coordinate groups (gpytorch's AdditiveKernel of two ScaleKernels, each on its active dims):
 *   k(x, x') = os_a kappa_a(r_a) + os_b kappa_b(r_b),
 * r_a over the first Da coordinates, r_b over the other D - Da, each with its own form (kernel_a, kernel_b: any of the four ids
 * above, kappa the form at outputscale 1), its own outputscale and the ARD lengthscales of its coordinates (log_lengthscale: D
 * entries in coordinate order) -- phenotype = genotype effect + spatial trend + noise.  The prior variance of a site is
 * os_a + os_b.  2 <= D <= 8 and 1 <= Da <= D - 1; anything else is ALGP_ERR_BAD_ARG and the context keeps the hyper-parameters
 * it had.  Replaces the hyper-parameters exactly as algp_set_hypers does (factor and candidate solve invalidated, the pool
 * rescaled, a pool of another width dropped); a later algp_set_hypers returns the context to a single kernel.  Every entry
 * point then works on the additive kernel; algp_get_mll_grad / algp_fit_step return D + 3 entries (below), and
 * algp_posterior_mean_component splits the posterior mean.                                       */
int algp_set_hypers_additive(algp_ctx* ctx, int D, int kernel_a, int Da, double log_outputscale_a, int kernel_b,
                             double log_outputscale_b, const double* log_lengthscale, double log_noise);
/* The relationship kernel: a spatial part plus a genotype part given by a TABLE (GBLUP with a spatial term),
 *   k((s, g), (s', g')) = os_a kappa_a(r(s, s')) + os_g G[g, g'].
 * Pool layout: coordinates [0, D-1) are spatial, each with its own ARD lengthscale (log_lengthscale: D-1 entries), kernel_a any of
 * the four ids above; coordinate D-1 is the genotype id, an integer in [0, Q).  The id is never scaled (its inverse lengthscale
 * is exactly 1), so the resident scaled pool holds it exactly: an fp32 context requires Q <= 2^24.  2 <= D <= 8, Q >= 1.
 * G: Q x Q row-major host doubles, symmetric positive semi-definite (genomic, pedigree based, ...), copied to the device in the
 * context's dtype; NULL: the identity (independent genotype effects) -- no table is stored and the part's value is os_g (g == g').
 * G must be finite and bitwise symmetric (G[p, q] and G[q, p] the same bits), else ALGP_ERR_BAD_ARG; it is NOT tested for
 * definiteness: a matrix S that is not positive definite is reported by the factorisation, as always.  Its diagonal need not be
 * constant: the prior variance of site j is os_a + os_g G[g_j, g_j], and every criterion, posterior and utility uses the
 * site's own.  (The jitter of algp_get_posterior_cov is scaled by the largest prior variance.)
 * Replaces the hyper-parameters exactly as algp_set_hypers_additive does (factor and candidate solve invalidated, the pool
 * rescaled, a pool of another width dropped); a later algp_set_hypers or algp_set_hypers_additive returns the context to those
 * forms and frees the table.  Those two keep refusing every kernel id outside 0..3: this form has no id, only this entry point.
 * Ids are validated on the host, before any launch, wherever coordinates meet these hyper-parameters: algp_set_pool,
 * algp_kernel_matrix (both operands) and this call itself when a coordinate pool of width D is resident.  An id that is no
 * integer, below 0 or >= Q: ALGP_ERR_BAD_ARG, the message names the row.  A refused call changes nothing: the context keeps the
 * pool and the hyper-parameters it had.
 * Under this kernel: algp_get_mll_grad / algp_fit_step return D + 2 entries, (log_lengthscale[0..D-1), log_outputscale_a,
 * log_outputscale_g, log_noise), with dS/dlog os_g = os_g G[g_i, g_j], from fixed-order sums (the same bits in every run);
 * algp_posterior_mean_component splits the mean (0: spatial, 1: genotype); algp_genotype_posterior gives the genotype effects;
 * algp_factorize_from takes two contexts' hyper-parameters as equal only if Q, os_g and the tables' contents (by a 64-bit
 * fingerprint of the caller's doubles) agree; algp_sample_posterior works in values mode (F == 0) and refuses features mode with
 * ALGP_ERR_BAD_ARG -- the genotype part has no spectral density.  The fused right-hand-side generation stays off.                */
int algp_set_hypers_relationship(algp_ctx* ctx, int D, int kernel_a, double log_outputscale_a, const double* log_lengthscale,
                                 double log_outputscale_g, const double* G, int64_t Q, double log_noise);
/* The separable kernel: a PRODUCT of two forms over disjoint coordinate groups, with or without the relationship kernel's genotype
 * term,
 *   k((x, g), (x', g')) = os kappa_a(r_a) kappa_b(r_b)  [ + os_g G[g, g'] ].
 * r_a over the first Da coordinates, r_b over the next Db >= 1, each factor any of the four ids above at outputscale 1 with the
 * ARD lengthscales of its coordinates; ONE outputscale os for the product.  kernel_a = kernel_b = ALGP_KERNEL_MATERN05 with
 * Da = Db = 1 is AR1(row) x AR1(col), rho_d = exp(-1 / ls_d) per unit of distance -- not Matern-1/2 over (row, col), and not the
 * additive form, which has no row x column interaction.
 * Q == 0: no genotype term.  G must be NULL, log_outputscale_g is ignored, all D coordinates are spatial (log_lengthscale: D
 * entries) and 1 <= Da <= D - 1.  Q >= 1: coordinate D - 1 is the genotype id, exactly as under algp_set_hypers_relationship (an
 * integer in [0, Q), never scaled, validated on the host at algp_set_pool, algp_kernel_matrix and in this call against a resident
 * pool of width D; G a Q x Q table or NULL for the identity; fp32: Q <= 2^24); log_lengthscale has D - 1 entries and
 * 1 <= Da <= D - 2.  The prior variance of site j is os (+ os_g G[g_j, g_j]).  2 <= D <= 8.
 * Every refusal (D, the split, a kernel id, Q < 0, a table with Q == 0, a table that is not finite or not bitwise symmetric, a bad
 * id in the resident pool, Q > 2^24 in fp32) is ALGP_ERR_BAD_ARG, and the context keeps the hyper-parameters, the table and the
 * pool it had.  Replaces the hyper-parameters as the sibling setters do; a later algp_set_hypers* call of another form returns
 * the context to that form and frees the table.
 * Under this kernel: the gradient and the average information have D + 2 parameters either way, in the order
 * (log_lengthscale[...], log_outputscale, [log_outputscale_g,] log_noise), with
 *   dk/dlog ls_d = os kappa_b dk_a u_d^2 for d in part a (dk_a: factor a's lengthscale factor at outputscale 1; symmetric for b),
 *   dk/dlog os = os kappa_a kappa_b,  dk/dlog os_g = os_g G[g_i, g_j];
 * algp_get_mll_grad, algp_fit_step, algp_get_mll_ai, algp_get_reml_grad, algp_get_reml_ai and algp_reml_step all work on it.
 * With the genotype term algp_posterior_mean_component splits the mean (0: spatial, 1: genotype) and algp_genotype_posterior
 * gives the genotype effects; without it both return ALGP_ERR_STATE (a product has no additive shares).
 * algp_sample_posterior works in values mode; features mode works for Q == 0 -- the product's spectral measure is the product of
 * the factors', so the caller draws omega_a from factor a's law and omega_b from factor b's and concatenates them -- and is
 * refused for Q >= 1 as under the relationship kernel.  The fused right-hand-side generation stays off.                        */
int algp_set_hypers_separable(algp_ctx* ctx, int D, int kernel_a, int Da, int kernel_b, double log_outputscale,
                              const double* log_lengthscale, double log_outputscale_g, const double* G, int64_t Q,
                              double log_noise);

/* ---- a1: GPR.cov_mat (models.py:161-181) -------------------------------------------------
 * out[n1*n2] (host) = K(x1,x2) ; x2 == NULL -> symmetric K(x1,x1) (models.py:169-170);
 * diag_add (len n1, may be NULL): += diag(white_noise_var) (models.py:175-176), symmetric only;
 * add_likelihood_var: += exp(log_noise) * I (models.py:179-180), symmetric only.              */
int algp_kernel_matrix(algp_ctx* ctx, const void* x1, int64_t n1, const void* x2, int64_t n2,
                       const void* diag_add, int add_likelihood_var, void* out);

/* ---- pool: env.X (agent.py:90) ------------------------------------------------------------
 * algp_set_pool: coordinates n x D (kernel evaluated on the fly on the device).
 * algp_set_pool_cov: an explicit n x n covariance that already contains sigma_n^2 on its
 *   diagonal -- literally Agent.cov_matrix (agent.py:90) -- for callers that hand one over.   */
int algp_set_pool(algp_ctx* ctx, const void* x, int64_t n);
int algp_set_pool_cov(algp_ctx* ctx, const void* cov, int64_t n);

/* ---- a2 + "GP-fit": GPR.set_train_data (models.py:126-135) + factorisation ----------------
 * idx[N] pool indices, y[N] targets (mean-centred inside: models.py:129-130), var[N] per-point
 * noise (may be NULL = 0).  algp_factorize builds S = C_AA + diag(var) (+ sigma_n^2 I unless the
 * pool is an explicit cov that already has it), factors S = L L^T (blocked, MFMA), solves
 * z = L^-1 (y-ybar), alpha = L^-T z, and accumulates log det S.  Replaces np.linalg.inv at
 * utils.py:300 and slogdet at utils.py:193.
 * A pool index may occur in more than one row: independent measurements of the same site, each
 * with its own var (cross entries are C(i,i), the site's first row stands for it as a candidate).
 * Keeping a site's static and mobile means as two rows gives the posterior of the reference's
 * fused row (agent.py:100-109) with log det S larger by exactly log(ss + sm) per such site, and
 * turns a re-measurement into an append for algp_factorize_update.  (Not with the MI criterion.)  */
int algp_set_train(algp_ctx* ctx, const int64_t* idx, int64_t N, const void* y, const void* var);
/* The GP's constant mean is the mean of the train targets (models.py:129-130).  enable != 0 replaces it by
 * `value` for the following algp_set_train calls -- needed when the rows are not one per site (a site kept
 * as two rows must not count twice in the reference's mean of the fused targets).                         */
int algp_set_constant_mean(algp_ctx* ctx, int enable, double value);
int algp_factorize(algp_ctx* ctx);
/* f1: like algp_factorize, but keeps the leading 128-row blocks of the resident
 * factor whose train rows (pool index, noise, order) and hyper-parameters are unchanged and rebuilds
 * only the rest; appending k sites to N costs O((128+k) N^2).  kept_rows (may be NULL) reports how
 * many rows were reused.  The reference refactorises from scratch at every step (agent.py:210).   */
int algp_factorize_update(algp_ctx* ctx, int64_t* kept_rows);
/* Take the factor of the SAME train set (indices, noise, order; same hyper-parameters, dtype and device) from
 * another context instead of computing it: an agent keeps one context per candidate set (the pool for
 * Agent.greedy, the held-out points for Agent.predict, agent.py:289-356) and both need chol(C_AA + D).  Rows this
 * context already holds for an unchanged leading part are kept (*kept_rows), the rest is a device-to-device copy;
 * z / MLL terms are computed for THIS context's targets.  Both pools must address the train sites by the same
 * indices.  ALGP_ERR_STATE when the source's factor belongs to another train set or other hyper-parameters.    */
int algp_factorize_from(algp_ctx* ctx, algp_ctx* src, int64_t* kept_rows);
/* algp_factorize + algp_solve_candidates back to back in one call (one ABI crossing per planning step; what bench.py's
 * step uses).  Needs algp_set_train and algp_set_candidates; same results as the two separate calls.  (Round 1 overlapped
 * the two on separate streams: slower, removed -- the factorisation is now a single dependency-driven launch.)          */
int algp_fit_and_solve(algp_ctx* ctx);
int algp_get_logdet(algp_ctx* ctx, double* logdet);          /* log det S                        */
int algp_get_entropy(algp_ctx* ctx, double* H);              /* N*CONST + 1/2 log det S (utils.py:188) */
int algp_get_alpha(algp_ctx* ctx, void* alpha_out);          /* N values                         */
int algp_get_factor(algp_ctx* ctx, void* L_out);             /* N x N lower, zeros above         */
int algp_get_mll(algp_ctx* ctx, double* mll);                /* -1/2 y0'alpha - 1/2 logdet - N/2 log 2pi */
/* ---- f2: gradient of the MLL for GPR.fit (models.py:137-159; the loss there is -MLL/N) ------
 * grad_out[D+2] = d MLL / d (log_lengthscale[0..D), log_outputscale, log_noise), NOT divided by N.
 * Needs a coordinate pool and a current factorisation.  With a site in more than one train row the
 * cross entries of its rows hold sigma_n^2 (algp_set_train) and count in the log_noise entry.
 * Under an additive kernel (algp_set_hypers_additive) grad_out has D+3 entries: (log_lengthscale[0..D), log_outputscale_a,
 * log_outputscale_b, log_noise); lengthscale entry d belongs to the part that owns coordinate d.  The same holds for
 * algp_fit_step.  Every sum is a fixed-order sum of per-workgroup partials: the same bits in every run.       */
int algp_get_mll_grad(algp_ctx* ctx, double* grad_out);
/* The average-information matrix of the MLL (Gilmour, Thompson & Cullis 1995; what AI-REML iterates on), in algp_get_mll_grad's
 * parameters and order under the kernel in force (P = D+2 | D+3 additive | D+2 relationship):
 *   ai_out[a * P + b] = 1/2 alpha' dS/dtheta_a S^-1 dS/dtheta_b alpha,   alpha = S^-1 (y - ybar),
 * P x P host doubles, row-major.  dS/dtheta per pair as for the gradient: the noise entry is sigma_n^2 E alpha with E_ij = 1
 * where rows i and j are the same pool site; the per-point var is no parameter; the relationship form's id coordinate has no
 * entry.  Positive semi-definite by construction, so (AI + lambda diag AI)^-1 grad is an ascent direction: the curvature of a
 * Newton fit and, inverted at a stationary point, the covariance of the estimates.  Costs one pass over the N^2 pairs, one
 * triangular solve of P right-hand sides and a P x P Gram product beside the factorisation's N^3.
 * Needs a coordinate pool (ALGP_ERR_BAD_ARG with an explicit covariance or ai_out == NULL) and a current factorisation
 * (ALGP_ERR_STATE).  Brings alpha up to date and writes nothing else of the resident state (factor, z, log det, a candidate
 * solve and its picks, the criteria's state).  Every sum has one order and both triangles come from one value: the same bits
 * in every call, ai_out[a * P + b] == ai_out[b * P + a].  ALGP_ERR_OOM (with the byte count) when its scratch does not fit.   */
int algp_get_mll_ai(algp_ctx* ctx, double* ai_out);
/* ---- fixed effects: the mean ybar + h(x)' beta, beta estimated by generalised least squares -------------------------------
 * H[n_pool * p], row-major host doubles: one row of basis values per pool site, 1 <= p <= 16 (block, replicate, trend terms);
 * kept on the device in the context's dtype, zero-padded to 16 columns.  H == NULL or p == 0 detaches.  The basis belongs to
 * its pool (of either kind): a new pool drops it, n_pool must match (ALGP_ERR_BAD_ARG, as a non-finite entry; no pool:
 * ALGP_ERR_STATE).  Nothing resident depends on it: the factor, a candidate solve and the criteria's state stay as they are,
 * and the entry points without `fixed`, `gls` or `reml` in their names ignore it: the read-outs algp_get_posterior,
 * algp_posterior_mean(_component), algp_genotype_posterior, algp_group_posterior and algp_sample_posterior keep the known-mean
 * values and bits and have the siblings below; the acquisition criteria and the path utilities keep the known-mean variances
 * and have none yet.
 * With H_A the rows of the train sites, S = L L', y0 = y - ybar, z = L^-1 y0:
 *   F = L^-1 H_A    A = F'F = H_A' S^-1 H_A    b = F'z    beta = A^-1 b    cov beta = A^-1 = C C'  (C = R^-1, A = R'R, R upper)
 *   l_R = -1/2 [ (N - p) log 2 pi + log|S| + log|A| + z'z - b' beta ]
 * the restricted log-likelihood in Harville's convention (no + 1/2 log|H_A' H_A|: up to that constant the likelihood of N - p
 * error contrasts).  With the constant in the span of H every quantity is invariant to ybar.
 * algp_get_gls: beta_out[p]; cov_out[p * p] and reml_out may be NULL.  Needs a current factorisation and a basis
 * (ALGP_ERR_STATE); N <= p: ALGP_ERR_BAD_ARG.  F' comes from one blocked triangular solve of a 128-row panel, A, b and z'z
 * from a Gram product summed in double in one order, the p x p work runs in double on A scaled to a unit diagonal.  A column of
 * H_A in the span of the columns before it (a scaled pivot <= 64 eps of the context's dtype): ALGP_ERR_NOT_PD,
 * algp_last_pivot = its 1-based number.
 * algp_get_posterior_fixed: the candidates of the resident solve (V' = B' L^-T) with the estimated trend,
 *   R_j = h_j - V_j F    mu_j = mu_j(algp_get_posterior) + R_j beta    var_j = var_j(algp_get_posterior) + |C' R_j|^2
 * mu_out[M], var_out[M], proj_out[M * p] (row j = R_j C: the covariance is algp_get_posterior_cov's + proj proj') in the
 * context's dtype, each may be NULL.  One pass over V' on the matrix cores.  Refused with ALGP_ERR_STATE, as
 * algp_get_posterior_cov refuses and for its reasons: a train site among the candidates under prior_includes_noise = 1 (a unit
 * row: R_j is not the residual basis), picks committed since the solve; also a solve that is not the current factor's.
 * Both write nothing resident, return the same bits in every call, synchronise once, and keep their scratch in one buffer of
 * the context (counted by algp_device_bytes, freed by algp_destroy; ALGP_ERR_OOM with the byte count up front).  After
 * ALGP_ERR_NOT_PD the outputs are unspecified.                                                                                  */
int algp_set_fixed_effects(algp_ctx* ctx, const double* H, int64_t n_pool, int p);
int algp_get_gls(algp_ctx* ctx, double* beta_out, double* cov_out, double* reml_out);
int algp_get_posterior_fixed(algp_ctx* ctx, void* mu_out, void* var_out, void* proj_out);
/* The other read-outs with the estimated effects.  alpha_R = P y0 = L^-T (z - F beta), P = S^-1 - S^-1 H_A A^-1 H_A' S^-1; for a
 * panel X of rows solved against the factor (V', or another) and their basis rows h: R = h - X F, R beta joins a mean,
 * |C' R|^2 a variance and (R C)(R' C)' a covariance -- the pass of algp_get_posterior_fixed over that panel, and a rank-p fold
 * out[i][j] += sum_a (R C)[i][a] (R' C)[j][a] streamed over the matrix with one writer per entry, ascending a, no atomics.
 * Each keeps its known-mean sibling's arguments, shapes, NULL rules, preconditions and refusals, adds algp_get_gls's (no basis:
 * ALGP_ERR_STATE; N <= p: ALGP_ERR_BAD_ARG; a dependent column: ALGP_ERR_NOT_PD with its pivot, outputs unspecified), writes
 * nothing resident, returns the same bits in every call, and keeps its scratch in the sibling's buffer and the fixed effects'.
 * algp_genotype_posterior_fixed: the genotype effects u (no trend share of their own: h = 0) from W = B L^-T, R_u = -W F:
 *   mean = W z + R_u beta = B alpha_R    var_q = os_g G_qq - |W_q|^2 + |C' R_u,q|^2    cov = os_g G - W W' + (R_u C)(R_u C)'
 * = os_g G - B P B', the prediction-error variances of the mixed-model equations; both triangles of cov carry identical bits.
 * One synchronisation.
 * algp_group_posterior_fixed: the functionals of the total signal ybar + h(x)' beta + f(x) over groups of candidate rows.  With
 * A_g the Q x M coefficients, T = A_g V' and R_g = A_g H_C - T F (H_C: the candidates' basis rows):
 *   mean = A_g mu + R_g beta    cov = A_g Sigma A_g' + (R_g C)(R_g C)'    cross = A_g Sigma + (R_g C) proj'   (proj: R_j C)
 * i.e. A_g applied to algp_get_posterior_fixed's mu and to algp_get_posterior_cov's matrix + proj proj'.  Without cross_out
 * neither the Q x M product nor the pass over V' is launched; mean_out alone forms T and no Q x M matrix.  Also refused
 * (ALGP_ERR_STATE) when the candidate solve is not the current factor's.  One synchronisation.
 * algp_posterior_mean_fixed: the mean at M pool sites without a candidate solve, the kernel-GEMV of algp_posterior_mean on
 * alpha_R.  component -1: ybar + h_j' beta + k_j' alpha_R; 0, 1: that kernel part's share k_c,j' alpha_R under the rules of
 * algp_posterior_mean_component; 2: the trend's share h_j' beta; another value: ALGP_ERR_BAD_ARG.  -1 = ybar + 0 + 1 + 2 to
 * rounding under a two-part kernel; with a genotype term component 1 at a site equals algp_genotype_posterior_fixed's mean of
 * its id to rounding.  Does not need alpha.  One synchronisation.
 * algp_sample_posterior_fixed: draws of ybar + h' beta + f at the candidates with beta's uncertainty in them, Matheron's rule on
 * the universal-kriging predictor from the same arguments as algp_sample_posterior (both prior modes, tiles of 128 samples,
 * the library draws nothing):
 *   z_s = L^-1 (y0 - g_s(A) - sqrt(v) o eps_s)    beta_s = C C' F' z_s    f_s(j) = ybar + g_s(j) + V_j . z_s + R_j beta_s
 * The mean over draws is algp_get_posterior_fixed's mu, their covariance algp_get_posterior_cov's + proj proj'.  One
 * synchronisation for the rank flag before the first tile (a dependent column returns there), then one per tile as the sibling.  */
int algp_genotype_posterior_fixed(algp_ctx* ctx, void* mean_out, void* var_out, void* cov_out);
int algp_group_posterior_fixed(algp_ctx* ctx, const int32_t* group, const double* weight, int64_t Q, void* mean_out, void* cov_out,
                               void* cross_out);
int algp_posterior_mean_fixed(algp_ctx* ctx, int component, const int64_t* idx, int64_t M, void* mu_out);
int algp_sample_posterior_fixed(algp_ctx* ctx, int S, int F, const double* omega, const double* phase, const double* weights,
                                const double* prior, const double* eps, void* out);
/* The restricted likelihood as a fit objective (REML: the variance components are not biased by the degrees of freedom the
 * fixed effects consume).  With P = S^-1 - G G', G = S^-1 H_A C = L^-T F C, and alpha_R = P y0 = L^-T (z - F beta):
 *   d l_R / d theta_a = 1/2 tr((alpha_R alpha_R' - P) dS/dtheta_a)
 *   AI_R,ab = 1/2 alpha_R' dS_a P dS_b alpha_R = 1/2 [ v_a . v_b - (F'v_a)' A^-1 (F'v_b) ],  v_a = L^-1 dS_a alpha_R
 * algp_get_reml_grad / algp_get_reml_ai: algp_get_mll_grad's / algp_get_mll_ai's parameters and order under every kernel form,
 * with repeated sites, and their refusals (a current factorisation: ALGP_ERR_STATE; a coordinate pool: ALGP_ERR_BAD_ARG),
 * besides those of algp_get_gls.  The gradient runs the MLL gradient's kernel unchanged on (P, alpha_R): S^-1 is turned into P
 * on the lower triangle by a rank-p downdate (p fused multiply-adds per entry in a fixed order, no atomics).  The AI runs
 * algp_get_mll_ai's pass with alpha_R and p more rows in its Gram product.  Both bring alpha up to date and write nothing else
 * resident; the same bits in every call; ai_out is symmetric bit for bit; one synchronisation each.
 * algp_reml_step: algp_fit_step for l_R -- the factorisation with L^-T and S^-1 out of its launch where algp_fit_step gets
 * them there, then the tail above; = algp_factorize + algp_get_gls + algp_get_reml_grad with the same values.  reml / grad_out
 * may each be NULL.                                                                                                              */
int algp_get_reml_grad(algp_ctx* ctx, double* grad_out);
int algp_get_reml_ai(algp_ctx* ctx, double* ai_out);
int algp_reml_step(algp_ctx* ctx, double* reml, double* grad_out);
/* The device work of ONE iteration of GPR.fit (models.py:145-158: output = model(train_x); loss = -mll(output, train_y);
 * loss.backward()) in one call, for the current hyper-parameters and train set: = algp_factorize + algp_get_mll +
 * algp_get_mll_grad with the same values, but L^-T comes out of the launch that factors S (the identity rides along as a
 * row panel of the task list) instead of from a separate launch sequence.  mll / grad_out[D+2] may each be NULL. */
int algp_fit_step(algp_ctx* ctx, double* mll, double* grad_out);

/* ---- candidates / test points: predictive_distribution (utils.py:293-319), greedy's pool ---
 * idx[M] pool indices.  A candidate that is itself in the train set (a mobile-sampled site,
 * agent.py:318 only skips static ones) is detected by index equality.
 * prior_includes_noise: 1 -> prior var = C_jj = outputscale + sigma_n^2 (greedy, agent.py:90),
 *                       0 -> prior var = K_jj (+ extra_var[j]) (cov_xx of utils.py:297).
 * algp_solve_candidates: V^T = B^T L^-T by blocked TRSM on MFMA, then row reductions
 *   pv_j = prior_j - |V_j|^2, mu_j = ybar + V_j . z.                                            */
int algp_set_candidates(algp_ctx* ctx, const int64_t* idx, int64_t M, int prior_includes_noise,
                        const void* extra_var);
int algp_solve_candidates(algp_ctx* ctx);
/* f1: like algp_solve_candidates, but keeps the columns of V^T that were solved against unchanged
 * leading rows of the factor (same candidate list, same hyper-parameters) and solves only the
 * rest: exactly the columns an append added when there are at most 64 of them (*kept_cols is then the
 * old train size; one pass over V^T, HBM-bound), else the trailing 128-column blocks.  alive[M] (may
 * be NULL) disables candidates that became static-sampled.                                         */
int algp_solve_candidates_update(algp_ctx* ctx, const uint8_t* alive, int64_t* kept_cols);
/* disable / enable candidates after a solve (alive[M] bytes; 0 = scored as -inf, agent.py:318)      */
int algp_set_candidate_alive(algp_ctx* ctx, const uint8_t* alive);
int algp_get_posterior(algp_ctx* ctx, void* mu_out, void* var_out);      /* either may be NULL  */
/* full M x M posterior covariance (utils.py:305) and mi = H(cov_xx) - H(cov) (utils.py:314);
 * cov_out / mi_out may be NULL.  cov_xx = K_xx + diag(extra_var) never carries sigma_n^2 (utils.py:297), also under
 * prior_includes_noise = 1: diag(cov) is then algp_get_posterior's variance minus sigma_n^2.  extra_var is per row: two
 * rows of one site share K(x, x) without it.  M = 0: nothing is written to cov_out, mi = 0.
 * The product cov_xx - V^T V is the covariance only for ordinary rows solved against the train set alone, so two
 * states are refused with ALGP_ERR_STATE instead of answered:
 *  - a candidate that is a train site under prior_includes_noise = 1 (a unit row of B^T; the message names it):
 *    set the candidates with prior_includes_noise = 0, where such a row is an ordinary point;
 *  - picks committed since the candidate solve (algp_commit_pick / algp_greedy), which algp_get_posterior's variances
 *    include and this product would not: solve the candidates again.
 * An explicit-covariance pool: ALGP_ERR_BAD_ARG.                                               */
int algp_get_posterior_cov(algp_ctx* ctx, void* cov_out, double* mi_out);
/* mean only, mu = ybar + K_xa alpha with K never materialised (utils.py:301)                   */
int algp_posterior_mean(algp_ctx* ctx, const int64_t* idx, int64_t M, void* mu_out);
/* One part's share of the posterior mean under an additive kernel (component 0 = a, 1 = b):
 *   mu_c(j) = sum_i os_c kappa_c(r_c(x_j, x_A_i)) alpha_i,
 * the same kernel-GEMV with the other part switched off.  The constant mean belongs to neither part: component 0 + component 1
 * + ybar is algp_posterior_mean to rounding.  (With a = genotype coordinates: the genotype effect adjusted for spatial trend.)
 * A single kernel in force: ALGP_ERR_STATE.  An explicit-covariance pool, a component other than 0 / 1: ALGP_ERR_BAD_ARG.
 * Component variances are not computed.                                                          */
int algp_posterior_mean_component(algp_ctx* ctx, int component, const int64_t* idx, int64_t M, void* mu_out);
/* (Under the relationship kernel, algp_set_hypers_relationship: component 0 = the spatial part, 1 = the genotype part, whose
 * value at a site equals algp_genotype_posterior's mean of the site's id to rounding.)
 * The posterior of the genotype effects u ~ N(0, os_g G) themselves under the relationship kernel -- BLUPs, their prediction-error
 * variances and their joint covariance -- for all Q genotypes, those without an observed plot included (predicted through their
 * relatives; under G = NULL such a genotype has mean exactly 0 and variance os_g).  With B = os_g G[:, g_A] (Q x N, gathered by
 * the train rows' ids), L the resident factor of S, W = B L^-T and z = L^-1 (y - ybar):
 *   mean_out[Q]    = W z                      (no constant mean: u has prior mean 0)
 *   var_out[Q]     = os_g G_qq - |W_q|^2      (or NULL)
 *   cov_out[Q * Q] = os_g G - W W^T           (or NULL; both triangles written, identical bits; var is its diagonal to rounding)
 * host arrays in the context's dtype.  Needs a current factorisation and a coordinate pool under this kernel, else ALGP_ERR_STATE;
 * picks committed since the factorisation: ALGP_ERR_STATE (the effects would not include them, as algp_get_posterior_cov).
 * mean_out NULL, more than 65 408 genotypes: ALGP_ERR_BAD_ARG.  The scratch (Q_pad x N_pad, and Q_pad x Q_pad + Q x Q for cov) belongs to the context, is
 * counted by algp_device_bytes and freed by algp_destroy; if it does not fit the call returns ALGP_ERR_OOM with the byte count
 * before allocating.  Reads resident state and writes none of it; the same bits on every call.                                  */
int algp_genotype_posterior(algp_ctx* ctx, void* mean_out, void* var_out, void* cov_out);

/* ---- joint posterior draws at the candidates: pathwise conditioning (no reference counterpart) ------------------------------
 * algp_sample_posterior: out[s * M + j] = draw s of the LATENT field f at candidate j (candidate order, the context's dtype; no
 * observation noise is added).  Matheron's rule on the resident candidate solve (V^T = B^T L^-T): a prior draw g becomes
 *   f_s(j) = ybar + g_s(j) + V_j . L^-1 (y - ybar - g_s(A) - sqrt(v) o eps_s),     v_i = var_i + sigma_n^2
 * (v_i: the train row's whole noise, S_ii - K_ii) by one triangular solve of the S right-hand sides and one product against
 * V^T: 2 (M + N) F S + 2 M N S + N^2 S flop; no M x M and no M x F matrix exists anywhere.  The library draws NO random
 * numbers: everything random is an argument (host doubles, converted to the context's dtype on the device), so the call is
 * deterministic.  eps: S x N standard-normal draws for the train noise.  The prior draw G (S x n_pool sites) comes from
 *   F > 0, features mode: G = sqrt(2 os / F) cos(Xs omega^T + phase) W^T -- random Fourier features of the kernel's spectral
 *     density: omega (F x D) frequencies for UNIT lengthscale (N(0, I) for RBF; z sqrt(2 nu / c), z ~ N(0, I), c ~ chi^2(2 nu)
 *     for Matern-nu), phase (F) ~ U[0, 2 pi), weights W (S x F) standard normal; Xs = x / lengthscale is the resident pool.
 *     prior must be NULL.  Needs a coordinate pool (an explicit covariance: ALGP_ERR_BAD_ARG).  The product runs on the matrix
 *     cores with its cosines generated in registers; phase and cosine are computed in the context's dtype.
 *     Under an additive kernel the amplitude is sqrt(2 (os_a + os_b) / F) and every row of omega is drawn for ONE part: from that
 *     part's spectral density in its own coordinates, ZERO in the other part's.  The caller picks the part of each feature with
 *     probability os_c / (os_a + os_b).  That is unbiased because the normalised spectral density of a sum of kernels is the
 *     mixture of the parts' normalised densities with exactly those weights: E[2 (os_a + os_b) cos(w.x + p) cos(w.x' + p)]
 *     = (os_a + os_b) sum_c os_c / (os_a + os_b) kappa_c = k(x, x').
 *   F == 0, values mode: G = prior (S x n_pool values of a prior draw at EVERY pool site, e.g. chol(K_pool) xi on a small
 *     pool); omega, phase, weights must be NULL.  Both pool kinds.
 * Any other combination of NULL / non-NULL, S < 1, F < 0, eps NULL with N > 0, out NULL with M > 0: ALGP_ERR_BAD_ARG.
 * Preconditions (ALGP_ERR_STATE), those of algp_get_posterior_cov for its reasons: a candidate solve is resident; no pick
 * committed since; no candidate solved as a unit row (a train site under prior_includes_noise = 1; the message names it: use
 * prior_includes_noise = 0, where such a row is an ordinary one and is sampled like any other) -- and the train set lists no
 * pool site in more than one row (such rows share a sigma_n^2 term that independent eps cannot describe; the MI criterion
 * refuses that state too).  algp_set_candidate_alive masks are ignored: every row gets a value.  M = 0: nothing written,
 * ALGP_OK.  N = 0: ybar + G, the prior draw.  (An explicit-covariance pool takes prior_includes_noise = 1 only, so there a
 * candidate that is a train site is always a unit row: leave train sites out of its candidate list.)
 * The call reads the resident state and writes none of it (V^T, z, the variances, the lazy-greedy bounds, the criteria's
 * state).  Samples go through in tiles of 128; S has no cap.  The scratch of one tile belongs to the context (counted by
 * algp_device_bytes, freed by algp_destroy); if it does not fit: ALGP_ERR_OOM with the byte count, before anything is allocated.
 * Profiling: the feature product and the product against V^T under ALGP_PROF_GEMM_OTHER, the solve under ALGP_PROF_GEMM_TRSM. */
int algp_sample_posterior(algp_ctx* ctx, int S, int F, const double* omega, const double* phase, const double* weights,
                          const double* prior, const double* eps, void* out);

/* ---- the joint posterior of group aggregates: genotype, row and plot means (no reference counterpart) -----------------------
 * algp_group_posterior: Q linear functionals g_q = sum_{j in q} a_j f(x_j) of the LATENT field f over groups of candidate rows
 * (no observation noise is added), from the resident candidate solve.  group[M]: one label per candidate row, in candidate
 * order: a label in [0, Q) puts the row into that group, -1 into none.  weight[M] (host doubles, finite, any sign) are the
 * coefficients as given, a_j = weight[j] (a labelled row may carry 0); weight == NULL: the plain group mean, a_j = 1 / n_q.
 * With A the Q x M matrix of coefficients, in the context's dtype, host memory, row-major, each may be NULL (which of them are
 * non-NULL decides what is computed):
 *   mean_out[Q]      = A mu, mu what algp_get_posterior reports
 *   cov_out[Q * Q]   = A Sigma A^T, Sigma = K_xx + diag(extra_var) - V^T V exactly the matrix algp_get_posterior_cov defines
 *                      (no sigma_n^2; extra_var per row; two rows of one site share K(x, x)); both triangles, identical bits
 *   cross_out[Q * M] = A Sigma: cross[q * M + j] = cov(g_q, f_j)
 * No M x M matrix exists anywhere: the kernel values are summed by group as they are formed (Q x M), the rows of V^T are summed
 * by group (Q x N), and cross = A K - (A V^T) V is one product; without cross_out that product is not launched
 * (cov = A K A^T - (A V^T)(A V^T)^T), and mean_out alone needs neither.  M N + M L kernel evaluations and flop for L labelled
 * rows, plus 2 Q M N for cross.
 * weight == NULL and a group without members: ALGP_ERR_BAD_ARG (the message names the group); with explicit weights an empty
 * group is the zero functional: mean 0, its row and column of cov 0.  Q < 1, group NULL with M > 0, a label outside [-1, Q)
 * (the message names the row), a non-finite weight: ALGP_ERR_BAD_ARG, before anything is launched.
 * Preconditions, those of algp_get_posterior_cov for its reasons: a candidate solve is resident, no pick committed since, no
 * candidate solved as a unit row (the message names it) -- ALGP_ERR_STATE; a coordinate pool (an explicit covariance:
 * ALGP_ERR_BAD_ARG).  algp_set_candidate_alive masks are ignored.  The call reads the resident state and writes none of it (V^T,
 * z, the variances, the lazy-greedy bounds, the criteria's state).  Every sum has one fixed order (no floating-point atomics):
 * the results carry the same bits in every run.  The scratch belongs to the context (counted by algp_device_bytes, freed by
 * algp_destroy); if it does not fit: ALGP_ERR_OOM with the byte count, before anything is allocated.
 * Profiling: the kernel sums under ALGP_PROF_KMAT, the grouped sums under ALGP_PROF_ROWS, the products under ALGP_PROF_GEMM_OTHER. */
int algp_group_posterior(algp_ctx* ctx, const int32_t* group, const double* weight, int64_t Q, void* mean_out, void* cov_out,
                         void* cross_out);

/* ---- a7: Agent.greedy (agent.py:295-356) ---------------------------------------------------
 * algp_scores: utilities of every candidate under the current state
 *   entropy: CONST + 1/2 log(pv_j + ss) (unsampled) | 1/2 log(1 + delta s_jj) (mobile-sampled)
 *   (identical to the reference's ent_a - cond, agent.py:341).
 *   out: M doubles; out_is_device != 0 -> `out` is a device pointer (multi-GPU all-gather
 *   buffers owned by the caller).  Committed candidates get -inf (agent.py:314, 318).
 * algp_argmax: first maximum (np.argmax, agent.py:349) over the local scores.
 * algp_best_candidate: the local first maximum of the utilities without scoring every row again.
 *   Entropy gains never grow when more sites are sampled (submodularity), so a utility computed
 *   before the last picks is an upper bound; only the rows whose bound can still win are brought
 *   up to date.  Same winner and value as algp_scores + algp_argmax, bit for bit.  (MI: full scoring.)
 * algp_commit_pick: make pool index `pool_idx` static-sampled (agent.py:352-354): the rank-1 row
 *   append to V^T and to every candidate's pv / s.  The pick is recorded and the rows catch up on
 *   demand (all of them before algp_scores / algp_get_posterior read them).  The index need not be
 *   a local candidate (sharded scoring: every rank commits the global winner).  A candidate switched off with
 *   algp_set_candidate_alive is accepted too: the mask takes a row out of the scoring and out of the library's own picks,
 *   not out of the sites a caller may name; the row stays at -inf.  A site already committed since the candidate solve:
 *   ALGP_ERR_BAD_ARG.  At most 128 picks fit behind one candidate solve (the appended columns of V^T): the 129th
 *   algp_commit_pick is refused with ALGP_ERR_STATE and algp_greedy with k > 128 with ALGP_ERR_BAD_ARG before anything is
 *   committed; either leaves the state, and what algp_scores returns, untouched.  Solve the candidates again to go on.
 *   The capacity is checked before the repeat: once 128 picks are committed, naming one of them again is ALGP_ERR_STATE
 *   too.  algp_greedy checks k alone, not k plus the picks already committed: a call that would pass 128 in total commits
 *   the picks that fit and returns ALGP_ERR_STATE at the first that does not.
 * algp_greedy: k picks on one GPU.  utilities_out (k*M doubles, local candidate order) may be
 *   NULL; forced_picks (k pool indices) may be NULL.  With both NULL and the entropy criterion a pick
 *   is one host round trip (see algp_greedy_sharded: the same chain without the gather).
 * MI criterion (agent.py:330-339) is exact; here it holds the pool-wide inverses on one GPU (algp_comm_set_mi_groups deals
 * them over the ranks of algp_greedy_sharded).
 * Variance-reduction criterion (ALGP_CRIT_VARIANCE_REDUCTION; Cohn's ALC / integrated-variance reduction): the utility of a
 * candidate is how much its static reading lowers the summed predictive variance of the targets.  With ss = static_std^2,
 * sm = mobile_std^2, delta = 1/(1/ss + 1/sm) - sm (the entropy score's delta), the rows of V^T ordinary (a site without a
 * train row) or unit (a mobile-sampled site), G = V V^T over all current columns of V^T (the committed picks' included),
 * and the targets T = the ordinary rows of the candidate set, fixed by the solve (a target stays one after it is picked or
 * switched off with algp_set_candidate_alive):
 *   signed cross term, j in T:   E_jc = [c ordinary] C(j, c) - G_jc     (ordinary c: the posterior covariance of j and c;
 *                                unit c at train row u: -C_jA S^-1 e_u; C: the pool covariance, sigma_n^2 where the pool
 *                                indices coincide)
 *   ordinary c:  u_c = sum_{j in T} E_jc^2 / (pv_c + ss)         unit c:  u_c = -delta sum_{j in T} E_jc^2 / (1 + delta s_cc)
 * with pv_c / s_cc the statistic the entropy criterion reads.  That is sum_{j in T} var(j | A) - sum_{j in T} var(j | A with
 * c static-sampled), train noise fused as 1/(1/static_var + 1/mobile_var) (agent.py:302-308, 321-328).  Committed,
 * static-sampled and switched-off rows get -inf, as for the entropy criterion.  The first scoring after a candidate solve is
 * one fused M x M x (N + picks) product on the matrix cores (2 M^2 K flop; no M x M matrix is written); each pick committed
 * after it is folded in with E' = E - r_T r_c^T (r: the pick's column of V^T): one fused kernel-GEMV and two passes over
 * V^T.  algp_scores, algp_best_candidate (full scoring, as MI) and algp_greedy accept it; algp_greedy_sharded accepts it with a
 * layout of algp_comm_set_vr_exchange (below) and refuses it without one (ALGP_ERR_BAD_ARG); candidates set with an extra
 * variance, or a candidate set that lists a pool site twice, are refused with ALGP_ERR_STATE.
 * On a context with that layout attached and more than one rank the targets are the ordinary rows of EVERY rank's shard, and
 * under this criterion algp_scores is a COLLECTIVE: every rank calls it, in the same sequence; it brings the state over the
 * ranks up to the committed picks (a build, or one fold per pick) and returns the utilities of this rank's own rows against
 * the targets of all ranks.  With algp_commit_pick on every rank that is how forced picks are driven.  algp_greedy and
 * algp_best_candidate under this criterion, and algp_score_paths_vr, return ALGP_ERR_STATE there (they would count this rank's
 * targets only).
 * Target weights (algp_set_target_weights below): with a weight omega_q >= 0 per pool site attached, target j counts omega_j
 * times -- sum_{j in T} omega_j E_jc^2 in both utilities, i.e. sum_j omega_j var(j | A) - sum_j omega_j var(j | A with c
 * static-sampled): a region of interest, plots that matter more, the sites a later prediction is read at.  The targets stay
 * the ordinary rows of the candidate set; every candidate may still be picked.  The fold of a pick reads
 * w'_c = w_c - 2 r_c y_c + r_c^2 sum_T omega_j r_j^2 with y = E^T (omega r)_T.  The entropy and MI criteria ignore weights. */
int algp_scores(algp_ctx* ctx, int criterion, double static_std, double mobile_std, void* out,
                int out_is_device);
int algp_argmax(algp_ctx* ctx, int64_t* local_pos, int64_t* pool_idx, double* value);
int algp_best_candidate(algp_ctx* ctx, int criterion, double static_std, double mobile_std,
                        int64_t* local_pos, int64_t* pool_idx, double* value);
int algp_commit_pick(algp_ctx* ctx, int64_t pool_idx, double static_std, double mobile_std);
int algp_greedy(algp_ctx* ctx, int criterion, double static_std, double mobile_std, int k,
                const int64_t* forced_picks, int64_t* picks_out, double* utilities_out);
/* algp_set_target_weights: the variance-reduction criterion's weight of every pool site as a target (w: n_pool doubles, each
 * finite and >= 0; n_pool must be the current pool's size: otherwise ALGP_ERR_BAD_ARG with the offending index in the
 * message, nothing changed; without a pool ALGP_ERR_STATE).  w = NULL detaches the weights: every target counts once again,
 * with the bits of a context that never had any.  The weights are held on the device in the context's dtype and belong to
 * their pool: algp_set_pool and algp_set_pool_cov drop them, as they drop an owner map.  Setting, changing or detaching them
 * drops the criterion's resident sums -- the next scoring is the full product, committed picks included -- but not the
 * candidate solve.  A weight on a site that is not a target (a unit row, a site outside the candidate set) is accepted and
 * ignored; all weights zero is legal (every utility 0, -inf where it is today).  algp_scores / algp_greedy under
 * ALGP_CRIT_VARIANCE_REDUCTION and algp_score_paths_vr (Phi = E Omega E^T) read them; nothing else does.
 * algp_get_target_variance: the criterion's objective under the current state, committed picks included:
 *   *sum = sum_{j in T} omega_j pv_j, pv_j the variance algp_get_posterior reports for target row j (omega = 1 without weights).
 * A pick's utility is this sum before its commit minus the sum after.  Needs a candidate solve (ALGP_ERR_STATE), brings the rows
 * up to date as algp_get_posterior does, applies the criterion's two refusals (ALGP_ERR_STATE), and is one device reduction in
 * a fixed order, accumulated in double: the same bits in every run.  It stays LOCAL on a context that scores the criterion over
 * ranks (algp_comm_set_vr_exchange) and is no collective: *sum = this rank's share, over the targets of its own shard; the
 * objective is the sum over the ranks.  The weights are per pool site, so every rank attaches all of them; a hash of what was
 * attached travels in the criterion's agreement word, and ranks holding different weights all get ALGP_ERR_BAD_ARG. */
int algp_set_target_weights(algp_ctx* ctx, const double* w, int64_t n_pool);
int algp_get_target_variance(algp_ctx* ctx, double* sum);

/* ---- a8 / f3: Agent.best_path (agent.py:358-403), entropy criterion, all paths at once -----------------------------
 * algp_score_paths: dH_out[p] = H(A u path_p) - H(A) for npaths enumerated paths, where path p adds a mobile reading
 * (noise mobile_std^2) at each of its distinct sites sites[p*maxlen + a] (pool indices, -1 = no site): the reference
 * takes one slogdet of the enlarged covariance per path (agent.py:386-399); here every path is the log-determinant of
 * its posterior block of at most 256 x 256 (config 5's paths run along field rows of up to ~250 sites, env.py:197-310),
 * computed from the rows of V^T that algp_solve_candidates left resident (all sites of all paths must be resident
 * candidates, no pick committed since the solve): up to 64 distinct sites per path in one LDS kernel, one workgroup per
 * path; 65 .. 256 with the paths' rows gathered, the Gram matrices as one batched MFMA product and the blocks factored as
 * 2 x 2 tiles of 128 (batches of paths sized to ~4 GB of scratch).  More than 256 distinct sites: ALGP_ERR_BAD_ARG.  A site that already is a train row
 * (a statically sampled site crossed by the path) receives a second row, which is the same GP as the reference's fused
 * noise (agent.py:100-109) up to the constant log(sigma_s^2 + sigma_m^2)/2 + CONST per such site (the caller's to
 * subtract, see algp_amd/agent.py); the caller leaves out sites that already have a mobile row (no new reading).  The MI
 * criterion's path utility is algp_score_paths_mi below. */
int algp_score_paths(algp_ctx* ctx, const int64_t* sites, int npaths, int maxlen, double mobile_std, double* dH_out);
/* algp_score_paths_mi: Agent.best_path under the mutual-information criterion (agent.py:374-400: ent_a + ent_abar - ent_all
 * per path, the last two pool-sized).  The train set is the fused base A0 (one row per site, its noise v_a); sites[] as for
 * algp_score_paths, holding the sites path p CHANGES: a site outside A0 joins it with noise mobile_std^2 and leaves the
 * complement; a train site is re-measured, its noise v_a -> v_a sm / (v_a + sm) (sm = mobile_std^2).  The caller leaves out
 * sites whose reading changes nothing (already mobile-sampled); -1 entries are skipped, a site listed twice counts once.
 * dMI_out[p] = dH_A + dH_Abar - dH_all, the path's utility minus the base's; terms_out (npaths x 3: the three terms, may be
 * NULL).  dH_A = the fused-form entropy gain (algp_score_paths' rows form minus CONST + log(v_a + sm)/2 per re-measured site);
 * dH_Abar = 1/2 log det P[S_new, S_new] - |S_new| CONST with P = C_AbarAbar^-1 (Jacobi's identity); dH_all = 1/2 log det
 * (I + G^T D G), Q[S, S] = G G^T, Q = (C + D0)^-1, D = diag of the noise changes (matrix determinant lemma).  P and Q are
 * the two pool-wide inverses the MI greedy keeps resident: built once per candidate solve (ALGP_ERR_OOM with the byte count,
 * before any allocation, when they do not fit), reused by every later call on the same state.  Per batch of paths their
 * rows are gathered, the blocks are batched MFMA Gram products, factored as 2 x 2 tiles of 128.  Preconditions as for
 * algp_score_paths (a candidate solve with prior_includes_noise, every site a resident candidate, no pick committed since):
 * ALGP_ERR_STATE; a train set that lists a site twice: ALGP_ERR_STATE; more than 256 changing sites: ALGP_ERR_BAD_ARG. */
int algp_score_paths_mi(algp_ctx* ctx, const int64_t* sites, int npaths, int maxlen, double static_std, double mobile_std,
                        double* dMI_out, double* terms_out);
/* algp_score_paths_vr: the variance-reduction (ALC) utility of whole paths, the criterion's sentence applied to a set: with the
 * targets T = the ordinary rows of the candidate set (fixed by the solve; a row switched off with algp_set_candidate_alive
 * stays a target) and path p read once at each of its distinct sites with variance sm = mobile_std^2 -- a new site joins the
 * train set with noise sm, a site that has a train row of noise v ends with v sm / (v + sm), i.e. receives a second row --
 *   dV_out[p] = sum_{j in T} var(j | A) - sum_{j in T} var(j | A u path_p) = tr((Gamma_SS + sm I)^-1 Phi_SS),
 * S the path's sites, Gamma = C - R R^T their posterior covariance (R_s: the site's row of V^T, second-row form for a train
 * site; C: the pool covariance, sigma_n^2 where the pool indices coincide), E_sj = C(s, j) - R_s . V_j their cross covariance
 * with the targets, Phi = E E^T (E Omega E^T and sum_j omega_j var(j | .) with target weights attached, algp_set_target_weights).  Gamma and Phi are built once over the union U of a group of consecutive paths (max_union:
 * the most union sites per group, at least 256; <= 0: the library's default, the largest union whose rows of V^T and whose two
 * U x U matrices each stay within ~4 GB -- 15 744 sites in fp64, 22 272 in fp32, fewer beyond N of about 31 000 / 44 000; a site shared by
 * paths of two groups is computed in both, so paths that share sites belong next to each other), then every path costs O(k^3) on its gathered k x k blocks: 2 U M N + 2 U^2 M flop per group (M candidate rows, N
 * train rows), the first term one matrix-core product whose epilogue forms E, the second Phi += E E^T over chunks of the
 * targets in a fixed order.  The grouping changes the result by rounding only.  sites[] as for algp_score_paths (-1 entries
 * skipped, a site listed twice counts once); an empty path scores 0; a path whose block meets a pivot that is not positive
 * scores NaN.  Preconditions as for algp_score_paths (a candidate solve with prior_includes_noise, no pick committed since:
 * ALGP_ERR_STATE; every site a resident candidate, at most 256 distinct sites per path: ALGP_ERR_BAD_ARG), and the criterion's
 * two refusals: candidates with an extra variance, or a candidate set that lists a pool site twice: ALGP_ERR_STATE. */
int algp_score_paths_vr(algp_ctx* ctx, const int64_t* sites, int npaths, int maxlen, double mobile_std, int64_t max_union,
                        double* dV_out);

/* ---- (e) multi-GPU: the loop over candidates (agent.py:317-347) cut into shards, one process and one ctx per GPU ----
 * Every rank factorises the same train set (algp_factorize / algp_fit_and_solve) and holds a share of the candidate list
 * (algp_set_candidates + a solve; ANY partition -- contiguous slices, the strided owner map of algp_comm_set_owners below --
 * and a share may be empty: the first maximum breaks ties by the smaller pool index whatever the shards).  The only communication of the path is ONE
 * all-gather per pick, issued by the library on the context's stream: each rank contributes 32 bytes -- (its best local
 * utility, that candidate's pool index, a status word, the candidate's statistic) -- plus that candidate's row of V^T
 * (Npad + 128 elements: ~80 KB at N = 10 000 fp64), so that a rank which does not own the winner copies the winner's row
 * instead of rebuilding it from the factor ($ALGP_GATHER_ROWS=0: the 32 bytes only, rows rebuilt).
 * algp_comm_unique_id: 128 opaque bytes (ncclUniqueId); one rank calls it, the caller hands them to the others.
 * algp_comm_init: joins this ctx to an RCCL communicator (xGMI) of `nranks` ranks as `rank` (collective: every rank
 *   calls it).  RCCL is opened with dlopen here; without it these return ALGP_ERR_HIP and nothing else is affected.
 * algp_comm_init_host: the same loop over a transport the CALLER owns (MPI, gloo, shared memory): `fn(user, send, recv,
 *   bytes_per_rank)` must all-gather `bytes_per_rank` bytes of host memory in rank order and return 0; it is called
 *   once per pick (twice in the rare extra round) by every rank; one stream synchronisation per pick, in front of it
 *   (the winner is then chosen on the host and only its row goes back to the device).
 *   This is also how two ranks can share one card.
 * Both reserve the exchange's buffers for the current train set; algp_set_train re-reserves them when its size changes.
 * algp_greedy_sharded: k picks (entropy criterion; the MI criterion with a layout of algp_comm_set_mi_groups, the
 *   variance-reduction criterion with one of algp_comm_set_vr_exchange, both below).  Per pick, stream-ordered and with
 *   a single read-back (40 bytes): each rank's best candidate resolved on the device (argmax, refresh of the rows
 *   whose bound can still win, argmax), the all-gather, the first maximum in rank order (= np.argmax over the
 *   concatenated scores, agent.py:349, shards being contiguous in rank order), then the commit of the winner on every
 *   rank (enqueued, not waited for).  picks_out: k pool indices (equal on all ranks); utilities_out: their k utilities,
 *   or NULL.  A rank that cannot take part in a pick (no solve, an allocation failure, a failed pack launch, a stalled
 *   one-launch kernel) still joins the gather and reports its error code in the status word: EVERY rank then returns that
 *   code, nobody commits the pick, nobody hangs.  A commit that fails on one rank AFTER the exchange that chose the winner
 *   is reported in that rank's status word of its next pick (every rank returns it from that call); after the LAST pick of
 *   a call it is returned by that rank at once and reported again in the first exchange of its next call -- the one case
 *   in which ranks leave a call with different codes (closing it would take a second collective per call).
 * The active-learning LOOP on sharded candidates (agent.py:125-229: greedy :141 -> _add_samples :66-82 -> predict :196-210,
 * with the loop of agent.py:313-354 cut into shards) -- algp_comm_set_owners: owner[q] = the rank that holds pool site q as
 *   a candidate (-1: nobody; NULL clears the map), the same array on every rank, after algp_comm_init[_host] and
 *   algp_set_pool (which DROPS a map attached before it: the map belongs to its pool; the communicator stays -- it is
 *   joined once per context).  With a map attached algp_factorize_update becomes a COLLECTIVE whatever a rank finds locally
 *   -- a rank that keeps nothing of its factor (an earlier factorisation failed, other hyper-parameters) or cannot
 *   re-allocate it still enters the agreement and says so there; the agreement word also carries a hash of the whole map
 *   (every rank calls it with the same train set): the sites a step appends to the train set are candidates of one rank each, and that rank's row of V^T is
 *   the site's new row of the replicated factor left of the tail block -- so instead of solving those rows against the
 *   kept factor on every rank (38 ms per 256 rows at N = 50 000) the ranks exchange them: a 32-byte agreement word per
 *   rank (status, first changed row, train size, a hash of the plan), then ONE all-gather of cap rows of the kept width
 *   per rank, cap = the largest number of new sites any rank owns (every rank derives the same plan from the train set
 *   and the map).  A rank whose V^T cannot supply its rows (no resident solve for these hyper-parameters / this
 *   candidate list) says so in the agreement and EVERY rank falls back to the solve; an error (allocation, injected) is
 *   returned by every rank, the second collective is then not entered by anyone.  (What is left: a HIP failure of the
 *   pack launch or its copies BETWEEN the two collectives returns from that rank alone -- the buffers are reserved before
 *   the agreement, so this means a lost device, not a full one.)  With any map other than contiguous
 *   shards in rank order the pick's first maximum still equals np.argmax in pool order: equal utilities go to the smaller
 *   pool index.  The calls that follow -- algp_solve_candidates_update on the rank's shard, algp_greedy_sharded -- are
 *   unchanged.  algp_debug_counter(ctx, 1..4): rows of L the last factor update placed without a triangular solve, how many
 *   of them came from other ranks, row exchanges so far, agreed fall-backs so far.                                        */
typedef int (*algp_allgather_fn)(void* user, const void* send, void* recv, int64_t bytes_per_rank);
int algp_comm_set_owners(algp_ctx* ctx, const int32_t* owner, int64_t n_pool);
int algp_comm_unique_id(void* out128);
int algp_comm_init(algp_ctx* ctx, int nranks, int rank, const void* unique_id128);
int algp_comm_init_host(algp_ctx* ctx, int nranks, int rank, algp_allgather_fn fn, void* user);
int algp_comm_destroy(algp_ctx* ctx);
int algp_greedy_sharded(algp_ctx* ctx, int criterion, double static_std, double mobile_std, int k, int64_t* picks_out,
                        double* utilities_out);
/* algp_comm_set_mi_groups: the layout under which algp_greedy_sharded scores the MUTUAL-INFORMATION criterion (agent.py:330-339)
 * with its two pool-wide inverses dealt over the ranks instead of whole on one GPU (without a layout that criterion is refused
 * there with ALGP_ERR_BAD_ARG).  Ranks [0, n_complement_ranks) hold P = C_AbarAbar^-1 (the unsampled sites, no noise), ranks
 * [n_complement_ranks, world) hold Q = (C + D_all)^-1 (the whole pool with its noise); 1 <= n_complement_ranks < world.  A
 * world of one takes 1 and keeps exactly the one-GPU state of algp_greedy (both inverses in place, two pool-sized matrices).
 * 0 detaches the layout.  Call it on every rank with the same value, after algp_comm_init[_host] (which drops a layout
 * attached before); a rank attached with another value makes every rank return ALGP_ERR_BAD_ARG from its next
 * algp_greedy_sharded.  The split is the caller's choice between memory and time.
 * What the sharded criterion costs (api_mi.hip): at the first pick after a solve every member of a group of g ranks
 * builds and factors its group's matrix (m^3 / 3 flop, replicated), computes only its 128-row blocks b = member + j g of
 * X = L^-T (~ m^3 / (3 g) flop on the MFMA GEMM path) and releases the factor.  PEAK device memory of the MI state per rank:
 * the matrix (m_pad^2 elements, m = its group's size) + its rows of X (~ m_pad^2 / g) + 256 whole vectors of n_pool; AFTER
 * the build the rows and the vectors only.  Config 4's 110 000 sites in fp64, 8 ranks split 4 + 4: 121 GB peak and 24.5 GB
 * of MI state after the build, against 194 GB on one GPU (the rest of a rank's device memory -- train factor, candidate
 * solve, the train set's entropy scratch -- comes on top, as on one GPU).  Every rank checks its peak BEFORE anything is
 * allocated and the check is agreed on: a rank that does not fit makes every rank return ALGP_ERR_OOM with the byte count.
 * Collectives (all of them all-gathers through the attached transport, no other RCCL call): at the first pick of a call a
 * 32-byte agreement word per rank (+ a stream synchronisation), and after a solve one gather of every rank's diagonal entries;
 * per committed pick folded, two gathers of O(n_pool) bytes per rank (the owners' rows of X at the pick, then every rank's
 * entries of the pick's columns); each gather carries every rank's status word, so that a rank which fails in its share of a
 * step (memory, a matrix that is not positive definite, a HIP error) still joins every collective and every rank returns its
 * code from the same call; the MI state is then rebuilt by the next call.  Not covered: a HIP failure AFTER a step's last
 * gather (the copies behind the build's gather, the launches that fold a gathered column, a header copy inside a gather)
 * returns from that rank alone while its peers go on to the pick's exchange -- as for algp_factorize_update, a caller that
 * sees ALGP_ERR_HIP must tear the job down.  Picks and utilities equal algp_greedy's on one GPU (to rounding: the diagonals
 * come from differently blocked products).  algp_scores with the MI criterion on such a context scores from the sharded
 * state while it is current; with picks committed outside algp_greedy_sharded it builds the whole inverses on this GPU. */
int algp_comm_set_mi_groups(algp_ctx* ctx, int n_complement_ranks);
/* algp_comm_set_vr_exchange: the layout under which the VARIANCE-REDUCTION criterion is scored over the ranks (without it
 * algp_greedy_sharded refuses that criterion with ALGP_ERR_BAD_ARG).  The targets become the union over the ranks of the
 * ordinary rows of each rank's candidate set -- the shards must be disjoint: a pool site listed by two ranks, as a target or as
 * a unit row, makes every rank return ALGP_ERR_STATE from the build; empty shards are legal -- and a rank keeps w_c = sum_{j in T_all} omega_j E_jc^2 for its
 * own rows c only.  rows_per_round > 0: every rank contributes that many rows of its V^T (rounded up to a multiple of 128) to
 * each all-gather of the build; -1: the library's default,
 *   B = max(128, floor(((2^30 / (world + 1) - 32) / (8 + es (Npad + 128))) / 128) * 128),   es = the element size,
 * the largest multiple of 128 for which the (world + 1) slices [32-byte header | 8-byte pool index and Npad + 128 elements per
 * row] of the staging buffer stay within 1 GiB (config 4, 8 ranks, fp64: 1 408 rows, 9 rounds); either is capped at the largest
 * shard, rounded up to 128.  0 detaches the layout.  After algp_comm_init[_host] (else ALGP_ERR_STATE), which drops a layout
 * attached before; the same value on every rank: differing values make every rank return ALGP_ERR_BAD_ARG from its next
 * collective scoring (they are compared in the agreement word, before any payload travels).  A world of one keeps the
 * one-GPU state, bit for bit.
 * Collectives (all-gathers through the attached transport only), on the context's stream, a gather and the product behind it
 * one after the other: at the first scoring of a call an 80-byte agreement word per rank (status, rows, picks committed and
 * folded, whether it needs a build -- no valid state, another solve, new weights, ALGP_VR_RANK1=0; any rank's need is every
 * rank's -- the rows per round, the weights' hash, Npad, n_pool); a build is a 32-byte word (allocations), R = ceil(largest
 * shard / B) gathers of 32 + B (8 + es K) bytes per rank (per row its pool site -- tagged where the row is a unit row, which
 * travels as zeros -- and its K columns) (K = Npad, or Npad + 128 once picks are committed), each followed by
 * ONE rectangular product of the rank's whole V^T against the world x B gathered rows (2 M_loc_pad world B K flop), and a last
 * 32-byte gather with the outcome of the disjointness check; every committed pick folded is one gather of
 * 48 + es (Npad + 128) + (8 + es) max_shard bytes per rank (the rank's partial sums over its targets and its targets' (pool
 * index, omega r) pairs).  The partial sums are added in a fixed order (round, rank, tile; rank): the same bits in every run
 * for a given world, partition and rows per round; across worlds the utilities differ by rounding only.  Every gather carries
 * each rank's status word: a rank that fails still takes part, every rank returns its code from the same call, and the state
 * is rebuilt by the next call.  Ranks with different numbers of committed picks: ALGP_ERR_STATE. */
int algp_comm_set_vr_exchange(algp_ctx* ctx, int64_t rows_per_round);
/* ---- test hooks -----------------------------------------------------------------------------------------------------
 * Compiled in when ALGP_TEST_HOOKS is 1 -- the default of algp_amd/csrc/Makefile, and what this repository's tests and
 * bench.py (its one-stream leg, the strong-scaling emulation) need; `make TEST_HOOKS=0` builds the library without them
 * (tests/test_abi.py checks that such an object exports no algp_debug_* symbol). */
#ifndef ALGP_TEST_HOOKS
#define ALGP_TEST_HOOKS 1
#endif
#if ALGP_TEST_HOOKS
/* Test hooks of the exchange (no reference counterpart).  algp_debug_first_max: the reduction kernel of the gather on a
 * caller-made buffer of nranks triples (utility, pool index or -1, status) -> out5 = (utility, pool index, owner rank,
 * status, first rank with a non-zero status).  algp_debug_fail_next_pick: this rank reports `code` (an ALGP_ERR_* >= 2)
 * instead of a candidate in its next pick.  algp_debug_counter(ctx, 0): stream synchronisations issued so far.
 * algp_debug_set_trsm_chunks: row-chunk streams of the candidate solve, 1..4 (0: back to the default 3 / $ALGP_TRSM_CHUNKS);
 * every setting gives the same bits -- bench.py uses 1 to time the GEMM launches back to back.
 * algp_debug_dag_stall: in the next one-launch factorisation (chol_dag.hip) the task that draws `ticket` never publishes its
 * tile and the spin limit drops from 2 s to 0.2 s: its consumers run into the limit, the launch aborts itself and
 * algp_factorize returns ALGP_ERR_HIP ("stalled") -- the path a lost hand-off would take; the context stays usable. */
/* algp_debug_trsv_stall: in the next one-launch forward or backward substitution (potrf.hip) the workgroup of 128-block
 * `block` never sets its flag and the spin limit drops to 0.2 s: the launch abandons itself, the context's sticky stall
 * word is set and the call that reads the result back (algp_factorize, algp_get_alpha, algp_commit_pick, the next pick of
 * algp_greedy[_sharded]) returns ALGP_ERR_HIP ("stalled"); the context stays usable.
 * algp_debug_get_pick: pick number q since the last candidate solve as every rank committed it: row_out = the winner's row
 * of V^T (ncols_out elements, the context's dtype; ncols = Npad + q), d_out = its statistic when it was committed.  What a
 * rank receives in the pick's all-gather from the winner's owner; bench.py uses it to fabricate the seven absent ranks of
 * an eight-rank run on one GPU. */
/* algp_debug_fail_at: inject `code` (an ALGP_ERR_* >= 2; 0 disarms) into this rank's next greedy pick at `where`:
 * 0 = while resolving its best candidate (= algp_debug_fail_next_pick), 1 = in the commit of the winner, AFTER the exchange
 * that chose it (the code travels in this rank's status word of its next pick: every rank returns it from that call; after
 * the last pick of a call it is returned by this rank at once and reported again in its next call's first exchange),
 * 2 = the launch that packs its contribution counts as failed (ALGP_ERR_HIP in its status word, the gather still runs),
 * 3 = this rank's agreement word of its next sharded algp_factorize_update carries `code`: every rank returns it,
 * 4 = the next step of the sharded MI criterion on this rank (its build after a solve, else the fold of a committed pick) fails
 * with `code`; every rank returns it from that algp_greedy_sharded call (a world of one has no such step),
 * 5 = the same for the variance-reduction criterion over the ranks (algp_comm_set_vr_exchange): this rank's next step (the
 * build, else the fold of a committed pick) fails with `code`; every rank returns it from that algp_scores or
 * algp_greedy_sharded call. */
int algp_debug_fail_at(algp_ctx* ctx, int where, int code);
int algp_debug_trsv_stall(algp_ctx* ctx, int block);
int algp_debug_get_pick(algp_ctx* ctx, int q, void* row_out, int64_t row_capacity, int64_t* ncols_out, double* d_out);
/* algp_debug_get_factor_rows: rows [row0, row0 + nrows) of the resident factor, columns [0, ncols), row-major into out (the
 * context's dtype) -- what the owners of a step's new train sites contribute to the row exchange; bench.py uses it to
 * fabricate the seven absent ranks of an eight-rank config-5 step on one GPU. */
int algp_debug_get_factor_rows(algp_ctx* ctx, int64_t row0, int64_t nrows, int64_t ncols, void* out);
int algp_debug_first_max(algp_ctx* ctx, const double* triples, int nranks, double out5[5]);
int algp_debug_set_trsm_chunks(algp_ctx* ctx, int chunks);
int algp_debug_fail_next_pick(algp_ctx* ctx, int code);
int algp_debug_dag_stall(algp_ctx* ctx, int ticket);
int64_t algp_debug_counter(algp_ctx* ctx, int which);
#endif /* ALGP_TEST_HOOKS */

/* ---- a5 / a8: entropy_from_cov (utils.py:188-194) and set entropies for best_path --------
 * algp_entropy_from_cov: k*CONST + 1/2 log det cov for a host k x k SPD matrix.
 * algp_set_entropy: H(C[idx,idx] + diag(var)) for pool indices (agent.py:386-387).              */
int algp_entropy_from_cov(algp_ctx* ctx, const void* cov, int64_t k, double* H);
int algp_set_entropy(algp_ctx* ctx, const int64_t* idx, int64_t m, const void* var, double* H);
/* diag((C[idx,idx] + diag(var))^-1), m values, and its entropy (MI terms agent.py:331-338)     */
int algp_set_inverse_diag(algp_ctx* ctx, const int64_t* idx, int64_t m, const void* var,
                          void* diag_out, double* H);

/* ---- dense building blocks on host matrices (parity tests; also usable on their own) ------
 * algp_cholesky: L (n x n lower, zeros above) of a host SPD matrix, optional log det.
 * algp_gemm_nt: D = alpha * A(m x k) * B(n x k)^T + beta * C(m x n).
 * algp_trsm_right_lt: X = B * L^-T for B (m x n), L (n x n lower) -- the candidate solve.     */
int algp_cholesky(algp_ctx* ctx, const void* A, int64_t n, void* L_out, double* logdet);
int algp_gemm_nt(algp_ctx* ctx, int64_t m, int64_t n, int64_t k, double alpha, const void* A,
                 const void* B, double beta, const void* C, void* D);
int algp_trsm_right_lt(algp_ctx* ctx, const void* L, int64_t n, const void* B, int64_t m,
                       void* X_out);
/* MFMA fragment-layout probe: runs one 16x16x4 MFMA per dtype on exact integer operands and
 * returns the number of mismatching outputs (0 expected).                                      */
int algp_selftest_mfma(algp_ctx* ctx, int* mismatches);
/* device-resident GEMM timing on pseudo-random operands (no host traffic): average ms per launch
 * of D = C - A B^T (beta_one) or D = -A B^T, m x n x k, lower tiles only or all.                      */
int algp_bench_gemm(algp_ctx* ctx, int64_t m, int64_t n, int64_t k, int lower_only, int beta_one, int reps,
                    double* ms_per_launch);
/* the same for D = C - A B^T with C not loaded but generated in the epilogue from synthetic coordinates,
 * as the candidate sweep's update products form the right-hand sides (the scheduled launcher only: an
 * error where it is switched off).                                                                    */
int algp_bench_gemm_generated(algp_ctx* ctx, int64_t m, int64_t n, int64_t k, int reps, double* ms_per_launch);
/* the fixed effects' rank-p fold on a zeroed rows x cols matrix and a device-to-device copy of that matrix, average ms per
 * launch each (the fold reads and writes every entry once: the copy is its yardstick); and the posterior pass over a zeroed
 * rows x ncols panel (ncols a multiple of 128) with a zero basis row, as W, T and a sample tile go through it.  1 <= p <= 16.   */
int algp_bench_fixed_fold(algp_ctx* ctx, int64_t rows, int64_t cols, int p, int reps, double* fold_ms, double* copy_ms);
int algp_bench_fixed_panel(algp_ctx* ctx, int64_t rows, int64_t ncols, int p, int reps, double* ms_per_launch);

/* ---- resident-buffer access for benchmarks / multi-GPU plumbing --------------------------- */
int algp_sync(algp_ctx* ctx);
int64_t algp_device_bytes(const algp_ctx* ctx);

/* ---- profiling: HIP events around every launch of a class, on the ctx stream ------------- */
int algp_prof_enable(algp_ctx* ctx, int on);
int algp_prof_reset(algp_ctx* ctx);
int algp_prof_get(algp_ctx* ctx, int klass, double* ms, double* flops, double* bytes,
                  int64_t* launches);
/* In-kernel accounting of the one-launch Cholesky since the last algp_prof_reset (collected only while profiling is
 * enabled): out[0] = microseconds spent inside the rank-k update products ("panel update", reference: the LU inside
 * np.linalg.inv / slogdet, utils.py:193, 300), summed over workgroups; out[1] = their K = 128 steps (2 * 128^3 flop
 * each); out[2], out[3] = the same for the triangular-solve tile products (microseconds, count). Two workgroups
 * share a CU, so the update rate while computing is 2 * 128^3 * out[1] / (out[0] / 2 / CUs) flop/s. */
int algp_cholesky_task_stats(algp_ctx* ctx, double out[4]);

#ifdef __cplusplus
}
#endif
#endif /* ALGP_HIP_H */
