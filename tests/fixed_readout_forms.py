"""The read-outs that carry the estimated fixed effects (algp_genotype_posterior_fixed, algp_group_posterior_fixed,
algp_posterior_mean_fixed) in NumPy fp64, built on tests/ai_forms.py and tests/reml_forms.py and written with the DENSE projector
P = S^-1 - S^-1 H A^-1 H' S^-1 where the library goes through the Cholesky factor: what tests/test_fixed_readout_forms_host.py
and tests/test_fixed_readouts.py compare against.

    genotype effects u ~ N(0, os_g G), B = cov(u, y_A) = os_g G[:, g_A]:   mean = B P y0,   cov = os_g G - B P B'
    groups, A_g the Q x M coefficients:   A_g applied to reml_forms.posterior_fixed's mu and cov (+ diag(extra)), A_g cov the cross
    the mean at sites (k: their kernel rows against the train rows, h: their basis rows), alpha_R = P y0:
        mean + h' beta + k' alpha_R;   a kernel part's share k_c' alpha_R;   the trend's share h' beta
    sample_rule: Matheron's rule on the universal-kriging predictor, literally, from a prior draw g and noise draws eps

A model is ai_forms' (family, spec) with theta in the gradient's order; the separable kernel goes through
separable_forms._in_reml_forms as its restricted likelihood does (model_scope below).
"""
import contextlib

import numpy as np

import additive_forms as AF
import relationship_forms as RF
import reml_forms as RM
import separable_forms as SF


def model_scope(family, spec):
    """The context in which reml_forms serves this family (the separable kernel stands in for ai_forms there)."""
    return SF._in_reml_forms(spec) if family == SF.FAMILY else contextlib.nullcontext()


def _part_forms(family):
    return {'additive': AF, 'relationship': RF, SF.FAMILY: SF}[family]


def part_matrix(family, spec, theta, part, x1, x2):
    """Part 0 or 1 of a two-part kernel between the sites x1 and x2, noise-free."""
    with model_scope(family, spec):
        log_ls, log_os, _ = RM.AI.unpack(family, theta, x2)
    return _part_forms(family).part_matrix(spec, part, log_ls, log_os, x1, x2)


def genotype_prior(family, spec, theta, x):
    """(B, os_g G): cov(u, y_A) = os_g G[:, g_A] (Q x N) and the effects' prior covariance."""
    with model_scope(family, spec):
        log_os = RM.AI.unpack(family, theta, x)[1]
    G = _part_forms(family).table(spec)
    ids = np.asarray(x, np.float64).reshape(len(x), -1)[:, -1].astype(np.int64)
    osg = np.exp(log_os[1])
    return osg * G[:, ids], osg * G


def genotype_posterior_fixed(family, spec, theta, x, y, H, var=None, sites=None, mean=None):
    """(mean, cov) of the genotype effects with beta estimated: B P y0 and os_g G - B P B' (the prediction-error variances of
    Henderson's mixed-model equations)."""
    with model_scope(family, spec):
        P, y0 = RM._parts(family, spec, theta, x, y, H, var, sites, mean)[4:6]
    B, G = genotype_prior(family, spec, theta, x)
    return B @ (P @ y0), G - B @ P @ B.T


def genotype_posterior_known(family, spec, theta, x, y, var=None, sites=None, mean=None):
    """(mean, cov) for the constant mean alone: what algp_genotype_posterior returns."""
    with model_scope(family, spec):
        S = RM.AI.train_matrix(family, spec, theta, x, var, sites)
    y = np.asarray(y, np.float64)
    B, G = genotype_prior(family, spec, theta, x)
    return B @ np.linalg.solve(S, y - (y.mean() if mean is None else mean)), G - B @ np.linalg.solve(S, B.T)


def genotype_posterior_diffuse(family, spec, theta, x, y, H, tau2, var=None, sites=None, mean=None):
    """(mean, cov) under the prior beta ~ N(0, tau2 I) folded into the train covariance; B carries no tau2 term (u and beta are
    independent a priori)."""
    with model_scope(family, spec):
        S = RM.AI.train_matrix(family, spec, theta, x, var, sites)
    y = np.asarray(y, np.float64)
    H = np.asarray(H, np.float64).reshape(len(y), -1)
    Sd = S + tau2 * H @ H.T
    B, G = genotype_prior(family, spec, theta, x)
    return B @ np.linalg.solve(Sd, y - (y.mean() if mean is None else mean)), G - B @ np.linalg.solve(Sd, B.T)


def group_posterior_fixed(family, spec, theta, x, y, H, xc, Hc, A_g, var=None, sites=None, mean=None, extra=None):
    """dict(mean, cov, cross) of the functionals A_g (mean + h' beta + f) at xc: A_g applied to the universal-kriging posterior
    (extra: variances added to the candidates' diagonal, algp_set_candidates' extra_var)."""
    with model_scope(family, spec):
        post = RM.posterior_fixed(family, spec, theta, x, y, H, xc, Hc, var, sites, mean)
    cov = post['cov'] if extra is None else post['cov'] + np.diag(np.asarray(extra, np.float64))
    A_g = np.asarray(A_g, np.float64)
    return dict(mean=A_g @ post['mu'], cov=A_g @ cov @ A_g.T, cross=A_g @ cov)


def mean_fixed(family, spec, theta, x, y, H, xs, Hs, component=-1, var=None, sites=None, mean=None):
    """The posterior mean at the sites xs (basis rows Hs) with beta estimated.  component -1: mean + h' beta + k' alpha_R; 0, 1:
    the kernel part's share k_c' alpha_R; 2: the trend's share h' beta."""
    y = np.asarray(y, np.float64)
    with model_scope(family, spec):
        _, Si, _, Ai, P, y0, H = RM._parts(family, spec, theta, x, y, H, var, sites, mean)
        if component == -1:
            K = RM.prior_blocks(family, spec, theta, x, xs)[1]
    Hs = np.asarray(Hs, np.float64).reshape(len(xs), -1)
    beta = Ai @ (H.T @ (Si @ y0))
    aR = P @ y0
    if component == 2:
        return Hs @ beta
    if component in (0, 1):
        return part_matrix(family, spec, theta, component, xs, x) @ aR
    return (y.mean() if mean is None else mean) + Hs @ beta + K @ aR


def sample_rule(family, spec, theta, x, y, H, xc, Hc, g_train, g_cand, eps, var=None, sites=None, mean=None):
    """Draws of mean + h' beta + f at xc by Matheron's rule on the universal-kriging predictor, evaluated literally through the
    Cholesky factor: z_s = L^-1 (y - mean - g_s(A) - sqrt(v) eps_s), beta_s = A^-1 F' z_s, f_s = mean + g_s + V z_s + R beta_s
    with F = L^-1 H_A, V = K_*A L^-T, R = H_C - V F.  g_train (S, N), g_cand (S, M): one prior draw per sample at the train
    sites and at xc; eps (S, N) standard normal."""
    y = np.asarray(y, np.float64)
    with model_scope(family, spec):
        S_, _, _, _, _, y0, H = RM._parts(family, spec, theta, x, y, H, var, sites, mean)
        Kca = RM.prior_blocks(family, spec, theta, x, xc, var, sites)[1]
        noise = np.exp(RM.AI.unpack(family, theta, x)[2])
    Hc = np.asarray(Hc, np.float64).reshape(len(xc), -1)
    v = noise + (0.0 if var is None else np.asarray(var, np.float64))
    L = np.linalg.cholesky(S_)
    F = np.linalg.solve(L, H)
    V = np.linalg.solve(L, Kca.T).T
    R = Hc - V @ F
    Ai = np.linalg.inv(F.T @ F)
    Z = np.linalg.solve(L, (y0[None, :] - np.asarray(g_train, np.float64) - np.sqrt(v)[None, :] * np.asarray(eps, np.float64)).T)   # N x S
    Bt = Ai @ (F.T @ Z)                                                                                                    # p x S
    m = y.mean() if mean is None else mean
    return m + np.asarray(g_cand, np.float64) + (V @ Z + R @ Bt).T
