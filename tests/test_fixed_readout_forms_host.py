"""tests/fixed_readout_forms.py (the NumPy reference of the read-outs that carry the estimated fixed effects) held to statements
that do not share its algebra; no GPU.

Inputs: test_fit_regimes.py's draws (x ~ U(0, side)^2, y = sin(x_0) + 0.1 randn, var ~ U(0.005, 0.05)) with a genotype id per site
and a planted H beta added to y, under the relationship kernel (Matern-3/2 + a marker relationship of Q = 7 genotypes) at the
hyper-parameters of test_average_information.py; N = 60 train sites, M = 25 candidates, the bases of reml_forms.basis with p = 3
and 16 columns.

* the genotype effects and the group aggregates against the GP with the diffuse prior beta ~ N(0, tau^2 I) folded into the
  kernel, at tests/test_reml_forms_host.py's tau^2 = 1e6 and bound 1e-5, with an error that shrinks from tau^2 = 1e4; the
  effects' B carries no tau^2 term
* with the constant in the span of H nothing depends on the mean (1e-11, that file's bound)
* the prediction-error variances are never below the known-mean ones; the covariances are positive semi-definite
* sample_rule as a linear map of (g, eps): its exact covariance is the known-mean covariance + proj proj' to 1e-10, its mean
  is the universal-kriging mean
* component 1 of the mean at a site is the genotype effect of its id; -1 = mean + 0 + 1 + 2
"""
import functools

import numpy as np
import pytest

import ai_forms as AI
import fixed_readout_forms as FO
import matern_forms as MF
import relationship_forms as RF
import reml_forms as RM
import test_fit_regimes as FR

N, M, Q = 60, 25, 7
LOG_OS = (np.log(FR.OUTPUTSCALE), np.log(0.3))
LOG_NOISE = np.log(FR.NOISE)
PS = [3, 16]


@functools.lru_cache(maxsize=None)
def _case(p):
    x, y, var, log_ls = FR._draw(N, 2, N + M)
    rng = np.random.RandomState(7 + p)
    x = np.c_[x, rng.randint(0, Q, len(x)).astype(np.float64)]
    H = RM.basis(x[:, :2], p)
    y = y + H[:N] @ RM.planted_beta(p)
    theta = AI.pack(log_ls, LOG_OS, LOG_NOISE)
    group = rng.randint(0, Q, M)
    A = np.zeros((Q, M))
    A[group, np.arange(M)] = 1.0
    A /= np.maximum(A.sum(1, keepdims=True), 1.0)
    for a in (x, y, var, H, theta, A):
        a.setflags(write=False)
    return dict(args=('relationship', (MF.MATERN15, RF.marker_relationship(Q=Q), Q), theta), x=x[:N], y=y, var=var, H=H[:N], xc=x[N:],
                Hc=H[N:], A=A)


def _rel(u, v):
    return float(np.max(np.abs(np.asarray(u) - np.asarray(v))) / max(1.0, float(np.max(np.abs(v)))))


@pytest.mark.parametrize('p', PS)
def test_genotype_effects_are_the_diffuse_prior_limit(p):
    c = _case(p)
    a = (*c['args'], c['x'], c['y'], c['H'])
    mean, cov = FO.genotype_posterior_fixed(*a, c['var'])
    err = {}
    for tau2 in (1e4, 1e6):
        m, cv = FO.genotype_posterior_diffuse(*a, tau2, c['var'])
        err[tau2] = max(np.max(np.abs(m - mean)), np.max(np.abs(cv - cov)))
    assert err[1e6] <= 1e-5 and err[1e6] < err[1e4], err


@pytest.mark.parametrize('p', PS)
def test_group_aggregates_are_the_diffuse_prior_limit(p):
    c = _case(p)
    a = (*c['args'], c['x'], c['y'], c['H'], c['xc'], c['Hc'])
    got = FO.group_posterior_fixed(*a, c['A'], c['var'])
    err = {}
    for tau2 in (1e4, 1e6):
        mu, cov = RM.posterior_diffuse(*a, tau2, c['var'])
        err[tau2] = max(np.max(np.abs(c['A'] @ mu - got['mean'])), np.max(np.abs(c['A'] @ cov @ c['A'].T - got['cov'])),
                        np.max(np.abs(c['A'] @ cov - got['cross'])))
    assert err[1e6] <= 1e-5 and err[1e6] < err[1e4], err


@pytest.mark.parametrize('p', PS)
def test_nothing_depends_on_the_mean_with_the_constant_in_the_span(p):
    c = _case(p)
    a = (*c['args'], c['x'], c['y'], c['H'])
    for u, v in zip(FO.genotype_posterior_fixed(*a, c['var'], None, 0.3), FO.genotype_posterior_fixed(*a, c['var'])):
        assert _rel(u, v) <= 1e-11
    g0 = FO.group_posterior_fixed(*a, c['xc'], c['Hc'], c['A'], c['var'])
    g1 = FO.group_posterior_fixed(*a, c['xc'], c['Hc'], c['A'], c['var'], None, 0.3)
    assert all(_rel(g1[k], g0[k]) <= 1e-11 for k in g0)
    for comp in (-1, 0, 1):
        assert _rel(FO.mean_fixed(*a, c['xc'], c['Hc'], comp, c['var'], None, 0.3), FO.mean_fixed(*a, c['xc'], c['Hc'], comp, c['var'])) <= 1e-11


@pytest.mark.parametrize('p', PS)
def test_prediction_error_variances_carry_the_effects_uncertainty(p):
    c = _case(p)
    a = (*c['args'], c['x'], c['y'])
    mean, cov = FO.genotype_posterior_fixed(*a, c['H'], c['var'])
    mean0, cov0 = FO.genotype_posterior_known(*a, c['var'])
    assert np.all(np.diag(cov) >= np.diag(cov0) - 1e-12)
    assert np.max(np.diag(cov) - np.diag(cov0)) >= 1e-4          # no rounding matter on these inputs
    assert np.max(np.abs(mean - mean0)) >= 1e-3                   # nor is the adjustment of the BLUPs
    for S in (cov, FO.group_posterior_fixed(*a, c['H'], c['xc'], c['Hc'], c['A'], c['var'])['cov']):
        ev = np.linalg.eigvalsh(0.5 * (S + S.T))
        assert ev[0] >= -1e-12 * ev[-1]
        assert np.max(np.abs(S - S.T)) <= 1e-12 * np.max(np.abs(S))


@pytest.mark.parametrize('p', PS)
def test_sample_rule_has_the_universal_kriging_moments(p):
    """The rule is affine in (g_A, g_X, eps): f = m + g_X - Lam (g_A + sqrt(v) eps) with Lam read off by feeding it unit vectors.
    With cov(g) = K and independent eps its covariance is K_XX - Lam K_AX - K_XA Lam' + Lam S Lam'."""
    c = _case(p)
    fam, spec, theta = c['args']
    a = (fam, spec, theta, c['x'], c['y'], c['H'], c['xc'], c['Hc'])
    zN, zM = np.zeros((1, N)), np.zeros((1, M))
    post = RM.posterior_fixed(*a, c['var'])
    m = FO.sample_rule(*a, zN, zM, zN, c['var'])[0]                                # no randomness: the mean
    assert np.max(np.abs(m - post['mu'])) <= 1e-10
    Lam = -(FO.sample_rule(*a, np.eye(N), np.zeros((N, M)), np.zeros((N, N)), c['var']) - m).T        # M x N
    v = np.exp(LOG_NOISE) + c['var']
    Le = -(FO.sample_rule(*a, np.zeros((N, N)), np.zeros((N, M)), np.eye(N), c['var']) - m).T
    assert np.max(np.abs(Le - Lam * np.sqrt(v)[None, :])) <= 1e-10
    Gx = FO.sample_rule(*a, np.zeros((M, N)), np.eye(M), np.zeros((M, N)), c['var']) - m
    assert np.max(np.abs(Gx - np.eye(M))) <= 1e-10
    S, Kca, Kcc = RM.prior_blocks(fam, spec, theta, c['x'], c['xc'], c['var'])
    Kaa = S - np.diag(v)
    cov = Kcc - Lam @ Kca.T - Kca @ Lam.T + Lam @ Kaa @ Lam.T + (Lam * v[None, :]) @ Lam.T
    cov0 = RM.posterior_known_mean(fam, spec, theta, c['x'], c['y'], c['xc'], c['var'])[1]
    assert np.max(np.abs(cov - (cov0 + post['proj'] @ post['proj'].T))) <= 1e-10
    assert np.max(np.abs(cov - post['cov'])) <= 1e-10


@pytest.mark.parametrize('p', PS)
def test_mean_shares_add_up_and_component_1_is_the_genotype_effect(p):
    c = _case(p)
    a = (*c['args'], c['x'], c['y'], c['H'])
    sites, Hs = np.vstack([c['x'], c['xc']]), np.vstack([c['H'], c['Hc']])
    part = {k: FO.mean_fixed(*a, sites, Hs, k, c['var']) for k in (-1, 0, 1, 2)}
    assert np.max(np.abs(part[-1] - (c['y'].mean() + part[0] + part[1] + part[2]))) <= 1e-10
    mean = FO.genotype_posterior_fixed(*a, c['var'])[0]
    assert np.max(np.abs(part[1] - mean[sites[:, -1].astype(int)])) <= 1e-10
    assert np.max(np.abs(part[-1][N:] - RM.posterior_fixed(*a, c['xc'], c['Hc'], c['var'])['mu'])) <= 1e-10
