"""tests/reml_forms.py (the NumPy reference of the fixed effects) held to statements that do not share its algebra; no GPU.

Inputs are test_fit_regimes.py's draws (x ~ U(0, side)^2, y = sin(x_0) + 0.1 randn, var ~ U(0.005, 0.05)) with a planted H beta
added to y, the hyper-parameters of test_average_information.py, and the three bases of reml_forms.basis (p = 1, 3, 16).  The
bounds are what those statements measured for N = 65 ... 1025 plus an order of magnitude:

* l_R = the likelihood of N - p orthonormal error contrasts - 1/2 log|H'H|                          (measured 2e-12, bound 1e-10)
* the closed-form gradient against central differences of l_R, relative to its largest entry         (5e-10, 1e-8)
* AI_R symmetric and positive semi-definite
* with the constant in the span of H: beta-adjusted predictions, l_R, gradient and AI do not depend on the mean  (5e-13, 1e-11)
* the posterior against the GP with the diffuse prior beta ~ N(0, tau^2 I) at tau^2 = 1e6             (1.2e-6, 1e-5),
  with an error that shrinks from tau^2 = 1e4
* proj proj' = the covariance with the estimated trend - the known-mean covariance
"""
import functools

import numpy as np
import pytest

import ai_forms as AI
import matern_forms as MF
import reml_forms as RM
import test_fit_regimes as FR

LOG_OS, LOG_NOISE = np.log(FR.OUTPUTSCALE), np.log(FR.NOISE)
CASES = [(65, 1), (65, 3), (129, 16), (300, 3), (300, 16)]
IDS = ['N%d-p%d' % c for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(N, p, M=40):
    x, y, var, log_ls = FR._draw(N, 2, N + M)
    H = RM.basis(x, p)
    y = y + H[:N] @ RM.planted_beta(p)
    theta = AI.pack(log_ls, LOG_OS, LOG_NOISE)
    for a in (x, y, var, H, theta):
        a.setflags(write=False)
    return dict(args=('single', MF.MATERN15, theta), x=x[:N], y=y, var=var, H=H[:N], xc=x[N:], Hc=H[N:])


@pytest.mark.parametrize('N,p', CASES, ids=IDS)
def test_reml_is_the_contrast_likelihood(N, p):
    c = _case(N, p)
    want = RM.contrast_likelihood(*c['args'], c['x'], c['y'], c['H'], c['var']) - 0.5 * np.linalg.slogdet(c['H'].T @ c['H'])[1]
    got = RM.reml(*c['args'], c['x'], c['y'], c['H'], c['var'])
    assert abs(got - want) <= 1e-10 * abs(want)


@pytest.mark.parametrize('N,p', CASES[:3], ids=IDS[:3])
def test_gradient_against_central_differences(N, p):
    c = _case(N, p)
    fam, spec, theta = c['args']
    g = RM.reml_grad(fam, spec, theta, c['x'], c['y'], c['H'], c['var'])
    h = 1e-5
    num = np.empty_like(g)
    for a in range(len(theta)):
        e = np.zeros(len(theta))
        e[a] = h
        num[a] = (RM.reml(fam, spec, theta + e, c['x'], c['y'], c['H'], c['var']) -
                  RM.reml(fam, spec, theta - e, c['x'], c['y'], c['H'], c['var'])) / (2 * h)
    assert np.max(np.abs(g - num)) <= 1e-8 * np.max(np.abs(g))


@pytest.mark.parametrize('N,p', CASES, ids=IDS)
def test_ai_is_symmetric_and_positive_semidefinite(N, p):
    c = _case(N, p)
    ai = RM.reml_ai(*c['args'], c['x'], c['y'], c['H'], c['var'])
    assert np.max(np.abs(ai - ai.T)) <= 1e-12 * np.max(np.abs(ai))
    ev = np.linalg.eigvalsh(0.5 * (ai + ai.T))
    assert ev[0] >= -1e-12 * ev[-1]


@pytest.mark.parametrize('N,p', CASES, ids=IDS)
def test_nothing_depends_on_the_mean_with_the_constant_in_the_span(N, p):
    c = _case(N, p)
    a = (*c['args'], c['x'], c['y'], c['H'])
    rel = lambda u, v: float(np.max(np.abs(np.asarray(u) - np.asarray(v))) / max(1.0, float(np.max(np.abs(v)))))
    for f in (RM.reml, RM.reml_grad, RM.reml_ai):
        assert rel(f(*a, c['var'], None, 0.3), f(*a, c['var'])) <= 1e-11
    p0 = RM.posterior_fixed(*a, c['xc'], c['Hc'], c['var'])
    p1 = RM.posterior_fixed(*a, c['xc'], c['Hc'], c['var'], None, 0.3)
    assert rel(p1['mu'], p0['mu']) <= 1e-11 and rel(p1['cov'], p0['cov']) <= 1e-11
    shift = np.r_[0.3 - c['y'].mean(), np.zeros(p - 1)]           # the intercept absorbs the shift
    assert rel(p1['beta'] + shift, p0['beta']) <= 1e-11


@pytest.mark.parametrize('N,p', CASES, ids=IDS)
def test_posterior_is_the_diffuse_prior_limit(N, p):
    c = _case(N, p)
    a = (*c['args'], c['x'], c['y'], c['H'], c['xc'], c['Hc'])
    got = RM.posterior_fixed(*a, c['var'])
    err = {}
    for tau2 in (1e4, 1e6):
        mu, cov = RM.posterior_diffuse(*a, tau2, c['var'])
        err[tau2] = max(np.max(np.abs(mu - got['mu'])), np.max(np.abs(np.diag(cov) - got['var'])))
    assert err[1e6] <= 1e-5 and err[1e6] < err[1e4]


@pytest.mark.parametrize('N,p', CASES, ids=IDS)
def test_proj_carries_the_covariance_of_the_trend(N, p):
    c = _case(N, p)
    got = RM.posterior_fixed(*c['args'], c['x'], c['y'], c['H'], c['xc'], c['Hc'], c['var'])
    mu0, cov0 = RM.posterior_known_mean(*c['args'], c['x'], c['y'], c['xc'], c['var'])
    assert np.max(np.abs(got['proj'] @ got['proj'].T - (got['cov'] - cov0))) <= 1e-10
    assert np.all(got['var'] >= np.diag(cov0) - 1e-12)
    # the term is no rounding matter on these inputs: a read-out that drops it fails by a wide margin
    assert np.max(got['var'] - np.diag(cov0)) >= 1e-2
    beta, cov_beta = RM.gls(*c['args'], c['x'], c['y'], c['H'], c['var'])
    assert np.allclose(beta, got['beta'], rtol=0, atol=1e-10)
    assert np.allclose(cov_beta, cov_beta.T) and np.all(np.diag(cov_beta) > 0)
