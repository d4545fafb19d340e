"""GPR(fixed_effects=..., fit_objective='reml'): the restricted-likelihood fit, the trend-aware prediction and the estimates of
the fixed effects, on N <= 300 sites.

The data: ai_forms.newton_case('matern15')'s 300 sites and its draw from the model (lengthscales (1.3, 2.0), outputscale 0.9,
noise 0.05) plus a planted trend H beta on GPR's own 'linear' basis, beta = (1.0, 3.0, -2.0).  The 60 sites with the largest
x_0 are held out: a strip at the field's edge, where a constant-mean model falls back to the mean and the trend extrapolates.

* both fit methods increase l_R (Adam: 200 steps at lr 0.1, the command line's defaults -- the statements below are about a
  fitted model); the Newton fit ends by its gradient test; fit_info names the objective;
* the held-out MAE is below the constant-mean model's, the predictive variance at the held-out sites is nowhere below the
  known-mean variance at the same hyper-parameters, and predict's covariance carries the same diagonal;
* fixed_effect_estimates covers the planted beta within 4 standard errors;
* hyper_covariance is the inverse of the restricted likelihood's AI (tests/reml_forms.py) and heritability runs under the
  genotype kernel with REML;
* GPR() without the new arguments gives the same bits before and after fixed effects have been used in the process and on the
  same context.
"""
import functools

import numpy as np
import pytest

import ai_forms as AI
import reml_forms as RM
from algp_amd import utils
from algp_amd.models import GPR

pytestmark = pytest.mark.gpu

BETA = np.array([1.0, 3.0, -2.0])
CAP = 40


@functools.lru_cache(maxsize=None)
def _data():
    c = AI.newton_case('matern15')
    x = np.array(c['x'])
    held = np.argsort(x[:, 0])[-60:]
    train = np.setdiff1d(np.arange(len(x)), held)
    lo, hi = x[train].min(0), x[train].max(0)
    H = np.c_[np.ones(len(x)), (x - 0.5 * (lo + hi)) / (hi - lo)]           # GPR's 'linear' basis, from the train sites
    y = np.array(c['y']) + H @ BETA
    out = dict(x=x, y=y, H=H, train=train, held=held, var=np.array(c['var']), kernel_params=c['kernel_params'])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _theta(gp):
    ls, los, ln, _ = gp.hypers()
    return AI.pack(ls, los, ln)


@functools.lru_cache(maxsize=None)
def _fit(method, fixed='linear', objective='reml'):
    d = _data()
    tr, te = d['train'], d['held']
    gp = GPR(fit_method=method, max_iterations=CAP if method == 'ai' else 200, lr=0.1, kernel_params=d['kernel_params'],
             fixed_effects=fixed, fit_objective=objective)
    try:
        losses = gp.fit(d['x'][tr], d['y'][tr], d['var'][tr])
        out = dict(losses=losses, info=gp.fit_info, theta=_theta(gp), fixed=gp.fixed_effects)
        out['mean'] = gp.predict(d['x'][te])
        mu, var = gp.predict(d['x'][te], return_std=True)
        known = gp.ctx.posterior()[1] + np.exp(out['theta'][-1])          # the same solve, the constant mean taken as known
        mu2, cov = gp.predict(d['x'][te], return_cov=True)
        out.update(mu=mu, var=var, known=known, mu_cov=mu2, cov=cov)
        if fixed is not None:
            out['beta'], out['cov_beta'] = gp.fixed_effect_estimates()
        out['names'], out['hyper_cov'] = gp.hyper_covariance()
        return out
    finally:
        gp.ctx.close()


@pytest.mark.parametrize('method', ['ai', 'adam'])
def test_reml_fit_increases_the_restricted_likelihood(method):
    got = _fit(method)
    print('%s: -l_R/N %.4f -> %.4f in %d evaluations' % (method, got['losses'][0], got['losses'][-1], len(got['losses'])))
    assert got['losses'][-1] < got['losses'][0]
    assert got['info']['objective'] == 'reml'
    if method == 'ai':
        assert got['info']['reason'] == 'gradient' and got['info']['evaluations'] <= CAP
        # the fit's last value is l_R of the forms at its parameters
        d = _data()
        tr = d['train']
        want = RM.reml('single', AI.MF.MATERN15, got['theta'], d['x'][tr], d['y'][tr], d['H'][tr], d['var'][tr])
        assert -got['losses'][-1] * len(tr) == pytest.approx(want, rel=1e-9)


@pytest.mark.parametrize('method', ['ai', 'adam'])
def test_trend_aware_prediction_beats_the_constant_mean(method):
    d = _data()
    got, base = _fit(method), _fit(method, None, 'mll')
    truth = d['y'][d['held']]
    mae, mae0 = utils.compute_mae(truth, got['mu']), utils.compute_mae(truth, base['mu'])
    print('%s: held-out MAE %.4f with the trend, %.4f with the constant mean' % (method, mae, mae0))
    assert mae < mae0
    assert np.all(got['var'] >= got['known']) and np.max(got['var'] - got['known']) > 1e-3
    assert np.array_equal(got['mean'], got['mu']) and np.array_equal(got['mu_cov'], got['mu'])
    assert np.allclose(np.diag(got['cov']), got['var'], rtol=1e-9, atol=1e-12)
    assert np.all(base['var'] == base['known'])                         # without a basis: the known-mean variance itself


def test_estimates_cover_the_planted_effects():
    d = _data()
    got = _fit('ai')
    se = np.sqrt(np.diag(got['cov_beta']))
    shifted = got['beta'] + np.r_[d['y'][d['train']].mean(), 0.0, 0.0]   # the constant mean is part of the intercept
    print('beta %s +- %s (planted %s)' % (shifted, se, BETA))
    assert np.all(np.abs(shifted - BETA) <= 4.0 * se)
    tr = d['train']
    want, want_cov = RM.gls('single', AI.MF.MATERN15, got['theta'], d['x'][tr], d['y'][tr], d['H'][tr], d['var'][tr])
    assert np.allclose(got['beta'], want, rtol=0, atol=1e-8) and AI.relative_error(got['cov_beta'], want_cov) <= 1e-8


def test_hyper_covariance_is_the_inverse_of_the_restricted_ai():
    d = _data()
    got = _fit('ai')
    tr = d['train']
    want = np.linalg.inv(RM.reml_ai('single', AI.MF.MATERN15, got['theta'], d['x'][tr], d['y'][tr], d['H'][tr], d['var'][tr]))
    assert AI.relative_error(got['hyper_cov'], want) <= 1e-6


def test_heritability_runs_under_the_genotype_kernel_with_reml():
    c = AI.newton_case('relationship')
    gp = GPR(fit_method='ai', max_iterations=CAP, kernel_params=c['kernel_params'], fit_objective='reml')
    try:
        assert gp.fixed_effects == 'intercept'                            # REML of the constant mean
        gp.fit(c['x'], c['y'], c['var'])
        assert gp.fit_info['objective'] == 'reml' and gp.fit_info['trace'][-1] > gp.fit_info['trace'][0]
        h2, se = gp.heritability()
        theta = _theta(gp)
        cov = np.linalg.inv(RM.reml_ai(c['family'], c['spec'], theta, c['x'], c['y'], np.ones((len(c['y']), 1)), c['var']))
        want = utils.heritability(theta[2], theta[3], theta[4], float(np.mean(np.diag(c['spec'][1]))), cov[2:, 2:])
        print('REML h2 = %.4f +- %.4f (forms: %.4f +- %.4f)' % (h2, se, want[0], want[1]))
        assert 0.0 < h2 < 1.0 and h2 == pytest.approx(want[0], rel=1e-12) and se == pytest.approx(want[1], rel=1e-6)
    finally:
        gp.ctx.close()


def test_without_the_new_arguments_nothing_changes():
    """The default GPR's fit and predict before fixed effects were ever used in the process, after a model with them has run,
    and on a context that had a basis attached and detached: the same bits."""
    d = _data()
    tr, te = d['train'], d['held']

    def run(gp):
        losses = gp.fit(d['x'][tr], d['y'][tr], d['var'][tr])
        return (np.array(losses), _theta(gp), gp.predict(d['x'][te])) + gp.predict(d['x'][te], return_std=True) + \
            gp.predict(d['x'][te], return_cov=True)

    gp = GPR(max_iterations=12, kernel_params=d['kernel_params'])
    try:
        assert gp.fixed_effects is None and gp.fit_objective == 'mll'
        before = run(gp)
        assert gp.fit_info is None
        _fit('ai')                                                        # fixed effects run on a context of their own
        gp.ctx.set_pool(d['x'])
        gp.ctx.set_fixed_effects(d['H'])                                  # and on this one: attached, used, detached
        gp.ctx.set_train(tr, d['y'][tr], d['var'][tr])
        gp.ctx.reml_step()
        gp.ctx.set_fixed_effects(None)
        for u, v in zip(before, run(gp)):
            assert np.array_equal(u, v)
    finally:
        gp.ctx.close()
    with pytest.raises(ValueError):
        GPR(fit_objective='ml')
    with pytest.raises(ValueError):
        GPR(fixed_effects='quadratic')
