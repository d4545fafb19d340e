"""GPR(fit_method='ai'): the average-information Newton fit on the device against utils.ai_newton driven by tests/ai_forms.py on
the host, on the six N = 300 inputs of ai_forms.newton_case (the four single forms, the additive and the relationship kernel;
data drawn from the model, all parameters start at 0), and what hangs off it: hyper_covariance, hyper_standard_errors,
heritability.

fp64: the fit ends by 'gradient' within 40 evaluations at the host's parameters (1e-5), no lower than the default Adam fit
(200 iterations, lr 0.01) on the same data; hyper_covariance is the inverse of the forms' AI matrix there (1e-6 relative to
sqrt(C_aa C_bb)).  fp32 (RBF and relationship): the loop ends by 'gradient' or 'stalled' within the cap, and every final
parameter lies within 0.1 standard errors (the fp64 run's) of the fp64 run's value: rounding stays an order below the
statistical uncertainty the feature reports.

Measured on an MI355X (fp64; evaluations = device steps, the host loop takes the same number; MLL of the whole train set):

    case          evaluations   max |theta - host|   MLL ai      MLL adam (200 steps)   covariance error
    rbf           15            5.6e-15              -156.64     -193.79                2.5e-15
    matern15      10            6.7e-15              -240.70     -259.65                3.6e-15
    matern05      15            1.6e-14              -326.74     -333.93                3.0e-15
    matern25      11            7.1e-15              -210.23     -234.94                2.9e-15
    additive      11            1.6e-14              -225.68     -250.17                1.8e-14
    relationship  13            8.0e-15              -247.31     -264.47                7.3e-15

fp32: rbf ends 'stalled' after 25 evaluations, |theta32 - theta64| / se = (0.0009, 0.0023, 0.0011, 0.0007); relationship 'stalled'
after 29, at most 2.4e-4 of a standard error (the MLL's own rounding stops the ascent before max|g| / N < 1e-6 is seen).
"""
import functools

import numpy as np
import pytest

import ai_forms as AI
from algp_amd import utils
from algp_amd.models import GPR

pytestmark = pytest.mark.gpu

CAP = 40


def _theta(gp):
    ls, los, ln, _ = gp.hypers()
    return AI.pack(ls, los, ln)


@functools.lru_cache(maxsize=None)
def _fit(name, dtype='float64', method='ai', learn_noise=True):
    """One fit, shared by the tests that look at it: final parameters, fit_info, losses, the final MLL, covariance, heritability."""
    c = AI.newton_case(name)
    gp = GPR(fit_method=method, max_iterations=CAP if method == 'ai' else 200, kernel_params=c['kernel_params'],
             learn_likelihood_noise=learn_noise, dtype=np.dtype(dtype))
    try:
        losses = gp.fit(c['x'], c['y'], c['var'])
        out = dict(theta=_theta(gp), info=gp.fit_info, losses=losses, mll=gp.ctx.fit_step(want_grad=False)[0])
        out['names'], out['cov'] = gp.hyper_covariance()
        out['se'] = gp.hyper_standard_errors()
        if c['family'] == 'relationship':
            out['h2'] = gp.heritability()
        return out
    finally:
        gp.ctx.close()


@pytest.mark.parametrize('name', AI.NEWTON_CASES)
def test_fit_reaches_the_hosts_optimum_and_beats_adam(name):
    c = AI.newton_case(name)
    got = _fit(name)
    want_theta, want_info = AI.newton_host_fit(name)
    info = got['info']
    print('%s: device %d evaluations (%s), host %d; max |theta - host| %.2e' %
          (name, info['evaluations'], info['reason'], want_info['evaluations'], np.max(np.abs(got['theta'] - want_theta))))
    assert info['reason'] == 'gradient' and info['evaluations'] <= CAP
    assert np.max(np.abs(got['theta'] - want_theta)) <= 1e-5
    assert got['losses'] == [-m / AI.NEWTON_N for m in info['trace']] and len(got['losses']) == info['iterations'] + 1
    assert got['mll'] == pytest.approx(info['mll'], rel=1e-12)
    adam = _fit(name, method='adam')
    print('%s: MLL ai %.4f, adam (200 steps) %.4f' % (name, got['mll'], adam['mll']))
    assert adam['info'] is None and len(adam['losses']) == 200
    assert got['mll'] >= adam['mll']


@pytest.mark.parametrize('name', AI.NEWTON_CASES)
def test_hyper_covariance_is_the_inverse_of_the_forms_ai(name):
    c = AI.newton_case(name)
    got = _fit(name)
    want = np.linalg.inv(AI.average_information(c['family'], c['spec'], got['theta'], c['x'], c['y'], c['var']))
    P = len(c['theta_true'])
    assert got['cov'].shape == (P, P) and len(got['names']) == P == len(set(got['names']))
    assert got['names'][-1] == 'likelihood.log_noise' and got['names'][0].endswith('log_lengthscale[0]')
    err = AI.relative_error(got['cov'], want)
    print('%s: covariance error %.2e' % (name, err))
    assert err <= 1e-6
    assert list(got['se']) == got['names']
    assert np.array_equal(np.array(list(got['se'].values())), np.sqrt(np.diag(got['cov'])))
    # after an Adam fit the same call works (at that fit's parameters)
    adam = _fit(name, method='adam')
    want_a = np.linalg.inv(AI.average_information(c['family'], c['spec'], adam['theta'], c['x'], c['y'], c['var']))
    assert AI.relative_error(adam['cov'], want_a) <= 1e-6


def test_heritability_from_the_device_equals_the_forms():
    c = AI.newton_case('relationship')
    got = _fit('relationship')
    theta = got['theta']
    cov = np.linalg.inv(AI.average_information(c['family'], c['spec'], theta, c['x'], c['y'], c['var']))
    gbar = float(np.mean(np.diag(c['spec'][1])))
    want = utils.heritability(theta[2], theta[3], theta[4], gbar, cov[2:, 2:])
    print('h2 = %.4f +- %.4f (forms: %.4f +- %.4f)' % (got['h2'] + want))
    assert got['h2'][0] == pytest.approx(want[0], rel=1e-12) and got['h2'][1] == pytest.approx(want[1], rel=1e-6)
    gp = GPR(kernel_params={'type': 'rbf'})
    gp.reset(c['x'][:, :2], c['y'], c['var'])
    with pytest.raises(ValueError):
        gp.heritability()


@pytest.mark.parametrize('name', ['rbf', 'relationship'])
def test_noise_not_learned_stays_and_drops_out_of_the_covariance(name):
    c = AI.newton_case(name)
    got = _fit(name, learn_noise=False)
    P = len(c['theta_true'])
    assert got['theta'][-1] == 0.0                                      # log_noise keeps its initial value
    assert got['cov'].shape == (P - 1, P - 1) and 'likelihood.log_noise' not in got['names']
    assert got['info']['evaluations'] <= CAP and got['info']['trace'][-1] > got['info']['trace'][0]
    ai = AI.average_information(c['family'], c['spec'], got['theta'], c['x'], c['y'], c['var'])
    assert AI.relative_error(got['cov'], np.linalg.inv(ai[:-1, :-1])) <= 1e-6
    if name == 'relationship':
        gbar = float(np.mean(np.diag(c['spec'][1])))
        want = utils.heritability(got['theta'][2], got['theta'][3], 0.0, gbar, np.linalg.inv(ai[:-1, :-1])[2:, 2:])
        assert got['h2'][1] == pytest.approx(want[1], rel=1e-6)


def test_adam_is_the_default_and_unchanged():
    c = AI.newton_case('matern15')
    fits = []
    for kw in ({}, {'fit_method': 'adam'}):
        gp = GPR(max_iterations=12, kernel_params=c['kernel_params'], **kw)
        try:
            fits.append((gp.fit(c['x'], c['y'], c['var']), _theta(gp)))
            assert gp.fit_method == 'adam' and gp.fit_info is None
        finally:
            gp.ctx.close()
    assert fits[0][0] == fits[1][0] and np.array_equal(fits[0][1], fits[1][1]) and len(fits[0][0]) == 12
    with pytest.raises(ValueError):
        GPR(fit_method='newton')


@pytest.mark.parametrize('name', ['rbf', 'relationship'])
def test_fp32_fit_stays_within_a_tenth_of_a_standard_error(name):
    ref = _fit(name)
    got = _fit(name, dtype='float32')
    info = got['info']
    se = np.sqrt(np.diag(ref['cov']))
    dist = np.abs(got['theta'] - ref['theta']) / se
    print('%s fp32: %d evaluations (%s), |theta32 - theta64| / se = %s' % (name, info['evaluations'], info['reason'], np.array2string(dist, precision=4)))
    assert info['reason'] in ('gradient', 'stalled') and info['evaluations'] <= CAP
    assert np.max(dist) <= 0.1
