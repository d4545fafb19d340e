"""tests/ai_forms.py against itself by independent routes, and utils.ai_newton / utils.heritability on the host (no GPU).

* average_information (Cholesky route) equals the explicit-inverse form 1/2 alpha' dS_a S^-1 dS_b alpha;
* the linear-parameter identity: the dS of the outputscales and the noise sum to S - diag(var), so
  sum_{a linear} AI_ab = 1/2 (alpha - S^-1 (var o alpha))' dS_b alpha for every b;
* each dS_a equals a central difference of train_matrix in theta_a;
* ai_newton driven by the forms from theta = 0 on the six N = 300 inputs of ai_forms.newton_case ends by 'gradient' within 40
  evaluations.  Evaluations seen here: rbf 15, matern15 10, matern05 15, matern25 11, additive 11, relationship 13 (40 is a
  cap that keeps a broken loop from passing, not a measurement);
* heritability: the value, its derivative vector against central differences, the marginal block of the whole inverse.
"""
import numpy as np
import pytest

import ai_forms as AI
import matern_forms as MF
import relationship_forms as RF
from algp_amd import utils

MODELS = {
    'rbf': ('single', MF.RBF), 'matern15': ('single', MF.MATERN15), 'matern05': ('single', MF.MATERN05), 'matern25': ('single', MF.MATERN25),
    'additive': ('additive', (MF.MATERN15, MF.RBF, 2)),
    'additive_1of4': ('additive', (MF.RBF, MF.MATERN25, 1)),
    'relationship': ('relationship', (MF.MATERN15, RF.marker_relationship(), 12)),
    'relationship_identity': ('relationship', (MF.RBF, None, 12)),
}


def _inputs(name, N=60):
    """A small case with a site listed three times (rows 3, 17, 40), per-point noise and every parameter different."""
    family, spec = MODELS[name]
    rng = np.random.RandomState(7)
    D = 2 if family == 'single' else 3 if family == 'relationship' or spec[2] == 2 else 4
    x = rng.uniform(0, 6.0, (N, D))
    if family == 'relationship':
        x[:, -1] = rng.randint(0, 12, N)
    sites = np.arange(N)
    sites[17] = sites[40] = 3
    x[17] = x[40] = x[3]
    nl = AI.n_lengthscales(family, x)
    nos = 1 if family == 'single' else 2
    theta = np.r_[np.log(rng.uniform(0.8, 2.1, nl)), np.log(rng.uniform(0.5, 1.2, nos)), np.log(0.07)]
    y = np.sin(x[:, 0]) + 0.1 * rng.standard_normal(N)
    var = rng.uniform(0.005, 0.05, N)
    return family, spec, theta, x, y, var, sites


@pytest.mark.parametrize('name', sorted(MODELS))
def test_cholesky_route_equals_the_explicit_inverse(name):
    family, spec, theta, x, y, var, sites = _inputs(name)
    ai = AI.average_information(family, spec, theta, x, y, var, sites)
    S, _, alpha = AI.alpha_of(family, spec, theta, x, y, var, sites)
    Sinv = np.linalg.inv(S)
    dS = AI.derivative_matrices(family, spec, theta, x, sites)
    assert len(dS) == len(theta)
    want = np.array([[0.5 * alpha @ a @ Sinv @ b @ alpha for b in dS] for a in dS])
    assert AI.relative_error(ai, want) <= 1e-10
    assert np.linalg.eigvalsh(ai)[0] >= -1e-12 * np.linalg.eigvalsh(ai)[-1]


@pytest.mark.parametrize('name', sorted(MODELS))
def test_linear_parameters_sum_to_s_minus_var(name):
    family, spec, theta, x, y, var, sites = _inputs(name)
    ai = AI.average_information(family, spec, theta, x, y, var, sites)
    S, L, alpha = AI.alpha_of(family, spec, theta, x, y, var, sites)
    dS = AI.derivative_matrices(family, spec, theta, x, sites)
    nl = AI.n_lengthscales(family, x)
    assert np.max(np.abs(sum(dS[nl:]) - (S - np.diag(var)))) <= 1e-13 * np.max(np.abs(S))
    w = alpha - np.linalg.solve(S, var * alpha)
    want = np.array([0.5 * w @ b @ alpha for b in dS])
    got = ai[nl:].sum(axis=0)
    scale = np.sqrt(np.diag(ai)) * np.sqrt(np.diag(ai)[nl:]).sum()
    assert np.max(np.abs(got - want) / scale) <= 1e-10


@pytest.mark.parametrize('name', sorted(MODELS))
def test_derivative_matrices_equal_central_differences(name):
    family, spec, theta, x, y, var, sites = _inputs(name)
    dS = AI.derivative_matrices(family, spec, theta, x, sites)
    h = 1e-6
    for a in range(len(theta)):
        e = np.zeros(len(theta))
        e[a] = h
        fd = (AI.train_matrix(family, spec, theta + e, x, var, sites) - AI.train_matrix(family, spec, theta - e, x, var, sites)) / (2 * h)
        assert np.max(np.abs(fd - dS[a])) <= 1e-7 * np.max(np.abs(dS[a])), (name, a)


@pytest.mark.parametrize('name', AI.NEWTON_CASES)
def test_ai_newton_converges_from_zero(name):
    c = AI.newton_case(name)
    theta, info = AI.newton_host_fit(name)
    print('%s: %d evaluations, %d accepted, mll %.4f, reason %s' % (name, info['evaluations'], info['iterations'], info['mll'], info['reason']))
    assert info['reason'] == 'gradient' and info['evaluations'] <= 40
    assert info['grad_max'] < 1e-6 and len(info['trace']) == info['iterations'] + 1
    assert all(b > a for a, b in zip(info['trace'], info['trace'][1:]))
    f, g = AI.mll_and_grad(c['family'], c['spec'], theta, c['x'], c['y'], c['var'])
    assert f == info['mll'] and np.max(np.abs(g)) / AI.NEWTON_N < 1e-6
    assert f >= AI.mll_and_grad(c['family'], c['spec'], c['theta_true'], c['x'], c['y'], c['var'])[0]


def test_ai_newton_leaves_a_fixed_entry_untouched():
    """The noise held at 0.03 (not its estimate): the other three converge, its entry keeps its bits and its gradient stays."""
    c = AI.newton_case('rbf')
    theta0 = np.r_[0.0, 0.0, 0.0, np.log(0.03)]
    theta, info = utils.ai_newton(theta0, lambda t: AI.mll_and_grad(c['family'], c['spec'], t, c['x'], c['y'], c['var']),
                                  lambda t: AI.average_information(c['family'], c['spec'], t, c['x'], c['y'], c['var']),
                                  free=[0, 1, 2], max_evaluations=40, n=AI.NEWTON_N)
    assert theta[-1] == theta0[-1] and info['reason'] == 'gradient' and info['evaluations'] <= 40
    g = AI.mll_and_grad(c['family'], c['spec'], theta, c['x'], c['y'], c['var'])[1]
    assert np.max(np.abs(g[:-1])) / AI.NEWTON_N < 1e-6 and abs(g[-1]) / AI.NEWTON_N > 1e-6
    # a mask selects the same entries
    theta_m, _ = utils.ai_newton(theta0, lambda t: AI.mll_and_grad(c['family'], c['spec'], t, c['x'], c['y'], c['var']),
                                 lambda t: AI.average_information(c['family'], c['spec'], t, c['x'], c['y'], c['var']),
                                 free=np.array([True, True, True, False]), max_evaluations=40, n=AI.NEWTON_N)
    assert np.array_equal(theta_m, theta)


def test_ai_newton_takes_a_raising_trial_as_a_rejection():
    c = AI.newton_case('rbf')
    calls = []

    def vg(t):
        calls.append(t.copy())
        if len(calls) == 2:                               # the first trial
            raise np.linalg.LinAlgError('not positive definite')
        return AI.mll_and_grad(c['family'], c['spec'], t, c['x'], c['y'], c['var'])

    theta, info = utils.ai_newton(np.zeros(4), vg, lambda t: AI.average_information(c['family'], c['spec'], t, c['x'], c['y'], c['var']),
                                  max_evaluations=40, n=AI.NEWTON_N)
    assert info['reason'] == 'gradient' and info['evaluations'] == len(calls) <= 40
    assert np.array_equal(calls[0], np.zeros(4)) and not np.array_equal(calls[2], calls[1])   # retried from the same point, damped more
    assert np.max(np.abs(theta - AI.newton_host_fit('rbf')[0])) < 1e-4
    nan_first = iter([True])

    def vg_nan(t):
        f, g = AI.mll_and_grad(c['family'], c['spec'], t, c['x'], c['y'], c['var'])
        return (np.nan if np.any(t != 0) and next(nan_first, False) else f), g

    _, info2 = utils.ai_newton(np.zeros(4), vg_nan, lambda t: AI.average_information(c['family'], c['spec'], t, c['x'], c['y'], c['var']),
                               max_evaluations=40, n=AI.NEWTON_N)
    assert info2['reason'] == 'gradient'
    with pytest.raises(RuntimeError):                     # any other error propagates
        utils.ai_newton(np.zeros(4), lambda t: (_ for _ in ()).throw(RuntimeError('boom')), lambda t: np.eye(4))


def test_ai_newton_exits():
    c = AI.newton_case('rbf')
    vg = lambda t: AI.mll_and_grad(c['family'], c['spec'], t, c['x'], c['y'], c['var'])
    info_of = lambda t: AI.average_information(c['family'], c['spec'], t, c['x'], c['y'], c['var'])
    _, info = utils.ai_newton(np.zeros(4), vg, info_of, max_evaluations=3, n=AI.NEWTON_N)
    assert info['reason'] == 'max_evaluations' and info['evaluations'] == 3
    # an objective that never improves: lambda climbs past 1e8
    _, info = utils.ai_newton(np.zeros(2), lambda t: (0.0, np.ones(2)), lambda t: np.eye(2), max_evaluations=60)
    assert info['reason'] == 'stalled' and info['iterations'] == 0 and info['damping'] > 1e8


def test_heritability_value_gradient_and_marginal_block():
    la, lg, ln, gbar = np.log(0.6), np.log(0.8), np.log(0.1), 1.37
    rng = np.random.RandomState(3)
    B = rng.standard_normal((5, 5))
    info = B @ B.T + 5 * np.eye(5)                       # a 5 x 5 information matrix with cross terms everywhere
    cov = np.linalg.inv(info)
    C = cov[2:, 2:]                                      # the marginal covariance of the last three parameters
    h2, se = utils.heritability(la, lg, ln, gbar, C)
    assert h2 == pytest.approx(gbar * 0.8 / (gbar * 0.8 + 0.6 + 0.1), rel=1e-14)
    f = lambda p: utils.heritability(p[0], p[1], p[2], gbar, C)[0]
    p0, h = np.array([la, lg, ln]), 1e-6
    d = np.array([(f(p0 + h * e) - f(p0 - h * e)) / (2 * h) for e in np.eye(3)])
    tot = gbar * 0.8 + 0.6 + 0.1
    want_d = np.array([-h2 * 0.6 / tot, h2 * (1 - h2), -h2 * 0.1 / tot])
    assert np.max(np.abs(d - want_d)) < 1e-9
    assert se == pytest.approx(np.sqrt(want_d @ C @ want_d), rel=1e-12)
    # the inverse of the block is another matrix and gives another (smaller) standard error
    se_block = utils.heritability(la, lg, ln, gbar, np.linalg.inv(info[2:, 2:]))[1]
    assert se_block < se and abs(se_block - se) > 1e-3 * se
    # the noise not learned: its entry drops
    h2b, se2 = utils.heritability(la, lg, ln, gbar, C[:2, :2])
    assert h2b == h2 and se2 == pytest.approx(np.sqrt(want_d[:2] @ C[:2, :2] @ want_d[:2]), rel=1e-12)
    with pytest.raises(ValueError):
        utils.heritability(la, lg, ln, gbar, np.eye(4))
