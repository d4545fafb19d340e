"""CPU checks of what tests/test_pathwise_samples.py relies on: the reference formula of tests/pathwise_forms.py has the
posterior's moments exactly, utils.spectral_draws draws from the kernels' spectral densities, and every train matrix of the GPU
cases factors in fp32-rounded NumPy (the check tests/test_matern_forms_host.py makes for its problems)."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import matern_forms as MF                            # noqa: E402
import pathwise_forms as PF                          # noqa: E402
from algp_amd import utils                           # noqa: E402

kernels = pytest.mark.parametrize('kid', PF.KIDS, ids=PF.KNAMES)


@kernels
def test_reference_formula_has_the_posterior_moments(kid):
    """Values mode with g = L_pool xi: (xi, eps) -> f is linear, f = mu + A xi + B eps.  A A^T + B B^T must be the posterior
    covariance K_XX - K_XA S^-1 K_AX and mu the posterior mean, to 1e-8 absolute (os = 1; observed 2e-10): this pins the sign
    and the sqrt(v) scaling of the noise term without any statistics."""
    p = PF.grid_problem()
    n, N = len(p.X), len(p.A)
    K = MF.kernel_matrix(kid, p.log_ls, p.log_os, p.X)
    Lp = np.linalg.cholesky(K + 1e-10 * np.eye(n))
    zero = PF.problem_draws(p, kid, 0, 1, eps=np.zeros((1, N)), prior=np.zeros((1, n)))
    A = (PF.problem_draws(p, kid, 0, n, eps=np.zeros((n, N)), prior=Lp.T) - zero).T          # column k: the image of xi = e_k
    B = (PF.problem_draws(p, kid, 0, N, eps=np.eye(N), prior=np.zeros((N, n))) - zero).T
    S = PF.train_matrix(p, kid)
    K_XA = K[np.ix_(p.cand, p.A)]
    cov = K[np.ix_(p.cand, p.cand)] - K_XA @ np.linalg.solve(S, K_XA.T)
    err = float(np.max(np.abs(A @ A.T + B @ B.T - cov)))
    mu = MF.posterior(kid, p.log_ls, p.log_os, p.log_noise, p.X[p.A], p.y, p.var, p.X[p.cand])[0]
    err_mu = float(np.max(np.abs(zero[0] - mu)))
    print('kernel %d: covariance %.3g mean %.3g' % (kid, err, err_mu))
    assert err <= 1e-8 and err_mu <= 1e-8


@kernels
def test_spectral_draws(kid):
    """Phi Phi^T of F = 20 000 draws against k on the first 60 grid sites scaled by the lengthscale: every entry is a mean of F
    independent terms of variance <= 1.5 os^2 (over the phase, E[4 cos^2(a + phi) cos^2(b + phi)] = 1 + cos(2 (a - b)) / 2), so
    6 os sqrt(1.5 / F) = 0.052 is six standard deviations (observed 0.015 .. 0.025).  Shapes, dtype, determinism."""
    p = PF.grid_problem()
    F = 20000
    om, ph = utils.spectral_draws(kid, 2, F, 1)
    assert om.shape == (F, 2) and ph.shape == (F,) and om.dtype == np.float64 and ph.dtype == np.float64
    assert np.all(ph >= 0) and np.all(ph < 2 * np.pi)
    om2, ph2 = utils.spectral_draws(kid, 2, F, np.random.RandomState(1))
    assert np.array_equal(om, om2) and np.array_equal(ph, ph2)
    om3, _ = utils.spectral_draws(kid, 2, F, 2)
    assert not np.array_equal(om, om3)
    xs = p.X[:60] * np.exp(-p.log_ls)[None, :]
    Phi = PF.features(om, ph, xs, 1.0)
    err = float(np.max(np.abs(Phi @ Phi.T - PF.spectral_target(kid, xs))))
    print('kernel %d: max |Phi Phi^T - K| = %.4f' % (kid, err))
    assert err <= 6.0 * np.sqrt(1.5 / F)


def test_spectral_draws_widths():
    om, ph = utils.spectral_draws(MF.MATERN05, 5, 7, 3)
    assert om.shape == (7, 5) and ph.shape == (7,)
    with pytest.raises(NotImplementedError):
        utils.spectral_draws(9, 2, 4, 0)


def test_gpu_problems_factor_in_fp32():
    for p, kid in PF.all_problems():
        assert MF.factors_in_fp32(PF.train_matrix(p, kid)), (p.D, kid)
        assert len(p.A) == 200 and len(p.cand) == 300 and len(np.intersect1d(p.cand, p.A)) == 10
