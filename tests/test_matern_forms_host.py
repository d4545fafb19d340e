"""The closed forms of tests/matern_forms.py (what the GPU tests of the Matern family compare against) checked on the CPU against
the general Matern form, the oracle's Matern-3/2 and central differences of their own MLL; and the host plumbing of the two new
forms: GPR's kernel_params['nu'] and --matern_nu."""
import numpy as np
import pytest
from scipy.special import gamma, kv

import matern_forms as MF
from oracle import gp_oracle as O


@pytest.mark.parametrize('kid', [MF.MATERN05, MF.MATERN15, MF.MATERN25])
def test_closed_forms_equal_the_general_matern(kid):
    nu = MF.NU[kid]
    rng = np.random.RandomState(7)
    r = 20.0 * (1.0 - rng.uniform(0, 1, 200))                # (0, 20]
    z = np.sqrt(2 * nu) * r
    want = 2.0 ** (1 - nu) / gamma(nu) * z ** nu * kv(nu, z)
    got = MF.k_of_r(kid, r)
    assert np.max(np.abs(got - want) / want) < 1e-12
    assert MF.k_of_r(kid, 0.0) == 1.0
    x = np.array([[1.5, -2.0], [1.5, -2.0]])
    K = MF.kernel_matrix(kid, np.log([0.7, 1.9]), np.log(1.7), x)
    assert np.all(K == np.exp(np.log(1.7)))


def test_matern15_equals_the_oracle():
    rng = np.random.RandomState(1)
    x1, x2 = rng.uniform(0, 10, (50, 3)), rng.uniform(0, 10, (31, 3))
    ls = np.log([1.3, 2.1, 0.8])
    hyp = O.Hypers(ls, np.log(0.9), np.log(0.05), O.KERNEL_MATERN15)
    assert np.max(np.abs(MF.kernel_matrix(MF.MATERN15, ls, np.log(0.9), x1, x2) - O.kernel_matrix(hyp, x1, x2))) < 1e-14
    assert np.max(np.abs(MF.kernel_matrix(MF.MATERN15, ls, np.log(0.9), x1) - O.kernel_matrix(hyp, x1))) < 1e-14
    hyp0 = O.Hypers(ls, np.log(0.9), np.log(0.05), O.KERNEL_RBF)
    assert np.max(np.abs(MF.kernel_matrix(MF.RBF, ls, np.log(0.9), x1, x2) - O.kernel_matrix(hyp0, x1, x2))) < 1e-14


@pytest.mark.parametrize('kid', [MF.RBF, MF.MATERN15, MF.MATERN05, MF.MATERN25])
def test_gradient_equals_central_differences_of_the_mll(kid):
    """N = 40, D = 3, one site listed twice: rows 5 and 33 are the same point (r = 0 off the diagonal, sigma_n^2 in their
    cross entry)."""
    rng = np.random.RandomState(11)
    N, D = 40, 3
    x = rng.uniform(0, 6, (N, D))
    x[33] = x[5]
    sites = np.arange(N)
    sites[33] = 5
    y = np.sin(x[:, 0]) + 0.1 * rng.standard_normal(N)
    var = rng.uniform(0.005, 0.05, N)
    theta = np.r_[np.log([1.3, 2.1, 0.8]), np.log(0.9), np.log(0.05)]

    def f(t):
        return MF.mll(kid, t[:D], t[D], t[D + 1], x, y, var, sites)

    g = MF.mll_grad(kid, theta[:D], theta[D], theta[D + 1], x, y, var, sites)
    assert np.all(np.isfinite(g))
    eps = 1e-5
    for k in range(D + 2):
        e = np.zeros(D + 2)
        e[k] = eps
        fd = (f(theta + e) - f(theta - e)) / (2 * eps)
        assert abs(fd - g[k]) <= 1e-6 * abs(fd), (k, fd, g[k])


def test_oracle_gradient_agrees_where_the_oracle_knows_the_kernel():
    rng = np.random.RandomState(3)
    x = rng.uniform(0, 6, (30, 2))
    y, var = rng.standard_normal(30), rng.uniform(0.01, 0.05, 30)
    for kid in (O.KERNEL_RBF, O.KERNEL_MATERN15):
        hyp = O.Hypers(np.log([1.3, 2.1]), np.log(0.9), np.log(0.05), kid)
        f0, go = O.mll_and_grad(hyp, x, y, var)
        assert MF.mll(kid, hyp.log_lengthscale, hyp.log_outputscale, hyp.log_noise, x, y, var) == pytest.approx(30 * f0, rel=1e-12)
        want = 30 * np.r_[go['log_lengthscale'], go['log_outputscale'], go['log_noise']]
        assert np.allclose(MF.mll_grad(kid, hyp.log_lengthscale, hyp.log_outputscale, hyp.log_noise, x, y, var), want, rtol=1e-10, atol=1e-12)


def test_gpr_and_arguments_plumbing():
    from algp_amd import _hip
    from algp_amd.arguments import get_args
    from algp_amd.models import GPR
    assert (_hip.KERNEL_RBF, _hip.KERNEL_MATERN15, _hip.KERNEL_MATERN05, _hip.KERNEL_MATERN25) == (0, 1, 2, 3)
    x = np.zeros((4, 2))

    def kid(params):
        gp = GPR(kernel_params=params)
        gp.reset(x, np.zeros(4), None)
        return gp.hypers()[3]

    assert kid({'type': 'matern', 'nu': 0.5}) == 2
    assert kid({'type': 'matern', 'nu': 1.5}) == 1
    assert kid({'type': 'matern', 'nu': 2.5}) == 3
    assert kid({'type': 'matern'}) == 1                      # no nu: Matern-3/2, as before
    assert kid({'type': 'rbf', 'nu': 2.5}) == 0              # nu is ignored for rbf
    assert kid({'type': 'rbf', 'nu': 3.5}) == 0
    with pytest.raises(NotImplementedError, match='0.5, 1.5, 2.5'):
        kid({'type': 'matern', 'nu': 3.5})
    with pytest.raises(NotImplementedError):
        kid({'type': 'spectral_mixture'})
    assert get_args([]).matern_nu == 1.5
    assert get_args(['--matern_nu', '2.5']).matern_nu == 2.5
    with pytest.raises(SystemExit):
        get_args(['--matern_nu', '3.5'])


def test_agent_passes_matern_nu_on():
    import types
    from algp_amd.agent import Agent
    a = Agent.__new__(Agent)
    a.learn_likelihood_noise = True
    args = types.SimpleNamespace(latent=None, lr=.1, max_iterations=1, kernel='matern', matern_nu=2.5)
    a._init_model(args)
    assert a.gp.kernel_params == {'type': 'matern', 'nu': 2.5}
    del args.matern_nu                                       # argument objects built by hand, without the new flag
    a._init_model(args)
    assert a.gp.kernel_params == {'type': 'matern', 'nu': 1.5}


def test_every_train_matrix_of_the_gpu_tests_factors_in_fp32():
    """The problems of tests/test_matern_family.py are built by functions that need no device.  Every train matrix S among them,
    rounded to fp32 and factored by NumPy's fp32 Cholesky, meets no non-positive pivot: the fp32 cases of that file cannot
    fail for conditioning.  GPR.fit's matrices are checked along a fit run here with the helper's own gradient."""
    import torch
    import test_matern_family as T
    for kid in T.KIDS:
        assert MF.factors_in_fp32(T.pool_problem(kid).S)
        q = T.fused_problem(kid)
        assert MF.factors_in_fp32(MF.train_matrix(kid, T.LOG_LS, T.LOG_OS, T.LOG_NOISE, q.pool[q.A], q.var))
        assert MF.factors_in_fp32(T.mid_problem(kid).S)
    for prm in T.MLL_CASES:
        assert MF.factors_in_fp32(T.mll_problem(*prm.values).S)
    x, y, var = T.fit_problem()
    th = torch.zeros(4, dtype=torch.float64)
    opt = torch.optim.Adam([th], lr=.1)
    losses = []
    for i in range(30):
        v = th.numpy().copy()
        assert MF.factors_in_fp32(MF.train_matrix(MF.MATERN25, v[:2], v[2], v[3], x, var))
        losses.append(-MF.mll(MF.MATERN25, v[:2], v[2], v[3], x, y, var) / len(y))
        th.grad = torch.from_numpy(-MF.mll_grad(MF.MATERN25, v[:2], v[2], v[3], x, y, var) / len(y))
        opt.step()
    assert losses[-1] < losses[0]
