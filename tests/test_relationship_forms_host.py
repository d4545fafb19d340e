"""CPU checks behind tests/test_relationship_kernel.py: the NumPy helper tests/relationship_forms.py is held to central differences
and to the dense joint Gaussian; every train matrix the GPU tests build factors in fp32-rounded NumPy; the reference runs whose
picks are compared are separated by more than the bound of tests/test_greedy_regimes.py:54; and the Python plumbing that needs
no device (GPR's parameters, the command-line flags, the host-side prior draw of the posterior samples).  No GPU.
"""
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import matern_forms as MF                            # noqa: E402
import relationship_forms as RL                      # noqa: E402
import test_relationship_kernel as TR                # noqa: E402
import test_variance_reduction as VR                 # noqa: E402

ALL4 = [MF.RBF, MF.MATERN15, MF.MATERN05, MF.MATERN25]


def _problem(ka, G, Q=6, N=40, D=3, seed=4):
    rng = np.random.RandomState(seed)
    x = np.column_stack([rng.uniform(0, 5, (N, D - 1)), rng.randint(Q, size=N)])
    y = np.sin(x[:, 0]) + rng.standard_normal(Q)[x[:, -1].astype(int)] + 0.1 * rng.standard_normal(N)
    var = rng.uniform(0.01, 0.05, N)
    return (ka, G, Q), x, y, var


@pytest.mark.parametrize('ka', ALL4)
@pytest.mark.parametrize('with_table', [False, True], ids=['identity', 'marker'])
def test_gradient_against_central_differences(ka, with_table):
    spec, x, y, var = _problem(ka, RL.marker_relationship(6, 20) if with_table else None)
    idx = np.arange(len(x))
    idx[7] = 3                                                                  # a site listed twice
    x = x[idx]
    th = np.r_[np.log([1.4, 2.2]), np.log(0.8), np.log(0.6), np.log(0.05)]

    def f(t):
        return RL.mll(spec, t[:2], (t[2], t[3]), t[4], x, y, var, idx)
    g = RL.mll_grad(spec, th[:2], (th[2], th[3]), th[4], x, y, var, idx)
    assert g.shape == (5,)
    h = 1e-5
    for k in range(5):
        e = np.zeros(5)
        e[k] = h
        num = (f(th + e) - f(th - e)) / (2 * h)
        assert abs(num - g[k]) <= 1e-6 * max(1.0, abs(g[k])), (k, num, g[k])


@pytest.mark.parametrize('with_table', [False, True], ids=['identity', 'marker'])
def test_genotype_posterior_against_the_joint_gaussian(with_table):
    """(u, y) is jointly Gaussian with covariance [[os_g G, B], [B^T, S]] of size Q + N: conditioning it densely gives the helper's
    mean and covariance."""
    Q = 6
    spec, x, y, var = _problem(MF.MATERN15, RL.marker_relationship(Q, 20) if with_table else None, Q=Q)
    x[x[:, -1] == Q - 1, -1] = 0                                                # the last genotype on no plot
    ls, los, ln = np.log([1.4, 2.2]), (np.log(0.8), np.log(0.6)), np.log(0.05)
    mean, cov = RL.genotype_posterior(spec, ls, los, ln, x, y, var)
    # the joint covariance from the kernel itself: pseudo-sites (any position, id q) for u -- only their genotype part
    ids = x[:, -1].astype(int)
    Gd = RL.table(spec)
    J = np.zeros((Q + len(x), Q + len(x)))
    J[:Q, :Q] = np.exp(los[1]) * Gd
    J[:Q, Q:] = np.exp(los[1]) * Gd[:, ids]
    J[Q:, :Q] = J[:Q, Q:].T
    J[Q:, Q:] = RL.train_matrix(spec, ls, los, ln, x, var)
    assert np.min(np.linalg.eigvalsh(J)) > -1e-10
    P = np.linalg.inv(J + 1e-12 * np.eye(len(J)))                               # precision of (u, y): cov(u | y) = inv(P_uu)
    cov_j = np.linalg.inv(P[:Q, :Q])
    mean_j = -cov_j @ P[:Q, Q:] @ (y - y.mean())
    assert np.max(np.abs(cov - cov_j)) < 1e-7 and np.max(np.abs(mean - mean_j)) < 1e-7
    if not with_table:
        assert mean[Q - 1] == 0 and cov[Q - 1, Q - 1] == np.exp(los[1])
    else:
        assert abs(mean[Q - 1]) > 1e-4
    # the components: 0 + 1 + ybar is the posterior mean, component 1 is the genotype posterior's mean by id
    mu, _ = RL.posterior(spec, ls, los, ln, x, y, var, x[:9])
    ma, mg = RL.component_means(spec, ls, los, ln, x, y, var, x[:9])
    assert np.max(np.abs(ma + mg + y.mean() - mu)) < 1e-12
    assert np.max(np.abs(mg - mean[ids[:9]])) < 1e-10


def _factors_in_fp32(S):
    L = np.linalg.cholesky(np.asarray(S, np.float64).astype(np.float32))
    return bool(np.all(np.isfinite(L)) and np.min(np.diag(L)) > 0)


def test_every_train_matrix_of_the_gpu_tests_factors_in_fp32():
    for tab in TR.TABLES:
        assert _factors_in_fp32(TR.pool_problem(tab).S), tab
        assert _factors_in_fp32(TR.mid_problem(tab).S), tab
        for D in TR.MLL_D:
            for N, twice in TR.MLL_N:
                assert _factors_in_fp32(TR.mll_problem(tab, D, N, twice).S), (tab, D, N, twice)
    for tab in ('identity', 'marker'):
        for Q, N in TR.GP_SHAPES:
            assert _factors_in_fp32(TR.genotype_problem(tab, Q, N).S), (tab, Q, N)
    q = TR.fit_problem()
    spec = (MF.MATERN15, None, 10)
    assert _factors_in_fp32(RL.train_matrix(spec, np.zeros(2), (0.0, 0.0), 0.0, q.x, q.var))
    # the marker tables are positive definite and hold fp32 values, bitwise symmetric
    for Q, m in ((12, 40), (130, 394)):
        G = RL.marker_relationship(Q, m, seed=7 if Q == 130 else 5)
        assert np.array_equal(G, G.T) and np.array_equal(G, G.astype(np.float32)) and np.min(np.linalg.eigvalsh(G)) > 1e-3
        assert np.ptp(np.diag(G)) > 0.05


@pytest.mark.parametrize('tab', TR.TABLES)
def test_reference_picks_are_separated(tab):
    """Every reference run whose picks tests/test_relationship_kernel.py compares: top-two gaps above tests/test_greedy_regimes.py:54
    in both precisions (entropy), above twice the MI tolerance in fp64, above twice the variance-reduction tolerance."""
    p = TR.pool_problem(tab)
    _, ut = TR.entropy_reference(p)
    print('%s entropy gap %.3g' % (tab, TR._top_gap(ut)))
    assert TR._top_gap(ut) > TR.GAP[np.dtype(np.float32)]
    _, utm = TR.mi_reference(p)
    scale = max(float(np.max(np.abs(r[np.isfinite(r)]))) for r in utm)
    print('%s MI gap %.3g of %.3g' % (tab, TR._top_gap(utm), scale))
    assert TR._top_gap(utm) > 2 * 1e-7 * scale
    _, U = TR.vr_reference(p)
    for r in range(3):
        top = np.sort(U[r][np.isfinite(U[r])])[-2:]
        print('%s vr round %d gap %.3g' % (tab, r, (top[1] - top[0]) / top[1]))
        assert (top[1] - top[0]) / top[1] > 2 * VR.TOL[np.float32]


def test_fp32_error_of_the_reference_genotype_posterior():
    """The measured basis of GP_BAR in tests/test_relationship_kernel.py: the helper's own fp32-rounded evaluation stays well inside
    the margin tests/test_group_posterior.py:37 allows (1e-3 of the largest entry in fp32)."""
    worst = 0.0
    for tab in ('identity', 'marker'):
        for Q, N in TR.GP_SHAPES:
            q = TR.genotype_problem(tab, Q, N)
            m32, c32 = TR.genotype_posterior_f32(q)
            e = float(np.max(np.abs(c32 - q.cov)) / np.max(np.abs(q.cov)))
            print('%s Q=%d N=%d: fp32 NumPy cov error %.3g of max|cov|, mean error %.3g' % (tab, Q, N, e, float(np.max(np.abs(m32 - q.mean)))))
            worst = max(worst, e)
    assert worst < 1e-5 < TR.GP_BAR[np.dtype(np.float32)]


def test_gpr_builds_the_named_parameters():
    from algp_amd.models import GPR
    G = RL.marker_relationship(5, 12)
    x = np.column_stack([np.random.RandomState(0).uniform(0, 4, (9, 2)), np.arange(9) % 5])
    for rel, nq in ((G, None), (None, 5)):
        gp = GPR(kernel_params={'type': 'genotype', 'spatial': {'type': 'matern', 'nu': 2.5}, 'relationship': rel, 'n_genotypes': nq})
        gp.reset(x, np.zeros(9), np.full(9, 0.1))
        named = dict(gp.model.named_parameters())
        assert tuple(named['kernel_covar_module.kernels.0.base_kernel.log_lengthscale'].shape) == (1, 1, 2)
        assert tuple(named['kernel_covar_module.kernels.0.log_outputscale'].shape) == (1,)
        assert tuple(named['kernel_covar_module.kernels.1.log_outputscale'].shape) == (1,)
        assert 'likelihood.log_noise' in named and len(named) == 4
        ls, los, ln, kt = gp.hypers()
        assert ls.shape == (2,) and len(los) == 2 and kt[0] == 'genotype' and kt[1] == MF.MATERN25
        assert gp.model.relationship[1] == 5
        state = gp.model.state_dict()
        gp.model.load_state_dict(state)
    with pytest.raises(ValueError):
        GPR(kernel_params={'type': 'genotype', 'spatial': {'type': 'rbf'}}).reset(x, np.zeros(9), np.full(9, 0.1))
    with pytest.raises(NotImplementedError):
        GPR(kernel_params={'type': 'genotype', 'spatial': {'type': 'spectral_mixture'}, 'n_genotypes': 5}).reset(x, np.zeros(9), np.full(9, 0.1))
    with pytest.raises(NotImplementedError):
        GPR(kernel_params={'type': 'spectral_mixture'}).reset(x, np.zeros(9), np.full(9, 0.1))
    with pytest.raises(ValueError):
        GPR(kernel_params={'type': 'rbf'}).genotype_effects()


def test_argument_parsing(tmp_path):
    from algp_amd.arguments import get_args
    a = get_args(['--kernel', 'genotype'])
    assert a.kernel == 'genotype' and a.relationship is None and a.kernel_a == 'matern' and a.matern_nu == 1.5
    path = str(tmp_path / 'G.npy')
    np.save(path, RL.marker_relationship(4, 9))
    a = get_args(['--kernel', 'genotype', '--relationship', path, '--kernel_a', 'rbf'])
    assert a.relationship == path and a.kernel_a == 'rbf'
    # the agent turns the flags into the model's description without touching a device
    from algp_amd.agent import Agent
    ag = Agent.__new__(Agent)
    ag.learn_likelihood_noise = True
    ag.env = types.SimpleNamespace(num_genotypes=12)
    ag._init_model(a)
    kp = ag.gp.kernel_params
    assert kp['type'] == 'genotype' and kp['spatial'] == {'type': 'rbf', 'nu': 1.5} and kp['relationship'].shape == (4, 4)
    ag._init_model(get_args(['--kernel', 'genotype']))
    assert ag.gp.kernel_params['relationship'] is None and ag.gp.kernel_params['n_genotypes'] == 12
    with pytest.raises(SystemExit):
        get_args(['--kernel', 'spectral_mixture'])


def test_synthetic_field_keeps_the_simulated_effects():
    from algp_amd.field import SyntheticField
    np.random.seed(3)
    env = SyntheticField(8, 8, num_test=10, num_genotypes=5)
    assert env.num_genotypes == 5 and env.genotype_effect.shape == (5,) and env.X.shape[1] == 3
    np.random.seed(3)
    plain = SyntheticField(8, 8, num_test=10)
    assert plain.num_genotypes == 0 and plain.genotype_effect is None and plain.X.shape[1] == 2


@pytest.mark.parametrize('with_table', [False, True], ids=['identity', 'marker'])
def test_host_prior_draw_has_the_kernel_as_its_covariance(with_table):
    """utils.relationship_prior_draws on a small pool with many draws: the sample covariance against the helper's K.  With S draws
    and F features an entry's standard error is about (os_a + os_g max G_qq) sqrt(2 / S) (Gaussian part) plus O(os_a / sqrt(F))
    (a finite feature set): 6 standard errors at S = 20 000, F = 4 096 allow 0.12."""
    from algp_amd.utils import relationship_prior_draws
    Q = 5
    G = RL.marker_relationship(Q, 12) if with_table else None
    rng = np.random.RandomState(1)
    x = np.column_stack([rng.uniform(0, 4, (14, 2)), np.arange(14) % Q])
    ls, osa, osg = np.log([1.5, 2.5]), 0.8, 0.6
    S, F = 20000, 4096
    draws = relationship_prior_draws(MF.MATERN15, ls, osa, osg, G, Q, x, S, F, rng=7, chunk=5)
    assert draws.shape == (S, 14)
    K = RL.kernel_matrix((MF.MATERN15, G, Q), ls, (np.log(osa), np.log(osg)), x)
    emp = draws.T @ draws / S
    print('prior draws: worst covariance error %.3g, mean %.3g' % (float(np.max(np.abs(emp - K))), float(np.max(np.abs(draws.mean(axis=0))))))
    assert np.max(np.abs(emp - K)) < 0.12
    assert np.max(np.abs(draws.mean(axis=0))) < 6 * np.sqrt(np.max(np.diag(K)) / S) + 0.05
    # the documented draw order: the same seed gives the same draws, chunking does not matter
    again = relationship_prior_draws(MF.MATERN15, ls, osa, osg, G, Q, x, 3, 64, rng=7)
    once = relationship_prior_draws(MF.MATERN15, ls, osa, osg, G, Q, x, 3, 64, rng=7, chunk=3)
    assert np.allclose(again, once, rtol=0, atol=1e-12)
