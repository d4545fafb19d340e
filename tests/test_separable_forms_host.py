"""CPU checks behind tests/test_separable_kernel.py: the NumPy helper tests/separable_forms.py is held to central differences of
its own MLL and restricted likelihood and to identities that need no reference; every train matrix the GPU tests build factors in
fp32-rounded NumPy; the reference runs whose picks are compared are separated by more than the bound of
tests/test_greedy_regimes.py:54; the fp32 kernel-value bound is measured; and the Python plumbing that needs no device (the
spectral draws, GPR's parameter names, ar1_correlations' closed form, the command-line flags, the synthetic field).  No GPU.

The fp32 kernel-value bound.  test_fp32_product_rounding computes the spatial product as an fp32 evaluation rounds it at best --
each factor rounded to fp32, their product rounded, the product with os rounded (separable_forms.fp32_product) -- against fp64
over the problems of the GPU file.  Measured worst case: 1.29e-7 of the largest entry (two fp32 roundings), against the 2e-5 that
tests/test_matern_family.py allows a single form.  The product's own roundings take less than a hundredth of that tolerance, so
the GPU file applies the single form's tolerance times 1 (KVAL_FACTOR); the test fails if the measurement ever passes a tenth.
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
import pathwise_forms as PF                          # noqa: E402
import reml_forms as RM                              # noqa: E402
import relationship_forms as RL                      # noqa: E402
import separable_forms as SF                         # noqa: E402
import test_separable_kernel as TS                   # noqa: E402
import test_variance_reduction as VR                 # noqa: E402

ALL4 = [MF.RBF, MF.MATERN15, MF.MATERN05, MF.MATERN25]
VARIANTS = ['plain', 'identity', 'marker']


def _problem(ka, kb, variant, Q=6, N=40, seed=4):
    """N sites with three spatial coordinates, split (1, 2), one site listed twice; an id column under the genotype variants."""
    rng = np.random.RandomState(seed)
    xs = rng.uniform(0, 5, (N, 3))
    geno = rng.randint(Q, size=N)
    eff = rng.standard_normal(Q)
    G = RL.marker_relationship(Q, 20) if variant == 'marker' else None
    spec = (ka, kb, 1, G, 0 if variant == 'plain' else Q)
    x = np.column_stack([xs, geno]) if SF.has_g(spec) else xs
    y = np.sin(xs[:, 0]) + (eff[geno] if SF.has_g(spec) else 0.0) + 0.1 * rng.standard_normal(N)
    var = rng.uniform(0.01, 0.05, N)
    idx = np.arange(N)
    idx[7] = 3                                                                  # a site listed twice: r_a = r_b = 0 off the diagonal
    los = (np.log(0.8), np.log(0.6)) if SF.has_g(spec) else np.log(0.8)
    return spec, x[idx], y, var, idx, SF.pack(np.log([1.4, 2.2, 0.9]), los, np.log(0.05))


def _central(f, theta, k, h=1e-5):
    e = np.zeros(len(theta))
    e[k] = h
    return (f(theta + e) - f(theta - e)) / (2 * h)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('kb', ALL4)
@pytest.mark.parametrize('ka', ALL4)
def test_gradients_against_central_differences(ka, kb, variant):
    """The MLL gradient against central differences of the MLL and the REML gradient against those of the REML value, for every
    pair of forms and every variant: the step (1e-5) and the bound (1e-6 of max(|fd|, 1e-3)) of tests/test_additive_forms_host.py."""
    spec, x, y, var, idx, theta = _problem(ka, kb, variant)
    P = len(theta)
    assert P == x.shape[1] + 2
    g = SF.mll_and_grad(spec, theta, x, y, var, idx)[1]
    assert g.shape == (P,) and np.all(np.isfinite(g))
    H = RM.basis(x[:, :3], 3)
    gr = SF.reml_grad(spec, theta, x, y, H, var, idx)
    assert gr.shape == (P,) and np.all(np.isfinite(gr))
    for k in range(P):
        fd = _central(lambda t: SF.mll_and_grad(spec, t, x, y, var, idx)[0], theta, k)
        assert abs(fd - g[k]) <= 1e-6 * max(abs(fd), 1e-3), ('mll', k, fd, g[k])
        fd = _central(lambda t: SF.reml(spec, t, x, y, H, var, idx), theta, k)
        assert abs(fd - gr[k]) <= 1e-6 * max(abs(fd), 1e-3), ('reml', k, fd, gr[k])
    # the average information is symmetric, positive semi-definite, and the restricted one is what reml_forms makes of a model
    ai, air = SF.average_information(spec, theta, x, y, var, idx), SF.reml_ai(spec, theta, x, y, H, var, idx)
    for a in (ai, air):
        assert a.shape == (P, P) and np.allclose(a, a.T, rtol=0, atol=1e-12 * np.max(np.abs(a))) and np.linalg.eigvalsh(a)[0] > -1e-10 * np.max(np.abs(a))
    assert RM.AI.__name__ == 'ai_forms'                                         # reml_forms is left as it was found


def test_identities_that_need_no_reference():
    rng = np.random.RandomState(2)
    x, xt = rng.uniform(0, 5, (30, 4)), rng.uniform(0, 5, (7, 4))
    ls, los = np.log([1.3, 2.1, 0.8, 1.7]), np.log(0.9)
    # (rbf, rbf) is the single RBF form over all coordinates with the same lengthscales, whatever the split
    for split in (1, 2, 3):
        K = SF.kernel_matrix((MF.RBF, MF.RBF, split, None, 0), ls, los, x, xt)
        assert np.allclose(K, MF.kernel_matrix(MF.RBF, ls, los, x, xt), rtol=1e-13, atol=0)
    # (m05, m05) with Da = Db = 1 is os rho_r^|dr| rho_c^|dc| with rho = exp(-1 / l): AR1 x AR1 on a grid of plots
    rr, cc = np.meshgrid(np.arange(6), np.arange(5), indexing='ij')
    g = np.column_stack([rr.ravel(), cc.ravel()]).astype(np.float64)
    l2 = np.log([2.5, 1.2])
    rho = np.exp(-1.0 / np.exp(l2))
    K = SF.kernel_matrix((MF.MATERN05, MF.MATERN05, 1, None, 0), l2, los, g)
    want = np.exp(los) * rho[0] ** np.abs(np.subtract.outer(g[:, 0], g[:, 0])) * rho[1] ** np.abs(np.subtract.outer(g[:, 1], g[:, 1]))
    assert np.allclose(K, want, rtol=1e-13, atol=0)
    # ... which is neither Matern-1/2 over (row, col) nor a sum of a row and a column process
    assert np.max(np.abs(K - MF.kernel_matrix(MF.MATERN05, l2, los, g))) > 0.05
    # with os_g -> 0 the genotype variant's matrix is the plain one; the term itself is the relationship kernel's
    G = RL.marker_relationship(5, 12)
    xg, xtg = np.column_stack([x, np.arange(30) % 5]), np.column_stack([xt, np.arange(7) % 5])
    plain = SF.kernel_matrix((MF.MATERN15, MF.MATERN05, 2, None, 0), ls, los, x, xt)
    for G_ in (G, None):
        spec = (MF.MATERN15, MF.MATERN05, 2, G_, 5)
        assert np.array_equal(SF.kernel_matrix(spec, ls, (los, -np.inf), xg, xtg), plain)
        both = SF.kernel_matrix(spec, ls, (los, np.log(0.6)), xg, xtg)
        assert np.allclose(both - plain, RL.part_matrix((MF.RBF, G_, 5), 1, ls, (0.0, np.log(0.6)), xg, xtg), rtol=0, atol=1e-15)
        assert np.allclose(np.diag(SF.kernel_matrix(spec, ls, (los, np.log(0.6)), xg)), SF.prior_var(spec, (los, np.log(0.6)), xg), rtol=1e-15)
    # the components: 0 + 1 + ybar is the posterior mean, component 1 is the genotype posterior's mean by id
    spec = (MF.MATERN15, MF.MATERN05, 2, G, 5)
    y, var = rng.standard_normal(30), rng.uniform(0.01, 0.05, 30)
    th = (ls, (los, np.log(0.6)), np.log(0.05))
    mu, pv = SF.posterior(spec, *th, xg, y, var, xtg)
    ms, mg = SF.component_means(spec, *th, xg, y, var, xtg)
    gm, gc = SF.genotype_posterior(spec, *th, xg, y, var)
    assert np.max(np.abs(ms + mg + y.mean() - mu)) < 1e-12 and np.max(np.abs(mg - gm[np.arange(7) % 5])) < 1e-10
    assert np.all(pv > 0) and np.all(pv < SF.prior_var(spec, th[1], xtg)) and np.min(np.linalg.eigvalsh(gc)) > 0


def _gpu_train_matrices():
    """(what, S) of every train matrix tests/test_separable_kernel.py builds."""
    for model in TS.MLL_MODELS:
        for N, twice in TS.MLL_N:
            yield ('mll', model, N, twice), TS.mll_problem(model, N, twice).S
    for model in TS.AI_MODELS:
        for p in (0, 1, 3):
            c = TS.ai_case(model, p)
            yield ('ai', model, p), SF.train_matrix(c['spec'], *SF.unpack(c['spec'], c['theta'], c['x']), c['x'][c['idx']], c['var'])
    for model in TS.POOL_MODELS:
        p = TS.pool_problem(model)
        yield ('pool', model), p.S
        A2 = np.r_[p.A, p.free[:5]]
        yield ('pool updated', model), p.C[np.ix_(A2, A2)] + np.diag(np.r_[p.var, np.full(5, TS.SS)])
    for model in TS.ROUTE_MODELS:
        yield ('mid', model), TS.mid_problem(model).S
    q = TS.sweep_problem()
    b = q.base
    yield ('sweep',), SF.train_matrix(q.spec, TS.ROUTE_LOG_LS, TS.ROUTE_LOG_OS[0], TS.TM.LOG_NOISE, b.pool[b.A], b.var)
    for tab in ('identity', 'marker'):
        for Q, N in TS.GP_SHAPES:
            yield ('genotype', tab, Q, N), TS.genotype_problem(tab, Q, N).S
    f = TS.fit_problem()
    yield ('fit',), SF.train_matrix((MF.MATERN05, MF.MATERN05, 1, None, 12), np.zeros(2), (0.0, 0.0), 0.0, f.x, f.var)
    yield ('fit plain',), SF.train_matrix((MF.MATERN05, MF.MATERN05, 1, None, 0), np.zeros(2), 0.0, 0.0, f.x[:, :2], f.var)


def test_every_train_matrix_of_the_gpu_tests_factors_in_fp32():
    n = 0
    for what, S in _gpu_train_matrices():
        assert MF.factors_in_fp32(S), what
        n += 1
    assert n > 80
    G = TS.table_of('marker')[0]                     # positive definite, fp32 values, bitwise symmetric, a non-constant diagonal
    assert np.array_equal(G, G.T) and np.array_equal(G, G.astype(np.float32)) and np.min(np.linalg.eigvalsh(G)) > 1e-3
    assert np.ptp(np.diag(G)) > 0.05


@pytest.mark.parametrize('model', TS.POOL_MODELS, ids=TS.POOL_IDS)
def test_reference_picks_are_separated(model):
    """Every reference run whose picks tests/test_separable_kernel.py compares: top-two gaps above tests/test_greedy_regimes.py:54
    in both precisions (entropy), above twice the MI tolerance in fp64 (where alone its free run is compared), above twice the
    fp32 variance-reduction tolerance with and without target weights (tests/test_variance_reduction.py:206-209)."""
    p = TS.pool_problem(model)
    _, ut = TS.entropy_reference(p)
    print('%s entropy gap %.3g' % (model, TS._top_gap(ut)))
    assert TS._top_gap(ut) > TS.GAP[np.dtype(np.float32)]
    _, utm = TS.mi_reference(p)
    scale = max(float(np.max(np.abs(r[np.isfinite(r)]))) for r in utm)
    print('%s MI gap %.3g of %.3g' % (model, TS._top_gap(utm), scale))
    assert TS._top_gap(utm) > 2 * 1e-7 * scale
    for which, ref in (('vr', TS.vr_reference), ('weighted vr', TS.wvr_reference)):
        _, U = ref(p)
        for r in range(3):
            top = np.sort(U[r][np.isfinite(U[r])])[-2:]
            print('%s %s round %d gap %.3g' % (model, which, r, (top[1] - top[0]) / top[1]))
            assert (top[1] - top[0]) / top[1] > 2 * VR.TOL[np.float32]
    assert np.min(TS.TA.vr_paths(p)[1]) > 1e-2       # the path utilities are compared relatively (tests/test_paths_vr.py:37)


def test_fp32_product_rounding():
    """The measurement behind KVAL_FACTOR (this file's docstring): over the kernel-matrix, pool and MLL problems of the GPU file."""
    worst = 0.0

    def measure(spec, log_ls, log_os, x1, x2=None):
        nonlocal worst
        k64 = SF.part_matrix(spec, 0, log_ls, log_os, x1, x2)
        k32 = SF.fp32_product(spec, log_ls, log_os, x1, x2)
        assert k32.dtype == np.float32
        worst = max(worst, float(np.max(np.abs(k32 - k64)) / np.max(np.abs(k64))))

    for Da, Db, with_id in TS.KM_SPLITS:
        q = TS.kmat_problem(Da, Db, with_id)
        for pair in TS.PAIRS:
            variant = 'marker' if with_id else 'plain'
            spec = TS.spec_of(variant, pair, Da)
            measure(spec, q.log_ls, TS.log_os_of(variant, TS.KM_LOG_OS), q.x1)
            measure(spec, q.log_ls, TS.log_os_of(variant, TS.KM_LOG_OS), q.x1[:130], q.x2)
    for model in TS.POOL_MODELS:
        p = TS.pool_problem(model)
        measure(p.spec, p.log_ls, p.log_os, p.X)
    for model in TS.MLL_MODELS:
        q = TS.mll_problem(model, 200, False)
        measure(q.spec, q.th[0], q.th[1], q.x)
    print('fp32-rounded product against fp64: worst %.3g of the largest entry' % worst)
    single = 2e-5                                    # tests/test_matern_family.py::test_kernel_matrix, fp32
    assert worst <= 0.1 * single and TS.KVAL_FACTOR == 1
    assert TS.kval_tol(np.float32) == TS.KVAL_FACTOR * single and TS.kval_tol(np.float64) == 1e-13


@pytest.mark.parametrize('pair', TS.PAIRS, ids=TS.PIDS)
def test_spectral_draws_have_the_product_as_their_kernel(pair):
    """Phi Phi^T of F = 4 096 draws against k on 60 sites in three dimensions, split (1, 2): tests/test_pathwise_forms_host.py's
    bound for a single form, 6 os sqrt(1.5 / F) -- six standard deviations of an entry, each the mean of F independent terms of
    variance <= 1.5 os^2 (the feature is sqrt(2 os / F) cos(omega . x + phase) whatever law omega has) = 0.115 at F = 4 096."""
    from algp_amd import utils
    F, os_ = 4096, 1.0
    kid = ('separable', 1, pair[0], pair[1])
    om, ph = utils.spectral_draws(kid, 3, F, 1)
    assert om.shape == (F, 3) and ph.shape == (F,) and om.dtype == np.float64
    om2, ph2 = utils.spectral_draws(kid, 3, F, np.random.RandomState(1))
    assert np.array_equal(om, om2) and np.array_equal(ph, ph2)
    assert np.all(np.abs(om) > 0)                                               # every feature takes a frequency of BOTH parts
    # part a's column is the single form's draw of the same stream
    om_a, _ = utils.spectral_draws(pair[0], 1, F, 1)
    assert np.array_equal(om[:, :1], om_a)
    rng = np.random.RandomState(5)
    x = rng.uniform(0, 6, (60, 3))
    ls = np.log([1.5, 2.5, 2.0])
    Phi = PF.features(om, ph, x * np.exp(-ls)[None, :], os_)
    K = SF.kernel_matrix((pair[0], pair[1], 1, None, 0), ls, np.log(os_), x)
    err = float(np.max(np.abs(Phi @ Phi.T - K)))
    print('%s: worst |Phi Phi^T - k| = %.3g' % (kid, err))
    assert err < 6 * os_ * np.sqrt(1.5 / F)
    with pytest.raises(NotImplementedError):
        utils.spectral_draws(('separable', 1, 9, 0), 3, 4, 0)


def test_host_prior_draw_with_a_separable_spatial_part():
    """utils.relationship_prior_draws with the separable product as the spatial part: the sample covariance against the helper's
    K at the bound tests/test_relationship_forms_host.py derives for the same S and F (0.12)."""
    from algp_amd.utils import relationship_prior_draws
    Q = 5
    G = RL.marker_relationship(Q, 12)
    rng = np.random.RandomState(1)
    x = np.column_stack([rng.uniform(0, 4, (14, 2)), np.arange(14) % Q])
    ls, os_, osg = np.log([1.5, 2.5]), 0.8, 0.6
    S, F = 20000, 4096
    draws = relationship_prior_draws(('separable', 1, MF.MATERN05, MF.MATERN15), ls, os_, osg, G, Q, x, S, F, rng=7)
    K = SF.kernel_matrix((MF.MATERN05, MF.MATERN15, 1, G, Q), ls, (np.log(os_), np.log(osg)), x)
    err = float(np.max(np.abs(draws.T @ draws / S - K)))
    print('prior draws: worst covariance error %.3g' % err)
    assert draws.shape == (S, 14) and err < 0.12


def _reset(kp, x):
    from algp_amd.models import GPR
    gp = GPR(kernel_params=kp)
    gp.reset(x, np.zeros(len(x)), np.full(len(x), 0.1))
    return gp


def test_gpr_builds_the_named_parameters():
    """gpytorch's ScaleKernel(ProductKernel(...)) names, alone and as the genotype kernel's first part."""
    from algp_amd.models import GPR
    rng = np.random.RandomState(0)
    x = np.column_stack([rng.uniform(0, 4, (9, 3)), np.arange(9) % 5])
    sep = {'type': 'separable', 'split': 2, 'parts': ({'type': 'matern', 'nu': 0.5}, {'type': 'rbf'})}
    gp = _reset(sep, x[:, :3])
    named = dict(gp.model.named_parameters())
    assert tuple(named['kernel_covar_module.base_kernel.kernels.0.log_lengthscale'].shape) == (1, 1, 2)
    assert tuple(named['kernel_covar_module.base_kernel.kernels.1.log_lengthscale'].shape) == (1, 1, 1)
    assert tuple(named['kernel_covar_module.log_outputscale'].shape) == (1,) and 'likelihood.log_noise' in named and len(named) == 4
    ls, los, ln, kt = gp.hypers()
    assert ls.shape == (3,) and isinstance(los, float) and kt == ('separable', 2, MF.MATERN05, MF.RBF)
    assert [n for n, _, _, _ in gp._gradient_route()] == ['kernel_covar_module.base_kernel.kernels.0.log_lengthscale',
                                                          'kernel_covar_module.base_kernel.kernels.1.log_lengthscale',
                                                          'kernel_covar_module.log_outputscale', 'likelihood.log_noise']
    assert gp._gradient_route()[-1][3] == 5                                     # D + 2
    gp.model.load_state_dict(gp.model.state_dict())
    for rel, nq in ((RL.marker_relationship(5, 12), None), (None, 5)):
        gp = _reset({'type': 'genotype', 'spatial': sep, 'relationship': rel, 'n_genotypes': nq}, x)
        named = dict(gp.model.named_parameters())
        assert tuple(named['kernel_covar_module.kernels.0.base_kernel.kernels.0.log_lengthscale'].shape) == (1, 1, 2)
        assert tuple(named['kernel_covar_module.kernels.0.base_kernel.kernels.1.log_lengthscale'].shape) == (1, 1, 1)
        assert tuple(named['kernel_covar_module.kernels.0.log_outputscale'].shape) == (1,)
        assert tuple(named['kernel_covar_module.kernels.1.log_outputscale'].shape) == (1,) and len(named) == 5
        ls, los, ln, kt = gp.hypers()
        assert ls.shape == (3,) and len(los) == 2 and kt == ('genotype', ('separable', 2, MF.MATERN05, MF.RBF))
        assert gp.model.relationship[1] == 5 and gp._gradient_route()[-1][3] == 6   # D + 2 with D = 4
        gp.model.load_state_dict(gp.model.state_dict())
    for bad in ({'type': 'separable', 'split': 3, 'parts': sep['parts']}, {'type': 'separable', 'split': 0, 'parts': sep['parts']},
                {'type': 'separable', 'split': 1, 'parts': sep['parts'][:1]}, {'type': 'separable', 'parts': sep['parts']}):
        with pytest.raises(ValueError):
            _reset(bad, x[:, :3])
    with pytest.raises(ValueError):                                              # two spatial coordinates and the id: D >= 3
        _reset({'type': 'genotype', 'spatial': {'type': 'separable', 'split': 1, 'parts': sep['parts']}, 'n_genotypes': 5}, x[:, 2:])
    with pytest.raises(NotImplementedError):
        _reset({'type': 'separable', 'split': 1, 'parts': ({'type': 'spectral_mixture'}, {'type': 'rbf'})}, x[:, :3])
    with pytest.raises(ValueError):
        GPR(kernel_params={'type': 'rbf'}).ar1_correlations()


def test_ar1_correlations_against_the_closed_form():
    """rho = exp(-spacing / l) and se = rho (spacing / l) se(log l), with se(log l) from hyper_covariance (given here: no device);
    ValueError for a part that is not Matern-1/2 over a single coordinate."""
    rng = np.random.RandomState(0)
    x = np.column_stack([rng.uniform(0, 4, (9, 2)), np.arange(9) % 5])
    ar1 = {'type': 'separable', 'split': 1, 'parts': ({'type': 'matern', 'nu': 0.5}, {'type': 'matern', 'nu': 0.5})}
    for kp, xs in ((ar1, x[:, :2]), ({'type': 'genotype', 'spatial': ar1, 'n_genotypes': 5}, x)):
        gp = _reset(kp, xs)
        route = gp._gradient_route()
        import torch
        with torch.no_grad():
            for name, p, a, b in route[:2]:
                p.fill_(float(np.log(2.5 if a == 0 else 1.2)))
        names = gp._scalar_names(route)
        A = rng.standard_normal((len(names), len(names)))
        cov = A @ A.T
        gp.hyper_covariance = lambda: (names, cov)
        for spacing in (1.0, 0.5):
            got = gp.ar1_correlations(spacing)
            for k, l in enumerate((2.5, 1.2)):
                rho = np.exp(-spacing / l)
                assert got[k][0] == pytest.approx(rho, rel=1e-14)
                assert got[k][1] == pytest.approx(rho * (spacing / l) * np.sqrt(cov[k, k]), rel=1e-14)
    for parts, split, cols in ((({'type': 'matern', 'nu': 0.5}, {'type': 'rbf'}), 1, 2), (({'type': 'matern', 'nu': 1.5}, {'type': 'matern', 'nu': 0.5}), 1, 2),
                               (({'type': 'matern', 'nu': 0.5}, {'type': 'matern', 'nu': 0.5}), 2, 3)):
        gp = _reset({'type': 'separable', 'split': split, 'parts': parts}, np.column_stack([x[:, :2], x[:, 0]])[:, :cols])
        gp.hyper_covariance = lambda: pytest.fail('refused before any device work')
        with pytest.raises(ValueError, match='Matern-1/2 over a single coordinate'):
            gp.ar1_correlations()


def test_argument_parsing_and_the_agents_model():
    from algp_amd.arguments import get_args
    a = get_args(['--kernel', 'separable', '--kernel_split', '1', '--kernel_a', 'matern', '--kernel_b', 'matern', '--matern_nu', '0.5'])
    assert a.kernel == 'separable' and a.kernel_split == 1 and a.spatial == 'single'
    from algp_amd.agent import Agent
    ag = Agent.__new__(Agent)
    ag.learn_likelihood_noise = True
    ag.env = types.SimpleNamespace(num_genotypes=12)
    ag._init_model(a)
    m05 = {'type': 'matern', 'nu': 0.5}
    assert ag.gp.kernel_params == {'type': 'separable', 'split': 1, 'parts': (m05, m05)}
    a = get_args(['--kernel', 'genotype', '--spatial', 'separable', '--fit_method', 'ai', '--fit_objective', 'reml', '--fixed_effects', 'intercept'])
    assert a.spatial == 'separable'
    ag._init_model(a)
    kp = ag.gp.kernel_params
    assert kp['type'] == 'genotype' and kp['n_genotypes'] == 12 and kp['relationship'] is None
    assert kp['spatial'] == {'type': 'separable', 'split': 1, 'parts': (m05, m05)}       # AR1(row) x AR1(col)
    assert ag.gp.fit_objective == 'reml' and ag.gp.fixed_effects == 'intercept'
    assert get_args(['--kernel', 'genotype']).spatial == 'single'
    with pytest.raises(SystemExit):
        get_args(['--kernel', 'genotype', '--spatial', 'kronecker'])


def test_synthetic_field_draws_from_the_separable_process():
    """ar1 = (rho_row, rho_col): over many fields the sample correlation of neighbours along a row and along a column is rho_col
    and rho_row (800 fields of 64 plots: the standard error of a correlation is below 0.01); without it the field is unchanged."""
    from algp_amd.field import SyntheticField
    np.random.seed(3)
    a = SyntheticField(8, 8, num_test=10, num_genotypes=5)
    np.random.seed(3)
    b = SyntheticField(8, 8, num_test=10, num_genotypes=5, ar1=None)
    assert np.array_equal(a.all_y, b.all_y) and np.array_equal(a.all_x, b.all_x)
    np.random.seed(4)
    fields = np.stack([SyntheticField(8, 8, num_test=10, ar1=(0.8, 0.5)).all_y.reshape(8, 8) for _ in range(800)])
    down = np.mean(fields[:, 1:, :] * fields[:, :-1, :])                         # neighbours one ROW apart
    along = np.mean(fields[:, :, 1:] * fields[:, :, :-1])
    print('AR1 field: var %.3f, neighbour correlation %.3f across rows, %.3f across columns' % (np.mean(fields ** 2), down, along))
    assert abs(np.mean(fields ** 2) - 1.0) < 0.05 and abs(down - 0.8) < 0.05 and abs(along - 0.5) < 0.05
    env = SyntheticField(6, 7, num_test=5, num_genotypes=4, ar1=(0.8, 0.5))
    assert env.X.shape[1] == 3 and env.genotype_effect.shape == (4,) and int(env.all_x[9, 0]) == 1 and int(env.all_x[9, 1]) == 2
