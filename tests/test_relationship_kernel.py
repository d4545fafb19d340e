"""The relationship kernel k = os_a kappa_a(r_a) + os_g G[g, g'] (algp_set_hypers_relationship) through every layer that evaluates
a kernel value: the ABI and its id validation, the kernel-matrix build, MLL / gradient / fit_step, the criteria on a coordinate
pool against the same pool given as an explicit covariance, the solve routes, the incremental loop, the component means,
algp_genotype_posterior, the group posterior and the path utilities, the posterior samples, GPR.fit and a two-rank greedy run.
Modelled on tests/test_additive_kernel.py, whose shapes it uses for the same layers.

Every reference is tests/relationship_forms.py (NumPy fp64 on tests/matern_forms.py, held to central differences and to the
dense joint Gaussian by tests/test_relationship_forms_host.py) or an oracle function fed the helper's explicit matrix; never the
library.  Every tolerance is the one an existing test applies to the same quantity for a single kernel, cited where it is used.
The table term is one exact lookup and one rounded product, so a kernel value stays within the single kernel's relative bound
of os_a + os_g max G_qq: no tolerance below is widened.  The tables hold values both precisions represent exactly.  The problems
are built by module-level functions that need no device; tests/test_relationship_forms_host.py checks on the CPU that every train
matrix among them factors in fp32-rounded NumPy and that the reference runs whose picks are compared have a top-two gap above the
bound of tests/test_greedy_regimes.py:54.
"""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import additive_forms as AF                          # noqa: E402
import group_forms as GF                             # noqa: E402
import matern_forms as MF                            # noqa: E402
import mi_forms as MIF                               # noqa: E402
import pathwise_forms as PF                          # noqa: E402
import relationship_forms as RL                      # noqa: E402
import test_additive_kernel as TA                    # noqa: E402
import test_matern_family as TM                      # noqa: E402
import test_rhs_fused as RF                          # noqa: E402
import test_variance_reduction as VR                 # noqa: E402
from algp_amd import _hip                            # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

DT, DIDS = [np.float64, np.float32], ['f64', 'f32']
ALL4 = [MF.RBF, MF.MATERN15, MF.MATERN05, MF.MATERN25]
ENT, MI, VRC = _hip.CRIT_ENTROPY, _hip.CRIT_MUTUAL_INFORMATION, 2
S_STD, M_STD, SS, SM = TM.S_STD, TM.M_STD, TM.SS, TM.SM
GAP = TM.GAP                                                                             # tests/test_greedy_regimes.py:54
N_GENO = 12
# the three tables: the identity (G = NULL), G = A A^T / m from a random 12 x 40 marker matrix (its diagonal is not constant), and
# the same with genotype 11 on no plot
TABLES = ['identity', 'marker', 'marker-unobserved']

dtypes = pytest.mark.parametrize('dt', DT, ids=DIDS)
tables = pytest.mark.parametrize('tab', TABLES)
tol, relerr, _f32, _ut_bound, _top_gap, _memo = TM.tol, TM.relerr, TM._f32, TM._ut_bound, TM._top_gap, TM._memo


@functools.lru_cache(maxsize=None)
def table_of(tab, Q=N_GENO):
    """(G or None, the number of genotypes that occur on plots)"""
    if tab == 'identity':
        return None, Q
    G = RL.marker_relationship(Q, 40)
    G.setflags(write=False)
    return G, (Q - 1 if tab == 'marker-unobserved' else Q)


def spec_of(tab, ka=MF.MATERN15, Q=N_GENO):
    return (ka, table_of(tab, Q)[0], Q)


def set_rel(c, spec, log_ls, log_os, log_noise):
    c.set_hypers_relationship(log_ls, log_os[0], log_os[1], log_noise, kernel_a=spec[0], G=spec[1], n_genotypes=spec[2])


# ---------------------------------------------------------------------------------------------------- 1. ABI
def test_abi_good_and_bad_arguments():
    c = _hip.Context(np.float64)
    D, Q = 3, 4
    ls = np.ascontiguousarray(np.log([3.0, 2.0]))
    los, ln = (np.log(1.2), np.log(0.4)), np.log(1e-2)
    G = RL.marker_relationship(Q, 9)
    x = np.array([[0.0, 0.0, 1.0], [3.0, 0.0, 3.0], [0.0, 6.0, 2.0], [1.0, 1.0, 1.0]])
    dp = _hip._dblp

    def rc(D_, ka, G_, Q_, ls_=ls):
        g = None if G_ is None else np.ascontiguousarray(G_).ctypes.data_as(dp)
        return c.lib.algp_set_hypers_relationship(c.h, D_, ka, los[0], None if ls_ is None else ls_.ctypes.data_as(dp), los[1], g, Q_, ln)

    spec = (MF.MATERN15, G, Q)
    assert rc(D, spec[0], G, Q) == _hip.OK
    c.D, c.additive, c.relationship, c.Q = D, False, True, Q
    want = RL.kernel_matrix(spec, ls, los, x)
    assert relerr(c.kernel_matrix(x), want) < 1e-13
    bad_nan, bad_sym = G.copy(), G.copy()
    bad_nan[1, 2] = bad_nan[2, 1] = np.nan
    bad_sym[0, 3] = np.nextafter(bad_sym[0, 3], 1.0)
    for bad in ((1, 1, G, Q), (9, 1, G, Q), (D, -1, G, Q), (D, 4, G, Q), (D, 1, G, 0), (D, 1, None, -3), (D, 1, bad_nan, Q),
                (D, 1, bad_sym, Q), (D, 1, G, Q, None)):
        assert rc(*bad) == _hip.ERR_BAD_ARG, bad[:2]
        assert relerr(c.kernel_matrix(x), want) < 1e-13              # the context survives, with the hyper-parameters it had
    assert rc(D, 1, bad_sym, Q) == _hip.ERR_BAD_ARG and b'bitwise symmetric' in c.lib.algp_last_error(c.h)
    # every form of part a, a table and the identity
    for ka in ALL4:
        for G_ in (G, None):
            assert rc(D, ka, G_, Q) == _hip.OK
            assert relerr(c.kernel_matrix(x), RL.kernel_matrix((ka, G_, Q), ls, los, x)) < 1e-13
    # bad ids where coordinates meet the hyper-parameters: kernel_matrix (both operands), set_pool, and the setter itself with a
    # resident pool; the message names the row and the refused call changes nothing
    set_rel(c, spec, ls, los, ln)
    for col, val in ((2, 1.5), (0, -1.0), (3, float(Q))):
        xb = x.copy()
        xb[col, 2] = val
        with pytest.raises(ValueError, match='row %d' % col):
            c.kernel_matrix(xb)
        with pytest.raises(ValueError, match='x2: row %d' % col):
            c.kernel_matrix(x, xb)
    c.set_pool(x)
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])
    c.factorize()
    g_before, mll_before = c.mll_grad(), c.mll()
    assert g_before.shape == (D + 2,)
    xb = x.copy()
    xb[1, 2] = 7.0
    with pytest.raises(ValueError, match='set_pool: row 1'):
        c.set_pool(xb)
    assert c.n_pool == 4 and c.mll() == mll_before and np.array_equal(c.mll_grad(), g_before)      # pool, train set and factor stayed
    with pytest.raises(ValueError, match='resident pool: row 1'):
        c.set_hypers_relationship(ls, los[0], los[1], ln, kernel_a=MF.RBF, G=None, n_genotypes=3)     # the pool holds id 3
    assert c.mll() == mll_before and np.array_equal(c.mll_grad(), g_before)
    assert relerr(c.kernel_matrix(x), want) < 1e-13
    # round trips: single (D + 2), additive (D + 3), relationship (D + 2); the two existing setters still refuse id 4
    ls3 = np.ascontiguousarray(np.log([3.0, 2.0, 1.5]))
    c.set_hypers(ls3, los[0], ln, MF.MATERN25)
    assert c.lib.algp_set_hypers(c.h, 4, D, ls3.ctypes.data_as(dp), los[0], ln) == _hip.ERR_BAD_ARG
    assert c.lib.algp_set_hypers_additive(c.h, D, 4, 2, los[0], 0, los[1], ls3.ctypes.data_as(dp), ln) == _hip.ERR_BAD_ARG
    assert c.lib.algp_set_hypers_additive(c.h, D, 0, 2, los[0], 4, los[1], ls3.ctypes.data_as(dp), ln) == _hip.ERR_BAD_ARG
    assert relerr(c.kernel_matrix(x), MF.kernel_matrix(MF.MATERN25, ls3, los[0], x)) < 1e-13
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])          # the pool was rescaled and kept
    c.factorize()
    assert c.mll_grad().shape == (D + 2,)
    with pytest.raises(ValueError):
        c.genotype_posterior()                                       # a single kernel is in force
    assert c.lib.algp_genotype_posterior(c.h, _hip._ptr(np.zeros(Q)), None, None) == _hip.ERR_STATE
    c.set_hypers_additive(ls3, 2, los[0], los[1], ln, MF.MATERN15, MF.RBF)
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])
    c.factorize()
    assert c.mll_grad().shape == (D + 3,)
    set_rel(c, spec, ls, los, ln)
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])
    c.factorize()
    assert np.array_equal(c.mll_grad(), g_before) and c.mll() == mll_before
    c.close()


def test_abi_large_id_range_in_fp32():
    """Q = 20 000 with G = NULL in fp32: ids up to 19 999 on a 4-site pool are held exactly; 2^24 + 1 genotypes are refused."""
    c = _hip.Context(np.float32)
    ls, los, ln = np.log([2.0]), (np.log(0.8), np.log(0.5)), np.log(1e-2)
    spec = (MF.RBF, None, 20000)
    set_rel(c, spec, ls, los, ln)
    x = np.array([[0.0, 19999.0], [1.0, 19998.0], [2.0, 19999.0], [3.0, 0.0]])
    K = c.kernel_matrix(x)
    assert relerr(K, RL.kernel_matrix(spec, ls, los, x)) < 2e-5
    c.set_pool(x)
    c.set_train([0, 1, 3], [1.0, 0.0, -1.0], [0.1, 0.1, 0.1])
    c.factorize()
    mean, var, _ = c.genotype_posterior()
    mw, cw = RL.genotype_posterior(spec, ls, los, ln, x[[0, 1, 3]], [1.0, 0.0, -1.0], [0.1, 0.1, 0.1])
    assert mean.shape == (20000,) and np.max(np.abs(mean - mw)) < 1e-3 and np.max(np.abs(var - np.diag(cw))) < 1e-3
    assert np.all(mean[1:19998] == 0) and np.all(var[1:19998] == np.float32(np.exp(los[1])))
    with pytest.raises(ValueError, match='2\\^24'):
        c.set_hypers_relationship(ls, los[0], los[1], ln, n_genotypes=2 ** 24 + 1)
    c.close()


# ---------------------------------------------------------------------------------------------------- 2. kernel matrix
KM_LOG_OS = (np.log(1.7), np.log(0.6))


@functools.lru_cache(maxsize=None)
def kmat_problem(D, tab):
    """TM.kmat_inputs in D - 1 spatial dimensions with an id column behind them (x1[150] = x1[7], x2[3] = x1[5] ids included)."""
    q = TM.kmat_inputs(D - 1)
    rng = np.random.RandomState(90 + D)
    nq = table_of(tab)[1]
    g1, g2 = rng.randint(nq, size=200), rng.randint(nq, size=70)
    g1[150], g2[3] = g1[7], g1[5]
    return types.SimpleNamespace(log_ls=q.log_ls, log_noise=q.log_noise, var=q.var, x1=np.column_stack([q.x1, g1]),
                                 x2=np.column_stack([q.x2, g2]), g1=g1, g2=g2)


@dtypes
@tables
@pytest.mark.parametrize('D', [2, 3, 5, 8])
def test_kernel_matrix_every_form(D, tab, dt):
    """tests/test_additive_kernel.py::test_kernel_matrix_every_pair_of_forms (tests/test_hip_kernels.py:131, tolerance :142) for
    every kernel_a, DP = 2, 4, 8, 8: symmetric and cross builds; the diagonal is exactly os_a + os_g G_gg, a site 10^4
    lengthscales away keeps exactly the genotype part."""
    q = kmat_problem(D, tab)
    t = tol(dt, 1e-13, 2e-5)
    T = np.dtype(dt).type
    Gd = RL.table(spec_of(tab)).astype(dt)
    with np.errstate(over='ignore'):
        gpart = T(np.exp(KM_LOG_OS[1])) * Gd                                             # one rounded product, as the kernels form it
    c = _hip.Context(dt)
    for ka in ALL4:
        spec = spec_of(tab, ka)
        set_rel(c, spec, q.log_ls, KM_LOG_OS, q.log_noise)
        K = c.kernel_matrix(q.x1)
        Kw = RL.kernel_matrix(spec, q.log_ls, KM_LOG_OS, q.x1)
        assert K.dtype == np.dtype(dt) and K.shape == (200, 200) and np.all(np.isfinite(K))
        assert relerr(K, Kw) < t, ka
        assert np.array_equal(K, K.T)
        assert np.all(np.diag(K) == T(np.exp(KM_LOG_OS[0])) + gpart[q.g1, q.g1])          # exactly os_a + os_g G_gg
        assert K[7, 150] == K[7, 7] == K[150, 150]                                       # r = 0 off the diagonal, the same id
        assert np.all(K[199, :199] == gpart[q.g1[199], q.g1[:199]])                      # the spatial part exactly 0, not NaN
        Kx = c.kernel_matrix(q.x1[:130], q.x2)
        assert Kx.shape == (130, 70) and np.all(np.isfinite(Kx))
        assert relerr(Kx, RL.kernel_matrix(spec, q.log_ls, KM_LOG_OS, q.x1[:130], q.x2)) < t, ka
        assert Kx[5, 3] == K[5, 5] and np.all(Kx[:, 69] == gpart[q.g1[:130], q.g2[69]])
        Kd = c.kernel_matrix(q.x1, diag_add=q.var, add_likelihood_var=True)
        assert relerr(Kd, Kw + np.diag(q.var) + np.exp(q.log_noise) * np.eye(200)) < t, ka
    c.close()


# ---------------------------------------------------------------------------------------------------- 3. MLL, gradient, fit_step
MLL_LOG_OS, MLL_LOG_NOISE = (np.log(0.9), np.log(0.5)), np.log(0.05)
MLL_N = [(1, False), (63, False), (65, False), (130, False), (200, False), (130, True)]
MLL_D = [2, 4, 6]                                                                        # DP = 2, 4, 8


@functools.lru_cache(maxsize=None)
def mll_problem(tab, D, N, twice):
    """tests/test_additive_kernel.py:mll_problem with D - 1 spatial coordinates and an id column; `twice`: rows 5 and N - 3 name
    one pool site."""
    rng = np.random.RandomState(3)
    xs = _f32(rng.uniform(0, 6, (200, D - 1)))[:N]
    geno = rng.randint(table_of(tab)[1], size=200)[:N]
    eff = rng.standard_normal(N_GENO)
    x = np.column_stack([xs, geno])
    y = (np.sin(xs[:, 0]) + 0.6 * eff[geno] + 0.1 * rng.standard_normal(200)[:N])
    var = rng.uniform(0.005, 0.05, 200)[:N]
    idx = np.arange(N)
    if twice:
        idx[N - 3] = 5
    spec = spec_of(tab)
    th = (np.log([1.3, 2.1, 0.8, 1.6, 1.1])[:D - 1], MLL_LOG_OS, MLL_LOG_NOISE)
    xa = x[idx]
    q = types.SimpleNamespace(x=x, y=y, var=var, idx=idx, th=th, spec=spec)
    q.S = RL.train_matrix(spec, th[0], th[1], th[2], xa, var, idx)
    q.mll = RL.mll(spec, th[0], th[1], th[2], xa, y, var, idx)
    q.grad = RL.mll_grad(spec, th[0], th[1], th[2], xa, y, var, idx)
    return q


@tables
@dtypes
@pytest.mark.parametrize('D', MLL_D)
@pytest.mark.parametrize('N,twice', MLL_N, ids=['N%d%s' % (n, '-site-twice' if t else '') for n, t in MLL_N])
def test_mll_and_gradient(tab, D, N, twice, dt):
    """tests/test_additive_kernel.py::test_mll_and_gradient for the D + 2 gradient of this kernel.  fp64: tests/test_host_api.py:143-145
    (MLL 1e-10 relative, gradient 1e-8 of its largest entry); fp32: tests/test_fit_regimes.py:49 (2e-2).  Every width, both repeat
    states; the gradient is the same bits in two calls."""
    q = mll_problem(tab, D, N, twice)
    c = _hip.Context(dt)
    set_rel(c, q.spec, *q.th)
    c.set_pool(q.x)
    c.set_train(q.idx, q.y, q.var)
    c.factorize()
    mll, g = c.mll(), c.mll_grad()
    print('mll %.12e (want %.12e)  grad err %.2e' % (mll, q.mll, float(np.max(np.abs(g - q.grad)))))
    assert g.shape == (D + 2,) and np.isfinite(mll) and np.all(np.isfinite(g))
    if np.dtype(dt) == np.float64:
        assert mll == pytest.approx(q.mll, rel=1e-10)
        assert relerr(g, q.grad) < 1e-8
    else:
        assert abs(mll - q.mll) <= 2e-2 * abs(q.mll)
        assert np.max(np.abs(g - q.grad) / np.maximum(1.0, np.abs(q.grad))) <= 2e-2
    assert np.array_equal(c.mll_grad(), g)
    mll_s, g_s = c.fit_step()
    assert g_s.shape == (D + 2,)
    assert abs(mll_s - mll) <= tol(dt, 1e-12, 1e-6) * abs(mll)                            # tests/test_fold.py:213-214
    assert np.max(np.abs(g_s - g) / np.maximum(1.0, np.abs(g))) <= tol(dt, 1e-10, 2e-3)
    mll_b, g_b = c.fit_step()
    assert mll_b == mll_s and np.array_equal(g_b, g_s)
    c.close()


# ---------------------------------------------------------------------------------------------------- 4. criteria on a pool
POOL_LOG_LS = np.log([3.0, 3.0])
POOL_LOG_OS = (np.log(0.7), np.log(0.4))
POOL_LOG_NOISE = TM.LOG_NOISE
GENO_SEED = {'identity': 7, 'marker': 3, 'marker-unobserved': 7}     # checked on the CPU (tests/test_relationship_forms_host.py): every compared pick is separated


@functools.lru_cache(maxsize=None)
def pool_problem(tab):
    """tests/test_matern_family.py:pool_problem (300 sites, 80 train rows, six sites outside the covered square) with a genotype
    id behind the two positions.  Under the marker table the candidates' prior variances os_a + os_g G_gg differ from site to
    site (the per-site prior of cand_finalize)."""
    base = TM.pool_problem(MF.MATERN15)
    rng = np.random.RandomState(GENO_SEED[tab])
    geno = rng.randint(table_of(tab)[1], size=base.n)
    X = np.column_stack([base.X, geno])
    spec = spec_of(tab)
    p = types.SimpleNamespace(spec=spec, n=base.n, X=X, geno=geno, static=base.static, mobile=base.mobile, A=base.A, N=base.N,
                              var=base.var, cand=base.cand, alive=base.alive, free=base.free)
    effect = rng.standard_normal(N_GENO)
    p.y = np.sin(X[p.A, 0] / 3.0) + 0.5 * effect[geno[p.A]] + 0.1 * rng.standard_normal(p.N)
    p.K = RL.kernel_matrix(spec, POOL_LOG_LS, POOL_LOG_OS, X)
    p.C = p.K + np.exp(POOL_LOG_NOISE) * np.eye(p.n)
    p.S = p.C[np.ix_(p.A, p.A)] + np.diag(p.var)
    for a in (p.X, p.C, p.K, p.S, p.y):
        a.setflags(write=False)
    p.memo = {}
    return p


def _pool_ctx(p, dt, explicit, cand=None, alive=None, prior_includes_noise=True, solve=True):
    """Context A (coordinates and the relationship kernel) or B (the helper's matrix as an explicit pool covariance)."""
    c = _hip.Context(dt)
    if explicit:
        c.set_hypers(POOL_LOG_LS, 0.0, POOL_LOG_NOISE, _hip.KERNEL_RBF)
        c.set_pool_cov(p.C)
    else:
        set_rel(c, p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE)
        c.set_pool(p.X)
    c.set_train(p.A, p.y, p.var)
    c.factorize()
    c.set_candidates(p.cand if cand is None else cand, prior_includes_noise=prior_includes_noise)
    if solve:
        c.solve_candidates(alive=alive)
    return c


def entropy_reference(p):
    return _memo(p, 'ent', lambda: O.greedy_fast(p.C, p.static, p.mobile, S_STD, M_STD, 3, 'entropy'))


def mi_reference(p):
    return _memo(p, 'mi', lambda: O.greedy_fast(p.C, p.static, p.mobile, S_STD, M_STD, 3, 'mutual_information'))


def vr_reference(p):
    return _memo(p, 'vr', lambda: VR.vr_reference(p.C, p.A, p.var, p.cand, p.alive, SS, SM, 3))


@tables
@dtypes
def test_pool_posterior_and_covariance(tab, dt):
    """tests/test_additive_kernel.py::test_pool_posterior_and_covariance: mean and variance at the 220 free sites, both contexts
    and BOTH prior_includes_noise settings on the coordinate pool, against the helper (tests/test_rhs_fused.py:22 as its
    _check_oracle applies it); the posterior covariance at tests/test_posterior_cov_regimes.py:143's bound.  Under the marker
    table the free sites' priors differ (asserted): the variance is right only with the per-site prior."""
    p = pool_problem(tab)
    mu_w, pv_w = _memo(p, 'post', lambda: RL.posterior(p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE, p.X[p.A], p.y, p.var,
                                                       p.X[p.free]))
    if tab != 'identity':
        assert np.ptp(RL.prior_var(p.spec, POOL_LOG_OS, p.X[p.free])) > 0.05
    samp = np.arange(len(p.free))
    for explicit, pin in ((False, False), (False, True), (True, True)):
        c = _pool_ctx(p, dt, explicit, cand=p.free, prior_includes_noise=pin)
        mu, pv = c.posterior()
        RF._check_oracle(mu, pv, samp, dict(mu=mu_w, var=pv_w), RF.TOL[dt], np.exp(POOL_LOG_NOISE) if pin else 0.0,
                         'explicit' if explicit else 'coordinates pin=%d' % pin)
        if not explicit and not pin:
            B = p.K[np.ix_(p.A, p.free)]
            cov_w = p.K[np.ix_(p.free, p.free)] - B.T @ np.linalg.solve(p.S, B)
            cov, _ = c.posterior_cov()
            assert relerr(cov, cov_w) < tol(dt, 1e-9, 1e-3)
        c.close()


@tables
@dtypes
def test_pool_entropy_picks(tab, dt):
    """tests/test_additive_kernel.py::test_pool_entropy_picks (tests/test_greedy_regimes.py:169-179, bounds :165-166)."""
    p = pool_problem(tab)
    picks_o, ut_o = entropy_reference(p)
    assert _top_gap(ut_o) > GAP[np.dtype(dt)], 'the inputs no longer separate the picks'
    got = []
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, alive=p.alive)
        picks, ut = c.greedy(ENT, S_STD, M_STD, 3, want_utilities=True)
        c.close()
        fin = np.isfinite(ut_o)
        assert np.array_equal(np.isfinite(ut), fin)
        scale = float(np.max(np.abs(ut_o[fin])))
        err = float(np.max(np.abs(ut[fin] - ut_o[fin])))
        print('entropy %s: utilities %.2e of max|u| %.3f' % ('explicit' if explicit else 'coordinates', err, scale))
        assert err < _ut_bound(dt, scale)
        assert [int(q) for q in picks] == [int(q) for q in picks_o]
        got.append([int(q) for q in picks])
    assert got[0] == got[1]


@tables
@dtypes
def test_pool_mi_picks(tab, dt):
    """tests/test_additive_kernel.py::test_pool_mi_picks: every utility along the reference's picks at tests/test_hip_greedy.py:417's
    tolerance (1e-7 / 3e-3 of the largest utility), both contexts; the free run's picks in fp64, where the gap is resolved."""
    p = pool_problem(tab)
    picks_o, ut_o = mi_reference(p)
    cand = np.where(~p.static)[0]
    ut_f, H = _memo(p, 'mi_H', lambda: MIF.reference(p.C, p.static, p.mobile, S_STD, M_STD, picks_o))
    assert np.array_equal(ut_f, ut_o)
    rel = tol(dt, 1e-7, 3e-3)
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, cand=cand)
        got, ut = c.greedy(MI, S_STD, M_STD, 3, forced_picks=[int(q) for q in picks_o], want_utilities=True)
        assert [int(q) for q in got] == [int(q) for q in picks_o]
        for k in range(3):
            want = ut_o[k][cand]
            live = np.isfinite(want)
            assert np.array_equal(np.isfinite(ut[k]), live), k
            scale = float(np.max(np.abs(want[live])))
            err = float(np.max(np.abs(ut[k][live] - want[live])))
            print('MI %s pick %d: %.2e of %.3f' % ('explicit' if explicit else 'coordinates', k, err, scale))
            assert err <= rel * scale
            MIF.compare(ut[k], want, p.mobile[cand], dt, H[k], 'pick %d' % k)
        if np.dtype(dt) == np.float64:
            assert _top_gap(ut_o) > 2 * rel * scale, 'the inputs no longer separate the picks'
            c.solve_candidates()
            assert [int(q) for q in c.greedy(MI, S_STD, M_STD, 3)] == [int(q) for q in picks_o]
        c.close()


@tables
@dtypes
def test_pool_variance_reduction(tab, dt):
    """tests/test_additive_kernel.py::test_pool_variance_reduction_and_target_weights without the weights
    (tests/test_variance_reduction.py: vr_reference, compare, TOL at :52): three rounds along the brute force's picks, then the
    free run's picks."""
    p = pool_problem(tab)
    t = VR.TOL[dt]
    picks_o, U = vr_reference(p)
    for r in range(3):
        top = np.sort(U[r][np.isfinite(U[r])])[-2:]
        assert (top[1] - top[0]) / top[1] > 2 * t, 'the inputs no longer separate the picks'      # test_variance_reduction.py:206-209
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, alive=p.alive)
        got_p, got_u = c.greedy(VRC, S_STD, M_STD, 3, forced_picks=picks_o, want_utilities=True)
        assert [int(v) for v in got_p] == picks_o
        for r in range(3):
            VR.compare(got_u[r], U[r], t, '%s round %d' % ('explicit' if explicit else 'coordinates', r))
        c.solve_candidates(alive=p.alive)
        assert [int(v) for v in c.greedy(VRC, S_STD, M_STD, 3)] == picks_o
        c.close()


# ---------------------------------------------------------------------------------------------------- 5. solve routes, incremental
ROUTE_LOG_LS, ROUTE_LOG_OS = np.log([3.0, 3.0]), (np.log(0.6), np.log(0.5))


@functools.lru_cache(maxsize=None)
def mid_problem(tab):
    """tests/test_matern_family.py:mid_problem (N = 300, M = 700: the one-launch and mid-sized solves) with an id column."""
    base = TM.mid_problem(MF.MATERN15)
    rng = np.random.RandomState(8)
    pool = np.column_stack([base.pool, rng.randint(table_of(tab)[1], size=len(base.pool))])
    spec = spec_of(tab)
    mu, pv = RL.posterior(spec, ROUTE_LOG_LS, ROUTE_LOG_OS, TM.LOG_NOISE, pool[base.A], base.y, base.var, pool[base.cidx])
    S = RL.train_matrix(spec, ROUTE_LOG_LS, ROUTE_LOG_OS, TM.LOG_NOISE, pool[base.A], base.var)
    return types.SimpleNamespace(pool=pool, A=base.A, y=base.y, var=base.var, cidx=base.cidx, mu=mu, pv=pv, S=S, spec=spec,
                                 logdet=np.linalg.slogdet(S)[1])


@tables
@pytest.mark.parametrize('dt,t', [(np.float64, 1e-9), (np.float32, 2e-3)], ids=DIDS)     # tests/test_fold.py:41
def test_fit_and_solve_and_the_mean_only_posterior(tab, dt, t, monkeypatch):
    """tests/test_additive_kernel.py::test_fit_and_solve_and_the_mean_only_posterior: the folded launch and its two phases."""
    q = mid_problem(tab)
    c = _hip.Context(dt)
    set_rel(c, q.spec, ROUTE_LOG_LS, ROUTE_LOG_OS, TM.LOG_NOISE)
    c.set_pool(q.pool)
    c.set_train(q.A, q.y, q.var)
    c.set_candidates(q.cidx, prior_includes_noise=False)
    scale = max(1.0, np.max(np.abs(q.mu)))
    for fold in ('1', '0'):
        monkeypatch.setenv('ALGP_FOLD', fold)                                             # read per call
        c.fit_and_solve()
        mu, pv = c.posterior()
        assert np.all(np.isfinite(mu)) and np.all(np.isfinite(pv))
        assert np.max(np.abs(mu - q.mu)) <= t * scale                                     # tests/test_fold.py:57-58
        assert np.max(np.abs(pv - q.pv)) <= t * max(1.0, np.max(np.abs(q.pv)))
        assert abs(c.logdet() - q.logdet) <= t * abs(q.logdet)                            # :62
        mo = c.posterior_mean(q.cidx)
        assert np.max(np.abs(mo - mu)) <= tol(dt, 1e-8, 2e-2) * scale                     # tests/test_fold.py:186
    monkeypatch.delenv('ALGP_FOLD')
    c.close()


@functools.lru_cache(maxsize=None)
def sweep_problem():
    """tests/test_matern_family.py:fused_problem (51 300 candidates, 1 400 train rows: the scheduled sweep) with an id column."""
    base = TM.fused_problem(MF.MATERN15)
    rng = np.random.RandomState(9)
    pool = np.column_stack([base.pool, rng.randint(N_GENO, size=len(base.pool))])
    spec = spec_of('marker')
    mu, pv = RL.posterior(spec, ROUTE_LOG_LS, ROUTE_LOG_OS, TM.LOG_NOISE, pool[base.A], base.y, base.var, pool[base.cidx[base.samp]])
    return types.SimpleNamespace(base=base, pool=pool, spec=spec, ref=dict(mu=mu, var=pv))


@dtypes
def test_scheduled_sweep_takes_the_materialised_route(dt, monkeypatch):
    """tests/test_additive_kernel.py::test_scheduled_sweep_takes_the_materialised_route: under this kernel the sweep reads its
    right-hand sides from V^T whatever ALGP_RHS_FUSED says -- the same bits, the full kernel-matrix traffic -- and meets the
    helper at tests/test_rhs_fused.py:22."""
    q = sweep_problem()
    b = q.base
    c = _hip.Context(dt)
    set_rel(c, q.spec, ROUTE_LOG_LS, ROUTE_LOG_OS, TM.LOG_NOISE)
    c.set_pool(q.pool)
    c.set_train(b.A, b.y, b.var)
    c.factorize()
    c.set_candidates(b.cidx, prior_includes_noise=False)
    (mu, pv), (mu2, pv2), (mu0, pv0) = RF._posteriors(c, monkeypatch)
    RF._check_oracle(mu, pv, b.samp, q.ref, RF.TOL[dt], what='relationship')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)                  # ALGP_RHS_FUSED=0: bit for bit
    full, _ = RF._expected_bytes(TM.FUSED_M, TM.FUSED_N, np.dtype(dt).itemsize)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    assert RF._kmat_bytes(c) == full                                           # nothing was generated in an epilogue
    monkeypatch.delenv('ALGP_RHS_FUSED')
    c.close()


@tables
@dtypes
def test_incremental_update_equals_from_scratch(tab, dt):
    """tests/test_additive_kernel.py::test_incremental_update_equals_from_scratch (tests/test_incremental.py:196, :246)."""
    p = pool_problem(tab)
    extra = p.free[:5]
    A2 = np.r_[p.A, extra]
    y2 = np.r_[p.y, np.linspace(-0.3, 0.3, 5)]
    var2 = np.r_[p.var, np.full(5, SS)]
    c = _pool_ctx(p, dt, False, cand=p.free[5:], prior_includes_noise=False)
    c.set_train(A2, y2, var2)
    kept = c.factorize(incremental=True)
    c.solve_candidates(incremental=True)
    mu, pv = c.posterior()
    c.close()
    assert kept >= 0
    f = _hip.Context(dt)
    set_rel(f, p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE)
    f.set_pool(p.X)
    f.set_train(A2, y2, var2)
    f.factorize()
    f.set_candidates(p.free[5:], prior_includes_noise=False)
    f.solve_candidates()
    mu_f, pv_f = f.posterior()
    f.close()
    t = tol(dt, 1e-9, 3e-3)
    assert np.max(np.abs(mu - mu_f)) < t * max(1.0, np.max(np.abs(mu_f)))
    assert np.max(np.abs(pv - pv_f)) < t
    mu_w, pv_w = RL.posterior(p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE, p.X[A2], y2, var2, p.X[p.free[5:]])
    RF._check_oracle(mu, pv, np.arange(len(mu)), dict(mu=mu_w, var=pv_w), RF.TOL[dt], what='updated')


# ---------------------------------------------------------------------------------------------------- 6. component means
@tables
@dtypes
def test_component_means(tab, dt):
    """tests/test_additive_kernel.py::test_component_means (the mean's own tolerance, tests/test_fold.py:186): 0 + 1 + ybar =
    posterior_mean; component 1 at a site is genotype_posterior's mean of the site's id."""
    p = pool_problem(tab)
    ma_w, mg_w = _memo(p, 'comp', lambda: RL.component_means(p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE, p.X[p.A], p.y, p.var,
                                                            p.X[p.free]))
    c = _pool_ctx(p, dt, False, solve=False)
    ma, mg = c.posterior_mean_component(0, p.free), c.posterior_mean_component(1, p.free)
    mu = c.posterior_mean(p.free)
    gm, _, _ = c.genotype_posterior()
    scale = max(1.0, float(np.max(np.abs(ma_w + mg_w + p.y.mean()))))
    t = tol(dt, 1e-8, 2e-2)
    assert ma.dtype == np.dtype(dt) and ma.shape == (len(p.free),)
    assert np.max(np.abs(ma - ma_w)) <= t * scale and np.max(np.abs(mg - mg_w)) <= t * scale
    assert np.max(np.abs(ma.astype(np.float64) + mg + p.y.mean() - mu)) <= tol(dt, 1e-12, 1e-5) * scale
    assert np.max(np.abs(mg - gm[p.geno[p.free]])) <= tol(dt, 1e-12, 1e-5) * scale
    assert np.std(ma_w) > 0.05 and np.std(mg_w) > 0.05                          # both parts carry signal here
    for comp in (-1, 2):
        with pytest.raises(ValueError):
            c.posterior_mean_component(comp, p.free)
    c.close()


# ---------------------------------------------------------------------------------------------------- 7. genotype posterior
GP_SHAPES = [(12, 150), (130, 300)]                                            # neither a multiple of 128
GP_LOG_LS, GP_LOG_OS, GP_LOG_NOISE = np.log([3.0, 2.0]), (np.log(0.7), np.log(0.5)), np.log(2e-2)
# cov and var have no precedent: the reference's own fp32-rounded NumPy evaluation (inputs and every intermediate rounded to
# fp32, genotype_posterior_f32 below) differs from the fp64 reference by at most 1.6e-6 of max|cov| on these inputs, measured on
# the CPU (tests/test_relationship_forms_host.py prints it and holds it below 1e-5); tests/test_group_posterior.py:37 allows its
# cov 1e-5 / 1e-3 of the largest entry, the margin taken here
GP_BAR = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}


@functools.lru_cache(maxsize=None)
def genotype_problem(tab, Q, N):
    """N plots on a field with Q genotypes, the last of which is on no plot (so that its effect is predicted through its relatives
    under a table and stays at the prior under the identity)."""
    rng = np.random.RandomState(100 + Q)
    pos = _f32(rng.uniform(0.0, 12.0, (N, 2)))
    geno = rng.randint(Q - 1, size=N)
    G = None if tab == 'identity' else RL.marker_relationship(Q, 3 * Q + 4, seed=7)
    spec = (MF.MATERN15, G, Q)
    eff = rng.standard_normal(Q)
    x = np.column_stack([pos, geno])
    y = np.sin(pos[:, 0] / 3.0) + 0.7 * eff[geno] + 0.1 * rng.standard_normal(N)
    var = rng.uniform(0.01, 0.05, N)
    q = types.SimpleNamespace(spec=spec, x=x, y=y, var=var, Q=Q, N=N, geno=geno)
    q.S = RL.train_matrix(spec, GP_LOG_LS, GP_LOG_OS, GP_LOG_NOISE, x, var)
    q.mean, q.cov = RL.genotype_posterior(spec, GP_LOG_LS, GP_LOG_OS, GP_LOG_NOISE, x, y, var)
    return q


def genotype_posterior_f32(q):
    """The helper's genotype posterior with the inputs and every intermediate rounded to fp32: the reference's own fp32 error."""
    f = np.float32
    S = q.S.astype(f)
    B = RL.genotype_cross(q.spec, GP_LOG_OS, q.x).astype(f)
    L = np.linalg.cholesky(S).astype(f)
    from scipy.linalg import solve_triangular
    W = solve_triangular(L, B.T, lower=True).astype(f).T
    z = solve_triangular(L, (q.y - q.y.mean()).astype(f), lower=True).astype(f)
    pri = (f(np.exp(GP_LOG_OS[1])) * RL.table(q.spec).astype(f))
    return (W @ z).astype(f), (pri - (W @ W.T).astype(f)).astype(f)


@pytest.mark.parametrize('tab', ['identity', 'marker'])
@pytest.mark.parametrize('Q,N', GP_SHAPES, ids=['Q%d-N%d' % s for s in GP_SHAPES])
@dtypes
def test_genotype_posterior(tab, Q, N, dt):
    q = genotype_problem(tab, Q, N)
    c = _hip.Context(dt)
    set_rel(c, q.spec, GP_LOG_LS, GP_LOG_OS, GP_LOG_NOISE)
    c.set_pool(q.x)
    c.set_train(np.arange(N), q.y, q.var)
    c.factorize()
    before = c.device_bytes()
    mean, var, cov = c.genotype_posterior(want_var=True, want_cov=True)
    assert c.device_bytes() > before                                            # the scratch is the context's, and counted
    bar = GP_BAR[np.dtype(dt)]
    scale = float(np.max(np.abs(q.cov)))
    print('genotype posterior %s Q=%d N=%d: mean %.3g  var %.3g  cov %.3g (bar %g)' % (
        tab, Q, N, relerr(mean, q.mean), float(np.max(np.abs(var - np.diag(q.cov)))) / scale, relerr(cov, q.cov), bar))
    assert mean.shape == (Q,) and var.shape == (Q,) and cov.shape == (Q, Q)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))
    assert np.max(np.abs(mean - q.mean)) <= tol(dt, 1e-8, 2e-2) * max(1.0, np.max(np.abs(q.mean)))   # the mean's tolerance, tests/test_fold.py:186
    assert relerr(cov, q.cov) <= bar
    assert np.max(np.abs(var - np.diag(q.cov))) <= bar * scale
    assert np.max(np.abs(var - np.diag(cov))) <= tol(dt, 1e-12, 1e-5) * scale   # two reductions of the same row of W
    assert np.array_equal(cov, cov.T)                                           # identical bits in both triangles
    T = np.dtype(dt).type
    if tab == 'identity':                                                       # the genotype on no plot stays at its prior, exactly
        assert mean[Q - 1] == 0 and var[Q - 1] == T(np.exp(GP_LOG_OS[1])) and cov[Q - 1, Q - 1] == var[Q - 1]
        assert np.all(cov[Q - 1, :Q - 1] == 0)
    else:                                                                       # ... and is predicted through its relatives
        assert abs(q.mean[Q - 1]) > 1e-3 and abs(mean[Q - 1] - q.mean[Q - 1]) <= tol(dt, 1e-8, 2e-2)
        assert var[Q - 1] < T(np.exp(GP_LOG_OS[1])) * T(RL.table(q.spec)[Q - 1, Q - 1])
    # the same bits on a second call, whatever is asked for; nothing resident was written
    m2, v2, c2 = c.genotype_posterior(want_var=True, want_cov=True)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var) and np.array_equal(c2, cov)
    m3, v3, c3 = c.genotype_posterior(want_var=False, want_cov=False)
    assert np.array_equal(m3, mean) and v3 is None and c3 is None
    mu_before = c.posterior_mean(np.arange(5))
    c.genotype_posterior()
    assert np.array_equal(c.posterior_mean(np.arange(5)), mu_before)
    c.close()


def test_genotype_posterior_refusals():
    """Every state the call refuses, and the out-of-memory message before anything is allocated (a problem whose scratch exceeds
    any card)."""
    p = pool_problem('marker')
    c = _hip.Context(np.float64)
    set_rel(c, p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE)
    with pytest.raises(ValueError, match='coordinate pool'):
        c.genotype_posterior()                                                  # no pool
    c.set_pool(p.X)
    c.set_train(p.A, p.y, p.var)
    with pytest.raises(ValueError, match='factorize'):
        c.genotype_posterior()                                                  # no factor
    c.factorize()
    assert c.lib.algp_genotype_posterior(c.h, None, None, None) == _hip.ERR_BAD_ARG
    c.genotype_posterior()
    c.set_candidates(p.cand, prior_includes_noise=True)
    c.solve_candidates(alive=p.alive)
    c.greedy(ENT, S_STD, M_STD, 1)
    with pytest.raises(ValueError, match='pick'):
        c.genotype_posterior()                                                  # a pick was committed since the factorisation
    c.factorize()
    c.genotype_posterior()
    c.set_train(p.A[:-1], p.y[:-1], p.var[:-1])
    with pytest.raises(ValueError, match='factorize'):
        c.genotype_posterior()                                                  # the train set changed
    c.close()
    b = _hip.Context(np.float64)                                                # an explicit-covariance pool
    b.set_hypers_relationship(POOL_LOG_LS, POOL_LOG_OS[0], POOL_LOG_OS[1], POOL_LOG_NOISE, n_genotypes=N_GENO)
    b.set_pool_cov(p.C)
    b.set_train(p.A, p.y, p.var)
    b.factorize()
    with pytest.raises(ValueError, match='coordinate pool'):
        b.genotype_posterior()
    b.close()
    # out of memory, reported with the byte count before anything is allocated: 200 000 independent genotypes (no table is
    # stored) with cov ask for 2 x 200 064^2 doubles = 640 GB of scratch, beyond any card.  Through the C ABI with a cov
    # pointer that is never written: the refusal comes before the first launch
    big = _hip.Context(np.float64)
    Qb = 200000
    big.set_hypers_relationship(POOL_LOG_LS, POOL_LOG_OS[0], POOL_LOG_OS[1], POOL_LOG_NOISE, n_genotypes=Qb)
    big.set_pool(np.column_stack([p.X[:, :2], (np.arange(p.n) * 611) % Qb]))
    big.set_train(p.A, p.y, p.var)
    big.factorize()
    held = big.device_bytes()
    mean, dummy = np.zeros(Qb), np.zeros(1)
    assert big.lib.algp_genotype_posterior(big.h, _hip._ptr(mean), None, _hip._ptr(dummy)) == _hip.ERR_OOM
    msg = big.lib.algp_last_error(big.h).decode()
    need = 2 * 200064 * 200064 * 8
    assert 'bytes' in msg and any(int(w) > need for w in msg.replace(',', ' ').split() if w.isdigit()), msg
    assert big.device_bytes() == held                                           # nothing was allocated
    assert big.mll() == big.mll()                                               # the context stays usable
    big.close()


# ---------------------------------------------------------------------------------------------------- 8. group posterior, paths
@tables
@dtypes
def test_group_posterior_of_the_genotypes(tab, dt):
    """tests/test_additive_kernel.py::test_group_posterior_of_the_genotypes: tests/test_group_posterior.py's bar (:37, 1e-5 / 1e-3)."""
    p = pool_problem(tab)
    lab = p.geno[p.free].astype(np.int32)
    nq = table_of(tab)[1]
    assert len(np.unique(lab)) == nq

    def build():
        B = p.K[np.ix_(p.A, p.free)]
        Sigma = p.K[np.ix_(p.free, p.free)] - B.T @ np.linalg.solve(p.S, B)
        mu = p.y.mean() + B.T @ np.linalg.solve(p.S, p.y - p.y.mean())
        return GF.aggregates(mu, Sigma, GF.coefficients(lab, None, nq))
    ref = _memo(p, 'group', build)
    c = _pool_ctx(p, dt, False, cand=p.free, prior_includes_noise=False)
    mean, cov, cross = c.group_posterior(lab, n_groups=nq, want_cov=True, want_cross=True)
    c.close()
    bar = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}[np.dtype(dt)]
    for got, want, what in ((mean, ref[0], 'mean'), (cov, ref[1], 'cov'), (cross, ref[2], 'cross')):
        print('group %s relerr %.3g (bar %g)' % (what, relerr(got, want), bar))
        assert got.shape == want.shape and np.all(np.isfinite(got)) and relerr(got, want) <= bar, what


@tables
@dtypes
def test_score_paths_three_criteria(tab, dt):
    """tests/test_additive_kernel.py::test_score_paths_three_criteria with its path constructions on this file's pool problem:
    score_paths on both routes (tolerances tests/test_hip_greedy.py:565, :617), score_paths_mi (tests/test_mi_paths.py:119) and
    score_paths_vr (tests/test_paths_vr.py:37), coordinates and explicit covariance."""
    p = pool_problem(tab)
    c = _pool_ctx(p, dt, False)
    for (paths, want), t in zip(TA.entropy_paths(p), (tol(dt, 1e-9, 2e-3), tol(dt, 1e-9, 3e-3))):
        got = c.score_paths(paths, 0.7)
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want)) < t * max(1.0, np.max(np.abs(want))), np.max(np.abs(got - want))
    c.close()
    rows, want = TA.mi_paths(p)
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, cand=np.where(~p.mobile)[0])
        got = c.score_paths_mi(rows, S_STD, M_STD)
        c.close()
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want)) <= tol(dt, 1e-7, 3e-3) * np.max(np.abs(want)), np.max(np.abs(got - want))
    rows, want = TA.vr_paths(p)
    assert np.min(want) > 1e-2
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, alive=p.alive)
        got = c.score_paths_vr(rows, M_STD)
        c.close()
        err = np.abs(got - want) / np.abs(want)
        print('paths vr %s: worst %.3e' % ('explicit' if explicit else 'coordinates', float(np.max(err))))
        assert np.all(np.isfinite(got)) and np.max(err) < tol(dt, 1e-9, 1e-3)


# ---------------------------------------------------------------------------------------------------- 9. samples
@functools.lru_cache(maxsize=None)
def sample_case(tab):
    """Values mode: an exact prior draw on the helper's matrix."""
    p = pool_problem(tab)
    S = 5
    rng = np.random.RandomState(61)
    L = np.linalg.cholesky(p.K + 1e-10 * np.eye(p.n))
    prior = _f32(rng.standard_normal((S, p.n)) @ L.T)
    eps = _f32(rng.standard_normal((S, p.N)))
    v = p.var + np.exp(POOL_LOG_NOISE)
    ref = PF.pathwise(p.K[np.ix_(p.free, p.A)], p.S, p.y, v, prior[:, p.free], prior[:, p.A], eps)
    return types.SimpleNamespace(prior=prior, eps=eps, ref=ref)


@tables
@dtypes
def test_posterior_samples(tab, dt):
    """Values mode against tests/pathwise_forms.py on the helper's matrix at tests/test_pathwise_samples.py's bar (:35, 1e-5 / 1e-3
    of the largest draw); features mode is refused, and the message says why."""
    p = pool_problem(tab)
    q = sample_case(tab)
    c = _pool_ctx(p, dt, False, cand=p.free, prior_includes_noise=False)
    bar = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}[np.dtype(dt)]
    fv = c.sample_posterior(q.eps, prior=q.prior)
    assert fv.shape == (5, len(p.free)) and np.all(np.isfinite(fv))
    print('values %.3g (bar %g)' % (relerr(fv, q.ref), bar))
    assert relerr(fv, q.ref) <= bar
    rng = np.random.RandomState(2)
    with pytest.raises(ValueError, match='no spectral density'):
        c.sample_posterior(q.eps, weights=rng.standard_normal((5, 64)), omega=rng.standard_normal((64, 3)), phase=rng.uniform(size=64))
    assert np.array_equal(c.sample_posterior(q.eps, prior=q.prior), fv)          # the refusal changed nothing
    c.close()


# ---------------------------------------------------------------------------------------------------- 10. GPR.fit
@functools.lru_cache(maxsize=None)
def fit_problem():
    """tests/test_additive_kernel.py:fit_problem -- 150 plots of a 15 x 10 field, 10 genotypes scattered over them, y = g(genotype)
    + s(row, col) + noise -- with the coordinates in this kernel's layout (row, col | genotype id)."""
    q = TA.fit_problem()
    x = np.column_stack([q.x[:, 1], q.x[:, 2], q.geno])
    return types.SimpleNamespace(x=x, y=q.y, var=q.var, geno=q.geno, g=q.g, x_add=q.x, probe_add=q.probe)


@dtypes
def test_gpr_fit_and_genotype_effects(dt):
    from algp_amd.models import GPR
    q = fit_problem()
    kp = {'type': 'genotype', 'spatial': {'type': 'matern', 'nu': 1.5}, 'relationship': None, 'n_genotypes': 10}
    runs = []
    for _ in range(2):
        gp = GPR(lr=.1, max_iterations=30, kernel_params=kp, dtype=dt)
        losses = gp.fit(q.x, q.y, q.var)
        runs.append((losses, gp.hypers()))
    losses = runs[0][0]
    assert len(losses) == 30 and np.all(np.isfinite(losses))
    assert losses[-1] < losses[0]                                # the loss is -MLL / N: the likelihood went up
    assert runs[0][0] == runs[1][0]                              # the same trajectory, bit for bit
    assert np.array_equal(runs[0][1][0], runs[1][1][0]) and runs[0][1][1:] == runs[1][1][1:]
    ls, los, ln, kt = gp.hypers()
    assert kt == ('genotype', _hip.KERNEL_MATERN15) and ls.shape == (2,)
    spec = (MF.MATERN15, None, 10)
    C = gp.cov_mat(q.x, add_likelihood_var=True)
    assert relerr(C, RL.kernel_matrix(spec, ls, los, q.x) + np.exp(ln) * np.eye(150)) < tol(dt, 1e-13, 2e-5)
    # the genotype effects at the fitted hyper-parameters: the library against the helper
    mean, var = gp.genotype_effects()
    mean_c, cov = gp.genotype_effects(return_cov=True)
    mw, cw = RL.genotype_posterior(spec, ls, los, ln, q.x, q.y, q.var)
    bar = GP_BAR[np.dtype(dt)]
    assert np.array_equal(mean, mean_c)
    assert np.max(np.abs(mean - mw)) <= tol(dt, 1e-8, 2e-2) * max(1.0, np.max(np.abs(mw)))
    assert relerr(cov, cw) <= bar and np.max(np.abs(var - np.diag(cw))) <= bar * np.max(np.abs(cw))
    # predict and its components agree with the helper and with each other
    probe = np.column_stack([np.full(10, 7.0), np.full(10, 4.5), np.arange(10)])
    ma, mg = gp.predict_components(probe)
    t = tol(dt, 1e-8, 2e-2)
    ma_w, mg_w = RL.component_means(spec, ls, los, ln, q.x, q.y, q.var, probe)
    assert np.max(np.abs(ma - ma_w)) <= t * max(1.0, np.max(np.abs(ma_w))) and np.max(np.abs(mg - mg_w)) <= t * max(1.0, np.max(np.abs(mg_w)))
    assert np.max(np.abs(ma.astype(np.float64) + mg + q.y.mean() - gp.predict(probe))) <= tol(dt, 1e-10, 1e-4) * max(1.0, np.max(np.abs(q.y)))
    mu_p, var_p = gp.predict(probe, return_std=True)
    mu_w, pv_w = RL.posterior(spec, ls, los, ln, q.x, q.y, q.var, probe)
    assert np.max(np.abs(var_p - (pv_w + np.exp(ln)))) <= tol(dt, 1e-8, 2e-3)
    gm, gcov = gp.group_posterior(probe, np.arange(10), n_groups=10)
    assert gm.shape == (10,) and gcov.shape == (10, 10)
    smp = gp.sample_posterior(probe, n_samples=3, n_features=128, rng=5)
    assert smp.shape == (3, 10) and np.all(np.isfinite(smp))
    # printed, not asserted: the error of the genotype effects against the simulated ones, beside the additive RBF-over-id model's
    add = GPR(lr=.1, max_iterations=30, kernel_params={'type': 'additive', 'split': 1, 'parts': TA.FIT_PARTS}, dtype=dt)
    add.fit(q.x_add, q.y, q.var)
    la, loa, lna, _ = add.hypers()
    ma_add, _ = AF.component_means((MF.MATERN15, MF.RBF, 1), la, loa, lna, q.x_add, q.y, q.var, q.probe_add)
    print('genotype effect RMSE: relationship (identity) %.4f  additive Matern-over-id %.4f' % (
        TA._centred_error(mw, q.g), TA._centred_error(ma_add, q.g)))


# ---------------------------------------------------------------------------------------------------- 11. two ranks
WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, os.path.join(%(repo)r, 'tests'))
import torch
import torch.distributed as dist
from algp_amd import _hip
from algp_amd.sharded import partition
import relationship_forms as RL

dist.init_process_group('gloo')
rank, world = dist.get_rank(), dist.get_world_size()
rng = np.random.RandomState(11)
N, M, Q = 300, 1201, 12
X = np.column_stack([rng.uniform(0, 25, (N + M, 2)), rng.randint(Q, size=N + M)])
G = RL.marker_relationship(Q, 40)
static = rng.uniform(size=N) < 0.5
var = np.where(static, 0.01, 1.0)
y = rng.standard_normal(N)
cand = np.r_[np.where(~static)[0][:50], np.arange(N, N + M)]

def gather(send):
    t = torch.frombuffer(bytearray(send), dtype=torch.uint8)
    out = torch.empty(world * len(send), dtype=torch.uint8)
    dist.all_gather_into_tensor(out, t)
    return out.numpy().tobytes()

def make(idx_slice):
    c = _hip.Context(np.float64)
    c.set_hypers_relationship(np.log([3.0, 2.5]), np.log(0.7), np.log(0.5), np.log(1e-2), kernel_a=_hip.KERNEL_MATERN15, G=G)
    c.set_pool(X)
    c.set_train(np.arange(N), y, var)
    c.factorize()
    c.set_candidates(idx_slice, prior_includes_noise=True)
    c.solve_candidates()
    return c

for crit in (_hip.CRIT_ENTROPY,):
    full = make(cand)
    want, ut = full.greedy(crit, 0.1, 1.0, 4, want_utilities=True)
    want = [int(p) for p in want]
    full.close()
    lo, hi = partition(len(cand), world)[rank]
    c = make(cand[lo:hi])
    c.comm_init_host(world, rank, gather)
    got, gut = c.greedy_sharded(crit, 0.1, 1.0, 4, want_utilities=True)
    assert [int(p) for p in got] == want, (crit, rank, got, want)
    for p in range(4):
        top = np.nanmax(ut[p])
        assert abs(gut[p] - top) < 1e-9 * max(1.0, abs(top)), (crit, p, gut[p], top)
    c.comm_destroy(); c.close()
dist.barrier()
if rank == 0:
    print('SHARDED_REL_OK')
dist.destroy_process_group()
'''


@pytest.mark.parametrize('rows_in_gather', ['1', '0'], ids=['rows-travel', 'rows-rebuilt'])
def test_two_ranks_greedy(tmp_path, rows_in_gather):
    """tests/test_sharded_abi.py::test_two_ranks_through_the_abi_collective's transport (two processes, a host all-gather over
    gloo) at small shapes under the relationship kernel with a table: the sharded entropy picks and utilities equal one rank's.  rows-rebuilt: a remote winner's row and its per-site prior are rebuilt from the replicated factor."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'repo': REPO})
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', ALGP_GATHER_ROWS=rows_in_gather)
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                          '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), str(script)],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'SHARDED_REL_OK' in out.stdout


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]
