"""The separable kernel k = os kappa_a(r_a) kappa_b(r_b) [+ os_g G[g, g']] (algp_set_hypers_separable) through every layer that
evaluates a kernel value: the ABI and its refusals, the kernel-matrix build, MLL / gradient / fit_step, the average information
and the restricted likelihood, the criteria on a coordinate pool against the same pool given as an explicit covariance, the solve
routes, the incremental loop, the component means, algp_genotype_posterior, the group posterior, the fixed-effects posterior, the
path utilities, the posterior samples, GPR.fit and a two-rank greedy run.  Modelled section by section on
tests/test_relationship_kernel.py and tests/test_additive_kernel.py, whose shapes it uses for the same layers.

Every reference is tests/separable_forms.py (NumPy fp64 on tests/matern_forms.py, held to central differences by
tests/test_separable_forms_host.py) or an oracle function fed the helper's explicit matrix; never the library.  Every tolerance is
the one an existing test applies to the same quantity, cited where it is used.  The fp32 kernel values take the single form's
tolerance (tests/test_matern_family.py: 2e-5) times KVAL_FACTOR = 1: the product adds two roundings to the factors' own, measured
on these problems by tests/test_separable_forms_host.py (its docstring has the figure).  The problems are built by module-level
functions that need no device; the host file checks that every train matrix among them factors in fp32-rounded NumPy and that the
reference runs whose picks are compared have a top-two gap above the bound of tests/test_greedy_regimes.py:54.

Three variants: 'plain' (no genotype term, Q = 0), 'identity' (the term with G = NULL) and 'marker' (a dense table with a
non-constant diagonal).  Four pairs of forms: family 0 x 0, 1 x 1, 0 x 1 and (Matern-1/2, Matern-1/2), which with one coordinate
each is AR1 x AR1.
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

import group_forms as GF                             # noqa: E402
import matern_forms as MF                            # noqa: E402
import mi_forms as MIF                               # noqa: E402
import pathwise_forms as PF                          # noqa: E402
import relationship_forms as RL                      # noqa: E402
import reml_forms as RM                              # noqa: E402
import separable_forms as SF                         # noqa: E402
import test_additive_kernel as TA                    # noqa: E402
import test_average_information as TAI               # noqa: E402
import test_fit_regimes as FR                        # noqa: E402
import test_fixed_effects as TFX                     # noqa: E402
import test_matern_family as TM                      # noqa: E402
import test_rhs_fused as RF                          # noqa: E402
import test_variance_reduction as VR                 # noqa: E402
from algp_amd import _hip                            # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

DT, DIDS = [np.float64, np.float32], ['f64', 'f32']
ENT, MI, VRC = _hip.CRIT_ENTROPY, _hip.CRIT_MUTUAL_INFORMATION, 2
S_STD, M_STD, SS, SM = TM.S_STD, TM.M_STD, TM.SS, TM.SM
GAP = TM.GAP                                                                             # tests/test_greedy_regimes.py:54
KNAME = TA.KNAME
PAIRS = [(MF.MATERN15, MF.RBF), (MF.MATERN05, MF.MATERN25), (MF.RBF, MF.MATERN05), (MF.MATERN05, MF.MATERN05)]
PIDS = ['%sx%s' % (KNAME[a], KNAME[b]) for a, b in PAIRS]
VARIANTS = ['plain', 'identity', 'marker']
N_GENO = 12
KVAL_FACTOR = 1                                      # times the single form's fp32 tolerance: tests/test_separable_forms_host.py

dtypes = pytest.mark.parametrize('dt', DT, ids=DIDS)
tol, relerr, _f32, _ut_bound, _top_gap, _memo = TM.tol, TM.relerr, TM._f32, TM._ut_bound, TM._top_gap, TM._memo


def kval_tol(dt):
    """tests/test_hip_kernels.py:142 as tests/test_matern_family.py::test_kernel_matrix applies it, times KVAL_FACTOR in fp32."""
    return tol(dt, 1e-13, KVAL_FACTOR * 2e-5)


@functools.lru_cache(maxsize=None)
def table_of(variant, Q=N_GENO):
    """(G or None, Q); Q = 0 without the genotype term."""
    if variant == 'plain':
        return None, 0
    if variant == 'identity':
        return None, Q
    G = RL.marker_relationship(Q, 40)
    G.setflags(write=False)
    return G, Q


def spec_of(variant, pair, split, Q=N_GENO):
    G, Q = table_of(variant, Q)
    return (pair[0], pair[1], split, G, Q)


def log_os_of(variant, both):
    """The helper's log_os: a float without the genotype term, else the pair."""
    return both[0] if variant == 'plain' else both


def set_sep(c, spec, log_ls, log_os, log_noise):
    ka, kb, split, G, Q = spec
    if Q == 0:
        c.set_hypers_separable(log_ls, split, log_os, log_noise, kernel_a=ka, kernel_b=kb)
    else:
        c.set_hypers_separable(log_ls, split, log_os[0], log_noise, kernel_a=ka, kernel_b=kb, log_outputscale_g=log_os[1], G=G,
                               n_genotypes=Q)


# ---------------------------------------------------------------------------------------------------- 1. ABI
def test_abi_good_and_bad_arguments():
    c = _hip.Context(np.float64)
    D, Q = 4, 4
    ls = np.ascontiguousarray(np.log([3.0, 2.0, 1.5]))
    los, ln = (np.log(1.2), np.log(0.4)), np.log(1e-2)
    G = RL.marker_relationship(Q, 9)
    x = np.array([[0.0, 0.0, 1.0, 1.0], [3.0, 0.0, 0.5, 3.0], [0.0, 6.0, 2.0, 2.0], [1.0, 1.0, 0.0, 1.0]])
    dp = _hip._dblp

    def rc(D_, ka, Da, kb, G_, Q_, ls_=ls):
        g = None if G_ is None else np.ascontiguousarray(G_).ctypes.data_as(dp)
        return c.lib.algp_set_hypers_separable(c.h, D_, ka, Da, kb, los[0], None if ls_ is None else ls_.ctypes.data_as(dp), los[1], g, Q_, ln)

    spec = (MF.MATERN05, MF.MATERN15, 2, G, Q)
    assert rc(D, spec[0], 2, spec[1], G, Q) == _hip.OK
    c.D, c.additive, c.relationship, c.Q = D, False, True, Q
    want = SF.kernel_matrix(spec, ls, los, x)
    assert relerr(c.kernel_matrix(x), want) < 1e-13
    bad_nan, bad_sym = G.copy(), G.copy()
    bad_nan[1, 2] = bad_nan[2, 1] = np.nan
    bad_sym[0, 3] = np.nextafter(bad_sym[0, 3], 1.0)
    # D outside 2..8, an unknown form on either side, a bad split with and without the id, Q < 0, a table without the term, a
    # table that is not finite / not symmetric, no lengthscales
    for bad in ((1, 1, 1, 1, None, 0), (9, 1, 2, 1, G, Q), (D, -1, 2, 1, G, Q), (D, 4, 2, 1, G, Q), (D, 1, 2, 4, G, Q), (D, 1, 2, -1, G, Q),
                (D, 1, 0, 1, G, Q), (D, 1, 3, 1, G, Q), (D, 1, 0, 1, None, 0), (D, 1, 4, 1, None, 0), (D, 1, 2, 1, None, -3),
                (D, 1, 2, 1, G, 0), (D, 1, 2, 1, bad_nan, Q), (D, 1, 2, 1, bad_sym, Q), (D, 1, 2, 1, G, Q, None), (2, 1, 1, 1, None, 3)):
        assert rc(*bad) == _hip.ERR_BAD_ARG, bad[:4]
        assert relerr(c.kernel_matrix(x), want) < 1e-13              # the context survives, with the hyper-parameters it had
    assert rc(D, 1, 2, 1, bad_sym, Q) == _hip.ERR_BAD_ARG and b'bitwise symmetric' in c.lib.algp_last_error(c.h)
    # every pair of forms, a table and the identity; and without the term (all four coordinates spatial, the split up to D - 1)
    ls4 = np.ascontiguousarray(np.log([3.0, 2.0, 1.5, 2.5]))
    for ka, kb in PAIRS:
        for G_ in (G, None):
            assert rc(D, ka, 1, kb, G_, Q) == _hip.OK
            assert relerr(c.kernel_matrix(x), SF.kernel_matrix((ka, kb, 1, G_, Q), ls, los, x)) < 1e-13
        assert rc(D, ka, 3, kb, None, 0, ls4) == _hip.OK
        assert relerr(c.kernel_matrix(x), SF.kernel_matrix((ka, kb, 3, None, 0), ls4, los[0], x)) < 1e-13
    # bad ids where coordinates meet the hyper-parameters; the message names the row and the refused call changes nothing
    set_sep(c, spec, ls, los, ln)
    for row, val in ((2, 1.5), (0, -1.0), (3, float(Q))):
        xb = x.copy()
        xb[row, 3] = val
        with pytest.raises(ValueError, match='row %d' % row):
            c.kernel_matrix(xb)
        with pytest.raises(ValueError, match='x2: row %d' % row):
            c.kernel_matrix(x, xb)
    c.set_pool(x)
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])
    c.factorize()
    g_before, mll_before = c.mll_grad(), c.mll()
    assert g_before.shape == (D + 2,)
    xb = x.copy()
    xb[1, 3] = 7.0
    with pytest.raises(ValueError, match='set_pool: row 1'):
        c.set_pool(xb)
    assert c.n_pool == 4 and c.mll() == mll_before and np.array_equal(c.mll_grad(), g_before)      # pool, train set and factor stayed
    with pytest.raises(ValueError, match='resident pool: row 1'):
        c.set_hypers_separable(ls, 2, los[0], ln, log_outputscale_g=los[1], n_genotypes=3)          # the pool holds id 3
    assert c.mll() == mll_before and np.array_equal(c.mll_grad(), g_before)
    assert relerr(c.kernel_matrix(x), want) < 1e-13
    # the component and genotype calls: there with the term, ERR_STATE without it
    assert c.posterior_mean_component(1, [3]).shape == (1,) and c.genotype_posterior()[0].shape == (Q,)
    set_sep(c, (MF.MATERN05, MF.MATERN05, 2, None, 0), ls4, los[0], ln)
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])          # the pool was rescaled and kept: the ids are coordinates now
    c.factorize()
    assert c.mll_grad().shape == (D + 2,) and c.fit_step()[1].shape == (D + 2,) and c.mll_ai().shape == (D + 2, D + 2)
    out = np.zeros(3)
    assert c.lib.algp_posterior_mean_component(c.h, 0, _hip._i64(np.arange(3)), 3, _hip._ptr(out)) == _hip.ERR_STATE
    assert b'additive shares' in c.lib.algp_last_error(c.h)
    assert c.lib.algp_genotype_posterior(c.h, _hip._ptr(np.zeros(Q)), None, None) == _hip.ERR_STATE
    with pytest.raises(ValueError):
        c.genotype_posterior()
    # round trips: single (D + 2), additive (D + 3), relationship (D + 2) and back: the same bits as before
    c.set_hypers(ls4, los[0], ln, MF.MATERN25)
    assert relerr(c.kernel_matrix(x), MF.kernel_matrix(MF.MATERN25, ls4, los[0], x)) < 1e-13
    c.set_hypers_additive(ls4, 2, los[0], los[1], ln, MF.MATERN15, MF.RBF)
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])
    c.factorize()
    assert c.mll_grad().shape == (D + 3,)
    c.set_hypers_relationship(ls, los[0], los[1], ln, kernel_a=MF.RBF, G=G)
    assert relerr(c.kernel_matrix(x), RL.kernel_matrix((MF.RBF, G, Q), ls, los, x)) < 1e-13
    set_sep(c, spec, ls, los, ln)
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])
    c.factorize()
    assert np.array_equal(c.mll_grad(), g_before) and c.mll() == mll_before
    c.close()


def test_abi_fp32_id_range():
    """Q = 20 000 with G = NULL in fp32 is held exactly; 2^24 + 1 genotypes are refused (tests/test_relationship_kernel.py)."""
    c = _hip.Context(np.float32)
    ls, los, ln = np.log([2.0, 1.5]), (np.log(0.8), np.log(0.5)), np.log(1e-2)
    spec = (MF.RBF, MF.MATERN05, 1, None, 20000)
    set_sep(c, spec, ls, los, ln)
    x = np.array([[0.0, 0.5, 19999.0], [1.0, 0.0, 19998.0], [2.0, 1.0, 19999.0], [3.0, 2.0, 0.0]])
    assert relerr(c.kernel_matrix(x), SF.kernel_matrix(spec, ls, los, x)) < kval_tol(np.float32)
    with pytest.raises(ValueError, match='2\\^24'):
        c.set_hypers_separable(ls, 1, los[0], ln, log_outputscale_g=los[1], n_genotypes=2 ** 24 + 1)
    assert relerr(c.kernel_matrix(x), SF.kernel_matrix(spec, ls, los, x)) < kval_tol(np.float32)
    c.close()


# ---------------------------------------------------------------------------------------------------- 2. kernel matrix
KM_LOG_OS = (np.log(1.7), np.log(0.6))
# (Da, Db, with the id): DP = 2, 4, 8, 8 without it; 4, 4, 8 with it
KM_SPLITS = [(1, 1, False), (2, 1, False), (1, 7, False), (5, 3, False), (1, 1, True), (2, 1, True), (3, 4, True)]


@functools.lru_cache(maxsize=None)
def kmat_problem(Da, Db, with_id):
    """TM.kmat_inputs in Da + Db dimensions (x1[150] = x1[7], x2[3] = x1[5], x1[199] and x2[69] 10^4 lengthscales away), with an id
    column behind them where asked for (the coincident sites share their ids)."""
    q = TM.kmat_inputs(Da + Db)
    if not with_id:
        return types.SimpleNamespace(log_ls=q.log_ls, log_noise=q.log_noise, var=q.var, x1=q.x1, x2=q.x2, g1=None, g2=None)
    rng = np.random.RandomState(190 + Da + Db)
    g1, g2 = rng.randint(N_GENO, size=200), rng.randint(N_GENO, size=70)
    g1[150], g2[3] = g1[7], g1[5]
    return types.SimpleNamespace(log_ls=q.log_ls, log_noise=q.log_noise, var=q.var, x1=np.column_stack([q.x1, g1]),
                                 x2=np.column_stack([q.x2, g2]), g1=g1, g2=g2)


@dtypes
@pytest.mark.parametrize('Da,Db,with_id', KM_SPLITS, ids=['%d+%d%s' % (a, b, '+id' if i else '') for a, b, i in KM_SPLITS])
def test_kernel_matrix_every_split(Da, Db, with_id, dt):
    """tests/test_additive_kernel.py::test_kernel_matrix_every_pair_of_forms on its shapes (200 x 200 symmetric, 130 x 70 cross: a
    tile edge plus and minus one) for the four pairs, every split and, with the id, G NULL and dense.  The diagonal is exactly
    os (+ os_g G_gg); a site 10^4 lengthscales away keeps exactly the genotype term (0 without it, not NaN)."""
    q = kmat_problem(Da, Db, with_id)
    t = kval_tol(dt)
    T = np.dtype(dt).type
    c = _hip.Context(dt)
    for pair in PAIRS:
        for variant in (('identity', 'marker') if with_id else ('plain',)):
            spec = spec_of(variant, pair, Da)
            los = log_os_of(variant, KM_LOG_OS)
            set_sep(c, spec, q.log_ls, los, q.log_noise)
            K = c.kernel_matrix(q.x1)
            Kw = SF.kernel_matrix(spec, q.log_ls, los, q.x1)
            assert K.dtype == np.dtype(dt) and K.shape == (200, 200) and np.all(np.isfinite(K))
            assert relerr(K, Kw) < t, (pair, variant)
            assert np.array_equal(K, K.T)
            if with_id:
                gpart = T(np.exp(KM_LOG_OS[1])) * SF.table(spec).astype(dt)               # one rounded product, as the kernels form it
                assert np.all(np.diag(K) == T(np.exp(KM_LOG_OS[0])) + gpart[q.g1, q.g1])  # exactly os + os_g G_gg
                assert np.all(K[199, :199] == gpart[q.g1[199], q.g1[:199]])              # the product exactly 0, not NaN
            else:
                assert np.all(np.diag(K) == T(np.exp(KM_LOG_OS[0])))
                assert np.all(K[199, :199] == 0) and np.all(K[:199, 199] == 0)
            assert K[7, 150] == K[7, 7] == K[150, 150]                                   # r = 0 off the diagonal
            Kx = c.kernel_matrix(q.x1[:130], q.x2)
            assert Kx.shape == (130, 70) and np.all(np.isfinite(Kx))
            assert relerr(Kx, SF.kernel_matrix(spec, q.log_ls, los, q.x1[:130], q.x2)) < t, (pair, variant)
            assert Kx[5, 3] == K[5, 5]
            Kd = c.kernel_matrix(q.x1, diag_add=q.var, add_likelihood_var=True)
            assert relerr(Kd, Kw + np.diag(q.var) + np.exp(q.log_noise) * np.eye(200)) < t, (pair, variant)
    c.close()


# ---------------------------------------------------------------------------------------------------- 3. MLL, gradient, fit_step
MLL_LOG_OS, MLL_LOG_NOISE = (np.log(0.9), np.log(0.5)), np.log(0.05)
MLL_N = TA.MLL_N                                     # one row, 64 +- 1, a few tiles, a site listed twice
# (variant, pair, Da, Db): every pair, every variant and DP = 2, 4, 8 at least once, the id in the last coordinate of its width too
MLL_MODELS = [('plain', 3, 1, 1), ('plain', 0, 2, 1), ('plain', 1, 5, 3), ('plain', 2, 1, 7),
              ('identity', 3, 1, 1), ('marker', 0, 2, 1), ('marker', 1, 3, 4), ('identity', 2, 1, 2)]
MLL_IDS = ['%s-%s-%d+%d' % (v, PIDS[p], a, b) for v, p, a, b in MLL_MODELS]


@functools.lru_cache(maxsize=None)
def mll_problem(model, N, twice):
    """tests/test_relationship_kernel.py:mll_problem with Da + Db spatial coordinates and, under the genotype variants, an id
    column; `twice`: rows 5 and N - 3 name one pool site."""
    variant, pi, Da, Db = model
    nsp = Da + Db
    rng = np.random.RandomState(3)
    # the side grows with the width as test_fit_regimes._side's does, so that a product over eight coordinates is no identity
    xs = _f32(rng.uniform(0, 6, (200, nsp)))[:N]
    geno = rng.randint(N_GENO, size=200)[:N]
    eff = rng.standard_normal(N_GENO)
    noise = rng.standard_normal(200)[:N]
    var = rng.uniform(0.005, 0.05, 200)[:N]
    spec = spec_of(variant, PAIRS[pi], Da)
    x = np.column_stack([xs, geno]) if SF.has_g(spec) else xs
    y = np.sin(xs[:, 0]) + (0.6 * eff[geno] if SF.has_g(spec) else 0.0) + 0.1 * noise
    idx = np.arange(N)
    if twice:
        idx[N - 3] = 5
    th = (np.log([1.3, 2.1, 2.8, 1.6, 3.1, 2.4, 1.9, 2.6])[:nsp], log_os_of(variant, MLL_LOG_OS), MLL_LOG_NOISE)
    xa = x[idx]
    q = types.SimpleNamespace(x=x, y=y, var=var, idx=idx, th=th, spec=spec, P=x.shape[1] + 2)
    q.S = SF.train_matrix(spec, th[0], th[1], th[2], xa, var, idx)
    q.mll = SF.mll(spec, th[0], th[1], th[2], xa, y, var, idx)
    q.grad = SF.mll_grad(spec, th[0], th[1], th[2], xa, y, var, idx)
    return q


@dtypes
@pytest.mark.parametrize('model', MLL_MODELS, ids=MLL_IDS)
@pytest.mark.parametrize('N,twice', MLL_N, ids=['N%d%s' % (n, '-site-twice' if t else '') for n, t in MLL_N])
def test_mll_and_gradient(model, N, twice, dt):
    """tests/test_additive_kernel.py::test_mll_and_gradient for the D + 2 gradient of this kernel.  fp64: tests/test_host_api.py:143-145
    (MLL 1e-10 relative, gradient 1e-8 of its largest entry); fp32: tests/test_fit_regimes.py:49 (2e-2).  The gradient is the same
    bits in two calls, fit_step agrees with the separate calls (tests/test_fold.py:213-214) and repeats bit for bit."""
    q = mll_problem(model, N, twice)
    c = _hip.Context(dt)
    set_sep(c, q.spec, *q.th)
    c.set_pool(q.x)
    c.set_train(q.idx, q.y, q.var)
    c.factorize()
    mll, g = c.mll(), c.mll_grad()
    print('mll %.12e (want %.12e)  grad err %.2e' % (mll, q.mll, float(np.max(np.abs(g - q.grad)))))
    assert g.shape == (q.P,) and np.isfinite(mll) and np.all(np.isfinite(g))
    if np.dtype(dt) == np.float64:
        assert mll == pytest.approx(q.mll, rel=1e-10)
        assert relerr(g, q.grad) < 1e-8
    else:
        assert abs(mll - q.mll) <= 2e-2 * abs(q.mll)
        assert np.max(np.abs(g - q.grad) / np.maximum(1.0, np.abs(q.grad))) <= 2e-2
    assert np.array_equal(c.mll_grad(), g)
    mll_s, g_s = c.fit_step()
    assert g_s.shape == (q.P,)
    assert abs(mll_s - mll) <= tol(dt, 1e-12, 1e-6) * abs(mll)                            # tests/test_fold.py:213-214
    assert np.max(np.abs(g_s - g) / np.maximum(1.0, np.abs(g))) <= tol(dt, 1e-10, 2e-3)
    mll_b, g_b = c.fit_step()
    assert mll_b == mll_s and np.array_equal(g_b, g_s)
    c.close()


# ---------------------------------------------------------------------------------------------------- 4. AI and REML
LOG_OS, LOG_OS2, LOG_NOISE = TAI.LOG_OS, TAI.LOG_OS2, TAI.LOG_NOISE
# (variant, pair, Da, Db, N): test_average_information.py's TWO_PART sizes (129, 513), every variant and DP = 2, 4, 8
AI_MODELS = [('plain', 3, 1, 1, 129), ('plain', 0, 1, 1, 513), ('identity', 2, 2, 1, 129), ('marker', 1, 3, 4, 129),
             ('marker', 3, 1, 1, 513)]
AI_IDS = ['%s-%s-%d+%d-N%d' % (v, PIDS[p], a, b, n) for v, p, a, b, n in AI_MODELS]
FX_M = 40


@functools.lru_cache(maxsize=None)
def ai_case(model, p):
    """test_fixed_effects.py's _case for this kernel: test_fit_regimes._draw's inputs (N train sites and FX_M candidates), the
    hyper-parameters of test_average_information.py, an id column under the genotype variants, a planted H beta on
    reml_forms.basis with p columns (p = 0: no basis, the MLL's average information alone).  cond(S) <= 1e3 and the scaled
    cond(H' S^-1 H) <= 1e2 are asserted: the conditions of the bounds."""
    variant, pi, Da, Db, N = model
    nsp = Da + Db
    x, y, var, log_ls = FR._draw(N, nsp, N + FX_M)
    rng = np.random.RandomState(N + nsp + p)
    spec = spec_of(variant, PAIRS[pi], Da)
    if SF.has_g(spec):
        x = np.c_[x, rng.randint(0, N_GENO, len(x)).astype(np.float64)]
    idx, cand = np.arange(N), np.arange(N, N + FX_M)
    theta = SF.pack(log_ls, log_os_of(variant, (LOG_OS, LOG_OS2)), LOG_NOISE)
    ev = np.linalg.eigvalsh(SF.train_matrix(spec, *SF.unpack(spec, theta, x), x[idx], var))
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e3, 'the inputs are worse conditioned than the tolerances were set for'
    out = dict(model=model, spec=spec, theta=theta, x=x, var=var, idx=idx, cand=cand, p=p)
    if p == 0:
        out.update(y=y, want=dict(ai=SF.average_information(spec, theta, x[idx], y, var)))
        return out
    H = RM.basis(x[:, :nsp], p)
    y = y + H[idx] @ RM.planted_beta(p)
    args = (spec, theta, x[idx], y, H[idx])
    with SF._in_reml_forms(spec):
        assert RM.scaled_cond(RM.gram(SF.FAMILY, spec, theta, x[idx], H[idx], var)) <= 1e2
    b, cov = SF.gls(*args, var)
    post = SF.posterior_fixed(*args, x[cand], H[cand], var)
    out.update(y=y, H=H, want=dict(beta=b, cov=cov, reml=SF.reml(*args, var), mu=post['mu'], var=post['var'], proj=post['proj'],
                                   grad=SF.reml_grad(*args, var), ai=SF.reml_ai(*args, var)))
    return out


def _load(c, case):
    set_sep(c, case['spec'], *SF.unpack(case['spec'], case['theta'], case['x']))
    c.set_pool(case['x'])
    if case['p']:
        c.set_fixed_effects(case['H'])
    c.set_train(case['idx'], case['y'], case['var'])


@dtypes
@pytest.mark.parametrize('model', AI_MODELS, ids=AI_IDS)
def test_average_information(model, dt):
    """algp_get_mll_ai against the helper at tests/test_average_information.py's bound (test_fit_regimes.TOL, per entry relative
    to sqrt(AI_aa AI_bb)), as its _check does: symmetric bit for bit, positive semi-definite, the same bits twice."""
    case = ai_case(model, 0)
    c = _hip.Context(dt)
    _load(c, case)
    c.fit_step()
    ai = c.mll_ai()
    P = len(case['theta'])
    err = TAI._error(ai, case['want']['ai'])
    print('%s %s: AI error %.3e' % (np.dtype(dt).name, model, err))
    assert ai.shape == (P, P) and np.all(np.isfinite(ai)) and err <= FR.TOL[np.dtype(dt)]
    assert np.array_equal(ai, ai.T) and np.array_equal(c.mll_ai(), ai)
    ev = np.linalg.eigvalsh(ai)
    assert ev[0] >= -FR.TOL[np.dtype(dt)] * ev[-1]
    c.close()


@dtypes
@pytest.mark.parametrize('p', [1, 3])
@pytest.mark.parametrize('model', AI_MODELS, ids=AI_IDS)
def test_restricted_likelihood_and_fixed_effects(model, p, dt):
    """algp_get_gls, algp_get_reml_grad, algp_get_reml_ai, algp_reml_step and algp_get_posterior_fixed against the helper (through
    tests/reml_forms.py) at tests/test_fixed_effects.py's bounds: its TOL for beta, cov beta, mu, var and proj, TOL_REML for l_R,
    test_fit_regimes.TOL for the gradient and AI_R; reml_step against the separate calls as its
    test_reml_step_is_the_three_separate_calls holds them below test_fit_regimes.PANEL_FROM rows: the same bits."""
    case = ai_case(model, p)
    want = case['want']
    dtn = np.dtype(dt)
    c = _hip.Context(dt)
    _load(c, case)
    c.factorize()
    c.set_candidates(case['cand'], prior_includes_noise=False)
    c.solve_candidates()
    beta, cov, reml = c.gls()
    grad, ai = c.reml_grad(), c.reml_ai()
    mu, var, proj = c.posterior_fixed(want_var=True, want_proj=True)
    P = len(case['theta'])
    assert grad.shape == (P,) and ai.shape == (P, P)
    err = dict(beta=TFX._vec_err(beta, want['beta']), cov=TAI._error(cov, want['cov']), mu=TFX._vec_err(mu, want['mu']),
               var=TFX._vec_err(var, want['var']), proj=TFX._vec_err(proj, want['proj']), reml=abs(reml - want['reml']) / abs(want['reml']),
               grad=TFX._vec_err(grad, want['grad']), ai=TAI._error(ai, want['ai']))
    print('%s %s p=%d: %s' % (dtn.name, model, p, '  '.join('%s %.2e' % kv for kv in sorted(err.items()))))
    for k in ('beta', 'cov', 'mu', 'var', 'proj'):
        assert err[k] <= TFX.TOL[dtn], (k, err)
    assert err['reml'] <= TFX.TOL_REML[dtn], err
    assert err['grad'] <= FR.TOL[dtn] and err['ai'] <= FR.TOL[dtn], err
    assert np.array_equal(ai, ai.T) and np.array_equal(c.reml_ai(), ai)
    v2, g2 = c.reml_step()
    assert case['model'][4] < FR.PANEL_FROM and v2 == reml and np.array_equal(g2, grad)
    c.close()


# ---------------------------------------------------------------------------------------------------- 5. criteria on a pool
POOL_LOG_OS = (np.log(0.7), np.log(0.4))
POOL_LOG_NOISE = TM.LOG_NOISE
# (variant, pair): split (1, 1) over (row, col) -- AR1 x AR1 with and without the term, and the other three pairs once each
POOL_MODELS = [('plain', 3), ('plain', 0), ('identity', 2), ('marker', 1), ('marker', 3)]
POOL_IDS = ['%s-%s' % (v, PIDS[p]) for v, p in POOL_MODELS]
# model -> (the two lengthscales, the seed of the ids and of y): chosen on the CPU with the helper and the references alone so that
# every compared pick is separated (tests/test_separable_forms_host.py asserts it)
POOL_TUNE = {('plain', 3): ([4.0, 3.0], 0), ('plain', 0): ([3.0, 2.0], 0), ('identity', 2): ([3.0, 3.0], 7), ('marker', 1): ([3.0, 2.0], 3),
             ('marker', 3): ([3.0, 3.0], 2)}
pools = pytest.mark.parametrize('model', POOL_MODELS, ids=POOL_IDS)


@functools.lru_cache(maxsize=None)
def pool_problem(model):
    """tests/test_matern_family.py:pool_problem (300 sites, 80 train rows, six sites outside the covered square), (row | col) the
    two factors' coordinates, with a genotype id behind them under the genotype variants.  Under the marker table the candidates'
    prior variances os + os_g G_gg differ from site to site."""
    variant, pi = model
    base = TM.pool_problem(MF.MATERN15)
    spec = spec_of(variant, PAIRS[pi], 1)
    log_ls, seed = np.log(POOL_TUNE[model][0]), POOL_TUNE[model][1]
    rng = np.random.RandomState(seed)
    geno = rng.randint(N_GENO, size=base.n)
    effect = rng.standard_normal(N_GENO)
    X = np.column_stack([base.X, geno]) if SF.has_g(spec) else np.array(base.X)
    p = types.SimpleNamespace(spec=spec, model=model, n=base.n, X=X, geno=geno, static=base.static, mobile=base.mobile, A=base.A, N=base.N,
                              var=base.var, cand=base.cand, alive=base.alive, free=base.free, log_ls=log_ls, log_os=log_os_of(variant, POOL_LOG_OS))
    p.y = np.sin(X[p.A, 0] / 3.0) + (0.5 * effect[geno[p.A]] if SF.has_g(spec) else 0.0) + 0.1 * rng.standard_normal(p.N)
    p.K = SF.kernel_matrix(spec, log_ls, p.log_os, X)
    p.C = p.K + np.exp(POOL_LOG_NOISE) * np.eye(p.n)
    p.S = p.C[np.ix_(p.A, p.A)] + np.diag(p.var)
    for a in (p.X, p.C, p.K, p.S, p.y):
        a.setflags(write=False)
    p.memo = {}
    return p


def _pool_ctx(p, dt, explicit, cand=None, alive=None, prior_includes_noise=True, solve=True):
    """Context A (coordinates and the separable kernel) or B (the helper's matrix as an explicit pool covariance)."""
    c = _hip.Context(dt)
    if explicit:
        c.set_hypers(p.log_ls, 0.0, POOL_LOG_NOISE, _hip.KERNEL_RBF)
        c.set_pool_cov(p.C)
    else:
        set_sep(c, p.spec, p.log_ls, p.log_os, POOL_LOG_NOISE)
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


target_weights, wvr_reference = TA.target_weights, TA.wvr_reference           # the additive file's, on this file's pool problems


@pools
@dtypes
def test_pool_posterior_and_covariance(model, dt):
    """tests/test_relationship_kernel.py::test_pool_posterior_and_covariance: mean and variance at the 220 free sites, both contexts
    and both prior_includes_noise settings on the coordinate pool, against the helper (tests/test_rhs_fused.py:22 as its
    _check_oracle applies it); the posterior covariance at tests/test_posterior_cov_regimes.py:143's bound."""
    p = pool_problem(model)
    mu_w, pv_w = _memo(p, 'post', lambda: SF.posterior(p.spec, p.log_ls, p.log_os, POOL_LOG_NOISE, p.X[p.A], p.y, p.var, p.X[p.free]))
    if model[0] == 'marker':
        assert np.ptp(SF.prior_var(p.spec, p.log_os, p.X[p.free])) > 0.05
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


@pools
@dtypes
def test_pool_entropy_picks(model, dt):
    """tests/test_additive_kernel.py::test_pool_entropy_picks (tests/test_greedy_regimes.py:169-179, bounds :165-166)."""
    p = pool_problem(model)
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


@pools
@dtypes
def test_pool_mi_picks(model, dt):
    """tests/test_additive_kernel.py::test_pool_mi_picks: every utility along the reference's picks at tests/test_hip_greedy.py:417's
    tolerance (1e-7 / 3e-3 of the largest utility), both contexts; the free run's picks in fp64, where the gap is resolved."""
    p = pool_problem(model)
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


@pools
@dtypes
def test_pool_variance_reduction_and_target_weights(model, dt):
    """tests/test_additive_kernel.py::test_pool_variance_reduction_and_target_weights (tests/test_variance_reduction.py:
    vr_reference, compare, TOL at :52; tests/test_target_weights.py for the weights): three rounds along the brute force's picks,
    then the free run's picks, without and with target weights."""
    p = pool_problem(model)
    t = VR.TOL[dt]
    for weighted in (False, True):
        picks_o, U = wvr_reference(p) if weighted else vr_reference(p)
        for r in range(3):
            top = np.sort(U[r][np.isfinite(U[r])])[-2:]
            assert (top[1] - top[0]) / top[1] > 2 * t, 'the inputs no longer separate the picks'  # test_variance_reduction.py:206-209
        for explicit in (False, True):
            c = _pool_ctx(p, dt, explicit, alive=p.alive)
            if weighted:
                c.set_target_weights(target_weights(p))
            got_p, got_u = c.greedy(VRC, S_STD, M_STD, 3, forced_picks=picks_o, want_utilities=True)
            assert [int(v) for v in got_p] == picks_o
            for r in range(3):
                VR.compare(got_u[r], U[r], t, '%s%s round %d' % ('weighted ' if weighted else '', 'explicit' if explicit else 'coordinates', r))
            c.solve_candidates(alive=p.alive)
            assert [int(v) for v in c.greedy(VRC, S_STD, M_STD, 3)] == picks_o
            c.close()


@pools
@dtypes
def test_score_paths_three_criteria(model, dt):
    """tests/test_additive_kernel.py::test_score_paths_three_criteria with its path constructions on this file's pool problem:
    score_paths on both routes (tolerances tests/test_hip_greedy.py:565, :617), score_paths_mi (tests/test_mi_paths.py:119) and
    score_paths_vr (tests/test_paths_vr.py:37), coordinates and explicit covariance."""
    p = pool_problem(model)
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


# ---------------------------------------------------------------------------------------------------- 6. solve routes, updates
ROUTE_LOG_LS, ROUTE_LOG_OS = np.log([3.0, 3.0]), (np.log(0.6), np.log(0.5))
ROUTE_MODELS = [('plain', 3), ('marker', 0), ('identity', 1)]
ROUTE_IDS = ['%s-%s' % (v, PIDS[p]) for v, p in ROUTE_MODELS]


@functools.lru_cache(maxsize=None)
def mid_problem(model):
    """tests/test_matern_family.py:mid_problem (N = 300, M = 700: the one-launch and mid-sized solves), split (1, 1), with an id
    column under the genotype variants."""
    variant, pi = model
    base = TM.mid_problem(MF.MATERN15)
    spec = spec_of(variant, PAIRS[pi], 1)
    rng = np.random.RandomState(8)
    pool = np.column_stack([base.pool, rng.randint(N_GENO, size=len(base.pool))]) if SF.has_g(spec) else base.pool
    los = log_os_of(variant, ROUTE_LOG_OS)
    mu, pv = SF.posterior(spec, ROUTE_LOG_LS, los, TM.LOG_NOISE, pool[base.A], base.y, base.var, pool[base.cidx])
    S = SF.train_matrix(spec, ROUTE_LOG_LS, los, TM.LOG_NOISE, pool[base.A], base.var)
    return types.SimpleNamespace(pool=pool, A=base.A, y=base.y, var=base.var, cidx=base.cidx, mu=mu, pv=pv, S=S, spec=spec, log_os=los,
                                 logdet=np.linalg.slogdet(S)[1])


@pytest.mark.parametrize('model', ROUTE_MODELS, ids=ROUTE_IDS)
@pytest.mark.parametrize('dt,t', [(np.float64, 1e-9), (np.float32, 2e-3)], ids=DIDS)     # tests/test_fold.py:41
def test_fit_and_solve_and_the_mean_only_posterior(model, dt, t, monkeypatch):
    """tests/test_additive_kernel.py::test_fit_and_solve_and_the_mean_only_posterior: the folded launch and its two phases."""
    q = mid_problem(model)
    c = _hip.Context(dt)
    set_sep(c, q.spec, ROUTE_LOG_LS, q.log_os, TM.LOG_NOISE)
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
    """tests/test_matern_family.py:fused_problem (51 300 candidates, 1 400 train rows: the scheduled sweep) under AR1 x AR1 without
    the genotype term: DP = 2, where a single kernel generates its right-hand sides."""
    base = TM.fused_problem(MF.MATERN15)
    spec = spec_of('plain', PAIRS[3], 1)
    mu, pv = SF.posterior(spec, ROUTE_LOG_LS, ROUTE_LOG_OS[0], TM.LOG_NOISE, base.pool[base.A], base.y, base.var, base.pool[base.cidx[base.samp]])
    return types.SimpleNamespace(base=base, spec=spec, ref=dict(mu=mu, var=pv))


@dtypes
def test_scheduled_sweep_takes_the_materialised_route(dt, monkeypatch):
    """tests/test_additive_kernel.py::test_scheduled_sweep_takes_the_materialised_route: under this kernel the sweep reads its
    right-hand sides from V^T whatever ALGP_RHS_FUSED says -- the same bits, the full kernel-matrix traffic -- and meets the
    helper at tests/test_rhs_fused.py:22."""
    q = sweep_problem()
    b = q.base
    c = _hip.Context(dt)
    set_sep(c, q.spec, ROUTE_LOG_LS, ROUTE_LOG_OS[0], TM.LOG_NOISE)
    c.set_pool(b.pool)
    c.set_train(b.A, b.y, b.var)
    c.factorize()
    c.set_candidates(b.cidx, prior_includes_noise=False)
    (mu, pv), (mu2, pv2), (mu0, pv0) = RF._posteriors(c, monkeypatch)
    RF._check_oracle(mu, pv, b.samp, q.ref, RF.TOL[dt], what='separable')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)                  # ALGP_RHS_FUSED=0: bit for bit
    full, _ = RF._expected_bytes(TM.FUSED_M, TM.FUSED_N, np.dtype(dt).itemsize)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    assert RF._kmat_bytes(c) == full                                           # nothing was generated in an epilogue
    monkeypatch.delenv('ALGP_RHS_FUSED')
    c.close()


@pools
@dtypes
def test_incremental_update_equals_from_scratch(model, dt):
    """tests/test_additive_kernel.py::test_incremental_update_equals_from_scratch (tests/test_incremental.py:196, :246)."""
    p = pool_problem(model)
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
    set_sep(f, p.spec, p.log_ls, p.log_os, POOL_LOG_NOISE)
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
    mu_w, pv_w = SF.posterior(p.spec, p.log_ls, p.log_os, POOL_LOG_NOISE, p.X[A2], y2, var2, p.X[p.free[5:]])
    RF._check_oracle(mu, pv, np.arange(len(mu)), dict(mu=mu_w, var=pv_w), RF.TOL[dt], what='updated')


# ---------------------------------------------------------------------------------------------------- 7. posteriors
GENO_MODELS = [m for m in POOL_MODELS if m[0] != 'plain']
genos = pytest.mark.parametrize('model', GENO_MODELS, ids=['%s-%s' % (v, PIDS[p]) for v, p in GENO_MODELS])


@genos
@dtypes
def test_component_means(model, dt):
    """tests/test_relationship_kernel.py::test_component_means (the mean's own tolerance, tests/test_fold.py:186): 0 + 1 + ybar =
    posterior_mean; component 1 at a site is genotype_posterior's mean of the site's id."""
    p = pool_problem(model)
    ms_w, mg_w = _memo(p, 'comp', lambda: SF.component_means(p.spec, p.log_ls, p.log_os, POOL_LOG_NOISE, p.X[p.A], p.y, p.var, p.X[p.free]))
    c = _pool_ctx(p, dt, False, solve=False)
    ms, mg = c.posterior_mean_component(0, p.free), c.posterior_mean_component(1, p.free)
    mu = c.posterior_mean(p.free)
    gm, _, _ = c.genotype_posterior()
    scale = max(1.0, float(np.max(np.abs(ms_w + mg_w + p.y.mean()))))
    t = tol(dt, 1e-8, 2e-2)
    assert ms.dtype == np.dtype(dt) and ms.shape == (len(p.free),)
    assert np.max(np.abs(ms - ms_w)) <= t * scale and np.max(np.abs(mg - mg_w)) <= t * scale
    assert np.max(np.abs(ms.astype(np.float64) + mg + p.y.mean() - mu)) <= tol(dt, 1e-12, 1e-5) * scale
    assert np.max(np.abs(mg - gm[p.geno[p.free]])) <= tol(dt, 1e-12, 1e-5) * scale
    assert np.std(ms_w) > 0.05 and np.std(mg_w) > 0.05                          # both parts carry signal here
    for comp in (-1, 2):
        with pytest.raises(ValueError):
            c.posterior_mean_component(comp, p.free)
    c.close()


GP_SHAPES = [(12, 150), (130, 300)]                                            # tests/test_relationship_kernel.py: neither a multiple of 128
GP_LOG_LS, GP_LOG_OS, GP_LOG_NOISE = np.log([3.0, 2.0]), (np.log(0.7), np.log(0.5)), np.log(2e-2)
GP_BAR = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}               # tests/test_relationship_kernel.py's GP_BAR, as derived there


@functools.lru_cache(maxsize=None)
def genotype_problem(tab, Q, N):
    """tests/test_relationship_kernel.py:genotype_problem under AR1 x AR1 over (row | col): N plots with Q genotypes, the last of
    which is on no plot."""
    rng = np.random.RandomState(100 + Q)
    pos = _f32(rng.uniform(0.0, 12.0, (N, 2)))
    geno = rng.randint(Q - 1, size=N)
    G = None if tab == 'identity' else RL.marker_relationship(Q, 3 * Q + 4, seed=7)
    spec = (MF.MATERN05, MF.MATERN05, 1, G, Q)
    eff = rng.standard_normal(Q)
    x = np.column_stack([pos, geno])
    y = np.sin(pos[:, 0] / 3.0) + 0.7 * eff[geno] + 0.1 * rng.standard_normal(N)
    var = rng.uniform(0.01, 0.05, N)
    q = types.SimpleNamespace(spec=spec, x=x, y=y, var=var, Q=Q, N=N, geno=geno)
    q.S = SF.train_matrix(spec, GP_LOG_LS, GP_LOG_OS, GP_LOG_NOISE, x, var)
    q.mean, q.cov = SF.genotype_posterior(spec, GP_LOG_LS, GP_LOG_OS, GP_LOG_NOISE, x, y, var)
    return q


@pytest.mark.parametrize('tab', ['identity', 'marker'])
@pytest.mark.parametrize('Q,N', GP_SHAPES, ids=['Q%d-N%d' % s for s in GP_SHAPES])
@dtypes
def test_genotype_posterior(tab, Q, N, dt):
    """tests/test_relationship_kernel.py::test_genotype_posterior: mean (tests/test_fold.py:186), var and cov (GP_BAR), the
    unplotted genotype, the same bits twice."""
    q = genotype_problem(tab, Q, N)
    c = _hip.Context(dt)
    set_sep(c, q.spec, GP_LOG_LS, GP_LOG_OS, GP_LOG_NOISE)
    c.set_pool(q.x)
    c.set_train(np.arange(N), q.y, q.var)
    c.factorize()
    mean, var, cov = c.genotype_posterior(want_var=True, want_cov=True)
    bar = GP_BAR[np.dtype(dt)]
    scale = float(np.max(np.abs(q.cov)))
    print('genotype posterior %s Q=%d N=%d: mean %.3g  var %.3g  cov %.3g (bar %g)' % (
        tab, Q, N, relerr(mean, q.mean), float(np.max(np.abs(var - np.diag(q.cov)))) / scale, relerr(cov, q.cov), bar))
    assert mean.shape == (Q,) and var.shape == (Q,) and cov.shape == (Q, Q)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))
    assert np.max(np.abs(mean - q.mean)) <= tol(dt, 1e-8, 2e-2) * max(1.0, np.max(np.abs(q.mean)))
    assert relerr(cov, q.cov) <= bar
    assert np.max(np.abs(var - np.diag(q.cov))) <= bar * scale
    assert np.array_equal(cov, cov.T)                                           # identical bits in both triangles
    T = np.dtype(dt).type
    if tab == 'identity':                                                       # the genotype on no plot stays at its prior, exactly
        assert mean[Q - 1] == 0 and var[Q - 1] == T(np.exp(GP_LOG_OS[1])) and np.all(cov[Q - 1, :Q - 1] == 0)
    else:                                                                       # ... and is predicted through its relatives
        assert abs(q.mean[Q - 1]) > 1e-3 and abs(mean[Q - 1] - q.mean[Q - 1]) <= tol(dt, 1e-8, 2e-2)
    m2, v2, c2 = c.genotype_posterior(want_var=True, want_cov=True)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var) and np.array_equal(c2, cov)
    c.close()


@pools
@dtypes
def test_group_posterior_of_row_strips(model, dt):
    """tests/test_additive_kernel.py::test_group_posterior_of_the_genotypes with the free sites grouped by field row (eight strips
    of the square, the outliers with the nearest): tests/test_group_posterior.py's bar (:37, 1e-5 / 1e-3)."""
    p = pool_problem(model)
    nq = 8
    lab = np.clip(np.floor(p.X[p.free, 0]), 0, nq - 1).astype(np.int32)
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


# ---------------------------------------------------------------------------------------------------- 8. samples
@functools.lru_cache(maxsize=None)
def sample_case(model):
    """Values mode: an exact prior draw on the helper's matrix.  Features mode (without the genotype term): utils.spectral_draws'
    omega -- every row part a's draw and part b's, concatenated -- evaluated in NumPy with the same omega, phase and weights."""
    from algp_amd.utils import spectral_draws
    p = pool_problem(model)
    S, F = 5, 257
    rng = np.random.RandomState(61)
    L = np.linalg.cholesky(p.K + 1e-10 * np.eye(p.n))
    prior = _f32(rng.standard_normal((S, p.n)) @ L.T)
    eps = _f32(rng.standard_normal((S, p.N)))
    v = p.var + np.exp(POOL_LOG_NOISE)
    out = types.SimpleNamespace(prior=prior, eps=eps, ref_values=PF.pathwise(p.K[np.ix_(p.free, p.A)], p.S, p.y, v, prior[:, p.free],
                                                                            prior[:, p.A], eps))
    if not SF.has_g(p.spec):
        om, ph = spectral_draws(('separable', 1, p.spec[0], p.spec[1]), 2, F, rng)
        out.om, out.ph = _f32(om), _f32(ph)
        out.W = _f32(rng.standard_normal((S, F)))
        G = out.W @ PF.features(out.om, out.ph, p.X * np.exp(-p.log_ls)[None, :], np.exp(p.log_os)).T
        out.ref_features = PF.pathwise(p.K[np.ix_(p.free, p.A)], p.S, p.y, v, G[:, p.free], G[:, p.A], eps)
    return out


@pools
@dtypes
def test_posterior_samples(model, dt):
    """tests/test_additive_kernel.py::test_posterior_samples: values mode against tests/pathwise_forms.py on the helper's matrix,
    features mode (Q == 0) against the NumPy evaluation with the same omega, phase and weights, at tests/test_pathwise_samples.py's
    bar (:35, 1e-5 / 1e-3 of the largest draw); with the genotype term features mode is refused, and the message says why."""
    p = pool_problem(model)
    q = sample_case(model)
    c = _pool_ctx(p, dt, False, cand=p.free, prior_includes_noise=False)
    bar = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}[np.dtype(dt)]
    fv = c.sample_posterior(q.eps, prior=q.prior)
    assert fv.shape == (5, len(p.free)) and np.all(np.isfinite(fv))
    print('values %.3g (bar %g)' % (relerr(fv, q.ref_values), bar))
    assert relerr(fv, q.ref_values) <= bar
    if SF.has_g(p.spec):
        rng = np.random.RandomState(2)
        with pytest.raises(ValueError, match='no spectral density'):
            c.sample_posterior(q.eps, weights=rng.standard_normal((5, 64)), omega=rng.standard_normal((64, 3)), phase=rng.uniform(size=64))
        assert np.array_equal(c.sample_posterior(q.eps, prior=q.prior), fv)      # the refusal changed nothing
    else:
        ff = c.sample_posterior(q.eps, weights=q.W, omega=q.om, phase=q.ph)
        print('features %.3g (bar %g)' % (relerr(ff, q.ref_features), bar))
        assert ff.shape == fv.shape and np.all(np.isfinite(ff)) and relerr(ff, q.ref_features) <= bar
    c.close()


# ---------------------------------------------------------------------------------------------------- 9. GPR fits
FIT_RHO, FIT_OS, FIT_OSG, FIT_NOISE = (0.8, 0.6), 1.0, 0.6, 0.05
AR1_PARTS = ({'type': 'matern', 'nu': 0.5}, {'type': 'matern', 'nu': 0.5})


@functools.lru_cache(maxsize=None)
def fit_problem():
    """A 15 x 12 field (180 plots) drawn from AR1(0.8) x AR1(0.6) with unit variance plus the effects of 12 genotypes (variance
    0.6, 15 plots each) plus noise 0.05: (row, col | genotype id)."""
    rng = np.random.RandomState(12)
    R, Cn, Q = 15, 12, 12
    rr, cc = np.meshgrid(np.arange(R), np.arange(Cn), indexing='ij')
    pos = np.column_stack([rr.ravel(), cc.ravel()]).astype(np.float64)
    chol = [np.linalg.cholesky(rho ** np.abs(np.subtract.outer(np.arange(n), np.arange(n)))) for rho, n in zip(FIT_RHO, (R, Cn))]
    field = (chol[0] @ rng.standard_normal((R, Cn)) @ chol[1].T).ravel()
    geno = rng.permutation(np.repeat(np.arange(Q), R * Cn // Q))
    eff = np.sqrt(FIT_OSG) * rng.standard_normal(Q)
    y = field + eff[geno] + np.sqrt(FIT_NOISE) * rng.standard_normal(R * Cn)
    return types.SimpleNamespace(x=np.column_stack([pos, geno]), y=y, var=np.full(R * Cn, 1e-5), geno=geno, eff=eff, Q=Q)


def _fit_kp(with_g):
    sep = {'type': 'separable', 'split': 1, 'parts': AR1_PARTS}
    return {'type': 'genotype', 'spatial': sep, 'relationship': None, 'n_genotypes': 12} if with_g else sep


@pytest.mark.parametrize('with_g', [False, True], ids=['plain', 'genotype'])
@dtypes
def test_gpr_fit_by_adam(with_g, dt):
    """tests/test_relationship_kernel.py::test_gpr_fit_and_genotype_effects: 30 Adam steps raise the likelihood, the trajectory
    repeats bit for bit, and cov_mat / predict / genotype_effects / group_posterior / sample_posterior at the fitted
    hyper-parameters agree with the helper at the tolerances cited there."""
    from algp_amd.models import GPR
    q = fit_problem()
    x = q.x if with_g else q.x[:, :2]
    runs = []
    for _ in range(2):
        gp = GPR(lr=.1, max_iterations=30, kernel_params=_fit_kp(with_g), dtype=dt)
        losses = gp.fit(x, q.y, q.var)
        runs.append((losses, gp.hypers()))
    losses = runs[0][0]
    assert len(losses) == 30 and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1][0], runs[1][1][0]) and runs[0][1][1:] == runs[1][1][1:]
    ls, los, ln, kt = gp.hypers()
    sid = ('separable', 1, _hip.KERNEL_MATERN05, _hip.KERNEL_MATERN05)
    assert kt == (('genotype', sid) if with_g else sid) and ls.shape == (2,)
    spec = (MF.MATERN05, MF.MATERN05, 1, None, 12 if with_g else 0)
    C = gp.cov_mat(x, add_likelihood_var=True)
    assert relerr(C, SF.kernel_matrix(spec, ls, los, x) + np.exp(ln) * np.eye(len(x))) < kval_tol(dt)
    probe = np.column_stack([np.full(12, 7.5), np.full(12, 4.5), np.arange(12)])[:, :x.shape[1]]
    mu_p, var_p = gp.predict(probe, return_std=True)
    mu_w, pv_w = SF.posterior(spec, ls, los, ln, x, q.y, q.var, probe)
    assert np.max(np.abs(mu_p - mu_w)) <= tol(dt, 1e-8, 2e-2) * max(1.0, np.max(np.abs(mu_w)))
    assert np.max(np.abs(var_p - (pv_w + np.exp(ln)))) <= tol(dt, 1e-8, 2e-3)
    gm, gcov = gp.group_posterior(probe, np.arange(12) % 4, n_groups=4)
    assert gm.shape == (4,) and gcov.shape == (4, 4) and np.all(np.isfinite(gcov))
    smp = gp.sample_posterior(probe, n_samples=3, n_features=128, rng=5)
    assert smp.shape == (3, 12) and np.all(np.isfinite(smp))
    if with_g:
        mean, var = gp.genotype_effects()
        mw, cw = SF.genotype_posterior(spec, ls, los, ln, x, q.y, q.var)
        assert np.max(np.abs(mean - mw)) <= tol(dt, 1e-8, 2e-2) * max(1.0, np.max(np.abs(mw)))
        assert np.max(np.abs(var - np.diag(cw))) <= GP_BAR[np.dtype(dt)] * np.max(np.abs(cw))
        ms, mg = gp.predict_components(probe)
        assert np.max(np.abs(ms.astype(np.float64) + mg + q.y.mean() - gp.predict(probe))) <= tol(dt, 1e-10, 1e-4) * max(1.0, np.max(np.abs(q.y)))
    else:
        with pytest.raises(ValueError):
            gp.predict_components(probe)
        with pytest.raises(ValueError):
            gp.genotype_effects()
    gp.ctx.close()


@pytest.mark.parametrize('objective', ['mll', 'reml'])
def test_gpr_fit_by_average_information(objective):
    """tests/test_fixed_effects_fit.py's Newton fit (CAP = 40 evaluations) on the field above under AR1 x AR1 plus genotypes: the
    likelihood rises, the fit's last value is the helper's at its parameters (rel 1e-9, as there), heritability() and
    ar1_correlations() are finite with positive standard errors and equal the closed forms on the helper's average information,
    fixed_effect_estimates() runs under REML."""
    from algp_amd import utils
    from algp_amd.models import GPR
    q = fit_problem()
    gp = GPR(fit_method='ai', max_iterations=40, kernel_params=_fit_kp(True), fit_objective=objective)
    try:
        gp.fit(q.x, q.y, q.var)
        info = gp.fit_info
        assert info['objective'] == objective and info['trace'][-1] > info['trace'][0] and info['iterations'] >= 1
        ls, los, ln, _ = gp.hypers()
        spec = (MF.MATERN05, MF.MATERN05, 1, None, 12)
        theta = SF.pack(ls, los, ln)
        H = np.ones((len(q.y), 1))
        if objective == 'reml':
            assert gp.fixed_effects == 'intercept'
            assert info['trace'][-1] == pytest.approx(SF.reml(spec, theta, q.x, q.y, H, q.var), rel=1e-9)
            beta, cov_b = gp.fixed_effect_estimates()
            bw, cw = SF.gls(spec, theta, q.x, q.y, H, q.var)
            assert np.allclose(beta, bw, rtol=0, atol=1e-8) and cov_b[0, 0] == pytest.approx(cw[0, 0], rel=1e-8)
            ai = SF.reml_ai(spec, theta, q.x, q.y, H, q.var)
        else:
            assert info['trace'][-1] == pytest.approx(SF.mll(spec, ls, los, ln, q.x, q.y, q.var), rel=1e-9)
            ai = SF.average_information(spec, theta, q.x, q.y, q.var)
        cov = np.linalg.inv(ai)
        h2, se = gp.heritability()
        want = utils.heritability(theta[2], theta[3], theta[4], 1.0, cov[2:, 2:])
        print('%s: h2 = %.4f +- %.4f (forms %.4f +- %.4f)' % (objective, h2, se, want[0], want[1]))
        assert 0.0 < h2 < 1.0 and np.isfinite(se) and se > 0
        assert h2 == pytest.approx(want[0], rel=1e-12) and se == pytest.approx(want[1], rel=1e-6)   # tests/test_fixed_effects_fit.py:138
        rho = gp.ar1_correlations()
        for k, (r, s) in enumerate(rho):
            rw = np.exp(-1.0 / np.exp(ls[k]))
            sw = rw / np.exp(ls[k]) * np.sqrt(cov[k, k])
            print('%s: rho_%d = %.4f +- %.4f (simulated %.1f)' % (objective, k, r, s, FIT_RHO[k]))
            assert 0.0 < r < 1.0 and np.isfinite(s) and s > 0
            assert r == pytest.approx(rw, rel=1e-12) and s == pytest.approx(sw, rel=1e-6)
        ses = gp.hyper_standard_errors()
        assert len(ses) == 5 and all(np.isfinite(v) and v > 0 for v in ses.values())
    finally:
        gp.ctx.close()


# ---------------------------------------------------------------------------------------------------- 10. two ranks
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
    c.set_hypers_separable(np.log([3.0, 2.5]), 1, np.log(0.7), np.log(1e-2), kernel_a=_hip.KERNEL_MATERN05,
                           kernel_b=_hip.KERNEL_MATERN15, log_outputscale_g=np.log(0.5), G=G)
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
    print('SHARDED_SEP_OK')
dist.destroy_process_group()
'''


@pytest.mark.parametrize('rows_in_gather', ['1', '0'], ids=['rows-travel', 'rows-rebuilt'])
def test_two_ranks_greedy(tmp_path, rows_in_gather):
    """tests/test_relationship_kernel.py::test_two_ranks_greedy (two processes, a host all-gather over gloo, its time limit) under
    the separable kernel with a table: the sharded entropy picks and utilities equal one rank's.  rows-rebuilt: a remote winner's
    row and its per-site prior are rebuilt from the replicated factor."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'repo': REPO})
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', ALGP_GATHER_ROWS=rows_in_gather)
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                          '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), str(script)],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'SHARDED_SEP_OK' in out.stdout


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]
