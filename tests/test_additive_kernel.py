"""The additive kernel k = os_a kappa_a(r_a) + os_b kappa_b(r_b) (algp_set_hypers_additive) through every layer that evaluates a
kernel value: the ABI, the kernel-matrix build, MLL / gradient / fit_step, the criteria on a coordinate pool against the same
pool given as an explicit covariance, the solve routes, the incremental loop, the component means, the posterior samples, the
group posterior and GPR.fit.  Modelled on tests/test_matern_family.py.

Every reference is tests/additive_forms.py (NumPy fp64 on tests/matern_forms.py, held to central differences by
tests/test_additive_forms_host.py) or an oracle function fed the helper's explicit matrix; never the library.  Every tolerance
is the one an existing test applies to the same quantity for a single kernel, cited where it is used.  A kernel value is the
sum of two rounded terms, each within the single kernel's relative bound of its own outputscale, so the sum stays within that
bound of os_a + os_b: no tolerance below is doubled.  The problems are built by module-level functions that need no device;
tests/test_additive_forms_host.py checks on the CPU that every train matrix among them factors in fp32-rounded NumPy and that
the reference runs whose picks are compared have a top-two gap above the bound of tests/test_greedy_regimes.py:54.
"""
import functools
import json
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
import test_matern_family as TM                      # noqa: E402
import test_rhs_fused as RF                          # noqa: E402
import test_target_weights as TW                     # noqa: E402
import test_variance_reduction as VR                 # noqa: E402
from algp_amd import _hip                            # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

DT, DIDS = [np.float64, np.float32], ['f64', 'f32']
KNAME = {MF.RBF: 'rbf', MF.MATERN15: 'm15', MF.MATERN05: 'm05', MF.MATERN25: 'm25'}
ALL4 = [MF.RBF, MF.MATERN15, MF.MATERN05, MF.MATERN25]
PAIRS = [(MF.MATERN15, MF.RBF), (MF.MATERN05, MF.MATERN25), (MF.RBF, MF.MATERN05)]      # family 0 + 0, 1 + 1, 0 + 1
PIDS = ['%s+%s' % (KNAME[a], KNAME[b]) for a, b in PAIRS]
SPLITS = [(1, 1), (2, 1), (2, 2), (2, 4), (1, 7), (5, 3)]                                # DP = 2, 4, 4, 8, 8, 8
ENT, MI, VRC = _hip.CRIT_ENTROPY, _hip.CRIT_MUTUAL_INFORMATION, 2
S_STD, M_STD, SS, SM, VF = TM.S_STD, TM.M_STD, TM.SS, TM.SM, TM.VF
GAP = TM.GAP                                                                             # tests/test_greedy_regimes.py:54

pairs = pytest.mark.parametrize('pair', PAIRS, ids=PIDS)
dtypes = pytest.mark.parametrize('dt', DT, ids=DIDS)
tol, relerr, _f32, _ut_bound, _top_gap, _memo = TM.tol, TM.relerr, TM._f32, TM._ut_bound, TM._top_gap, TM._memo


def set_additive(c, spec, log_ls, log_os, log_noise):
    c.set_hypers_additive(log_ls, spec[2], log_os[0], log_os[1], log_noise, spec[0], spec[1])


# ---------------------------------------------------------------------------------------------------- 1. ABI
def test_abi_good_and_bad_arguments():
    c = _hip.Context(np.float64)
    D = 3
    ls = np.ascontiguousarray(np.log([3.0, 2.0, 1.5]))
    los, ln = (np.log(1.2), np.log(0.4)), np.log(1e-2)
    x = np.array([[0.0, 0.0, 1.0], [3.0, 0.0, 1.0], [0.0, 6.0, 2.0], [1.0, 1.0, 1.0]])

    def rc(D_, ka, Da, kb):
        return c.lib.algp_set_hypers_additive(c.h, D_, ka, Da, los[0], kb, los[1], ls.ctypes.data_as(_hip._dblp), ln)

    spec = (MF.MATERN15, MF.RBF, 2)
    assert rc(D, spec[0], 2, spec[1]) == _hip.OK
    c.D, c.additive = D, True
    want = AF.kernel_matrix(spec, ls, los, x)
    assert relerr(c.kernel_matrix(x), want) < 1e-13
    for bad in ((1, 1, 1, 0), (9, 1, 2, 0), (D, 1, 0, 0), (D, 1, D, 0), (D, -1, 2, 0), (D, 4, 2, 0), (D, 1, 2, -1), (D, 1, 2, 4)):
        assert rc(*bad) == _hip.ERR_BAD_ARG, bad
        assert relerr(c.kernel_matrix(x), want) < 1e-13              # the context survives, with the hyper-parameters it had
    assert c.lib.algp_set_hypers_additive(c.h, D, 1, 2, 0.0, 0, 0.0, None, ln) == _hip.ERR_BAD_ARG
    # every Da the ABI takes, every pair of ids
    for Da in (1, 2):
        for ka in ALL4:
            for kb in ALL4:
                assert rc(D, ka, Da, kb) == _hip.OK
                assert relerr(c.kernel_matrix(x), AF.kernel_matrix((ka, kb, Da), ls, los, x)) < 1e-13
    # back to a single kernel, which still refuses ids outside 0..3, and to the additive one again
    c.set_hypers(ls, los[0], ln, MF.MATERN25)
    assert relerr(c.kernel_matrix(x), MF.kernel_matrix(MF.MATERN25, ls, los[0], x)) < 1e-13
    assert c.lib.algp_set_hypers(c.h, 4, D, ls.ctypes.data_as(_hip._dblp), los[0], ln) == _hip.ERR_BAD_ARG
    c.set_pool(x)
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])
    c.factorize()
    assert c.mll_grad().shape == (D + 2,)
    with pytest.raises(ValueError):
        c.posterior_mean_component(0, [3])                           # a single kernel is in force: ALGP_ERR_STATE
    assert c.lib.algp_posterior_mean_component(c.h, 0, None, 0, None) == _hip.ERR_STATE
    set_additive(c, spec, ls, los, ln)
    assert relerr(c.kernel_matrix(x), want) < 1e-13
    c.set_train([0, 1, 2], [1.0, 2.0, 0.5], [0.1, 0.1, 0.1])          # the pool was rescaled and kept
    c.factorize()
    assert c.mll_grad().shape == (D + 3,)
    c.close()


# ---------------------------------------------------------------------------------------------------- 2. kernel matrix
KM_LOG_OS = (np.log(1.7), np.log(0.6))


@dtypes
@pytest.mark.parametrize('split', SPLITS, ids=['%d+%d' % s for s in SPLITS])
def test_kernel_matrix_every_pair_of_forms(split, dt):
    """tests/test_matern_family.py::test_kernel_matrix (from tests/test_hip_kernels.py:131, tolerance :142) on its inputs, for
    all 16 pairs of forms in one context per split."""
    Da, Db = split
    q = TM.kmat_inputs(Da + Db)
    t = tol(dt, 1e-13, 2e-5)
    T = np.dtype(dt).type
    diag = T(np.exp(KM_LOG_OS[0])) + T(np.exp(KM_LOG_OS[1]))
    c = _hip.Context(dt)
    for ka in ALL4:
        for kb in ALL4:
            spec = (ka, kb, Da)
            set_additive(c, spec, q.log_ls, KM_LOG_OS, q.log_noise)
            K = c.kernel_matrix(q.x1)
            Kw = AF.kernel_matrix(spec, q.log_ls, KM_LOG_OS, q.x1)
            assert K.dtype == np.dtype(dt) and K.shape == (200, 200) and np.all(np.isfinite(K))
            assert relerr(K, Kw) < t, spec
            assert np.array_equal(K, K.T)
            assert np.all(np.diag(K) == diag)                                              # exactly os_a + os_b
            assert K[7, 150] == K[7, 7] == K[150, 150]                                     # r = 0 off the diagonal
            assert np.all(K[199, :199] == 0) and np.all(K[:199, 199] == 0)                 # exactly 0, not NaN
            Kx = c.kernel_matrix(q.x1[:130], q.x2)
            assert Kx.shape == (130, 70) and np.all(np.isfinite(Kx))
            assert relerr(Kx, AF.kernel_matrix(spec, q.log_ls, KM_LOG_OS, q.x1[:130], q.x2)) < t, spec
            assert Kx[5, 3] == K[5, 5] and np.all(Kx[:, 69] == 0)
            Kd = c.kernel_matrix(q.x1, diag_add=q.var, add_likelihood_var=True)
            assert relerr(Kd, Kw + np.diag(q.var) + np.exp(q.log_noise) * np.eye(200)) < t, spec
            assert np.all(Kd[199, :199] == 0)
    c.close()


# ---------------------------------------------------------------------------------------------------- 3. MLL, gradient, fit_step
MLL_TH = (np.log([1.3, 2.1, 0.8, 1.6]), (np.log(0.9), np.log(0.5)), np.log(0.05))
MLL_N = [(1, False), (63, False), (65, False), (130, False), (200, False), (130, True)]


@functools.lru_cache(maxsize=None)
def mll_problem(pair, N, twice):
    """tests/test_matern_family.py:mll_problem in four dimensions, split (2, 2); `twice`: rows 5 and N - 3 name one pool site."""
    rng = np.random.RandomState(3)
    x = _f32(rng.uniform(0, 6, (200, 4)))[:N]
    y = (np.sin(x[:, 0]) + np.cos(x[:, 2]) + 0.1 * rng.standard_normal(200)[:N])
    var = rng.uniform(0.005, 0.05, 200)[:N]
    idx = np.arange(N)
    if twice:
        idx[N - 3] = 5
    spec = (pair[0], pair[1], 2)
    xs = x[idx]
    q = types.SimpleNamespace(x=x, y=y, var=var, idx=idx, th=MLL_TH, spec=spec)
    q.S = AF.train_matrix(spec, MLL_TH[0], MLL_TH[1], MLL_TH[2], xs, var, idx)
    q.mll = AF.mll(spec, MLL_TH[0], MLL_TH[1], MLL_TH[2], xs, y, var, idx)
    q.grad = AF.mll_grad(spec, MLL_TH[0], MLL_TH[1], MLL_TH[2], xs, y, var, idx)
    return q


@pairs
@dtypes
@pytest.mark.parametrize('N,twice', MLL_N, ids=['N%d%s' % (n, '-site-twice' if t else '') for n, t in MLL_N])
def test_mll_and_gradient(pair, N, twice, dt):
    """tests/test_matern_family.py::test_mll_and_gradient for the D + 3 gradient.  fp64: tests/test_host_api.py:143-145 (MLL 1e-10
    relative, gradient 1e-8 of its largest entry); fp32: tests/test_fit_regimes.py:49 (2e-2).  The sizes cross the gradient's
    64-row tiles and the factor's 128 blocks; the gradient is the same bits in two calls."""
    q = mll_problem(pair, N, twice)
    c = _hip.Context(dt)
    set_additive(c, q.spec, *q.th)
    c.set_pool(q.x)
    c.set_train(q.idx, q.y, q.var)
    c.factorize()
    mll, g = c.mll(), c.mll_grad()
    print('mll %.12e (want %.12e)  grad err %.2e' % (mll, q.mll, float(np.max(np.abs(g - q.grad)))))
    assert g.shape == (7,) and np.isfinite(mll) and np.all(np.isfinite(g))
    if np.dtype(dt) == np.float64:
        assert mll == pytest.approx(q.mll, rel=1e-10)
        assert relerr(g, q.grad) < 1e-8
    else:
        assert abs(mll - q.mll) <= 2e-2 * abs(q.mll)
        assert np.max(np.abs(g - q.grad) / np.maximum(1.0, np.abs(q.grad))) <= 2e-2
    assert np.array_equal(c.mll_grad(), g)
    mll_s, g_s = c.fit_step()
    assert g_s.shape == (7,)
    assert abs(mll_s - mll) <= tol(dt, 1e-12, 1e-6) * abs(mll)                            # tests/test_fold.py:213-214
    assert np.max(np.abs(g_s - g) / np.maximum(1.0, np.abs(g))) <= tol(dt, 1e-10, 2e-3)
    mll_b, g_b = c.fit_step()
    assert mll_b == mll_s and np.array_equal(g_b, g_s)
    c.close()


# ---------------------------------------------------------------------------------------------------- 4. criteria on a pool
POOL_LOG_LS = np.log([3.0, 3.0, 1.0, 1.0])
POOL_LOG_OS = (np.log(0.7), np.log(0.4))
POOL_LOG_NOISE = TM.LOG_NOISE
N_GENO = 12
GENO_SEED, WEIGHT_SEED = 3, 71        # chosen on the CPU with the helper and the references alone, so that every compared pick is separated


@functools.lru_cache(maxsize=None)
def pool_problem(pair):
    """tests/test_matern_family.py:pool_problem (300 sites, 80 train rows, six sites outside the covered square) with two
    genotype-like coordinates behind the two positions: every site carries one of 12 genotypes, a point of the plane each.
    Split (2, 2): part a the position, part b the genotype."""
    base = TM.pool_problem(MF.MATERN15)
    rng = np.random.RandomState(GENO_SEED)
    emb = _f32(rng.uniform(0.0, 4.0, (N_GENO, 2)))
    geno = rng.randint(N_GENO, size=base.n)
    X = np.hstack([base.X, emb[geno]])
    spec = (pair[0], pair[1], 2)
    p = types.SimpleNamespace(spec=spec, n=base.n, X=X, geno=geno, static=base.static, mobile=base.mobile, A=base.A, N=base.N,
                              var=base.var, cand=base.cand, alive=base.alive, free=base.free)
    effect = rng.standard_normal(N_GENO)
    p.y = np.sin(X[p.A, 0] / 3.0) + 0.5 * effect[geno[p.A]] + 0.1 * rng.standard_normal(p.N)
    p.K = AF.kernel_matrix(spec, POOL_LOG_LS, POOL_LOG_OS, X)
    p.C = p.K + np.exp(POOL_LOG_NOISE) * np.eye(p.n)
    p.S = p.C[np.ix_(p.A, p.A)] + np.diag(p.var)
    for a in (p.X, p.C, p.K, p.S, p.y):
        a.setflags(write=False)
    p.memo = {}
    return p


def _pool_ctx(p, dt, explicit, cand=None, alive=None, prior_includes_noise=True, solve=True):
    """Context A (coordinates and the additive kernel) or B (the helper's matrix as an explicit pool covariance)."""
    c = _hip.Context(dt)
    if explicit:
        c.set_hypers(POOL_LOG_LS, 0.0, POOL_LOG_NOISE, _hip.KERNEL_RBF)
        c.set_pool_cov(p.C)
    else:
        set_additive(c, p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE)
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


def target_weights(p):
    return np.random.RandomState(WEIGHT_SEED).uniform(0.25, 4.0, size=p.n)


def wvr_reference(p):
    return _memo(p, 'wvr', lambda: TW.wvr_reference(p.C, p.A, p.var, p.cand, p.alive, target_weights(p), SS, SM, 3))


@pairs
@dtypes
def test_pool_posterior_and_covariance(pair, dt):
    """Mean and variance at the 220 sites without a train row, both contexts against the helper (tests/test_rhs_fused.py:22 as
    its _check_oracle applies it); the posterior covariance of context A at tests/test_posterior_cov_regimes.py:143's bound."""
    p = pool_problem(pair)
    mu_w, pv_w = _memo(p, 'post', lambda: AF.posterior(p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE, p.X[p.A], p.y, p.var,
                                                       p.X[p.free]))
    samp = np.arange(len(p.free))
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, cand=p.free, prior_includes_noise=explicit)
        mu, pv = c.posterior()
        RF._check_oracle(mu, pv, samp, dict(mu=mu_w, var=pv_w), RF.TOL[dt], np.exp(POOL_LOG_NOISE) if explicit else 0.0,
                         'explicit' if explicit else 'coordinates')
        if not explicit:
            B = p.K[np.ix_(p.A, p.free)]
            cov_w = p.K[np.ix_(p.free, p.free)] - B.T @ np.linalg.solve(p.S, B)
            cov, _ = c.posterior_cov()
            assert relerr(cov, cov_w) < tol(dt, 1e-9, 1e-3)
        c.close()


@pairs
@dtypes
def test_pool_entropy_picks(pair, dt):
    """tests/test_matern_family.py::test_pool_entropy_picks (tests/test_greedy_regimes.py:169-179, bounds :165-166)."""
    p = pool_problem(pair)
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


_LAZY_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_additive_kernel as t
print(json.dumps(t.lazy_probe(int(sys.argv[1]), np.dtype(sys.argv[2]).type)))
""" % (REPO, os.path.join(REPO, 'tests'))


def lazy_probe(which, dt):
    """Three picks-only entropy picks on context A, then the flushed scores and variances: everything as hex of the bytes."""
    p = pool_problem(PAIRS[which])
    c = _pool_ctx(p, dt, False, alive=p.alive)
    picks = c.greedy(ENT, S_STD, M_STD, 3)
    s = c.scores(ENT, S_STD, M_STD)
    pv = c.posterior()[1]
    rows = [c.debug_get_pick(q) for q in range(3)]
    c.close()
    return dict(picks=[int(q) for q in picks], scores=s.tobytes().hex(), var=pv.tobytes().hex(),
                rows=[r.tobytes().hex() for r, _ in rows], d=[float(d).hex() for _, d in rows])


@pytest.mark.parametrize('which', range(len(PAIRS)), ids=PIDS)
@dtypes
def test_lazy_greedy_switch_bit_for_bit(which, dt):
    """tests/test_matern_family.py::test_lazy_greedy_switch_bit_for_bit: the lazy refresh recomputes b' = C(pick, j) by the
    additive pool_cov; ALGP_LAZY_GREEDY=0 runs in a child (the switch is read once per process).  The picks are the reference's."""
    env = dict(os.environ)
    env['ALGP_LAZY_GREEDY'] = '0'
    r = subprocess.run([sys.executable, '-c', _LAZY_CHILD, str(which), np.dtype(dt).name], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    full = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.environ.get('ALGP_LAZY_GREEDY', '1') != '0'
    lazy = lazy_probe(which, dt)
    assert lazy == full
    assert lazy['picks'] == [int(q) for q in entropy_reference(pool_problem(PAIRS[which]))[0]]


@pairs
@dtypes
def test_pool_mi_picks(pair, dt):
    """tests/test_matern_family.py::test_pool_mi_picks: every utility along the reference's picks at tests/test_hip_greedy.py:417's
    tolerance (1e-7 / 3e-3 of the largest utility), both contexts; the free run's picks in fp64, where the gap is resolved."""
    p = pool_problem(pair)
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


@pairs
@dtypes
def test_pool_variance_reduction_and_target_weights(pair, dt):
    """tests/test_matern_family.py::test_pool_variance_reduction (tests/test_variance_reduction.py: vr_reference, compare, TOL at
    :52): three rounds along the brute force's picks, then the free run's picks; and the same with target weights attached
    (tests/test_target_weights.py: wvr_reference, its TOL :48)."""
    p = pool_problem(pair)
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


# ---- paths: the constructions of tests/test_matern_family.py (entropy_paths, mi_paths, vr_paths) on this file's pool problem
def _slogdet(M):
    s, ld = np.linalg.slogdet(M)
    assert s > 0
    return ld


def entropy_paths(p):
    def build():
        rng = np.random.RandomState(17)
        sm = 0.7 ** 2
        ldA = _slogdet(p.S)
        out = []
        for lengths, width in (([1, 12, 32], 36), ([100], 104)):
            paths = np.full((len(lengths), width), -1, dtype=np.int64)
            want = np.zeros(len(lengths))
            for i, L in enumerate(lengths):
                sites = [int(v) for v in rng.permutation(p.free)[:L]]
                if i % 3 == 2:
                    sites[rng.randint(L)] = int(p.A[rng.randint(p.N)])
                uniq = list(dict.fromkeys(sites))
                row = list(sites) + [sites[0]]
                row.insert(rng.randint(len(row) + 1), -1)
                paths[i, :len(row)] = row
                idx = np.r_[p.A, uniq].astype(int)
                S = p.C[np.ix_(idx, idx)] + np.diag(np.r_[p.var, np.full(len(uniq), sm)])
                want[i] = len(uniq) * O.CONST + 0.5 * (_slogdet(S) - ldA)
            out.append((paths, want))
        return out
    return _memo(p, 'entropy_paths', build)


def mi_paths(p):
    def build():
        rng = np.random.RandomState(23)
        lists = [[int(v) for v in rng.permutation(p.free)[:L]] for L in (1, 17, 64, 70)]
        rows = np.full((len(lists), 74), -1, dtype=np.int64)
        for i, s in enumerate(lists):
            row = list(s) + [s[0]]
            row.insert(rng.randint(len(row) + 1), -1)
            rows[i, :len(row)] = row
        _, ut = O.best_path_ref(p.C, p.static, p.mobile, [[]] + lists, [], S_STD, M_STD, 'mutual_information')
        return rows, ut[1:] - ut[0]
    return _memo(p, 'mi_paths', build)


def vr_paths(p):
    def build():
        rng = np.random.RandomState(29)
        T = p.free
        dC = np.diag(p.C)

        def sumvar(tr, nz):
            B = p.C[np.ix_(tr, T)]
            return float(np.sum(dC[T]) - np.sum(B * np.linalg.solve(p.C[np.ix_(tr, tr)] + np.diag(nz), B)))

        base = sumvar(p.A, p.var)
        static_only = np.where(p.static & ~p.mobile)[0]
        lists = []
        for L in (3, 64, 70):
            lists.append([int(v) for v in rng.permutation(p.free)[:L]])
            lists.append([int(v) for v in rng.permutation(p.free)[:L - 1]] + [int(static_only[L % len(static_only)])])
        rows = np.full((len(lists), 72), -1, dtype=np.int64)
        want = np.zeros(len(lists))
        pos = {int(s): i for i, s in enumerate(p.A)}
        for i, s in enumerate(lists):
            rows[i, :len(s)] = s
            rows[i, len(s)] = s[0]
            tr, nz = [int(a) for a in p.A], [float(v) for v in p.var]
            for site in s:
                if site in pos:
                    nz[pos[site]] = nz[pos[site]] * SM / (nz[pos[site]] + SM)
                else:
                    tr.append(site)
                    nz.append(SM)
            want[i] = base - sumvar(tr, nz)
        return rows, want
    return _memo(p, 'vr_paths', build)


@pairs
@dtypes
def test_score_paths_three_criteria(pair, dt):
    """score_paths on both routes (tolerances tests/test_hip_greedy.py:565, :617), score_paths_mi (tests/test_mi_paths.py:119) and
    score_paths_vr (tests/test_paths_vr.py:37), coordinates and explicit covariance."""
    p = pool_problem(pair)
    c = _pool_ctx(p, dt, False)
    for (paths, want), t in zip(entropy_paths(p), (tol(dt, 1e-9, 2e-3), tol(dt, 1e-9, 3e-3))):
        got = c.score_paths(paths, 0.7)
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want)) < t * max(1.0, np.max(np.abs(want))), np.max(np.abs(got - want))
    c.close()
    rows, want = mi_paths(p)
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, cand=np.where(~p.mobile)[0])
        got = c.score_paths_mi(rows, S_STD, M_STD)
        c.close()
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want)) <= tol(dt, 1e-7, 3e-3) * np.max(np.abs(want)), np.max(np.abs(got - want))
    rows, want = vr_paths(p)
    assert np.min(want) > 1e-2
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, alive=p.alive)
        got = c.score_paths_vr(rows, M_STD)
        c.close()
        err = np.abs(got - want) / np.abs(want)
        print('paths vr %s: worst %.3e' % ('explicit' if explicit else 'coordinates', float(np.max(err))))
        assert np.all(np.isfinite(got)) and np.max(err) < tol(dt, 1e-9, 1e-3)


# ---------------------------------------------------------------------------------------------------- 5. solve routes
ROUTE_LOG_LS2, ROUTE_LOG_OS = np.log([3.0, 3.0]), (np.log(0.6), np.log(0.5))


@functools.lru_cache(maxsize=None)
def mid_problem(pair):
    """tests/test_matern_family.py:mid_problem (N = 300, M = 700: the one-launch and mid-sized solves), split (1, 1)."""
    base = TM.mid_problem(MF.MATERN15)
    spec = (pair[0], pair[1], 1)
    mu, pv = AF.posterior(spec, ROUTE_LOG_LS2, ROUTE_LOG_OS, TM.LOG_NOISE, base.pool[base.A], base.y, base.var, base.pool[base.cidx])
    S = AF.train_matrix(spec, ROUTE_LOG_LS2, ROUTE_LOG_OS, TM.LOG_NOISE, base.pool[base.A], base.var)
    return types.SimpleNamespace(pool=base.pool, A=base.A, y=base.y, var=base.var, cidx=base.cidx, mu=mu, pv=pv, S=S, spec=spec,
                                 logdet=np.linalg.slogdet(S)[1])


@pairs
@pytest.mark.parametrize('dt,t', [(np.float64, 1e-9), (np.float32, 2e-3)], ids=DIDS)     # tests/test_fold.py:41
def test_fit_and_solve_and_the_mean_only_posterior(pair, dt, t, monkeypatch):
    """tests/test_matern_family.py::test_fit_and_solve_and_the_mean_only_posterior: the folded launch and its two phases."""
    q = mid_problem(pair)
    c = _hip.Context(dt)
    set_additive(c, q.spec, ROUTE_LOG_LS2, ROUTE_LOG_OS, TM.LOG_NOISE)
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
def sweep_problem(pair):
    """tests/test_matern_family.py:fused_problem (51 300 candidates, 1 400 train rows: the scheduled sweep), split (1, 1)."""
    base = TM.fused_problem(MF.MATERN15)
    spec = (pair[0], pair[1], 1)
    mu, pv = AF.posterior(spec, ROUTE_LOG_LS2, ROUTE_LOG_OS, TM.LOG_NOISE, base.pool[base.A], base.y, base.var,
                          base.pool[base.cidx[base.samp]])
    return types.SimpleNamespace(base=base, spec=spec, ref=dict(mu=mu, var=pv))


@pairs
@dtypes
def test_scheduled_sweep_takes_the_materialised_route(pair, dt, monkeypatch):
    """tests/test_matern_family.py::test_fused_right_hand_sides at its size: under an additive kernel (DP = 2 here, where a single
    kernel generates its right-hand sides) the sweep reads them from V^T whatever ALGP_RHS_FUSED says -- the same bits, the full
    kernel-matrix traffic -- and meets the helper at tests/test_rhs_fused.py:22."""
    q = sweep_problem(pair)
    b = q.base
    c = _hip.Context(dt)
    set_additive(c, q.spec, ROUTE_LOG_LS2, ROUTE_LOG_OS, TM.LOG_NOISE)
    c.set_pool(b.pool)
    c.set_train(b.A, b.y, b.var)
    c.factorize()
    c.set_candidates(b.cidx, prior_includes_noise=False)
    (mu, pv), (mu2, pv2), (mu0, pv0) = RF._posteriors(c, monkeypatch)
    RF._check_oracle(mu, pv, b.samp, q.ref, RF.TOL[dt], what='additive')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)                  # ALGP_RHS_FUSED=0: bit for bit
    full, _ = RF._expected_bytes(TM.FUSED_M, TM.FUSED_N, np.dtype(dt).itemsize)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    assert RF._kmat_bytes(c) == full                                           # nothing was generated in an epilogue
    monkeypatch.delenv('ALGP_RHS_FUSED')
    c.close()


# ---------------------------------------------------------------------------------------------------- 6. incremental
@pairs
@dtypes
def test_incremental_update_equals_from_scratch(pair, dt):
    """factorize_update + solve_candidates_update after appending 5 train rows against a fresh context on the longer train set:
    tests/test_incremental.py:196, :246 for the same comparison (the mean 1e-9 / 3e-3 of its scale, the variance absolute)."""
    p = pool_problem(pair)
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
    set_additive(f, p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE)
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
    mu_w, pv_w = AF.posterior(p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE, p.X[A2], y2, var2, p.X[p.free[5:]])
    RF._check_oracle(mu, pv, np.arange(len(mu)), dict(mu=mu_w, var=pv_w), RF.TOL[dt], what='updated')


# ---------------------------------------------------------------------------------------------------- 7. component means
@pairs
@dtypes
def test_component_means(pair, dt):
    """algp_posterior_mean_component against the helper at the mean's own tolerance (tests/test_fold.py:186: 1e-8 / 2e-2 of the
    scale of the mean); a + b + ybar = algp_posterior_mean to rounding; the refusals."""
    p = pool_problem(pair)
    ma_w, mb_w = _memo(p, 'comp', lambda: AF.component_means(p.spec, POOL_LOG_LS, POOL_LOG_OS, POOL_LOG_NOISE, p.X[p.A], p.y, p.var,
                                                            p.X[p.free]))
    c = _pool_ctx(p, dt, False, solve=False)
    ma, mb = c.posterior_mean_component(0, p.free), c.posterior_mean_component(1, p.free)
    mu = c.posterior_mean(p.free)
    scale = max(1.0, float(np.max(np.abs(ma_w + mb_w + p.y.mean()))))
    t = tol(dt, 1e-8, 2e-2)
    assert ma.dtype == np.dtype(dt) and ma.shape == (len(p.free),)
    assert np.max(np.abs(ma - ma_w)) <= t * scale and np.max(np.abs(mb - mb_w)) <= t * scale
    assert np.max(np.abs(ma.astype(np.float64) + mb + p.y.mean() - mu)) <= tol(dt, 1e-12, 1e-5) * scale
    assert np.std(ma_w) > 0.05 and np.std(mb_w) > 0.05                          # both parts carry signal here
    for comp in (-1, 2):
        with pytest.raises(ValueError):
            c.posterior_mean_component(comp, p.free)
    c.close()
    b = _pool_ctx(p, dt, True, solve=False)
    b.additive = True
    assert b.lib.algp_posterior_mean_component(b.h, 0, _hip._i64(np.arange(3)), 3, _hip._ptr(np.zeros(3, dt))) == _hip.ERR_BAD_ARG
    b.close()


# ---------------------------------------------------------------------------------------------------- 8. samples
@functools.lru_cache(maxsize=None)
def sample_case(pair):
    """Values mode: an exact prior draw on the helper's matrix; features mode: omega rows that are zero in the other part's
    coordinates, the part of each feature drawn with probability os_c / (os_a + os_b) (utils.spectral_draws)."""
    from algp_amd.utils import spectral_draws
    p = pool_problem(pair)
    S, F = 5, 257
    rng = np.random.RandomState(61)
    L = np.linalg.cholesky(p.K + 1e-10 * np.eye(p.n))
    prior = _f32(rng.standard_normal((S, p.n)) @ L.T)
    eps = _f32(rng.standard_normal((S, p.N)))
    v = p.var + np.exp(POOL_LOG_NOISE)
    cand = p.free
    ref_values = PF.pathwise(p.K[np.ix_(cand, p.A)], p.S, p.y, v, prior[:, cand], prior[:, p.A], eps)
    osa, osb = np.exp(POOL_LOG_OS[0]), np.exp(POOL_LOG_OS[1])
    om, ph = spectral_draws(('additive', 2, pair[0], pair[1], osa, osb), 4, F, rng)
    om, ph = _f32(om), _f32(ph)
    W = _f32(rng.standard_normal((S, F)))
    G = W @ PF.features(om, ph, p.X * np.exp(-POOL_LOG_LS)[None, :], osa + osb).T
    ref_features = PF.pathwise(p.K[np.ix_(cand, p.A)], p.S, p.y, v, G[:, cand], G[:, p.A], eps)
    return types.SimpleNamespace(prior=prior, eps=eps, om=om, ph=ph, W=W, ref_values=ref_values, ref_features=ref_features)


@pairs
@dtypes
def test_posterior_samples(pair, dt):
    """Values mode against tests/pathwise_forms.py on the helper's matrix, features mode against the NumPy evaluation with the same
    omega, phase and weights: tests/test_pathwise_samples.py's bar (:35, 1e-5 / 1e-3 of the largest draw)."""
    p = pool_problem(pair)
    q = sample_case(pair)
    assert np.all((q.om[:, :2] == 0).all(axis=1) | (q.om[:, 2:] == 0).all(axis=1))
    c = _pool_ctx(p, dt, False, cand=p.free, prior_includes_noise=False)
    bar = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}[np.dtype(dt)]
    fv = c.sample_posterior(q.eps, prior=q.prior)
    ff = c.sample_posterior(q.eps, weights=q.W, omega=q.om, phase=q.ph)
    c.close()
    assert fv.shape == ff.shape == (5, len(p.free)) and np.all(np.isfinite(fv)) and np.all(np.isfinite(ff))
    print('values %.3g  features %.3g (bar %g)' % (relerr(fv, q.ref_values), relerr(ff, q.ref_features), bar))
    assert relerr(fv, q.ref_values) <= bar
    assert relerr(ff, q.ref_features) <= bar


# ---------------------------------------------------------------------------------------------------- 9. group posterior
@pairs
@dtypes
def test_group_posterior_of_the_genotypes(pair, dt):
    """Mean, cov and cross of the 12 genotype means over the 220 free sites against tests/group_forms.py's aggregates of the
    helper's posterior: tests/test_group_posterior.py's bar (:37, 1e-5 / 1e-3)."""
    p = pool_problem(pair)
    lab = p.geno[p.free].astype(np.int32)
    assert len(np.unique(lab)) == N_GENO

    def build():
        B = p.K[np.ix_(p.A, p.free)]
        Sigma = p.K[np.ix_(p.free, p.free)] - B.T @ np.linalg.solve(p.S, B)
        mu = p.y.mean() + B.T @ np.linalg.solve(p.S, p.y - p.y.mean())
        return GF.aggregates(mu, Sigma, GF.coefficients(lab, None, N_GENO))
    ref = _memo(p, 'group', build)
    c = _pool_ctx(p, dt, False, cand=p.free, prior_includes_noise=False)
    mean, cov, cross = c.group_posterior(lab, n_groups=N_GENO, want_cov=True, want_cross=True)
    c.close()
    bar = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}[np.dtype(dt)]
    for got, want, what in ((mean, ref[0], 'mean'), (cov, ref[1], 'cov'), (cross, ref[2], 'cross')):
        print('group %s relerr %.3g (bar %g)' % (what, relerr(got, want), bar))
        assert got.shape == want.shape and np.all(np.isfinite(got)) and relerr(got, want) <= bar, what


# ---------------------------------------------------------------------------------------------------- 10. GPR.fit
FIT_PARTS = ({'type': 'matern', 'nu': 1.5}, {'type': 'rbf'})


@functools.lru_cache(maxsize=None)
def fit_problem():
    """150 plots of a 15 x 10 field, 10 genotypes scattered over them: y = g(genotype) + s(row, col) + noise.  Coordinates:
    (genotype id | row, col): part a is the genotype, so predict_components' first mean is the genotype effect."""
    rng = np.random.RandomState(12)
    rr, cc = np.meshgrid(np.arange(15.0), np.arange(10.0), indexing='ij')
    geno = rng.permutation(np.arange(150) % 10)
    g = rng.standard_normal(10)
    s = 1.5 * np.sin(rr.ravel() / 4.0) * np.cos(cc.ravel() / 3.0)
    x = np.column_stack([3.0 * geno, rr.ravel(), cc.ravel()])
    y = g[geno] + s + 0.1 * rng.standard_normal(150)
    probe = np.column_stack([3.0 * np.arange(10), np.full(10, 7.0), np.full(10, 4.5)])     # every genotype at the field's centre
    return types.SimpleNamespace(x=x, y=y, var=np.full(150, 1e-2), geno=geno, g=g, probe=probe)


def _centred_error(est, g):
    est, g = np.asarray(est, np.float64), np.asarray(g, np.float64)
    return float(np.sqrt(np.mean(((est - est.mean()) - (g - g.mean())) ** 2)))


@dtypes
def test_gpr_fit_and_predict_components(dt):
    from algp_amd.models import GPR
    q = fit_problem()
    kp = {'type': 'additive', 'split': 1, 'parts': FIT_PARTS}
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
    assert kt == ('additive', 1, _hip.KERNEL_MATERN15, _hip.KERNEL_RBF)
    spec = (MF.MATERN15, MF.RBF, 1)
    C = gp.cov_mat(q.x, add_likelihood_var=True)
    assert relerr(C, AF.kernel_matrix(spec, ls, los, q.x) + np.exp(ln) * np.eye(150)) < tol(dt, 1e-13, 2e-5)
    # the genotype component at the fitted hyper-parameters: the library against the helper, at the mean's tolerance
    ma, mb = gp.predict_components(q.probe)
    ma_w, mb_w = AF.component_means(spec, ls, los, ln, q.x, q.y, q.var, q.probe)
    t = tol(dt, 1e-8, 2e-2)
    assert np.max(np.abs(ma - ma_w)) <= t * max(1.0, np.max(np.abs(ma_w)))
    assert np.max(np.abs(mb - mb_w)) <= t * max(1.0, np.max(np.abs(mb_w)))
    assert np.max(np.abs(ma.astype(np.float64) + mb + q.y.mean() - gp.predict(q.probe))) <= tol(dt, 1e-10, 1e-4) * max(1.0, np.max(np.abs(q.y)))
    # ... and it recovers g, up to the constant, better than the single Matern fit's prediction at the same probes does: both
    # errors computed by the helpers from the two models' fitted hyper-parameters
    single = GPR(lr=.1, max_iterations=30, kernel_params={'type': 'matern', 'nu': 1.5}, dtype=dt)
    single.fit(q.x, q.y, q.var)
    ls1, los1, ln1, _ = single.hypers()
    mu1, _ = MF.posterior(MF.MATERN15, ls1, los1, ln1, q.x, q.y, q.var, q.probe)
    e_add, e_single = _centred_error(ma_w, q.g), _centred_error(mu1, q.g)
    print('genotype effect: additive %.4f  single Matern %.4f' % (e_add, e_single))
    assert e_add < e_single
