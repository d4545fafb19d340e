"""Matern-1/2 (ALGP_KERNEL_MATERN05 = 2) and Matern-5/2 (ALGP_KERNEL_MATERN25 = 3) through every layer that evaluates a kernel
value: the ABI, the kernel-matrix build, the criteria on a coordinate pool against the same pool given as an explicit
covariance, the right-hand sides fused into the candidate sweep, the one-launch and mid-sized solves, the path utilities, the
MLL with its gradient, and GPR.fit.

Every reference is tests/matern_forms.py (the closed forms in NumPy fp64, held to the general Matern form and to central
differences by tests/test_matern_forms_host.py) or a function of oracle/gp_oracle.py that takes an explicit covariance matrix
built by that helper; never the library.  Every tolerance is the one an existing test applies to Matern-3/2, cited where it is
used.  Inputs come from fixed seeds; the problems are built by module-level functions that need no device, and
tests/test_matern_forms_host.py checks on the CPU that every train matrix among them factors in fp32-rounded NumPy.

Where picks of a free run are compared with the reference's, the reference's top-two gap at every pick is asserted to exceed the
bound the existing tests use (tests/test_greedy_regimes.py:54); the inputs were chosen with the helper alone so that it does.

Two places where a comparison is narrower than "the same picks in both precisions", or uses another reference than the oracle's
own function:
 - MI picks in fp32 (test_pool_mi_picks): the MI utilities are entropies of the whole pool (about 30 nats here) and their
   top-two gap (1e-3 .. 4e-3) is below what the fp32 tolerance of the existing MI tests (3e-3 of the largest utility,
   tests/test_hip_greedy.py:417) can resolve.  In fp32 both contexts are therefore scored along the reference's picks, every
   utility of every round compared, as that existing test does; a free run's picks are compared, context A, context B and the
   oracle, in fp64 only.
 - score_paths (test_score_paths_both_routes) is compared with NumPy log-determinants of the enlarged train matrix on the
   helper's covariance, formed as tests/test_hip_greedy.py:521-564 forms them, not with oracle.best_path_ref: a path that
   crosses a train site gets a second row for that site in the library (algp_score_paths), which best_path_ref's fused
   variances do not describe.  score_paths_mi is compared with oracle.best_path_ref; the oracle has no variance-reduction
   utilities, so score_paths_vr and the criterion are compared with brute-force refits on the helper's matrix.
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

import matern_forms as MF                            # noqa: E402
import mi_forms as MIF                               # noqa: E402
import test_rhs_fused as RF                          # noqa: E402
import test_variance_reduction as VR                 # noqa: E402
from algp_amd import _hip                            # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

KIDS = [MF.MATERN05, MF.MATERN25]
KNAMES = ['matern05', 'matern25']
DT = [np.float64, np.float32]
DIDS = ['f64', 'f32']
ENT, MI, VRC = _hip.CRIT_ENTROPY, _hip.CRIT_MUTUAL_INFORMATION, 2
S_STD, M_STD = 0.1, 1.0
SS, SM = S_STD ** 2, M_STD ** 2
VF = 1.0 / (1.0 / SS + 1.0 / SM)
LOG_LS, LOG_OS, LOG_NOISE = np.log([3.0, 3.0]), 0.0, np.log(1e-2)     # the grids' hyper-parameters, as in the existing tests
GAP = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-2}        # tests/test_greedy_regimes.py:54

both = pytest.mark.parametrize('kid', KIDS, ids=KNAMES)
dtypes = pytest.mark.parametrize('dt', DT, ids=DIDS)


def tol(dt, t64, t32):
    return t64 if np.dtype(dt) == np.float64 else t32


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _f32(a):
    """Values both precisions hold exactly: rounded to float32, kept as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _ut_bound(dt, scale):
    """tests/test_greedy_regimes.py:165-166"""
    return 1e-9 * max(1.0, scale) if np.dtype(dt) == np.float64 else 1e-3 * scale


def _top_gap(ut):
    """The smallest top-two gap over the picks of a reference run (tests/test_greedy_regimes.py:106-115)."""
    g = np.inf
    for row in ut:
        v = np.sort(row[np.isfinite(row)])
        if len(v) > 1 and v[-1] != v[0]:
            g = min(g, float(v[-1] - v[-2]))
    return g


# ---------------------------------------------------------------------------------------------------- 1. ABI
def test_abi_takes_ids_2_and_3_and_refuses_the_rest():
    c = _hip.Context(np.float64)
    ls = np.ascontiguousarray(LOG_LS)

    def rc(kid):
        return c.lib.algp_set_hypers(c.h, kid, 2, ls.ctypes.data_as(_hip._dblp), LOG_OS, LOG_NOISE)

    assert (_hip.KERNEL_MATERN05, _hip.KERNEL_MATERN25) == (2, 3)
    x = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, 6.0]])
    for kid in KIDS:
        assert rc(kid) == _hip.OK
        c.D = 2
        assert relerr(c.kernel_matrix(x), MF.kernel_matrix(kid, LOG_LS, LOG_OS, x)) < 1e-13
        for bad in (-1, 4):
            assert rc(bad) == _hip.ERR_BAD_ARG
            assert b'unknown kernel' in c.lib.algp_last_error(c.h)
            # the context stays usable, with the hyper-parameters it had
            assert relerr(c.kernel_matrix(x), MF.kernel_matrix(kid, LOG_LS, LOG_OS, x)) < 1e-13
    c.close()


# ---------------------------------------------------------------------------------------------------- 2. kernel matrix
@functools.lru_cache(maxsize=None)
def kmat_inputs(D):
    """200 and 70 points in D dimensions; x1[150] = x1[7] and x2[3] = x1[5] (r = 0 off the diagonal); x1[199] and x2[69] lie
    10^4 length-scales from everything else, on opposite sides."""
    rng = np.random.RandomState(40 + D)
    log_ls = np.log(rng.uniform(1.0, 3.0, D))
    x1 = rng.uniform(0, 10, (200, D))
    x2 = rng.uniform(0, 10, (70, D))
    x1[150] = x1[7]
    x2[3] = x1[5]
    x1[199] = x1[0] + 1e4 * np.exp(log_ls)
    x2[69] = x1[0] - 1e4 * np.exp(log_ls)
    var = rng.uniform(0.01, 1, 200)
    return types.SimpleNamespace(log_ls=log_ls, log_os=np.log(1.7), log_noise=np.log(0.03), x1=_f32(x1), x2=_f32(x2), var=_f32(var))


@both
@dtypes
@pytest.mark.parametrize('D', [1, 2, 3, 6])
def test_kernel_matrix(kid, dt, D):
    """tests/test_hip_kernels.py:131 (test_kernel_matrix) with the helper in the oracle's place; its tolerance, :142."""
    q = kmat_inputs(D)
    t = tol(dt, 1e-13, 2e-5)
    c = _hip.Context(dt)
    c.set_hypers(q.log_ls, q.log_os, q.log_noise, kid)
    K = c.kernel_matrix(q.x1)
    Kw = MF.kernel_matrix(kid, q.log_ls, q.log_os, q.x1)
    assert K.dtype == np.dtype(dt) and K.shape == (200, 200) and np.all(np.isfinite(K))
    assert relerr(K, Kw) < t
    assert np.array_equal(K, K.T)
    assert np.allclose(np.diag(K), np.exp(q.log_os), rtol=tol(dt, 1e-15, 1e-7))            # test_hip_kernels.py:146
    assert K[7, 150] == K[7, 7] == K[150, 150]                                             # r = 0 off the diagonal
    assert np.all(K[199, :199] == 0) and np.all(K[:199, 199] == 0)                         # exactly 0, not NaN
    Kx = c.kernel_matrix(q.x1[:130], q.x2)
    assert Kx.shape == (130, 70) and np.all(np.isfinite(Kx))
    assert relerr(Kx, MF.kernel_matrix(kid, q.log_ls, q.log_os, q.x1[:130], q.x2)) < t
    assert Kx[5, 3] == K[5, 5] and np.all(Kx[:, 69] == 0)
    Kd = c.kernel_matrix(q.x1, diag_add=q.var, add_likelihood_var=True)
    assert relerr(Kd, Kw + np.diag(q.var) + np.exp(q.log_noise) * np.eye(200)) < t
    assert np.all(Kd[199, :199] == 0)
    c.close()


# ---------------------------------------------------------------------------------------------------- 3. criteria on a pool
POOL_SEED = 0
POOL_SIDE = 8.0
POOL_OUT = np.array([0.5, 1.0, 1.6, 2.3, 3.2, 4.5])


@functools.lru_cache(maxsize=None)
def pool_problem(kid):
    """300 pool sites, 80 train rows (35 static, 55 mobile-sampled, 10 of them both), every site a candidate.  294 sites are
    uniform on a square of side 8 (l = 3), which the train sites cover closely; the last 6 stand outside it, one on each of six
    rays from its centre, 0.5 .. 4.5 units beyond the edge.  Their posterior variances lie far apart and above every inner
    site's, so the first picks of the entropy and the variance-reduction criterion are separated by far more than fp32
    rounding (seed and geometry chosen with the helper and the references alone; the tests assert the gaps)."""
    rng = np.random.RandomState(POOL_SEED)
    n, nout = 300, len(POOL_OUT)
    nin = n - nout
    X = rng.uniform(0.0, POOL_SIDE, (n, 2))
    ang = np.pi / 3 * np.arange(nout) + 0.2
    half = POOL_SIDE / 2
    reach = half / np.maximum(np.abs(np.cos(ang)), np.abs(np.sin(ang)))      # where the ray leaves the square
    X[nin:, 0] = half + (reach + POOL_OUT) * np.cos(ang)
    X[nin:, 1] = half + (reach + POOL_OUT) * np.sin(ang)
    X = _f32(X)
    perm = rng.permutation(nin)
    static = np.zeros(n, bool)
    mobile = np.zeros(n, bool)
    static[perm[:35]] = True
    mobile[perm[25:80]] = True
    p = types.SimpleNamespace(kid=kid, n=n, X=X, static=static, mobile=mobile)
    p.A = np.where(static | mobile)[0]
    p.N = len(p.A)
    assert p.N == 80
    p.var = np.where(static[p.A] & mobile[p.A], VF, np.where(static[p.A], SS, SM))
    p.y = np.sin(X[p.A, 0] / 3.0) + 0.1 * rng.standard_normal(p.N)
    p.K = MF.kernel_matrix(kid, LOG_LS, LOG_OS, X)
    p.C = p.K + np.exp(LOG_NOISE) * np.eye(n)
    p.S = p.C[np.ix_(p.A, p.A)] + np.diag(p.var)
    p.cand = np.arange(n)
    p.alive = ~static
    p.free = np.where(~static & ~mobile)[0]
    for a in (p.X, p.C, p.K, p.S, p.var, p.y):
        a.setflags(write=False)
    p.memo = {}
    return p


def _memo(p, key, fn):
    if key not in p.memo:
        p.memo[key] = fn()
    return p.memo[key]


def _pool_ctx(p, dt, explicit, cand=None, alive=None, prior_includes_noise=True):
    """Context A (coordinates and the kernel id) or B (the helper's matrix as an explicit pool covariance)."""
    c = _hip.Context(dt)
    c.set_hypers(LOG_LS, LOG_OS, LOG_NOISE, _hip.KERNEL_RBF if explicit else p.kid)
    if explicit:
        c.set_pool_cov(p.C)
    else:
        c.set_pool(p.X)
    c.set_train(p.A, p.y, p.var)
    c.factorize()
    c.set_candidates(p.cand if cand is None else cand, prior_includes_noise=prior_includes_noise)
    c.solve_candidates(alive=alive)
    return c


@both
@dtypes
def test_pool_posterior_from_coordinates_and_from_the_explicit_covariance(kid, dt):
    """Mean and variance at the 220 sites without a train row, both contexts against the helper's Cholesky posterior:
    tests/test_rhs_fused.py:22 (TOL) as applied in its _check_oracle."""
    p = pool_problem(kid)
    mu_w, pv_w = _memo(p, 'post', lambda: MF.posterior(kid, LOG_LS, LOG_OS, LOG_NOISE, p.X[p.A], p.y, p.var, p.X[p.free]))
    samp = np.arange(len(p.free))
    for explicit in (False, True):
        # an explicit covariance carries sigma_n^2 on its diagonal: its variances are the noisy observation's (test_rhs_fused.py:242)
        c = _pool_ctx(p, dt, explicit, cand=p.free, prior_includes_noise=explicit)
        mu, pv = c.posterior()
        c.close()
        RF._check_oracle(mu, pv, samp, dict(mu=mu_w, var=pv_w), RF.TOL[dt], np.exp(LOG_NOISE) if explicit else 0.0,
                         'explicit' if explicit else 'coordinates')


@both
@dtypes
def test_pool_entropy_picks(kid, dt):
    """Four entropy picks with every utility, both contexts, against oracle.greedy_fast on the helper's matrix
    (tests/test_greedy_regimes.py:169-179 with its bounds, :165-166)."""
    p = pool_problem(kid)
    picks_o, ut_o = _memo(p, 'ent', lambda: O.greedy_fast(p.C, p.static, p.mobile, S_STD, M_STD, 4, 'entropy'))
    assert _top_gap(ut_o) > GAP[np.dtype(dt)], 'the inputs no longer separate the picks'
    got = []
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, alive=p.alive)
        picks, ut = c.greedy(ENT, S_STD, M_STD, 4, want_utilities=True)
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


@both
@dtypes
def test_pool_mi_picks(kid, dt):
    """Three picks under the MI criterion (candidates: the sites that are not static, as in tests/test_hip_greedy.py:383):
    every utility along the reference's picks at that test's tolerance (:417, 1e-7 / 3e-3 of the largest utility), both
    contexts.  The utilities are entropies of the whole pool, several hundred nats, so only fp64 resolves the reference's
    top-two gap: there the free run's picks are compared too."""
    p = pool_problem(kid)
    picks_o, ut_o = _memo(p, 'mi', lambda: O.greedy_fast(p.C, p.static, p.mobile, S_STD, M_STD, 3, 'mutual_information'))
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
            # the offset all candidates share and each candidate's own part, bounded apart (tests/mi_forms.py)
            m = MIF.measure(ut[k], want, p.mobile[cand], H[k])
            print('MI %s pick %d: offset %.2e of sum|H| %.1f, per-candidate %.2e of spread %.3f' % (
                'explicit' if explicit else 'coordinates', k, abs(m.off), m.hsum, m.per, m.spread))
            MIF.compare(ut[k], want, p.mobile[cand], dt, H[k], 'pick %d' % k)
        if np.dtype(dt) == np.float64:
            assert _top_gap(ut_o) > 2 * rel * scale, 'the inputs no longer separate the picks'
            c.solve_candidates()
            assert [int(q) for q in c.greedy(MI, S_STD, M_STD, 3)] == [int(q) for q in picks_o]
        c.close()


def _vr_reference(p):
    return _memo(p, 'vr', lambda: VR.vr_reference(p.C, p.A, p.var, p.cand, p.alive, SS, SM, 4))


@both
@dtypes
def test_pool_variance_reduction(kid, dt, monkeypatch):
    """The variance-reduction criterion (vr_pool_cov, gemm.hip): four rounds along the brute force's own picks
    (tests/test_variance_reduction.py: vr_reference and compare, TOL at :52 -- the oracle has no such criterion), the first
    from the fused product, the rest from the rank-1 folds; the free run's picks; ALGP_VR_RANK1=0 against the default at
    :301's bounds; coordinates against the explicit covariance."""
    p = pool_problem(kid)
    picks_o, U = _vr_reference(p)
    t = VR.TOL[dt]
    for r in range(4):
        top = np.sort(U[r][np.isfinite(U[r])])[-2:]
        assert (top[1] - top[0]) / top[1] > 2 * t, 'the inputs no longer separate the picks'      # :206-209
    runs = {}
    for explicit in (False, True):
        for rank1 in ('1', '0'):
            monkeypatch.setenv('ALGP_VR_RANK1', rank1)                                           # read per call
            c = _pool_ctx(p, dt, explicit, alive=p.alive)
            got_p, got_u = c.greedy(VRC, S_STD, M_STD, 4, forced_picks=picks_o, want_utilities=True)
            assert [int(v) for v in got_p] == picks_o
            for r in range(4):
                VR.compare(got_u[r], U[r], t, '%s rank1=%s round %d' % ('explicit' if explicit else 'coordinates', rank1, r))
            c.solve_candidates(alive=p.alive)
            assert [int(v) for v in c.greedy(VRC, S_STD, M_STD, 4)] == picks_o
            c.close()
            runs[(explicit, rank1)] = got_u
    monkeypatch.delenv('ALGP_VR_RANK1')
    for explicit in (False, True):
        assert np.array_equal(runs[(explicit, '1')][0], runs[(explicit, '0')][0])                # no pick yet: the same product
        VR.compare(runs[(explicit, '1')], runs[(explicit, '0')], tol(dt, 1e-12, t), 'rank-1 against the full product')


_LAZY_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_matern_family as t
print(json.dumps(t.lazy_probe(int(sys.argv[1]), np.dtype(sys.argv[2]).type)))
""" % (REPO, os.path.join(REPO, 'tests'))


def lazy_probe(kid, dt):
    """Four picks-only entropy picks on context A, then the flushed scores and variances: everything as hex of the bytes."""
    p = pool_problem(kid)
    c = _pool_ctx(p, dt, False, alive=p.alive)
    picks = c.greedy(ENT, S_STD, M_STD, 4)
    s = c.scores(ENT, S_STD, M_STD)
    pv = c.posterior()[1]
    rows = [c.debug_get_pick(q) for q in range(4)]
    c.close()
    return dict(picks=[int(q) for q in picks], scores=s.tobytes().hex(), var=pv.tobytes().hex(),
                rows=[r.tobytes().hex() for r, _ in rows], d=[float(d).hex() for _, d in rows])


@both
@dtypes
def test_lazy_greedy_switch_bit_for_bit(kid, dt):
    """ALGP_LAZY_GREEDY=0 (every row brought up to date before every pick) against the default (the lazy refresh, which
    recomputes b' = C(pick, j) in pick_bprime, vecops.hip): the same picks, rows of V^T, scores and variances, bit for bit.
    The switch is read once per process (tests/test_env_switches.py), so the other setting runs in a child."""
    env = dict(os.environ)
    env['ALGP_LAZY_GREEDY'] = '0'
    r = subprocess.run([sys.executable, '-c', _LAZY_CHILD, str(kid), np.dtype(dt).name], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    full = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.environ.get('ALGP_LAZY_GREEDY', '1') != '0'
    lazy = lazy_probe(kid, dt)
    assert lazy == full


# ---------------------------------------------------------------------------------------------------- 4. fused right-hand sides
FUSED_M, FUSED_N, FUSED_SIDE = 51300, 1400, 40                  # tests/test_rhs_fused.py::test_matern_kernel's shape


@functools.lru_cache(maxsize=None)
def fused_problem(kid):
    """tests/test_rhs_fused.py:_setup without its context: train sites on a 40 x 40 grid, candidates scattered over it."""
    rng = np.random.RandomState(34)
    xx, yy = np.meshgrid(np.arange(FUSED_SIDE), np.arange(FUSED_SIDE))
    grid = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    cand_x = rng.uniform(0, FUSED_SIDE, (FUSED_M, 2))
    A = np.sort(rng.permutation(len(grid))[:FUSED_N])
    pool = np.vstack([grid, cand_x])
    var = rng.choice([0.01, 1.0], FUSED_N)
    y = rng.uniform(0, 1, FUSED_N)
    cidx = np.arange(len(grid), len(grid) + FUSED_M)
    samp = np.sort(rng.permutation(FUSED_M)[:192])
    samp[-1] = FUSED_M - 1                                      # a row of the last (cut) row panel is always among them
    mu, pv = MF.posterior(kid, LOG_LS, LOG_OS, LOG_NOISE, pool[A], y, var, pool[cidx[samp]])
    return types.SimpleNamespace(pool=pool, A=A, y=y, var=var, cidx=cidx, samp=samp, ref=dict(mu=mu, var=pv))


@both
@dtypes
def test_fused_right_hand_sides(kid, dt, monkeypatch):
    """tests/test_rhs_fused.py::test_matern_kernel for the two new forms, with its helpers and its TOL (:22)."""
    q = fused_problem(kid)
    c = _hip.Context(dt)
    c.set_hypers(LOG_LS, LOG_OS, LOG_NOISE, kid)
    c.set_pool(q.pool)
    c.set_train(q.A, q.y, q.var)
    c.factorize()
    c.set_candidates(q.cidx, prior_includes_noise=False)
    (mu, pv), (mu2, pv2), (mu0, pv0) = RF._posteriors(c, monkeypatch)
    RF._check_oracle(mu, pv, q.samp, q.ref, RF.TOL[dt], what='fused')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)                  # fused twice
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)                  # fused against materialised
    full, fused_most = RF._expected_bytes(FUSED_M, FUSED_N, np.dtype(dt).itemsize)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    assert 0 < RF._kmat_bytes(c) <= fused_most < full                          # the fused form ran
    monkeypatch.setenv('ALGP_RHS_FUSED', '0')
    assert RF._kmat_bytes(c) == full
    monkeypatch.delenv('ALGP_RHS_FUSED')
    c.set_candidates(q.cidx, prior_includes_noise=True)
    RF._same_picks(RF._picks(c, monkeypatch, '1'), RF._picks(c, monkeypatch, '0'))
    c.close()


# ---------------------------------------------------------------------------------------------------- 5. one-launch and mid-sized solves
@functools.lru_cache(maxsize=None)
def mid_problem(kid):
    """tests/test_fold.py:_field at N = 300, M = 700"""
    rng = np.random.RandomState(1000)
    xx, yy = np.meshgrid(np.arange(40), np.arange(40))
    grid = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    A = np.sort(rng.permutation(len(grid))[:300])
    pool = np.vstack([grid, rng.uniform(0, 40, (700, 2))])
    var = rng.choice([0.01, 1.0], 300)
    y = rng.uniform(0, 1, 300)
    cidx = np.arange(len(grid), len(grid) + 700)
    mu, pv = MF.posterior(kid, LOG_LS, LOG_OS, LOG_NOISE, pool[A], y, var, pool[cidx])
    S = MF.train_matrix(kid, LOG_LS, LOG_OS, LOG_NOISE, pool[A], var)
    return types.SimpleNamespace(pool=pool, A=A, y=y, var=var, cidx=cidx, mu=mu, pv=pv, S=S, logdet=np.linalg.slogdet(S)[1])


@both
@pytest.mark.parametrize('dt,t', [(np.float64, 1e-9), (np.float32, 2e-3)], ids=DIDS)     # tests/test_fold.py:41
def test_fit_and_solve_and_the_mean_only_posterior(kid, dt, t, monkeypatch):
    q = mid_problem(kid)
    c = _hip.Context(dt)
    c.set_hypers(LOG_LS, LOG_OS, LOG_NOISE, kid)
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
        # the mean-only posterior (posterior_mean_kernel, vecops.hip: no candidate solve behind it) against the solved mean
        mo = c.posterior_mean(q.cidx)
        assert np.max(np.abs(mo - mu)) <= tol(dt, 1e-8, 2e-2) * scale                     # tests/test_fold.py:186
    monkeypatch.delenv('ALGP_FOLD')
    c.close()


# ---------------------------------------------------------------------------------------------------- 6. paths
def _slogdet(M):
    s, ld = np.linalg.slogdet(M)
    assert s > 0
    return ld


@functools.lru_cache(maxsize=None)
def entropy_paths(kid):
    """6 paths of at most 32 sites (the LDS kernel) and 3 of 100 (the batched route) on the pool problem: new sites, one site
    listed twice, a -1 entry, and in every third path a site that is a train row already (a second row for it).  The wanted
    dH = H(A u path) - H(A) are NumPy log-determinants of the enlarged train matrix on the helper's covariance, one per path,
    exactly as tests/test_hip_greedy.py:521-564 forms them."""
    p = pool_problem(kid)
    rng = np.random.RandomState(17)
    sm = 0.7 ** 2
    ldA = _slogdet(p.S)
    out = []
    for lengths, width in (([1, 5, 12, 20, 31, 32], 36), ([100, 100, 100], 104)):
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


@both
@dtypes
def test_score_paths_both_routes(kid, dt):
    """path_score_kernel (<= 64 sites) and path_assemble_kernel (65 .. 256): tolerances of tests/test_hip_greedy.py:565, :617."""
    p = pool_problem(kid)
    c = _pool_ctx(p, dt, False)
    for (paths, want), t in zip(entropy_paths(kid), (tol(dt, 1e-9, 2e-3), tol(dt, 1e-9, 3e-3))):
        got = c.score_paths(paths, 0.7)
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want)) < t * max(1.0, np.max(np.abs(want))), np.max(np.abs(got - want))
    c.close()


@functools.lru_cache(maxsize=None)
def mi_paths(kid):
    """Paths of new sites on the pool problem (one of more than 64 sites: both regimes of the block scorer) and the oracle's
    per-path MI utilities on the helper's matrix, relative to a path that changes nothing (tests/test_mi_paths.py:133-135)."""
    p = pool_problem(kid)
    rng = np.random.RandomState(23)
    lists = [[int(v) for v in rng.permutation(p.free)[:L]] for L in (1, 4, 17, 40, 64, 70)]
    rows = np.full((len(lists), 74), -1, dtype=np.int64)
    for i, s in enumerate(lists):
        row = list(s) + [s[0]]
        row.insert(rng.randint(len(row) + 1), -1)
        rows[i, :len(row)] = row
    _, ut = O.best_path_ref(p.C, p.static, p.mobile, [[]] + lists, [], S_STD, M_STD, 'mutual_information')
    return rows, ut[1:] - ut[0]


@both
@dtypes
def test_score_paths_mi(kid, dt):
    """tests/test_mi_paths.py:102-135: candidates are the sites without a mobile reading; tolerance :119."""
    p = pool_problem(kid)
    rows, want = mi_paths(kid)
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, cand=np.where(~p.mobile)[0])
        got = c.score_paths_mi(rows, S_STD, M_STD)
        c.close()
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want)) <= tol(dt, 1e-7, 3e-3) * np.max(np.abs(want)), np.max(np.abs(got - want))


@functools.lru_cache(maxsize=None)
def vr_paths(kid):
    """Paths on the pool problem and their variance-reduction utilities by the definition (include/algp_hip.h;
    tests/test_paths_vr_host.py: brute_force): one refit per path on the helper's matrix.  A new site joins the train set with
    noise sm, a site with a train row of noise v ends with v sm / (v + sm).  Every path holds at least three new sites, so no
    utility is small enough for the difference of the two sums to lose digits."""
    p = pool_problem(kid)
    rng = np.random.RandomState(29)
    T = p.free
    dC = np.diag(p.C)

    def sumvar(tr, nz):
        B = p.C[np.ix_(tr, T)]
        return float(np.sum(dC[T]) - np.sum(B * np.linalg.solve(p.C[np.ix_(tr, tr)] + np.diag(nz), B)))

    base = sumvar(p.A, p.var)
    static_only = np.where(p.static & ~p.mobile)[0]
    lists = []
    for L in (3, 20, 64, 70):
        lists.append([int(v) for v in rng.permutation(p.free)[:L]])
        lists.append([int(v) for v in rng.permutation(p.free)[:L - 1]] + [int(static_only[L % len(static_only)])])
    rows = np.full((len(lists), 72), -1, dtype=np.int64)
    want = np.zeros(len(lists))
    pos = {int(s): i for i, s in enumerate(p.A)}
    for i, s in enumerate(lists):
        rows[i, :len(s)] = s
        rows[i, len(s)] = s[0]                                   # a site listed twice is read once
        tr, nz = [int(a) for a in p.A], [float(v) for v in p.var]
        for site in s:
            if site in pos:
                nz[pos[site]] = nz[pos[site]] * SM / (nz[pos[site]] + SM)
            else:
                tr.append(site)
                nz.append(SM)
        want[i] = base - sumvar(tr, nz)
    return rows, want


@both
@dtypes
def test_score_paths_vr(kid, dt):
    """tests/test_paths_vr.py:84-95 with its TOL (:37), per utility relative to the reference's own value."""
    p = pool_problem(kid)
    rows, want = vr_paths(kid)
    assert np.min(want) > 1e-2
    for explicit in (False, True):
        c = _pool_ctx(p, dt, explicit, alive=p.alive)
        got = c.score_paths_vr(rows, M_STD)
        c.close()
        err = np.abs(got - want) / np.abs(want)
        print('paths vr %s: worst %.3e' % ('explicit' if explicit else 'coordinates', float(np.max(err))))
        assert np.all(np.isfinite(got)) and np.max(err) < tol(dt, 1e-9, 1e-3)


# ---------------------------------------------------------------------------------------------------- 7. MLL and gradient
@functools.lru_cache(maxsize=None)
def mll_problem(kid, N, twice):
    """The problem of tests/test_host_api.py:130 (N = 150, D = 3); `twice`: rows 5 and N - 3 name the same pool site."""
    rng = np.random.RandomState(3)
    x = rng.uniform(0, 6, (N, 3))
    y = np.sin(x[:, 0]) + 0.1 * rng.standard_normal(N)
    var = rng.uniform(0.005, 0.05, N)
    idx = np.arange(N)
    if twice:
        idx[N - 3] = 5
    th = (np.log([1.3, 2.1, 0.8]), np.log(0.9), np.log(0.05))
    xs = x[idx]
    q = types.SimpleNamespace(x=x, y=y, var=var, idx=idx, th=th)
    q.S = MF.train_matrix(kid, th[0], th[1], th[2], xs, var, idx)
    q.mll = MF.mll(kid, th[0], th[1], th[2], xs, y, var, idx)
    q.grad = MF.mll_grad(kid, th[0], th[1], th[2], xs, y, var, idx)
    return q


MLL_CASES = [pytest.param(MF.MATERN05, 150, False, id='matern05-N150'), pytest.param(MF.MATERN25, 150, False, id='matern25-N150'),
             pytest.param(MF.MATERN05, 150, True, id='matern05-N150-site-twice'),
             pytest.param(MF.MATERN05, 70, True, id='matern05-N70-site-twice'), pytest.param(MF.MATERN25, 70, False, id='matern25-N70')]


@pytest.mark.parametrize('kid,N,twice', MLL_CASES)
@dtypes
def test_mll_and_gradient(kid, N, twice, dt):
    """algp_get_mll / algp_get_mll_grad against the helper, and algp_fit_step against the three calls.  fp64: the tolerances of
    tests/test_host_api.py:143-145 (MLL 1e-10 relative, gradient 1e-8 of its largest entry); fp32: tests/test_fit_regimes.py:49
    (2e-2, the MLL relative to |MLL|, the gradient elementwise relative to max(1, |want|)), which that file applies to
    Matern-3/2.  N = 70 crosses the 64-row tile of mll_grad_kernel; with a site in two rows the pair has r = 0 off the diagonal,
    where the nu = 1/2 derivative factor must be 0 and not NaN."""
    q = mll_problem(kid, N, twice)
    c = _hip.Context(dt)
    c.set_hypers(q.th[0], q.th[1], q.th[2], kid)
    c.set_pool(q.x)
    c.set_train(q.idx, q.y, q.var)
    c.factorize()
    mll, g = c.mll(), c.mll_grad()
    print('mll %.12e (want %.12e)  grad err %.2e' % (mll, q.mll, float(np.max(np.abs(g - q.grad)))))
    assert np.isfinite(mll) and np.all(np.isfinite(g))
    if np.dtype(dt) == np.float64:
        assert mll == pytest.approx(q.mll, rel=1e-10)
        assert relerr(g, q.grad) < 1e-8
    else:
        assert abs(mll - q.mll) <= 2e-2 * abs(q.mll)
        assert np.max(np.abs(g - q.grad) / np.maximum(1.0, np.abs(q.grad))) <= 2e-2
    mll_s, g_s = c.fit_step()
    # tests/test_fold.py:213-214: the step carries z as a row of the panel where the three calls substitute, rounding only
    assert abs(mll_s - mll) <= tol(dt, 1e-12, 1e-6) * abs(mll)
    assert np.max(np.abs(g_s - g) / np.maximum(1.0, np.abs(g))) <= tol(dt, 1e-10, 2e-3)
    mll_b, g_b = c.fit_step()
    assert mll_b == mll_s and np.array_equal(g_b, g_s)
    c.close()


# ---------------------------------------------------------------------------------------------------- 8. GPR.fit
@functools.lru_cache(maxsize=None)
def fit_problem():
    rng = np.random.RandomState(8)
    grid, field = O.generate_gaussian_data(12, 12, k=5, rng=rng)
    x = grid.astype(np.float64)
    y = field + 0.1 * rng.standard_normal(len(x))
    return x, y, np.full(len(x), 1e-2)


@dtypes
def test_gpr_fit_with_matern25(dt):
    from algp_amd.models import GPR
    x, y, var = fit_problem()
    gp = GPR(lr=.1, max_iterations=30, kernel_params={'type': 'matern', 'nu': 2.5}, dtype=dt)
    losses = gp.fit(x, y, var)
    assert len(losses) == 30 and np.all(np.isfinite(losses))
    assert losses[-1] < losses[0]                                # the loss is -MLL / N: the likelihood went up
    ls, los, ln, kt = gp.hypers()
    assert kt == _hip.KERNEL_MATERN25
    C = gp.cov_mat(x, add_likelihood_var=True)
    want = MF.kernel_matrix(MF.MATERN25, ls, los, x) + np.exp(ln) * np.eye(len(x))
    assert relerr(C, want) < tol(dt, 1e-13, 2e-5)                # tests/test_hip_kernels.py:142
    Cx = gp.cov_mat(x[:7], x2=x[5:20])
    assert relerr(Cx, MF.kernel_matrix(MF.MATERN25, ls, los, x[:7], x[5:20])) < tol(dt, 1e-13, 2e-5)
