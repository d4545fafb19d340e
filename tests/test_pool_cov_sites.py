"""Every instantiation of the kernels that evaluate the pool covariance through pool_cov (common.h) -- lazy_refresh_kernel,
kgemv_kernel, path_score_kernel, path_assemble_kernel, pvr_assemble_kernel and the variance-reduction epilogues of gemm.hip --
under an assertion: the (entry point x padded coordinate width DP x kernel form x pool kind x dtype) combinations that the rest
of the suite does not reach.

What the other files reach (DP = 2, 4, 8 for D <= 2, 3..4, 5..8; forms rbf, matern15, matern05, matern25):
 - algp_greedy / algp_best_candidate, entropy (lazy_refresh_kernel): DP 2, 4, 8 x rbf, matern15 x coordinates x both dtypes
   (test_greedy_regimes.py); DP 2 x rbf x covariance pool (same file); DP 2 x matern05, matern25 x both pools (test_matern_family.py).
 - algp_posterior_mean (kgemv_kernel): DP 2, 4, 8 x rbf (test_hip_kernels.py; matern15 only where the random draws of
   test_randomized_sweep.py land on it), DP 2 x matern05, matern25 (test_matern_family.py); a coordinate pool only, the call refuses
   a covariance pool.
 - variance-reduction scores and folds (the epilogues at width MAXD whatever D is; kgemv_kernel in the fold): DP 2 and 8 x rbf, matern15
   x both pools x both dtypes (test_variance_reduction.py), DP 2 x matern05, matern25 (test_matern_family.py).
 - algp_score_paths (path_score_kernel up to 64 sites, path_assemble_kernel beyond): short paths DP 2, 4, 8 in a few (dtype, form)
   pairs, coordinates only (test_hip_greedy.py); long paths DP 2 only; matern05, matern25 at DP 2.
 - algp_score_paths_vr (pvr_assemble_kernel): DP 2 and 8 x rbf, matern15 x both pools x both dtypes (test_paths_vr.py); DP 2 x
   matern05, matern25.
Missing, and run here: everything at DP 4 but the entropy greedy with the two older forms and the mean with rbf; matern05 and matern25 at DP 4 and 8
everywhere; the covariance pool at DP 4 and 8 in the entropy greedy and the path scores; the long paths beyond DP 2.  So this file
takes D = 3 and D = 5 and, per entry point, the forms and pools listed at its test.

Problems: the generator of tests/test_variance_reduction.py (coordinates in [0, 12]^D, length-scales in [2, 4], outputscale 1.3,
noise 0.05, the first third of the train sites static, every site a candidate) at its shape of 300 sites with 130 train sites, and
400 sites with 129 train sites for the paths of more than 64 sites, as tests/test_paths_vr.py; the entropy greedy on the width
problems of tests/test_greedy_regimes.py.  The covariance is oracle.gp_oracle.kernel_matrix for rbf and matern15 and
tests/matern_forms.py (fp64 NumPy, independent of the library) for matern05 and matern25, plus sigma_n^2 I; every train matrix is
asserted to factor in fp32-rounded NumPy when the problem is built.

References, none of them the library: oracle.gp_oracle.greedy_fast on that covariance (entropy greedy, through the helpers of
tests/test_greedy_regimes.py, picks compared as there: only where the oracle's top-two gap clears the bound at every pick); NumPy
solves for the mean; vr_reference of tests/test_variance_reduction.py (brute force per candidate); one NumPy log-determinant per
path as tests/test_hip_greedy.py:546-562; brute_force of tests/test_paths_vr_host.py (one refit per path).
Bars, each the one its entry point's existing file uses: utilities 1e-9 fp64 / 1e-3 fp32 (test_greedy_regimes.py:165,
test_variance_reduction.py:48, test_paths_vr.py:36); the mean 1e-8 / 2e-2 of the largest mean (test_hip_kernels.py:208);
algp_score_paths 1e-9 / 2e-3 of max(1, largest) (test_hip_greedy.py:565).
"""
import functools
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import matern_forms as MF                            # noqa: E402
import test_greedy_regimes as GR                     # noqa: E402
import test_paths_vr_host as H                       # noqa: E402
import test_variance_reduction as VR                 # noqa: E402
from algp_amd import _hip                            # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = {'rbf': MF.RBF, 'matern15': MF.MATERN15, 'matern05': MF.MATERN05, 'matern25': MF.MATERN25}
DT = [np.float64, np.float32]
DIDS = ['f64', 'f32']
SS, SM = VR.SS, VR.SM
SHORT, LONG = (300, 130), (400, 129)


def _ids(cases):
    return [pytest.param(*c, id='-'.join(str(v) for v in c)) for c in cases]


def covariance(kid, hyp, X):
    """C of the whole pool, sigma_n^2 on the diagonal: the oracle's kernel matrix for the forms it has, the helper's for the others"""
    if kid in (MF.RBF, MF.MATERN15):
        assert hyp.kernel == kid
        K = O.kernel_matrix(hyp, X)
    else:
        K = MF.kernel_matrix(kid, hyp.log_lengthscale, hyp.log_outputscale, X)
    return K + hyp.noise * np.eye(len(X))


@functools.lru_cache(maxsize=None)
def problem(shape, D, form):
    """tests/test_variance_reduction.py:98 with the covariance of any of the four forms; no device needed"""
    n, N = shape
    kid = FORMS[form]
    rng = np.random.RandomState(1000 * n + 10 * D + kid)
    p = types.SimpleNamespace(n=n, N=N, D=D)
    p.X = rng.uniform(0.0, 12.0, size=(n, D))
    p.hyp = O.Hypers(np.log(rng.uniform(2.0, 4.0, size=D)), np.log(1.3), np.log(0.05), kid)
    p.C = covariance(kid, p.hyp, p.X)
    p.cov = lambda rows, cols: p.C[np.ix_(np.asarray(rows, np.int64), np.asarray(cols, np.int64))]
    perm = rng.permutation(n)
    p.A, p.free = perm[:N], perm[N:]
    p.ns = N // 3
    p.noise = np.r_[np.full(p.ns, SS ** 2), np.full(N - p.ns, SM ** 2)]
    p.static = p.A[:p.ns]
    p.cand = np.arange(n)
    p.alive = np.ones(n, bool)
    p.alive[p.static] = False
    p.y = rng.standard_normal(N)
    assert MF.factors_in_fp32(p.cov(p.A, p.A) + np.diag(p.noise))
    return p


# --------------------------------------------------------------------------------------------- 1. entropy greedy
@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in DT}
    yield c
    for v in c.values():
        v.close()


@functools.lru_cache(maxsize=None)
def width_problem(D, form, explicit):
    """tests/test_greedy_regimes.py's width problem (400 sites: 60 static, 100 mobile, 20 both) under any form and pool kind"""
    kid = FORMS[form]
    p = GR._problem(('sites', D, form, explicit), GR.SEEDS[('w', D, GR.RBF)], GR.N_POOL, D, O.KERNEL_RBF, 60, 100, 20, explicit)
    p.hyp.kernel = kid
    p.C = covariance(kid, p.hyp, p.X)
    assert MF.factors_in_fp32(p.C[np.ix_(p.A, p.A)] + np.diag(p.var))
    return p


@pytest.mark.parametrize('dt', DT, ids=DIDS)
@pytest.mark.parametrize('D,form,pool', _ids([(D, f, 'coords') for D in (3, 5) for f in ('matern05', 'matern25')] +
                                              [(D, f, 'cov') for D in (3, 5) for f in ('rbf', 'matern25')]))
def test_entropy_greedy(ctxs, D, form, pool, dt):
    """6 picks through the full pass, the picks-only route and the stepwise route (refresh modes 2, 0 and 1), every utility against
    the oracle and the survivors against one dense solve"""
    c = ctxs[np.dtype(dt)]
    p = width_problem(D, form, pool == 'cov')
    GR._load(c, p)
    GR._three_routes(c, p, GR.K_WIDTHS, 'D=%d %s %s' % (D, form, pool))


# --------------------------------------------------------------------------------------------- 2. the mean-only posterior
@pytest.mark.parametrize('dt', DT, ids=DIDS)
@pytest.mark.parametrize('D,form', _ids([(D, f) for D in (3, 5) for f in ('matern15', 'matern05', 'matern25')]))
def test_posterior_mean(D, form, dt):
    p = problem(SHORT, D, form)
    want = p.y.mean() + p.cov(p.free, p.A) @ np.linalg.solve(p.cov(p.A, p.A) + np.diag(p.noise), p.y - p.y.mean())
    c = _hip.Context(dt)
    c.set_hypers(p.hyp.log_lengthscale, p.hyp.log_outputscale, p.hyp.log_noise, p.hyp.kernel)
    c.set_pool(p.X)
    c.set_train(p.A, p.y, p.noise)
    c.factorize()
    got = c.posterior_mean(p.free)
    c.close()
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print('posterior_mean D=%d %s %s: %.3e of the largest mean' % (D, form, np.dtype(dt).name, err))
    assert err < (1e-8 if dt is np.float64 else 2e-2)


# --------------------------------------------------------------------------------------------- 3. variance reduction: product, folds
VR_K = 3


@functools.lru_cache(maxsize=None)
def vr_reference(D, form):
    p = problem(SHORT, D, form)
    return VR.vr_reference(p.C, p.A, p.noise, p.cand, p.alive, SS ** 2, SM ** 2, VR_K)


@pytest.mark.parametrize('pool', VR.POOLS)
@pytest.mark.parametrize('dt', DT, ids=DIDS)
@pytest.mark.parametrize('D,form', _ids([(3, f) for f in FORMS] + [(5, 'matern05'), (5, 'matern25')]))
def test_variance_reduction_scores_and_folds(D, form, dt, pool):
    """the first scoring (the product's epilogue) and the scorings after one and two commits (a rank-1 fold each: the kernel-GEMV over
    the targets) along the reference's own picks, every candidate against the brute force"""
    p = problem(SHORT, D, form)
    picks, U = vr_reference(D, form)
    c = VR.context(p, dt, pool)
    got_p, got_u = c.greedy(VR.CRIT, SS, SM, VR_K, forced_picks=picks, want_utilities=True)
    c.close()
    assert [int(v) for v in got_p] == picks
    for r in range(VR_K):
        VR.compare(got_u[r], U[r], VR.TOL[dt], 'D=%d %s %s round %d' % (D, form, pool, r))


# --------------------------------------------------------------------------------------------- 4. path scores, both criteria
def make_paths(p, lengths):
    """per length an all-new path and one mixing new sites with statically sampled ones (a quarter of it)"""
    rng = np.random.RandomState(5 + p.n + p.D)
    rows = []
    for k in lengths:
        rows.append([int(v) for v in rng.choice(p.free, k, replace=False)])
        m = max(1, k // 4)
        mixed = [int(v) for v in rng.choice(p.free, k - m, replace=False)] + [int(v) for v in rng.choice(p.static, m, replace=False)]
        rows.append([mixed[i] for i in rng.permutation(k)])
    sites = np.full((len(rows), max(len(r) for r in rows)), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        sites[i, :len(r)] = r
    return sites


@functools.lru_cache(maxsize=None)
def path_reference(shape, D, form):
    """(sites, entropy gains by one log-determinant per path, variance reductions by one refit per path)"""
    p = problem(shape, D, form)
    sites = make_paths(p, (5, 64) if shape == SHORT else (65, 130))
    ldA = np.linalg.slogdet(p.cov(p.A, p.A) + np.diag(p.noise))[1]
    dH = np.zeros(len(sites))
    for i, row in enumerate(sites):
        uniq = H.distinct(row)
        idx = np.r_[p.A, uniq].astype(int)               # a site that is a train row already gets a second row
        S = p.cov(idx, idx) + np.diag(np.r_[p.noise, np.full(len(uniq), SM ** 2)])
        dH[i] = len(uniq) * O.CONST + 0.5 * (np.linalg.slogdet(S)[1] - ldA)
    return sites, dH, H.brute_force(p, sites)[0]


@pytest.mark.parametrize('pool', VR.POOLS)
@pytest.mark.parametrize('dt', DT, ids=DIDS)
@pytest.mark.parametrize('shape', [SHORT, LONG], ids=['n300-N130', 'n400-N129'])
@pytest.mark.parametrize('D,form', _ids([(D, f) for D in (3, 5) for f in FORMS]))
def test_path_scores(D, form, shape, dt, pool):
    """algp_score_paths and algp_score_paths_vr on paths of 5 and 64 sites (the LDS kernels) and of 65 and 130 (the batched route at
    both block paddings)"""
    p = problem(shape, D, form)
    sites, dH, dV = path_reference(shape, D, form)
    c = VR.context(p, dt, pool)
    got_h = c.score_paths(sites, SM)
    got_v = c.score_paths_vr(sites, SM)
    c.close()
    err = float(np.max(np.abs(got_h - dH)))
    print('score_paths D=%d %s %s %s: %.3e of max(1, %.3f)' % (D, form, pool, np.dtype(dt).name, err, np.max(np.abs(dH))))
    assert err < (1e-9 if dt is np.float64 else 2e-3) * max(1.0, np.max(np.abs(dH)))
    rel = np.abs(got_v - dV) / np.abs(dV)
    print('score_paths_vr: worst relative error %.3e' % rel.max())
    assert np.all(np.isfinite(got_v)) and rel.max() < VR.TOL[dt]
