"""The variance-reduction (ALC) criterion, ALGP_CRIT_VARIANCE_REDUCTION, against a brute force of its definition.

Definition (include/algp_hip.h): with the targets T = the candidates that have no train row, fixed by the candidate solve,
    u_c = sum_{j in T} var(j | A) - sum_{j in T} var(j | A with c static-sampled),
train noise per site static_std^2, mobile_std^2 or, for a site with both readings, 1/(1/ss + 1/sm) (reference
agent.py:302-308, 321-328).  `vr_reference` below is that sentence in fp64 NumPy: one refit per candidate, on an explicit
covariance C = oracle.gp_oracle.kernel_matrix + sigma_n^2 I.  The library computes the same numbers from one fused product
(first scoring after a solve) and one rank-1 fold per committed pick.

Shapes (sites n, train N, D): (100, 40, 2) one 128-tile; (300, 130, 2) three ragged tiles, two k blocks; (257, 129, 6) both
edges off by one, DP = 8.  Coordinates uniform in [0, 12]^D, lengthscales in [2, 4], outputscale 1.3, noise 0.05; a third
of the train sites static, the rest mobile; every site is a candidate, so the mobile-sampled ones are unit rows, the
static-sampled ones are unit rows switched off, and the rest are ordinary rows (the targets).

Tolerances, per finite entry, relative to the reference's own value:
  fp64 1e-9 (the project's bar for posterior quantities at this conditioning; the closed form itself matches the brute
       force to 4e-12 on the CPU, which is the brute force's own rounding);
  fp32 1e-3 (the project's fp32 bar).  A NumPy float32 evaluation of the same closed form (float32 Cholesky and solves)
       is off by 3.1e-5 on (300, 130, 2) and 2.3e-5 on (100, 40, 2).
Measured on an MI355X over all cases of this file: fp32 at most 6.1e-5, so the bar was not widened; fp64 at most 3.6e-10,
on a utility of 6e-5 (n = 100, RBF), where the brute force's own difference of two sums of 60 variances carries 1e-10; every
other fp64 case is below 2e-11.  ALGP_VR_RANK1=0 against the default: 1.2e-14 (fp64), 7.4e-6 (fp32).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from algp_amd import _hip
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS, SM = 0.1, 1.0                                    # static_std, mobile_std
CRIT = 2                                             # the value under test, spelled out: the header's enum is checked elsewhere
K = 4
SHAPES = [(100, 40, 2), (300, 130, 2), (257, 129, 6)]
SHAPE_IDS = ['n100-N40-D2', 'n300-N130-D2', 'n257-N129-D6']
KERNELS = [O.KERNEL_RBF, O.KERNEL_MATERN15]
KIDS = ['rbf', 'matern']
DTYPES = [np.float64, np.float32]
DIDS = ['f64', 'f32']
POOLS = ['coords', 'cov']
TOL = {np.float64: 1e-9, np.float32: 1e-3}


def vr_reference(C, train, noise, cand, alive, ss, sm, k, forced=None, ss_score=None):
    """(picks, utilities (k, M)) of k greedy rounds by brute force.  train / noise: the train sites and their noise
    variances; alive: which candidates may be picked; forced: the picks to commit instead of the maxima; ss_score: per
    round, the static variance the candidates are scored with (commits always use ss)."""
    train, noise, cand = [int(a) for a in train], [float(v) for v in noise], [int(c) for c in cand]
    T = [c for c in cand if c not in set(train)]     # fixed for all rounds
    dC = np.diag(C)

    def sumvar(tr, nz):
        S = C[np.ix_(tr, tr)] + np.diag(nz)
        B = C[np.ix_(tr, T)]
        return float(np.sum(dC[T]) - np.sum(B * np.linalg.solve(S, B)))

    done, U, picks = set(), [], []
    for r in range(k):
        s2 = ss if ss_score is None else ss_score[r]
        base = sumvar(train, noise)
        pos = {s: i for i, s in enumerate(train)}
        u = np.full(len(cand), -np.inf)
        for ci, c in enumerate(cand):
            if not alive[ci] or c in done:
                continue
            if c in pos:                             # a sampled site: its noise becomes the fused one
                nz = list(noise)
                nz[pos[c]] = 1.0 / (1.0 / s2 + 1.0 / sm)
                u[ci] = base - sumvar(train, nz)
            else:
                u[ci] = base - sumvar(train + [c], noise + [s2])
        U.append(u)
        p = int(forced[r]) if forced is not None else cand[int(np.argmax(u))]
        picks.append(p)
        done.add(p)
        if p in pos:
            noise[pos[p]] = 1.0 / (1.0 / ss + 1.0 / sm)
        else:
            train.append(p)
            noise.append(ss)
    return picks, np.array(U)


class Problem(object):
    pass


_PROBLEMS, _REFS = {}, {}


def problem(shape, kernel):
    key = (shape, kernel)
    if key not in _PROBLEMS:
        n, N, D = shape
        rng = np.random.RandomState(1000 * n + 10 * D + kernel)
        p = Problem()
        p.key, p.n, p.N, p.D = key, n, N, D
        p.X = rng.uniform(0.0, 12.0, size=(n, D))
        p.hyp = O.Hypers(np.log(rng.uniform(2.0, 4.0, size=D)), np.log(1.3), np.log(0.05), kernel)
        p.C = O.kernel_matrix(p.hyp, p.X) + p.hyp.noise * np.eye(n)
        perm = rng.permutation(n)
        p.A = perm[:N]
        p.ns = N // 3                                # the first third of the train sites is static
        p.noise = np.r_[np.full(p.ns, SS ** 2), np.full(N - p.ns, SM ** 2)]
        p.static = p.A[:p.ns]
        p.mobile = p.A[p.ns:]
        p.cand = np.arange(n)
        p.alive = np.ones(n, bool)
        p.alive[p.static] = False
        p.unit = np.zeros(n, bool)
        p.unit[p.A] = True
        p.free = perm[N:]                            # the ordinary rows = the targets
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


def reference(p, what):
    """References are computed once per problem and shared: 'own' = the reference's own greedy picks; 'mobile' = the same
    with its second pick replaced by a mobile-sampled site; 'masked' = some ordinary rows switched off (scores only)."""
    key = (p.key, what)
    if key not in _REFS:
        ss, sm = SS ** 2, SM ** 2
        if what == 'own':
            _REFS[key] = vr_reference(p.C, p.A, p.noise, p.cand, p.alive, ss, sm, K)
        elif what == 'mobile':
            forced = list(reference(p, 'own')[0])
            forced[1] = int(p.mobile[len(p.mobile) // 2])
            assert forced[1] not in (forced[0], forced[2], forced[3])
            _REFS[key] = vr_reference(p.C, p.A, p.noise, p.cand, p.alive, ss, sm, K, forced=forced)
        elif what == 'masked':
            alive = p.alive.copy()
            alive[p.free[::7]] = False
            _REFS[key] = (alive, vr_reference(p.C, p.A, p.noise, p.cand, alive, ss, sm, 1)[1][0])
    return _REFS[key]


def context(p, dtype, pool, cand=None, alive=None, prior_includes_noise=True):
    c = _hip.Context(dtype)
    c.set_hypers(p.hyp.log_lengthscale, p.hyp.log_outputscale, p.hyp.log_noise, p.hyp.kernel)
    if pool == 'cov':
        c.set_pool_cov(p.C)
    else:
        c.set_pool(p.X)
    c.set_train(p.A, np.zeros(p.N), p.noise)
    c.factorize()
    c.set_candidates(p.cand if cand is None else cand, prior_includes_noise=prior_includes_noise)
    c.solve_candidates(alive=p.alive if alive is None else alive)
    return c


def compare(got, want, tol, what):
    """every finite entry of the reference within tol (relative), -inf exactly where the reference has it"""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), what + ': -inf entries differ'
    assert np.all(np.isfinite(got[fin])), what + ': non-finite utilities'
    err = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin])))
    print('%s: max relative error %.3e (bar %.1e), utilities in [%.3e, %.3e]' % (what, err, tol, want[fin].min(), want[fin].max()))
    assert err < tol, (what, err, tol)
    return err


CASES = dict(argnames='dtype,kernel,shape,pool',
             argvalues=[pytest.param(dt, k, s, pl, id='-'.join([di, ki, si, pl]))
                        for dt, di in zip(DTYPES, DIDS) for k, ki in zip(KERNELS, KIDS) for s, si in zip(SHAPES, SHAPE_IDS)
                        for pl in POOLS])


@pytest.mark.parametrize(**CASES)
def test_scores_before_any_pick(dtype, kernel, shape, pool):
    """The first scoring after a solve (the fused product alone) equals the brute force on every candidate."""
    p = problem(shape, kernel)
    _, U = reference(p, 'own')
    c = context(p, dtype, pool)
    u = c.scores(CRIT, SS, SM)
    c.close()
    fin = np.isfinite(u)
    assert np.any(fin & p.unit) and np.any(fin & ~p.unit), 'both candidate kinds must be scored'
    assert np.all(np.isneginf(u[p.static]))
    compare(u, U[0], TOL[dtype], 'scores')


@pytest.mark.parametrize(**CASES)
def test_greedy_utilities_and_picks(dtype, kernel, shape, pool):
    """k = 4 rounds: with the reference's own picks forced, every round's utilities equal the reference's (rounds 2..4 come
    from the rank-1 folds); unforced, the picks are the reference's wherever its best-to-second gap exceeds the tolerance."""
    p = problem(shape, kernel)
    picks, U = reference(p, 'own')
    tol = TOL[dtype]
    c = context(p, dtype, pool)
    got_p, got_u = c.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)
    assert [int(v) for v in got_p] == picks
    for r in range(K):
        compare(got_u[r], U[r], tol, 'round %d' % r)
    c.solve_candidates(alive=p.alive)                # a new solve drops the picks and the criterion's state
    free_p = c.greedy(CRIT, SS, SM, K)
    c.close()
    for r in range(K):
        top = np.sort(U[r][np.isfinite(U[r])])[-2:]
        gap = (top[1] - top[0]) / top[1]
        print('round %d: reference gap %.3e, pick %d, got %d' % (r, gap, picks[r], int(free_p[r])))
        if gap <= 2 * tol:
            break                                    # a tie within the tolerance: the states may part from here on
        assert int(free_p[r]) == picks[r]


@pytest.mark.parametrize('pool', POOLS)
@pytest.mark.parametrize('kernel', KERNELS, ids=KIDS)
@pytest.mark.parametrize('dtype', DTYPES, ids=DIDS)
def test_greedy_with_a_mobile_site_picked(dtype, kernel, pool):
    """A forced pick of a mobile-sampled site (a unit row: its noise becomes the fused one) appends a column of the other
    kind; the rounds after it must still equal the brute force."""
    p = problem(SHAPES[1], kernel)
    picks, U = reference(p, 'mobile')
    assert p.unit[picks[1]] and not p.unit[picks[0]]
    c = context(p, dtype, pool)
    got_p, got_u = c.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)
    c.close()
    for r in range(K):
        compare(got_u[r], U[r], TOL[dtype], 'round %d' % r)
    assert np.isneginf(got_u[2][picks[1]]) and np.isneginf(got_u[3][picks[1]])


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[2]], ids=[SHAPE_IDS[1], SHAPE_IDS[2]])
@pytest.mark.parametrize('dtype', DTYPES, ids=DIDS)
def test_utility_is_the_drop_of_the_summed_variance(dtype, shape):
    """Through the public API alone: the posterior variances summed over the targets before and after commit_pick(p)
    differ by u_p, for an ordinary p and for a mobile-sampled p."""
    p = problem(shape, O.KERNEL_RBF)
    c = context(p, dtype, 'coords')
    tol = TOL[dtype]
    for site in (int(p.free[3]), int(p.mobile[5])):
        u = c.scores(CRIT, SS, SM)
        before = float(np.sum(c.posterior()[1][p.free].astype(np.float64)))
        c.commit_pick(site, SS, SM)
        after = float(np.sum(c.posterior()[1][p.free].astype(np.float64)))
        # the two sums carry the rounding of |T| variances each: eps |T| max(var) on top of the utility's own tolerance
        slack = np.finfo(dtype).eps * len(p.free) * 2.0
        print('site %d: u %.12e, drop %.12e' % (site, u[site], before - after))
        assert abs((before - after) - u[site]) < tol * abs(u[site]) + slack
    c.close()


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2]], ids=[SHAPE_IDS[0], SHAPE_IDS[2]])
@pytest.mark.parametrize('dtype', DTYPES, ids=DIDS)
def test_switched_off_rows_stay_targets(dtype, shape):
    """alive = 0 on some ordinary rows: they score -inf and still count as targets of every other row."""
    p = problem(shape, O.KERNEL_MATERN15)
    alive, want = reference(p, 'masked')
    c = context(p, dtype, 'coords', alive=alive)
    u = c.scores(CRIT, SS, SM)
    c.close()
    assert np.all(np.isneginf(u[p.free[::7]]))
    compare(u, want, TOL[dtype], 'masked scores')
    # they are still targets: switching rows off changes no other row's utility
    full = reference(p, 'own')[1][0]
    both = np.isfinite(want) & np.isfinite(full)
    assert np.allclose(want[both], full[both], rtol=1e-12)


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_variance_reduction as t
from algp_amd import _hip
dtype = np.dtype(sys.argv[1]).type
p = t.problem(t.SHAPES[1], t.O.KERNEL_RBF)
picks = [int(p.free[2]), int(p.mobile[3]), int(p.free[9]), int(p.free[11])]
c = t.context(p, dtype, 'coords')
_, u = c.greedy(t.CRIT, t.SS, t.SM, t.K, forced_picks=picks, want_utilities=True)
print(json.dumps({'u': [[float(v) if np.isfinite(v) else None for v in row] for row in u]}))
""" % (REPO, os.path.join(REPO, 'tests'))


def _child(dtype, env_extra):
    env = dict(os.environ)
    env.pop('ALGP_VR_RANK1', None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, '-c', _CHILD, np.dtype(dtype).name], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    u = json.loads(r.stdout.strip().splitlines()[-1])['u']
    return np.array([[-np.inf if v is None else v for v in row] for row in u])


@pytest.mark.parametrize('dtype', DTYPES, ids=DIDS)
def test_rank1_switch(dtype):
    """ALGP_VR_RANK1=0 (the full product at every scoring, over the appended columns too) against the default (one product,
    then a rank-1 fold per pick), each in a process of its own: fp64 to 1e-12, fp32 within the fp32 bar."""
    default = _child(dtype, {})
    full = _child(dtype, {'ALGP_VR_RANK1': '0'})
    assert np.array_equal(default[0], full[0])       # no pick yet: the same product, the same bits
    compare(default, full, 1e-12 if dtype is np.float64 else TOL[dtype], 'rank-1 against full product')


@pytest.mark.parametrize('dtype', DTYPES, ids=DIDS)
def test_state_follows_the_solve_and_not_the_noise_levels(dtype):
    p = problem(SHAPES[1], O.KERNEL_RBF)
    tol = TOL[dtype]
    picks, U = reference(p, 'own')
    c = context(p, dtype, 'coords')
    compare(c.scores(CRIT, SS, SM), U[0], tol, 'first set')
    # a new candidate set and solve: the state of the old one must not be reused
    sub = np.sort(np.r_[p.free[::2], p.mobile[::3], p.static[:4]])
    alive = ~np.isin(sub, p.static)
    c.set_candidates(sub, prior_includes_noise=True)
    c.solve_candidates(alive=alive)
    want = vr_reference(p.C, p.A, p.noise, sub, alive, SS ** 2, SM ** 2, 1)[1][0]
    compare(c.scores(CRIT, SS, SM), want, tol, 'second set')
    # back to the first set: two picks, then scoring with another static_std reuses the folded state
    c.set_candidates(p.cand, prior_includes_noise=True)
    c.solve_candidates(alive=p.alive)
    c.greedy(CRIT, SS, SM, 2, forced_picks=picks[:2])
    s2 = 0.3
    want = vr_reference(p.C, p.A, p.noise, p.cand, p.alive, SS ** 2, SM ** 2, 3, forced=picks[:3],
                        ss_score=[SS ** 2, SS ** 2, s2 ** 2])[1][2]
    compare(c.scores(CRIT, s2, SM), want, tol, 'other static_std after two picks')
    c.close()


def test_refusals():
    p = problem(SHAPES[0], O.KERNEL_RBF)
    c = context(p, np.float64, 'coords')
    picks = np.zeros(1, np.int64)
    rc = c.lib.algp_greedy_sharded(c.h, CRIT, SS, SM, 1, _hip._i64(picks), None)
    assert rc == _hip.ERR_BAD_ARG
    c.set_candidates(p.free, prior_includes_noise=False)
    c.solve_candidates()
    out = np.empty(len(p.free))
    rc = c.lib.algp_scores(c.h, CRIT, SS, SM, _hip._ptr(out), 0)
    assert rc == _hip.ERR_STATE
    # a pool site listed twice: two targets with sigma_n^2 between them, refused rather than scored
    twice = np.r_[p.free[:10], p.free[3]]
    c.set_candidates(twice, prior_includes_noise=True)
    c.solve_candidates()
    out = np.empty(len(twice))
    assert c.lib.algp_scores(c.h, CRIT, SS, SM, _hip._ptr(out), 0) == _hip.ERR_STATE
    assert np.all(np.isfinite(c.scores(_hip.CRIT_ENTROPY, SS, SM)))      # the other criteria keep taking such a set
    c.close()
