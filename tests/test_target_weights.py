"""Target weights for the variance-reduction criterion: algp_set_target_weights / algp_get_target_variance, and through
them algp_scores, algp_greedy and algp_score_paths_vr, against a brute force of the weighted definition.

Definition (include/algp_hip.h): a weight omega_q >= 0 per pool site; the targets T stay the candidates without a train row;
    u_c = sum_{j in T} omega_j var(j | A) - sum_{j in T} omega_j var(j | A with c static-sampled).
`wvr_reference` is that sentence in fp64 NumPy, one refit per candidate on C = kernel matrix + sigma_n^2 I, with the sum
formed PER TARGET, sum_j omega_j (var_before_j - var_after_j): the difference of two weighted sums loses 4.6e-10 (relative)
on (257, 129, 6) RBF, the per-target form 3.2e-11 against the closed form.

Problems, generator, shapes, kernels, dtypes, pools and bars are those of tests/test_variance_reduction.py (fp64 1e-9, fp32
1e-3, relative).  Three weight vectors per problem from RandomState(7 + n): `rand` uniform in [0.25, 4]; `mask` 1 with
probability 0.67 else 0; `roi` 1 where the first coordinate is below 4, else 0.  `rand` and `mask` are compared per finite
entry relative to the reference's own value.  Under `roi` candidates far from the region have utilities down to 1e-8 of the
largest, where the brute force's own per-entry error reaches 6.4e-7: `roi` is compared relative to the round's largest finite
utility (the reference alone is within 8e-14 there), and the picks must be the reference's.

Paths: the problems and path lists of tests/test_paths_vr.py ((400, 129, 6) restricted to lengths 65, 129, 256: the LDS
kernel, one block, two blocks), against the closed form of tests/test_paths_vr_host.py restated with Phi = E Omega E^T.
On the CPU that restatement agrees with one refit per path (the per-target form, `weighted_refits`) to 9.5e-11 relative
over every case used here (utilities down to 4e-5), ten times inside the fp64 bar.

Measured on an MI355X over all cases of this file (no bar was widened): scores and greedy rounds, per entry, fp64 at most
8.1e-11, fp32 1.9e-4; under `roi`, relative to the round's largest utility, fp64 1.4e-13, fp32 2.2e-5; ALGP_VR_RANK1=0
against the default 3.3e-14 / 2.1e-5; a pick's utility against the drop of the objective 3.0e-14 / 9.9e-6; weights changed
in flight against a fresh context 3.4e-14 / 1.7e-5; all-ones weights against none: the same bits; paths fp64 5.3e-13, fp32
1.5e-4; max_union = 256 against one group: the same bits.
"""
import copy
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import test_paths_vr_host as H                       # noqa: E402
import test_variance_reduction as V                  # noqa: E402
from algp_amd import _hip                            # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

SS, SM, CRIT, K = V.SS, V.SM, V.CRIT, V.K
TOL = V.TOL
WEIGHTS = ['rand', 'mask', 'roi']
PATH_LENGTHS = {H.SHAPES[2]: (65, 129, 256)}         # one length per route of the largest problem


def weights(X, n, which):
    """The three weight vectors of a problem with n sites at coordinates X, drawn in this order from RandomState(7 + n)."""
    rng = np.random.RandomState(7 + n)
    rand = rng.uniform(0.25, 4.0, size=n)
    mask = (rng.uniform(size=n) < 0.67).astype(np.float64)
    roi = (X[:, 0] < 4.0).astype(np.float64)
    return {'rand': rand, 'mask': mask, 'roi': roi, 'none': None, 'ones': np.ones(n)}[which]


def wvr_reference(C, train, noise, cand, alive, w, ss, sm, k, forced=None):
    """(picks, utilities (k, M)) of k greedy rounds by brute force, as vr_reference of tests/test_variance_reduction.py with
    target j counted w[j] times and the sum formed per target."""
    train, noise, cand = [int(a) for a in train], [float(v) for v in noise], [int(c) for c in cand]
    T = [c for c in cand if c not in set(train)]     # fixed for all rounds
    wT = np.ones(len(T)) if w is None else np.asarray(w, np.float64)[T]

    def explained(tr, nz):                           # per target: prior variance minus posterior variance
        S = C[np.ix_(tr, tr)] + np.diag(nz)
        B = C[np.ix_(tr, T)]
        return np.sum(B * np.linalg.solve(S, B), axis=0)

    done, U, picks = set(), [], []
    for r in range(k):
        base = explained(train, noise)
        pos = {s: i for i, s in enumerate(train)}
        u = np.full(len(cand), -np.inf)
        for ci, c in enumerate(cand):
            if not alive[ci] or c in done:
                continue
            if c in pos:                             # a sampled site: its noise becomes the fused one
                nz = list(noise)
                nz[pos[c]] = 1.0 / (1.0 / ss + 1.0 / sm)
                u[ci] = float(np.sum(wT * (explained(train, nz) - base)))
            else:
                u[ci] = float(np.sum(wT * (explained(train + [c], noise + [ss]) - base)))
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


_REFS = {}


def reference(p, which, what='own'):
    """Computed once per (problem, weights) and shared: 'own' = the reference's own greedy picks; 'mobile' = the same with
    its second pick replaced by a mobile-sampled site."""
    key = (p.key, which, what)
    if key not in _REFS:
        w = weights(p.X, p.n, which)
        forced = None
        if what == 'mobile':
            forced = list(reference(p, which)[0])
            forced[1] = int(p.mobile[len(p.mobile) // 2])
            assert forced[1] not in (forced[0], forced[2], forced[3])
        _REFS[key] = wvr_reference(p.C, p.A, p.noise, p.cand, p.alive, w, SS ** 2, SM ** 2, K, forced=forced)
    return _REFS[key]


def context(p, dtype, pool, which):
    c = V.context(p, dtype, pool)
    c.set_target_weights(weights(p.X, p.n, which))
    return c


def compare(got, want, tol, what, which):
    """`rand`, `mask`: every finite entry relative to its own reference value; `roi`: relative to the largest finite
    utility of the round.  -inf exactly where the reference has it."""
    if which != 'roi':
        return V.compare(got, want, tol, what)
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), what + ': -inf entries differ'
    assert np.all(np.isfinite(got[fin])), what + ': non-finite utilities'
    top = float(np.max(np.abs(want[fin])))
    err = float(np.max(np.abs(got[fin] - want[fin])) / top)
    print('%s: max error %.3e of the largest utility %.3e (bar %.1e)' % (what, err, top, tol))
    assert err < tol, (what, err, tol)
    return err


def gap(u):
    top = np.sort(u[np.isfinite(u)])[-2:]
    return (top[1] - top[0]) / top[1]


WCASES = dict(argnames='which,dtype,kernel,shape,pool',
              argvalues=[pytest.param(w, dt, k, s, pl, id='-'.join([w, di, ki, si, pl]))
                         for w in WEIGHTS for dt, di in zip(V.DTYPES, V.DIDS) for k, ki in zip(V.KERNELS, V.KIDS)
                         for s, si in zip(V.SHAPES, V.SHAPE_IDS) for pl in V.POOLS])


# ---- 1. scores before any pick ------------------------------------------------------------------------------------
@pytest.mark.parametrize(**WCASES)
def test_scores_before_any_pick(which, dtype, kernel, shape, pool):
    """The fused product's weighted epilogue alone, on every candidate; under `roi` the best candidate is the reference's."""
    p = V.problem(shape, kernel)
    _, U = reference(p, which)
    c = context(p, dtype, pool, which)
    u = c.scores(CRIT, SS, SM)
    c.close()
    fin = np.isfinite(u)
    assert np.any(fin & p.unit) and np.any(fin & ~p.unit), 'both candidate kinds must be scored'
    assert np.all(np.isneginf(u[p.static]))
    compare(u, U[0], TOL[dtype], 'scores', which)
    if which == 'roi':
        print('roi: reference gap %.3e' % gap(U[0]))
        assert int(np.argmax(u)) == int(np.argmax(U[0]))


# ---- 2. greedy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(**WCASES)
def test_greedy_utilities_and_picks(which, dtype, kernel, shape, pool):
    """k = 4: with the reference's picks forced every round's utilities equal the reference's (rounds 2..4 come from the
    weighted folds); unforced, the picks are the reference's wherever its best-to-second gap exceeds the bar."""
    p = V.problem(shape, kernel)
    picks, U = reference(p, which)
    tol = TOL[dtype]
    c = context(p, dtype, pool, which)
    got_p, got_u = c.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)
    assert [int(v) for v in got_p] == picks
    for r in range(K):
        compare(got_u[r], U[r], tol, 'round %d' % r, which)
        if which == 'roi':
            assert int(np.argmax(got_u[r])) == int(np.argmax(U[r])), 'round %d: the pick is not the reference\'s' % r
    c.solve_candidates(alive=p.alive)                # a new solve drops the picks and the sums, not the weights
    free_p = c.greedy(CRIT, SS, SM, K)
    c.close()
    for r in range(K):
        g = gap(U[r])
        print('round %d: reference gap %.3e, pick %d, got %d' % (r, g, picks[r], int(free_p[r])))
        if g <= 2 * tol:
            break                                    # a tie within the bar: the states may part from here on
        assert int(free_p[r]) == picks[r]


@pytest.mark.parametrize('pool', V.POOLS)
@pytest.mark.parametrize('kernel', V.KERNELS, ids=V.KIDS)
@pytest.mark.parametrize('dtype', V.DTYPES, ids=V.DIDS)
@pytest.mark.parametrize('which', WEIGHTS)
def test_greedy_with_a_mobile_site_picked(which, dtype, kernel, pool):
    """A forced pick of a mobile-sampled site (a unit row) appends a column of the other kind: its weighted fold"""
    p = V.problem(V.SHAPES[1], kernel)
    picks, U = reference(p, which, 'mobile')
    assert p.unit[picks[1]] and not p.unit[picks[0]]
    c = context(p, dtype, pool, which)
    _, got_u = c.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)
    c.close()
    for r in range(K):
        compare(got_u[r], U[r], TOL[dtype], 'round %d' % r, which)
    assert np.isneginf(got_u[2][picks[1]]) and np.isneginf(got_u[3][picks[1]])


# ---- 3. the full product at every scoring -------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', V.DTYPES, ids=V.DIDS)
def test_rank1_switch(dtype, monkeypatch):
    """ALGP_VR_RANK1=0 (read at every scoring) against the default under `rand`, the picks of the existing file's test"""
    p = V.problem(V.SHAPES[1], O.KERNEL_RBF)
    picks = [int(p.free[2]), int(p.mobile[3]), int(p.free[9]), int(p.free[11])]
    got = {}
    for name, value in (('default', None), ('full', '0')):
        if value is None:
            monkeypatch.delenv('ALGP_VR_RANK1', raising=False)
        else:
            monkeypatch.setenv('ALGP_VR_RANK1', value)
        c = context(p, dtype, 'coords', 'rand')
        got[name] = c.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)[1]
        c.close()
    assert np.array_equal(got['default'][0], got['full'][0])          # no pick yet: the same product, the same bits
    V.compare(got['default'], got['full'], TOL[dtype], 'rank-1 against full product')


# ---- 4. telescoping -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', V.SHAPES, ids=V.SHAPE_IDS)
@pytest.mark.parametrize('kernel', V.KERNELS, ids=V.KIDS)
@pytest.mark.parametrize('dtype', V.DTYPES, ids=V.DIDS)
@pytest.mark.parametrize('which', ['rand', 'none'])
def test_utility_is_the_drop_of_the_objective(which, dtype, kernel, shape):
    """Independent of the brute force: for each of 4 greedy picks, the objective before its commit minus the objective after
    equals the utility the library reported for it.  Without weights the objective is also the plain sum of
    algp_get_posterior's variances over the ordinary rows (both sums run in double over the same values: 1e-12)."""
    p = V.problem(shape, kernel)
    tol = TOL[dtype]
    c = context(p, dtype, 'coords', which)
    again = c.target_variance()
    for r in range(K):
        u = c.scores(CRIT, SS, SM)
        site = int(np.argmax(u))
        before = c.target_variance()
        assert before == again, 'the reduction must give the same bits in every run'
        if which == 'none':
            plain = float(np.sum(c.posterior()[1][p.free].astype(np.float64)))
            assert abs(before - plain) <= 1e-12 * abs(plain), (before, plain)
        c.commit_pick(site, SS, SM)
        after = c.target_variance()
        again = c.target_variance()
        err = abs((before - after) - u[site]) / abs(u[site])
        print('pick %d (site %d): u %.12e, drop %.12e, rel %.3e' % (r, site, u[site], before - after, err))
        assert err < tol, (r, site, err)
    c.close()


# ---- 5. identities ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pool', V.POOLS)
@pytest.mark.parametrize('dtype', V.DTYPES, ids=V.DIDS)
def test_all_ones_equal_no_weights(dtype, pool):
    p = V.problem(V.SHAPES[2], O.KERNEL_MATERN15)
    picks = reference(p, 'rand')[0]
    a = context(p, dtype, pool, 'none')
    b = context(p, dtype, pool, 'ones')
    ua = a.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)[1]
    ub = b.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)[1]
    a.close()
    b.close()
    V.compare(ub, ua, TOL[dtype], 'all ones against none')


@pytest.mark.parametrize('pool', V.POOLS)
@pytest.mark.parametrize('dtype', V.DTYPES, ids=V.DIDS)
def test_weights_changed_in_flight(dtype, pool):
    """Weights changed after a scoring and after two committed picks give what a fresh context with those weights and the
    same picks gives: the resident sums were dropped, the solve and the picks were kept."""
    p = V.problem(V.SHAPES[1], O.KERNEL_RBF)
    picks = reference(p, 'mask')[0]
    tol = TOL[dtype]
    fresh = context(p, dtype, pool, 'rand')
    want = fresh.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)[1]
    fresh.close()
    c = context(p, dtype, pool, 'mask')
    c.scores(CRIT, SS, SM)                           # sums resident under the other weights
    c.set_target_weights(weights(p.X, p.n, 'rand'))
    V.compare(c.scores(CRIT, SS, SM), want[0], tol, 'changed after a scoring')
    c.set_target_weights(weights(p.X, p.n, 'mask'))
    c.greedy(CRIT, SS, SM, 2, forced_picks=picks[:2])
    c.set_target_weights(weights(p.X, p.n, 'rand'))
    V.compare(c.scores(CRIT, SS, SM), want[2], tol, 'changed after two picks')
    c.commit_pick(picks[2], SS, SM)                  # and the state folds on from there
    V.compare(c.scores(CRIT, SS, SM), want[3], tol, 'a fold after the change')
    c.close()


@pytest.mark.parametrize('pool', V.POOLS)
@pytest.mark.parametrize('dtype', V.DTYPES, ids=V.DIDS)
def test_null_restores_the_unweighted_bits(dtype, pool):
    p = V.problem(V.SHAPES[1], O.KERNEL_MATERN15)
    picks = reference(p, 'rand')[0]
    never = V.context(p, dtype, pool)
    want = never.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)[1]
    never.close()
    c = context(p, dtype, pool, 'rand')
    c.scores(CRIT, SS, SM)
    c.set_target_weights(None)
    got = c.greedy(CRIT, SS, SM, K, forced_picks=picks, want_utilities=True)[1]
    c.close()
    assert np.array_equal(got, want)


# ---- 6. paths -----------------------------------------------------------------------------------------------------
_PATHS = {}


def path_reference(shape, kernel, which):
    """(problem, sites, names, utilities): the closed form of tests/test_paths_vr_host.py with Phi = E Omega E^T"""
    key = (shape, kernel, which)
    if key not in _PATHS:
        p = H.problem(shape, kernel)
        if shape in PATH_LENGTHS:
            p = copy.copy(p)
            p.lengths = PATH_LENGTHS[shape]
        sites, names = H.make_paths(p)
        w = weights(p.X, p.n, which)
        _PATHS[key] = (p, sites, names, weighted_closed_form(p, sites, w), w)
    return _PATHS[key]


def weighted_closed_form(p, sites, w, sm=SM ** 2):
    paths = [H.distinct(r) for r in sites]
    L = np.linalg.cholesky(p.cov(p.A, p.A) + np.diag(p.noise))
    Vf = np.linalg.solve(L, p.cov(p.A, p.free))
    U = sorted(set(j for pth in paths for j in pth))
    pos = {s: i for i, s in enumerate(U)}
    R = np.linalg.solve(L, p.cov(p.A, U))
    Gam = p.cov(U, U) - R.T @ R
    E = p.cov(U, p.free) - R.T @ Vf
    Phi = (E * w[p.free][None, :]) @ E.T
    out = np.zeros(len(paths))
    for i, pth in enumerate(paths):
        if pth:
            ix = np.ix_([pos[s] for s in pth], [pos[s] for s in pth])
            out[i] = np.trace(np.linalg.solve(Gam[ix] + sm * np.eye(len(pth)), Phi[ix]))
    return out


def weighted_refits(p, sites, w, sm=SM ** 2):
    """one refit per path, the weighted sum formed per target (the CPU check of the module docstring; no test runs it)"""
    T = p.free
    wT = w[T]

    def explained(train, nz):
        S = p.cov(train, train) + np.diag(nz)
        B = p.cov(train, T)
        return np.sum(B * np.linalg.solve(S, B), axis=0)

    train0, noise0 = [int(a) for a in p.A], [float(v) for v in p.noise]
    where = {s: i for i, s in enumerate(train0)}
    base = explained(train0, noise0)
    out = np.zeros(len(sites))
    for i, row in enumerate(sites):
        train, nz = list(train0), list(noise0)
        for s in H.distinct(row):
            if s in where:
                nz[where[s]] = nz[where[s]] * sm / (nz[where[s]] + sm)
            else:
                train.append(s)
                nz.append(sm)
        if len(train) > len(train0) or nz != noise0:
            out[i] = float(np.sum(wT * (explained(train, nz) - base)))
    return out


def path_context(p, dtype, pool, w):
    import test_paths_vr as PV
    c = PV.context(p, dtype, pool)
    c.set_target_weights(w)
    return c


def path_compare(got, want, names, tol, what):
    import test_paths_vr as PV
    return PV.compare(got, want, names, tol, what)


@pytest.mark.parametrize('pool', V.POOLS)
@pytest.mark.parametrize('shape', H.SHAPES, ids=H.SHAPE_IDS)
@pytest.mark.parametrize('kernel', H.KERNELS, ids=H.KIDS)
@pytest.mark.parametrize('dtype', V.DTYPES, ids=V.DIDS)
@pytest.mark.parametrize('which', ['rand', 'mask'])
def test_path_utilities_equal_the_weighted_closed_form(which, dtype, kernel, shape, pool):
    p, sites, names, want, w = path_reference(shape, kernel, which)
    c = path_context(p, dtype, pool, w)
    got = c.score_paths_vr(sites, SM)
    again = c.score_paths_vr(sites, SM)
    c.close()
    path_compare(got, want, names, TOL[dtype], 'utilities')
    assert np.array_equal(got, again), 'two identical calls must return identical bits'


@pytest.mark.parametrize('kernel', H.KERNELS, ids=H.KIDS)
def test_path_grouping_changes_rounding_only(kernel):
    """max_union = 256 cuts the paths of the largest problem into several groups"""
    p, sites, names, want, w = path_reference(H.SHAPES[2], kernel, 'rand')
    assert len(set(int(v) for v in sites.ravel() if v >= 0)) > 256
    c = path_context(p, np.float64, 'coords', w)
    one = c.score_paths_vr(sites, SM)
    cut = c.score_paths_vr(sites, SM, max_union=256)
    c.close()
    path_compare(cut, want, names, TOL[np.float64], 'grouped')
    nz = want != 0.0
    err = float(np.max(np.abs(cut[nz] - one[nz]) / np.abs(one[nz])))
    print('grouped against one group: %.3e' % err)
    assert err < TOL[np.float64] and np.array_equal(cut[~nz], one[~nz])


# ---- 7. refusals and lifetime -------------------------------------------------------------------------------------
def _raw_set(c, w, n=None):
    w = np.ascontiguousarray(w, dtype=np.float64)
    return c.lib.algp_set_target_weights(c.h, w.ctypes.data_as(_hip._dblp), len(w) if n is None else n)


def test_refused_weights_leave_the_state_untouched():
    p = V.problem(V.SHAPES[0], O.KERNEL_RBF)
    w = weights(p.X, p.n, 'rand')
    c = context(p, np.float64, 'coords', 'rand')
    before = c.scores(CRIT, SS, SM)
    assert _raw_set(c, w[:-1]) == _hip.ERR_BAD_ARG                    # wrong length
    assert _raw_set(c, np.r_[w, 1.0]) == _hip.ERR_BAD_ARG
    bad = w.copy()
    bad[17] = -0.5
    assert _raw_set(c, bad) == _hip.ERR_BAD_ARG
    assert '17' in c.lib.algp_last_error(c.h).decode()
    bad[17] = np.nan
    assert _raw_set(c, bad) == _hip.ERR_BAD_ARG
    assert '17' in c.lib.algp_last_error(c.h).decode()
    bad[17] = np.inf
    assert _raw_set(c, bad) == _hip.ERR_BAD_ARG
    with pytest.raises(ValueError):
        c.set_target_weights(w[:5])
    assert np.array_equal(c.scores(CRIT, SS, SM), before)             # the weights and the sums are what they were
    picks = reference(p, 'rand')[0]
    c.greedy(CRIT, SS, SM, 2, forced_picks=picks[:2])
    folded = c.scores(CRIT, SS, SM)
    assert _raw_set(c, bad) == _hip.ERR_BAD_ARG
    assert np.array_equal(c.scores(CRIT, SS, SM), folded)
    c.close()


@pytest.mark.parametrize('pool', V.POOLS)
def test_a_new_pool_drops_the_weights(pool):
    p = V.problem(V.SHAPES[0], O.KERNEL_MATERN15)
    never = V.context(p, np.float64, pool)
    want = never.scores(CRIT, SS, SM)
    never.close()
    c = context(p, np.float64, pool, 'rand')
    assert not np.array_equal(c.scores(CRIT, SS, SM), want)
    if pool == 'cov':
        c.set_pool_cov(p.C)
    else:
        c.set_pool(p.X)
    c.set_train(p.A, np.zeros(p.N), p.noise)
    c.factorize()
    c.set_candidates(p.cand, prior_includes_noise=True)
    c.solve_candidates(alive=p.alive)
    assert np.array_equal(c.scores(CRIT, SS, SM), want)
    c.close()


def test_states_the_calls_need():
    p = V.problem(V.SHAPES[0], O.KERNEL_RBF)
    c = _hip.Context(np.float64)
    c.set_hypers(p.hyp.log_lengthscale, p.hyp.log_outputscale, p.hyp.log_noise, p.hyp.kernel)
    assert _raw_set(c, np.ones(p.n)) == _hip.ERR_STATE                # no pool
    assert c.lib.algp_set_target_weights(c.h, None, 0) == _hip.ERR_STATE
    c.set_pool(p.X)
    assert _raw_set(c, np.ones(p.n)) == _hip.OK                       # a pool is enough: no train set, no solve
    v = _hip.C.c_double()
    assert c.lib.algp_get_target_variance(c.h, _hip.C.byref(v)) == _hip.ERR_STATE
    c.set_train(p.A, np.zeros(p.N), p.noise)
    c.factorize()
    assert c.lib.algp_get_target_variance(c.h, _hip.C.byref(v)) == _hip.ERR_STATE
    c.set_candidates(p.cand, prior_includes_noise=True)
    c.solve_candidates(alive=p.alive)
    assert c.lib.algp_get_target_variance(c.h, _hip.C.byref(v)) == _hip.OK and v.value > 0
    assert c.lib.algp_get_target_variance(c.h, None) == _hip.ERR_BAD_ARG
    # the criterion's two refusals
    c.set_candidates(p.free, prior_includes_noise=True, extra_var=np.full(len(p.free), 0.01))
    c.solve_candidates()
    assert c.lib.algp_get_target_variance(c.h, _hip.C.byref(v)) == _hip.ERR_STATE
    twice = np.r_[p.free[:10], p.free[3]]
    c.set_candidates(twice, prior_includes_noise=True)
    c.solve_candidates()
    assert c.lib.algp_get_target_variance(c.h, _hip.C.byref(v)) == _hip.ERR_STATE
    c.close()


def test_all_zero_weights_and_weights_off_the_targets():
    p = V.problem(V.SHAPES[0], O.KERNEL_RBF)
    plain = V.context(p, np.float64, 'coords')
    want = plain.scores(CRIT, SS, SM)
    plain.close()
    c = V.context(p, np.float64, 'coords')
    c.set_target_weights(np.zeros(p.n))
    u = c.scores(CRIT, SS, SM)
    assert np.array_equal(np.isneginf(u), np.isneginf(want)) and np.all(u[np.isfinite(u)] == 0.0)
    assert c.target_variance() == 0.0
    w = np.ones(p.n)
    w[p.A] = 37.0                                    # unit rows are no targets: their weights are ignored
    c.set_target_weights(w)
    assert np.array_equal(c.scores(CRIT, SS, SM), want)
    c.close()


@pytest.mark.parametrize('dtype', V.DTYPES, ids=V.DIDS)
def test_the_entropy_criterion_ignores_weights(dtype):
    p = V.problem(V.SHAPES[1], O.KERNEL_RBF)
    plain = V.context(p, dtype, 'coords')
    want = plain.greedy(_hip.CRIT_ENTROPY, SS, SM, K, want_utilities=True)
    plain.close()
    c = context(p, dtype, 'coords', 'rand')
    got = c.greedy(_hip.CRIT_ENTROPY, SS, SM, K, want_utilities=True)
    c.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 8. the Agent -------------------------------------------------------------------------------------------------
def _field_agent():
    from test_variance_reduction_host import _field_agent as make
    return make(True)


def _agent_reference(ag, w, k):
    static, mobile = ag._masks()
    n = ag.env.num_samples
    A = np.where(static | mobile)[0]
    noise = ag._fused_var(static[A], mobile[A])
    picks, U = wvr_reference(np.asarray(ag.cov_matrix, np.float64), A, noise, np.arange(n), ~static, w, ag.static_std ** 2,
                             ag.mobile_std ** 2, k)
    for u in U:                                      # the comparison below means something only without near-ties
        assert gap(u) > 1e-7
    return picks


def _agent_path_reference(ag, paths, static_indices, w):
    """one refit per path from agent.cov_matrix, the weighted sum formed per target (as _agent_brute_force of
    tests/test_paths_vr.py)"""
    C = np.asarray(ag.cov_matrix, np.float64)
    static, mobile = ag._masks()
    static = static.copy()
    static[static_indices] = True
    T = np.where(~(static | mobile))[0]

    def explained(st, mo):
        tr = np.where(st | mo)[0]
        S = C[np.ix_(tr, tr)] + np.diag(ag._fused_var(st[tr], mo[tr]))
        B = C[np.ix_(tr, T)]
        return np.sum(B * np.linalg.solve(S, B), axis=0)

    base = explained(static, mobile)
    out = []
    for path in paths:
        mo = mobile.copy()
        mo[[j for j in path if j != -1]] = True
        out.append(float(np.sum(w[T] * (explained(static, mo) - base))))
    return np.array(out)


def test_agent_plans_with_target_weights():
    ag = _field_agent()
    ag.run_greedy_ipp(num_runs=2, criterion='variance_reduction', disp=False)
    n = ag.env.num_samples
    roi = weights(ag.env.X, n, 'roi')
    assert 0 < roi.sum() < n
    plain = _agent_reference(ag, None, 3)
    want = _agent_reference(ag, roi, 3)
    assert want != plain, 'the region must change the picks, or the test shows nothing'
    assert ag.greedy(3) == plain
    ag.set_target_weights(roi)
    assert ag.greedy(3) == want
    ag.incremental = False                           # predict() then goes through the agent's own context
    generation = ag.gp.ctx.pool_generation
    ag.predict()                                     # loads another pool into it: the library drops the weights
    assert ag.gp.ctx.pool_generation > generation
    assert ag.greedy(3) == want                      # and the agent pushes them again with its own pool
    # the objective: the weighted sum of the posterior variances of every unsampled site
    static, mobile = ag._masks()
    A = np.where(static | mobile)[0]
    T = np.where(~(static | mobile))[0]
    C = np.asarray(ag.cov_matrix, np.float64)
    B = C[np.ix_(A, T)]
    var = np.diag(C)[T] - np.sum(B * np.linalg.solve(C[np.ix_(A, A)] + np.diag(ag._fused_var(static[A], mobile[A])), B), axis=0)
    tol = TOL[np.float64] if ag.gp.ctx.dtype == np.float64 else TOL[np.float32]
    got = ag.target_variance()
    assert abs(got - float(np.sum(roi[T] * var))) < tol * float(np.sum(roi[T] * var))
    # paths rank as the weighted reference ranks them
    rng = np.random.RandomState(3)
    free = np.where(~(static | mobile))[0]
    st = np.where(static & ~mobile)[0]
    waypoint = [int(free[0])]
    paths = [[int(v) for v in rng.choice(free[1:], 12, replace=False)] + [int(st[0]), -1],
             [int(v) for v in rng.choice(free[1:], 30, replace=False)] + [int(st[1])],
             [int(v) for v in rng.choice(free[1:], 7, replace=False)] * 2,
             [int(v) for v in rng.choice(free[1:], 70, replace=False)] + waypoint]
    got = ag.path_variance_reduction(paths, waypoint)
    ref = _agent_path_reference(ag, paths, waypoint, roi)
    for g, r in zip(got, ref):
        print('agent path: got %.10e want %.10e rel %.2e' % (g, r, abs(g - r) / r))
    assert np.all(np.abs(got - ref) < tol * np.abs(ref))
    assert list(np.argsort(got)) == list(np.argsort(ref))
    ag.set_target_weights(None)
    assert ag.greedy(3) == plain
    with pytest.raises(ValueError):
        ag.set_target_weights(np.ones(n - 1))
    with pytest.raises(ValueError):
        ag.set_target_weights(-np.ones(n))


def test_a_sharded_agent_refuses():
    ag = _field_agent()
    ag._comm = types.SimpleNamespace(world_size=2, rank=0)
    with pytest.raises(NotImplementedError, match='not sharded'):
        ag.set_target_weights(np.ones(ag.env.num_samples))
    with pytest.raises(NotImplementedError, match='not sharded'):
        ag.target_variance()
