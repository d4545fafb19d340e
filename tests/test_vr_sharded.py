"""The variance-reduction criterion scored over the ranks of a communicator (algp_comm_set_vr_exchange): every rank holds a
shard of the candidates, the targets are the ordinary rows of EVERY shard, and a rank's utilities -- the collective
algp_scores, algp_greedy_sharded -- count all of them.

Ranks are threads of this process, one context each, joined by a host all-gather (algp_comm_init_host), as in
tests/test_mi_sharded.py; the barrier gives up after 120 s, so a broken protocol fails instead of waiting.  Problems, shapes,
reference and bars are those of tests/test_variance_reduction.py: (n, N, D) = (100, 40, 2), (300, 130, 2), (257, 129, 6);
`vr_reference`, the fp64 brute force of the definition over ALL candidates (not the one-GPU library); `compare`, every finite
entry relative to the reference's own value, fp64 1e-9 and fp32 1e-3, -inf exactly where the reference has it.  The weighted
scores are compared with the brute force of tests/test_target_weights.py (the sum formed per target) evaluated in long double,
`wvr_reference_ld` below, which also says why.

(world, rows per round, partition): (2, 128, strided) gives 150 + 150 or 129 + 128 rows, two rounds, the second ragged or,
for one rank, padding only; (3, 128, contiguous); (2, -1, strided) one round of the default size; (4, 128, by hand) with
rank 2 holding nothing.  Every shard holds unit rows, switched-off rows and ordinary rows.

Largest errors measured on an MI355X over all cases of this file, per entry relative to the brute force (no bar was widened):
scores before any pick: fp64 3.6e-10 (n = 100, RBF: a utility of 6e-5, where the brute force's own difference of two sums
of 60 variances carries 1e-10, as on one GPU; every other fp64 case below 1.2e-11), fp32 6.0e-5; forced picks, all rounds and
the build with two picks committed: fp64 1.2e-11, fp32 5.1e-5; winners of greedy_sharded: fp64 1.8e-13, fp32 4.1e-7;
weighted scores against the long-double brute force: fp64 4.2e-14, fp32 2.2e-5; weighted scores across two rounds, relative
to the largest utility: fp64 2.4e-14, fp32 7.4e-6; a pick's utility against the drop of the objective summed over the ranks:
fp64 1.3e-13, fp32 3.4e-5; ALGP_VR_RANK1=0 against the default: 1.6e-15.
"""
import json
import os
import subprocess
import sys
import threading
import traceback

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import test_variance_reduction as V                  # noqa: E402
from algp_amd import _hip                            # noqa: E402
from algp_amd.sharded import LocalComm, ShardedGreedy, partition   # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

SS, SM, CRIT, K, TOL = V.SS, V.SM, V.CRIT, V.K, V.TOL
F64, F32 = np.float64, np.float32
RBF, MAT = O.KERNEL_RBF, O.KERNEL_MATERN15
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- the world
class _Gather(object):
    """the all-gather of `world` rank threads of this process (a barrier with a time limit: a broken protocol fails)"""

    def __init__(self, world):
        self.bar = threading.Barrier(world, timeout=120)
        self.slots = [None] * world

    def fn(self, rank):
        def gather(send):
            self.slots[rank] = bytes(send)
            self.bar.wait()
            out = b''.join(self.slots)
            self.bar.wait()
            return out
        return gather


def run_world(world, body):
    """body(rank, gather) on `world` threads; their results in rank order"""
    g = _Gather(world)
    res, errs = [None] * world, []

    def tgt(r):
        try:
            res[r] = body(r, g.fn(r))
        except BaseException:
            errs.append('rank %d:\n%s' % (r, traceback.format_exc()))
            g.bar.abort()
    ths = [threading.Thread(target=tgt, args=(r,)) for r in range(world)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, '\n'.join(errs)
    return res


def shards(n, world, how):
    """the candidates (pool sites 0 .. n-1) dealt over the ranks: ascending lists, disjoint, their union everything"""
    idx = np.arange(n)
    if how == 'strided':
        return [idx[r::world] for r in range(world)]
    if how == 'contiguous':
        return [idx[lo:hi] for lo, hi in partition(n, world)]
    assert how == 'hand' and world == 4                  # rank 2 holds nothing
    return [idx[idx % 3 == 0], idx[idx % 3 == 1], idx[:0], idx[idx % 3 == 2]]


WORLDS = {'w2-b128-strided': (2, 128, 'strided'), 'w3-b128-contiguous': (3, 128, 'contiguous'),
          'w2-default-strided': (2, -1, 'strided'), 'w4-b128-one-empty': (4, 128, 'hand')}


def rank_context(p, dtype, pool, mine, r, world, gather, rows, weights=None, prior_includes_noise=True):
    """rank r's context: the problem's pool, train set and factor (replicated), its shard solved, the communicator and the
    criterion's layout attached"""
    c = V.context(p, dtype, pool, cand=mine, alive=p.alive[mine], prior_includes_noise=prior_includes_noise)
    c.comm_init_host(world, r, gather)
    if weights is not None:
        c.set_target_weights(weights)
    if rows is not None:
        c.comm_set_vr_exchange(rows)
    return c


def pool_order(parts, per_rank, n):
    """the ranks' vectors (one entry per local candidate) mapped back to pool order"""
    out = np.full(n, np.nan)
    for mine, v in zip(parts, per_rank):
        out[mine] = v
    assert not np.any(np.isnan(out))
    return out


def sharded(p, dtype, pool, wname, body, weights=None):
    """body(c, rank, mine) on every rank of the named world; (parts, results in rank order)"""
    world, rows, how = WORLDS[wname]
    parts = shards(p.n, world, how)

    def rank_body(r, gather):
        c = rank_context(p, dtype, pool, parts[r], r, world, gather, rows, weights)
        try:
            return body(c, r, parts[r])
        finally:
            c.close()
    return parts, run_world(world, rank_body)


def rc_scores(c):
    out = np.empty(max(c.M, 1))
    return c.lib.algp_scores(c.h, CRIT, SS, SM, _hip._ptr(out), 0)


# ---------------------------------------------------------------------------------------------- 1. scores before any pick
def _score_cases():
    cases = []

    def add(dt, kernel, pool, si, wname):
        cases.append(pytest.param(dt, kernel, pool, V.SHAPES[si], wname,
                                  id='-'.join(['f64' if dt is F64 else 'f32', 'rbf' if kernel == RBF else 'matern', pool,
                                               V.SHAPE_IDS[si], wname])))
    for si in range(3):                                  # fp64, coordinates: both kernels in two worlds, the other two once
        for kernel in (RBF, MAT):
            add(F64, kernel, 'coords', si, 'w2-b128-strided')
            add(F64, kernel, 'coords', si, 'w3-b128-contiguous')
        add(F64, (RBF, MAT)[si % 2], 'coords', si, 'w2-default-strided')
        add(F64, (MAT, RBF)[si % 2], 'coords', si, 'w4-b128-one-empty')
    for si, wname in enumerate(['w2-b128-strided', 'w4-b128-one-empty', 'w3-b128-contiguous']):   # fp64, explicit covariance
        add(F64, (RBF, MAT)[si % 2], 'cov', si, wname)
    for si, wname in enumerate(['w2-b128-strided', 'w4-b128-one-empty', 'w2-b128-strided']):      # fp32
        add(F32, (MAT, RBF)[si % 2], 'coords', si, wname)
    add(F32, RBF, 'coords', 1, 'w3-b128-contiguous')
    add(F32, MAT, 'cov', 1, 'w2-b128-strided')
    add(F32, RBF, 'cov', 2, 'w2-default-strided')
    return cases


@gpu
@pytest.mark.parametrize('dtype,kernel,pool,shape,wname', _score_cases())
def test_scores_before_any_pick(dtype, kernel, pool, shape, wname):
    """Every rank calls the collective scores; the concatenation in pool order equals the brute force's round 0."""
    p = V.problem(shape, kernel)
    _, U = V.reference(p, 'own')
    parts, got = sharded(p, dtype, pool, wname, lambda c, r, mine: c.scores(CRIT, SS, SM))
    u = pool_order(parts, got, p.n)
    for mine in parts:
        if len(mine):
            fin = np.isfinite(u[mine])
            assert np.any(fin & p.unit[mine]) and np.any(fin & ~p.unit[mine]) and np.any(~fin), 'every shard holds every kind of row'
    V.compare(u, U[0], TOL[dtype], 'scores over ranks')


# ---------------------------------------------------------------------------------------------- 2. forced picks
@gpu
@pytest.mark.parametrize('what,wname,dtype,pool,si,kernel', [
    ('own', 'w2-b128-strided', F64, 'coords', 1, RBF), ('mobile', 'w3-b128-contiguous', F64, 'cov', 1, RBF),
    ('mobile', 'w2-b128-strided', F64, 'coords', 2, MAT), ('own', 'w3-b128-contiguous', F32, 'coords', 2, MAT),
    ('mobile', 'w2-b128-strided', F32, 'cov', 1, MAT), ('own', 'w2-default-strided', F64, 'cov', 0, RBF)],
    ids=['own-w2-f64-coords', 'mobile-w3-f64-cov', 'mobile-w2-f64-coords-D6', 'own-w3-f32-coords-D6', 'mobile-w2-f32-cov',
         'own-w2-f64-cov-n100'])
def test_forced_picks_four_rounds(what, wname, dtype, pool, si, kernel):
    """Round r: the reference's picks 0 .. r-1 committed on every rank (commit_pick), then the collective scores: the build at
    round 0, one fold per round after it.  Then, after a fresh solve, two picks committed BEFORE the first scoring: the build
    with the picks' block of columns."""
    p = V.problem(V.SHAPES[si], kernel)
    picks, U = V.reference(p, what)
    if what == 'mobile':
        assert p.unit[picks[1]] and not p.unit[picks[0]]
    world = WORLDS[wname][0]
    owner = np.empty(p.n, int)
    for r, mine in enumerate(shards(p.n, world, WORLDS[wname][2])):
        owner[mine] = r
    if what == 'own' and world == 2:
        assert len(set(owner[picks])) > 1, 'the picks must live on different ranks'

    def body(c, r, mine):
        out = []
        for rnd in range(K):
            if rnd:
                c.commit_pick(picks[rnd - 1], SS, SM)
            out.append(c.scores(CRIT, SS, SM))
        c.solve_candidates(alive=p.alive[mine])          # drops the picks and the state
        c.commit_pick(picks[0], SS, SM)
        c.commit_pick(picks[1], SS, SM)
        out.append(c.scores(CRIT, SS, SM))
        return out
    parts, got = sharded(p, dtype, pool, wname, body)
    for rnd in range(K):
        V.compare(pool_order(parts, [g[rnd] for g in got], p.n), U[rnd], TOL[dtype], 'round %d' % rnd)
    V.compare(pool_order(parts, [g[K] for g in got], p.n), U[2], TOL[dtype], 'build with two picks committed')


# ---------------------------------------------------------------------------------------------- 3. greedy_sharded
def _check_free_picks(got_p, got_u, picks, U, tol, what):
    """the picks are the reference's wherever its best-to-second gap exceeds the bar; the winners' utilities within the bar"""
    for r in range(len(got_p)):
        fin = np.isfinite(U[r])
        top = np.sort(U[r][fin])[-2:]
        gap = (top[1] - top[0]) / top[1]
        print('%s round %d: reference gap %.3e, pick %d, got %d' % (what, r, gap, picks[r], got_p[r]))
        if gap <= tol:
            break                                        # a tie within the bar: the states may part from here on
        assert got_p[r] == picks[r]
        err = abs(got_u[r] - top[1]) / top[1]
        print('%s round %d: winner utility error %.3e (bar %.1e)' % (what, r, err, tol))
        assert err < tol


def _greedy_world(p, dtype, pool, wname):
    def body(c, r, mine):
        pk, ut = c.greedy_sharded(CRIT, SS, SM, K, want_utilities=True)
        return [int(v) for v in pk], [float(v) for v in ut]
    return sharded(p, dtype, pool, wname, body)[1]


@gpu
@pytest.mark.parametrize('wname,dtype,pool,si,kernel', [
    ('w2-b128-strided', F64, 'coords', 1, RBF), ('w3-b128-contiguous', F64, 'cov', 2, MAT),
    ('w4-b128-one-empty', F32, 'coords', 2, RBF), ('w2-default-strided', F32, 'cov', 0, MAT)],
    ids=['w2-f64-coords', 'w3-f64-cov-D6', 'w4-f32-coords-D6', 'w2-f32-cov-n100'])
def test_greedy_sharded_unforced(wname, dtype, pool, si, kernel):
    """The fp32 cases are the problems whose reference gaps all exceed the fp32 bar (at least 6.7e-3 on (257, 129, 6) RBF and
    3.0e-3 on (100, 40, 2) Matern), so that all four picks are asserted."""
    p = V.problem(V.SHAPES[si], kernel)
    picks, U = V.reference(p, 'own')
    got = _greedy_world(p, dtype, pool, wname)
    for r, (pk, ut) in enumerate(got):
        assert pk == got[0][0] and ut == got[0][1], 'rank %d differs from rank 0' % r
    if dtype is F32:
        for r in range(K):
            top = np.sort(U[r][np.isfinite(U[r])])[-2:]
            assert (top[1] - top[0]) / top[1] > TOL[dtype], 'every round of this case must be asserted'
    _check_free_picks(got[0][0], got[0][1], picks, U, TOL[dtype], wname)


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_vr_sharded as t
p = t.V.problem(t.V.SHAPES[1], t.RBF)
print(json.dumps(t._greedy_world(p, np.float64, 'coords', 'w2-b128-strided')[0]))
""" % (REPO, os.path.join(REPO, 'tests'))


@gpu
def test_greedy_sharded_with_the_product_at_every_pick():
    """ALGP_VR_RANK1=0 (a build over the ranks at every pick, the picks' block of columns included) in a process of its own:
    the picks of the default, utilities equal to its to rounding."""
    p = V.problem(V.SHAPES[1], RBF)
    default = _greedy_world(p, F64, 'coords', 'w2-b128-strided')[0]
    env = dict(os.environ, ALGP_VR_RANK1='0')
    r = subprocess.run([sys.executable, '-c', _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    pk, ut = json.loads(r.stdout.strip().splitlines()[-1])
    assert pk == default[0]
    err = float(np.max(np.abs(np.array(ut) - default[1]) / np.abs(default[1])))
    print('ALGP_VR_RANK1=0 against the default: %.3e' % err)
    assert err < 1e-12


# ---------------------------------------------------------------------------------------------- 4. target weights
def roi_weights(p):
    """a region of interest: sites with a first coordinate beyond 8 do not count, those below 4 count 2.5 times"""
    return np.where(p.X[:, 0] >= 8.0, 0.0, np.where(p.X[:, 0] < 4.0, 2.5, 1.0))


_LD = {}


def wvr_reference_ld(p, w):
    """Round 0 of `wvr_reference` of tests/test_target_weights.py -- one refit per candidate, the sum formed per target -- with
    the factorisations and solves in long double.  Under these weights candidates far from the region have utilities down to
    1e-5 of the largest, and there the fp64 brute force is short of the bar itself: 1.2e-9 against this one on (300, 130, 2)
    Matern at a utility of 2.3e-5 (5.9e-12 on (100, 40, 2)).  A long-double refit of 131 rows per candidate takes 7 s for 300
    candidates and 0.1 s for the 100 of the smallest shape, which is why the weighted scores are compared on that one."""
    if p.key in _LD:
        return _LD[p.key]
    LD = np.longdouble

    def explained(S, B):                                 # diag(B^T S^-1 B) by a Cholesky factorisation with the solve carried along
        n = S.shape[0]
        L, Y = S.copy(), B.copy()
        for k in range(n):
            L[k, k] = np.sqrt(L[k, k])
            L[k + 1:, k] /= L[k, k]
            Y[k] /= L[k, k]
            L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
            Y[k + 1:] -= np.outer(L[k + 1:, k], Y[k])
        return np.sum(Y * Y, axis=0)
    C = p.C.astype(LD)
    train, noise = [int(a) for a in p.A], [LD(v) for v in p.noise]
    T = [int(c) for c in p.cand if int(c) not in set(train)]
    wT = np.asarray(w, LD)[T]
    ss, sm = LD(SS) ** 2, LD(SM) ** 2

    def ex(tr, nz):
        return explained(C[np.ix_(tr, tr)] + np.diag(np.asarray(nz, LD)), C[np.ix_(tr, T)])
    base = ex(train, noise)
    pos = {s: i for i, s in enumerate(train)}
    u = np.full(p.n, -np.inf)
    for ci, c in enumerate(int(c) for c in p.cand):
        if not p.alive[ci]:
            continue
        if c in pos:                                     # a sampled site: its noise becomes the fused one
            nz = list(noise)
            nz[pos[c]] = 1 / (1 / ss + 1 / sm)
            u[ci] = float(np.sum(wT * (ex(train, nz) - base)))
        else:
            u[ci] = float(np.sum(wT * (ex(train + [c], noise + [ss]) - base)))
    _LD[p.key] = u
    return u


@gpu
@pytest.mark.parametrize('dtype,pool', [(F64, 'coords'), (F32, 'coords'), (F64, 'cov')], ids=['f64-coords', 'f32-coords', 'f64-cov'])
def test_weighted_scores(dtype, pool):
    p = V.problem(V.SHAPES[0], MAT)
    w = roi_weights(p)
    assert np.any(w == 0) and np.any(w == 2.5) and np.any(w == 1)
    want = wvr_reference_ld(p, w)
    parts, got = sharded(p, dtype, pool, 'w2-b128-strided', lambda c, r, mine: c.scores(CRIT, SS, SM), weights=w)
    V.compare(pool_order(parts, got, p.n), want, TOL[dtype], 'weighted scores over ranks')


@gpu
@pytest.mark.parametrize('dtype,pool', [(F64, 'coords'), (F32, 'cov')], ids=['f64-coords', 'f32-cov'])
def test_weighted_scores_across_two_rounds(dtype, pool):
    """Non-unit weights across a ragged second round and three column tiles: (300, 130, 2), 150 + 150 rows at 128 per round,
    against the fp64 brute force of tests/test_target_weights.py, compared as that file compares its region-of-interest
    weights -- relative to the round's largest utility, where the fp64 brute force is exact to 8e-14 (per entry it is not:
    wvr_reference_ld above) -- at the unchanged bars."""
    import test_target_weights as TW
    p = V.problem(V.SHAPES[1], MAT)
    w = roi_weights(p)
    key = ('fp64 brute force', p.key)
    if key not in _LD:
        _LD[key] = TW.wvr_reference(p.C, p.A, p.noise, p.cand, p.alive, w, SS ** 2, SM ** 2, 1)[1][0]
    parts, got = sharded(p, dtype, pool, 'w2-b128-strided', lambda c, r, mine: c.scores(CRIT, SS, SM), weights=w)
    TW.compare(pool_order(parts, got, p.n), _LD[key], TOL[dtype], 'weighted scores, two rounds', 'roi')


@gpu
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_all_ones_weights_give_the_unweighted_bits(dtype):
    p = V.problem(V.SHAPES[2], RBF)

    def body(c, r, mine):
        out = [c.scores(CRIT, SS, SM)]
        c.commit_pick(int(p.free[3]), SS, SM)
        out.append(c.scores(CRIT, SS, SM))
        return out
    _, plain = sharded(p, dtype, 'coords', 'w2-b128-strided', body)
    _, ones = sharded(p, dtype, 'coords', 'w2-b128-strided', body, weights=np.ones(p.n))
    for a, b in zip(plain, ones):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@gpu
def test_different_weights_on_two_ranks_are_refused_by_both():
    p = V.problem(V.SHAPES[0], RBF)
    parts = shards(p.n, 2, 'strided')

    def body(r, gather):
        w = roi_weights(p)
        if r == 1:
            w = w.copy()
            w[5] += 0.5
        c = rank_context(p, F64, 'coords', parts[r], r, 2, gather, 128, weights=w)
        try:
            rc = rc_scores(c)
            c.set_target_weights(roi_weights(p))         # alike: the next call scores
            return rc, bool(np.all(np.isfinite(c.scores(CRIT, SS, SM)[p.alive[parts[r]]])))
        finally:
            c.close()
    assert run_world(2, body) == [(_hip.ERR_BAD_ARG, True)] * 2


@gpu
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_a_picks_utility_is_the_drop_of_the_objective_summed_over_ranks(dtype):
    """algp_get_target_variance stays local: this rank's share.  Summed over the ranks, before a pick minus after it, it is
    the pick's utility -- for an ordinary site and for a mobile-sampled one, with weights attached."""
    p = V.problem(V.SHAPES[1], RBF)
    w = roi_weights(p)
    sites = (int(p.free[3]), int(p.mobile[5]))

    def body(c, r, mine):
        out = []
        for site in sites:
            u = c.scores(CRIT, SS, SM)
            before = c.target_variance()
            c.commit_pick(site, SS, SM)
            out.append((u, before, c.target_variance()))
        return out
    parts, got = sharded(p, dtype, 'coords', 'w2-b128-strided', body, weights=w)
    for i, site in enumerate(sites):
        u = pool_order(parts, [g[i][0] for g in got], p.n)[site]
        drop = sum(g[i][1] for g in got) - sum(g[i][2] for g in got)
        print('site %d: u %.12e, drop %.12e, relative %.3e' % (site, u, drop, abs(drop - u) / abs(u)))
        assert abs(drop - u) < TOL[dtype] * abs(u)


# ---------------------------------------------------------------------------------------------- 5. a world of one
@gpu
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_a_world_of_one_keeps_the_one_gpu_state(dtype):
    p = V.problem(V.SHAPES[1], MAT)
    c = V.context(p, dtype, 'coords')
    want_p, want_u = c.greedy(CRIT, SS, SM, K, want_utilities=True)
    c.close()

    def body(r, gather):
        c = rank_context(p, dtype, 'coords', p.cand, 0, 1, gather, 128)
        try:
            first = c.scores(CRIT, SS, SM)
            pk, ut = c.greedy_sharded(CRIT, SS, SM, K, want_utilities=True)
            return first, pk, ut
        finally:
            c.close()
    first, pk, ut = run_world(1, body)[0]
    assert np.array_equal(first, want_u[0])
    assert [int(v) for v in pk] == [int(v) for v in want_p]
    assert np.array_equal(ut, [np.max(u[np.isfinite(u)]) for u in want_u])


# ---------------------------------------------------------------------------------------------- 6. refusals
@gpu
def test_refusals_on_both_ranks():
    p = V.problem(V.SHAPES[0], RBF)
    parts = shards(p.n, 2, 'strided')
    twice = int(parts[0][np.where(~p.unit[parts[0]])[0][2]])          # an ordinary site of rank 0 ...
    unit_twice = int(parts[0][np.where(p.unit[parts[0]] & p.alive[parts[0]])[0][1]])   # ... and a mobile-sampled one

    def body(r, gather):
        got = {}
        picks = np.zeros(1, np.int64)
        c = rank_context(p, F64, 'coords', parts[r], r, 2, gather, None)
        try:
            # the criterion without its layout, on a context that has a communicator
            got['no layout'] = c.lib.algp_greedy_sharded(c.h, CRIT, SS, SM, 1, _hip._i64(picks), None)
            # differing rows per round: compared in the agreement word
            c.comm_set_vr_exchange(128 if r == 0 else 256)
            got['rows differ'] = rc_scores(c)
            c.comm_set_vr_exchange(128)
            # what this context no longer answers alone
            got['greedy'] = c.lib.algp_greedy(c.h, CRIT, SS, SM, 1, None, _hip._i64(picks), None)
            pos, pool, val = _hip.C.c_int64(), _hip.C.c_int64(), _hip.C.c_double()
            got['best_candidate'] = c.lib.algp_best_candidate(c.h, CRIT, SS, SM, _hip.C.byref(pos), _hip.C.byref(pool), _hip.C.byref(val))
            sites = np.array([int(parts[r][0]), int(parts[r][1])], dtype=np.int64)
            out = np.empty(1)
            got['score_paths_vr'] = c.lib.algp_score_paths_vr(c.h, _hip._i64(sites), 1, 2, SM, 0, out.ctypes.data_as(_hip._dblp))
            assert np.all(np.isfinite(c.scores(_hip.CRIT_ENTROPY, SS, SM)[p.alive[parts[r]]]))   # the other criteria are untouched
            # ... listed by rank 1 too
            if r == 1:
                mine = np.sort(np.r_[parts[1], twice])
                c.set_candidates(mine, prior_includes_noise=True)
                c.solve_candidates(alive=p.alive[mine])
            got['site in two shards'] = rc_scores(c)
            if r == 1:                                   # the same for a unit row: no target, but still one site on two ranks
                mine = np.sort(np.r_[parts[1], unit_twice])
                c.set_candidates(mine, prior_includes_noise=True)
                c.solve_candidates(alive=p.alive[mine])
            got['unit row in two shards'] = rc_scores(c)
            # a rank whose candidates carry predictive semantics
            c.set_candidates(parts[r], prior_includes_noise=(r == 0))
            c.solve_candidates(alive=p.alive[parts[r]])
            got['predictive semantics'] = rc_scores(c)
            # put right, the same contexts score
            c.set_candidates(parts[r], prior_includes_noise=True)
            c.solve_candidates(alive=p.alive[parts[r]])
            return got, c.scores(CRIT, SS, SM)
        finally:
            c.close()
    res = run_world(2, body)
    want = {'no layout': _hip.ERR_BAD_ARG, 'rows differ': _hip.ERR_BAD_ARG, 'greedy': _hip.ERR_STATE, 'best_candidate': _hip.ERR_STATE,
            'score_paths_vr': _hip.ERR_STATE, 'site in two shards': _hip.ERR_STATE, 'unit row in two shards': _hip.ERR_STATE,
            'predictive semantics': _hip.ERR_STATE}
    for r in range(2):
        assert res[r][0] == want, (r, res[r][0])
    V.compare(pool_order(parts, [res[0][1], res[1][1]], p.n), V.reference(p, 'own')[1][0], 1e-9, 'after the refusals')


def test_sharded_greedy_refuses_the_criterion():
    """The torch.distributed route would score every rank against its own shard's targets: refused, on the CPU."""
    class Backend(object):
        M = 10

        def scores(self, *a, **k):
            raise AssertionError('not reached')
    sg = ShardedGreedy(Backend(), LocalComm(), np.arange(10))
    with pytest.raises(ValueError, match='algp_greedy_sharded'):
        sg.step(2, SS, SM)
    with pytest.raises(ValueError, match='algp_greedy_sharded'):
        sg.greedy(2, SS, SM, 3)


# ---------------------------------------------------------------------------------------------- 7. injected failure
@gpu
def test_a_failure_on_one_rank_is_returned_by_every_rank():
    """algp_debug_fail_at(5) on rank 1: once in the build, once in the fold of a pick; both ranks raise from the same call, the
    next call rebuilds (the second time with a pick's column in the product) and the picks end as the reference's."""
    p = V.problem(V.SHAPES[1], RBF)
    picks, U = V.reference(p, 'own')

    def body(c, r, mine):
        if r == 1:
            c.debug_fail_at(5, _hip.ERR_OOM)
        with pytest.raises(MemoryError):
            c.greedy_sharded(CRIT, SS, SM, 2)            # in the build
        pk, ut = c.greedy_sharded(CRIT, SS, SM, 1, want_utilities=True)
        pk, ut = [int(v) for v in pk], [float(v) for v in ut]
        if r == 1:
            c.debug_fail_at(5, _hip.ERR_OOM)
        with pytest.raises(MemoryError):
            c.greedy_sharded(CRIT, SS, SM, 2)            # in the fold of the pick committed above
        more = c.greedy_sharded(CRIT, SS, SM, K - 1, want_utilities=True)
        return pk + [int(v) for v in more[0]], ut + [float(v) for v in more[1]]
    _, got = sharded(p, F64, 'coords', 'w2-b128-strided', body)
    assert got[0] == got[1]
    _check_free_picks(got[0][0], got[0][1], picks, U, 1e-9, 'after two injected failures')


# ---------------------------------------------------------------------------------------------- 8. reproducibility
@gpu
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_the_same_world_twice_gives_the_same_bits(dtype):
    p = V.problem(V.SHAPES[2], MAT)
    picks, _ = V.reference(p, 'own')

    def body(c, r, mine):
        out = [c.scores(CRIT, SS, SM)]
        for q in picks[:2]:
            c.commit_pick(q, SS, SM)
        out.append(c.scores(CRIT, SS, SM))
        return out
    _, a = sharded(p, dtype, 'coords', 'w3-b128-contiguous', body)
    _, b = sharded(p, dtype, 'coords', 'w3-b128-contiguous', body)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
