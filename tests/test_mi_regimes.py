"""The mutual-information criterion (api_mi.hip: mi_sets, mi_build, mi_apply_pick, mi_scores_enqueue; vecops.hip:
rows_reduce_kernel's triangle walk, mi_rank1_kernel, mi_score_kernel; the dealt form of mi_shard.hip) on every set shape,
pick position, width, kernel form, candidate list and state it can be in, fp64 and fp32, every utility of every pick
against the fp64 oracle along the oracle's forced picks.

The comparison is tests/mi_forms.py's `compare`: the error common to all candidates (the three entropies) and the error of
each candidate about it are bounded separately, by 1e-9 / 1e-4 of |H(A)| + |H(Abar)| + |H(all)| and by 1e-9 / 1e-3 of
max(1, spread of the utilities) in fp64 / fp32.  tests/test_mi_forms_host.py shows on these same inputs that the bounds
reject a dropped fold, a wrong complement row and a fold with the wrong noise change.  This file holds no other tolerance.

No case needed a bar of its own from a float32-storage emulation: the table of such entries is empty.

Every comparison prints its figures before it asserts ('MI <case> <dtype> pick k: offset ... per-candidate ...', and the
largest of a run as 'MI-WORST').  Measured on an MI355X, largest over the picks checked, absolute (sum|H| is 250 .. 3000,
the spread 0.5 .. 3.7; the bars are then 2.5e-7 .. 3e-6 | 1e-9 x spread in fp64 and 0.025 .. 0.3 | 1e-3 x spread in fp32):

    case                                   fp64 offset, per-cand.   fp32 offset, per-cand.
    one_unsampled_n200                     5.53e-14 8.52e-14   7.37e-08 4.12e-06
    empty_train_n129                       1.91e-14 2.84e-14   5.41e-06 5.06e-06
    mb127_n260                             5.68e-14 8.53e-14   8.87e-06 6.24e-06
    mb128_n260                             1.28e-13 8.53e-14   1.21e-05 3.92e-06
    mb129_n260                             7.46e-14 8.88e-14   9.31e-06 6.78e-06
    pool_n128                              1.42e-14 3.55e-14   1.13e-05 3.67e-06
    pool_n129                              1.42e-14 3.55e-14   2.62e-06 3.01e-06
    pool_n512                              1.42e-13 1.56e-13   2.13e-05 5.93e-06
    pool_n513                              1.49e-13 1.49e-13   3.93e-06 4.57e-06
    pool_n640                              1.42e-13 1.71e-13   4.71e-06 8.94e-06
    pool_n1153                             3.41e-13 3.98e-13   2.30e-05 8.19e-06
    edges_n300                             5.68e-14 1.07e-13   6.45e-06 3.00e-06
    edges_n650                             1.99e-13 1.71e-13   2.10e-05 5.76e-06
    D1_rbf_n513                            8.28e-13 3.30e-13   2.57e-04 1.34e-04
    D3_matern05_n513                       5.68e-14 1.63e-13   4.53e-06 7.75e-07
    D5_matern15_n513                       3.55e-14 1.24e-13   1.44e-05 1.80e-06
    D8_matern25_n513                       8.88e-14 1.17e-13   6.35e-06 6.09e-07
    D8_rbf_n513                            8.88e-14 1.39e-13   3.64e-06 1.37e-06
    D1_matern25_n513                       6.54e-13 3.98e-13   1.13e-04 1.51e-04
    D3_matern15_n513                       8.53e-14 1.17e-13   4.70e-06 1.33e-06
    explicit_cov_n513                      1.14e-13 1.35e-13   7.28e-06 3.41e-06
    all_mobile_n130 (every utility is 0.0) 7.77e-16 1.50e-14   7.77e-16 1.50e-14
    full_new_n300                          1.14e-13 8.53e-14   1.56e-05 5.55e-06
    full_new_n300 after a fresh solve      2.84e-14 6.39e-14   1.56e-05 5.13e-06
    full_mixed_n300                        2.84e-13 8.17e-14   7.64e-06 8.97e-06
    full_mixed_n300 after a fresh solve    1.42e-14 6.75e-14   2.49e-06 3.35e-06
    subset (edges_n300, every third site)  1.14e-13 6.39e-14   7.36e-06 2.91e-06
    noise levels (edges_n300)              0.00e+00 7.11e-14   6.11e-06 2.98e-06
    edges_n300 built with four picks       2.84e-14 1.07e-13   3.17e-06 5.45e-06
    edges_n650 built with four picks       1.99e-13 1.71e-13   1.87e-05 6.44e-06
    incremental, before the update         5.68e-14 1.42e-13   1.30e-06 4.57e-06
    incremental, after it                  0.00e+00 1.28e-13   3.91e-06 4.56e-06
    after the refusal (pool_n128)          1.42e-14 3.55e-14   5.54e-06 3.67e-06
    dealt, edges_n300 rank 0 | rank 1      7.11e-15 5.68e-14 | 1.42e-14 7.82e-14   1.17e-05 3.50e-06 | 1.17e-05 4.47e-06
    dealt, edges_n650 rank 0 | rank 1      0.00e+00 1.71e-13 | 1.42e-14 1.28e-13   2.70e-05 5.25e-06 | 2.70e-05 5.76e-06
"""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import mi_forms as F                                 # noqa: E402
from test_mi_sharded import run_world                # noqa: E402
from algp_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

DT = [np.float64, np.float32]
IDS = ['f64', 'f32']
MI, ENT = _hip.CRIT_MUTUAL_INFORMATION, _hip.CRIT_ENTROPY
S_STD, M_STD = F.S_STD, F.M_STD
SS, SM = S_STD ** 2, M_STD ** 2
MAX_APPEND = 128                                     # common.h
OWN_TEST = ('all_mobile_n130', 'full_new_n300', 'full_mixed_n300')
GENERIC = [k for k in F.cases() if k not in OWN_TEST]


@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in DT}
    yield c
    for v in c.values():
        v.close()


def _pool(c, p):
    c.set_hypers(p.log_ls, p.log_os, p.log_noise, _hip.KERNEL_RBF if p.explicit else p.kid)
    if p.explicit:
        c.set_pool_cov(p.C)
    else:
        c.set_pool(p.X)


def _load(c, p, cand=None, alive=None):
    """Pool, train set, factor, candidates and a fresh solve."""
    _pool(c, p)
    c.set_train(p.A, np.zeros(len(p.A)), p.var)
    c.factorize()
    c.set_candidates(p.cand if cand is None else cand, prior_includes_noise=True)
    c.solve_candidates(alive=alive)


def _check(c, what, rows, unit):
    """rows: (label, got, want, entropies) of one run.  Prints every figure, then asserts every comparison."""
    ms = [(label, F.measure(got, want, unit, H)) for label, got, want, H in rows]
    for label, m in ms:
        print('MI %s %s %s: offset %.2e of sum|H| %.1f, per-candidate %.2e (unit rows %.2e, new-site rows %.2e) of spread %.3f, '
              '%d live rows, %d mask differences' % (what, c.dtype.name, label, abs(m.off), m.hsum, m.per, m.per_unit, m.per_new,
                                                     m.spread, m.rows, m.mask))
    if ms:
        print('MI-WORST %s %s: offset %.2e (%.2e of sum|H|), per-candidate %.2e' % (
            what, c.dtype.name, max(abs(m.off) for _, m in ms), max(abs(m.off) / max(m.hsum, 1e-300) for _, m in ms),
            max(m.per for _, m in ms)))
    for label, got, want, H in rows:
        F.compare(got, want, unit, c.dtype, H, '%s %s %s' % (what, c.dtype.name, label))


def _forced_run(c, p, what, cand=None):
    """algp_greedy along the case's forced picks on a loaded context: the checked picks' utilities against the reference."""
    cand = p.cand if cand is None else cand
    forced = F.forced_picks(p)
    ut, H = F.case_reference(p)
    got, gut = c.greedy(MI, S_STD, M_STD, len(forced), forced_picks=forced, want_utilities=True)
    assert [int(q) for q in got] == forced
    check = range(len(forced)) if p.case.check is None else p.case.check
    _check(c, what, [('pick %d' % (k + 1), gut[k], ut[k][cand], H[k]) for k in check], p.mobile[cand])
    return gut


# ------------------------------------------------------------------ 1. set shapes, pools, pick positions, widths and forms
@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('key', GENERIC)
def test_every_pick_along_the_forced_sequence(ctxs, key, dt):
    """One unsampled site, an empty train set, complements of 127 / 128 / 129 sites, pools of one tile, an exact block,
    block + tile and ragged with several blocks; eight picks at the complement rows 0, 127, 128, mb - 1 and the pool sites
    0, 127, 128, n - 1 (the triangle walk starts at cb / 128 * 128 and pool_idx / 128 * 128); D = 1, 3, 5, 8 with the four
    kernel forms and an explicit pool covariance.  A second run behind a fresh solve gives the same bits."""
    c = ctxs[np.dtype(dt)]
    p = F.problem(key)
    _load(c, p)
    gut = _forced_run(c, p, key)
    c.solve_candidates()
    forced = F.forced_picks(p)
    _, gut2 = c.greedy(MI, S_STD, M_STD, len(forced), forced_picks=forced, want_utilities=True)
    assert np.array_equal(gut, gut2)


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_every_site_mobile_sampled(ctxs, dt):
    """No site outside the train set (mb = 0: mi_build skips the complement's matrix) and none static: H(A) = H(all),
    H(Abar) = 0 and the entropy gain of a site equals the change of H(all), so every utility is zero up to the offset
    bound, before and after a mobile-sampled site is committed."""
    c = ctxs[np.dtype(dt)]
    p = F.problem('all_mobile_n130')
    forced = F.forced_picks(p)
    ut, H = F.case_reference(p)
    assert len(p.Abar) == 0 and np.all(H[:, 1] == 0.0) and np.max(np.abs(ut[np.isfinite(ut)])) < 1e-10
    _load(c, p)
    s0, e0 = c.scores(MI, S_STD, M_STD), c.scores(ENT, S_STD, M_STD)
    c.commit_pick(forced[0], S_STD, M_STD)
    s1, e1 = c.scores(MI, S_STD, M_STD), c.scores(ENT, S_STD, M_STD)
    for k, (s, e) in enumerate(((s0, e0), (s1, e1))):
        live = np.isfinite(s)
        print('MI all_mobile_n130 %s state %d: max|u| %.3e, bound %.3e (entropy gains %.3f .. %.3f cancel against H(all_i))' % (
            c.dtype.name, k, np.max(np.abs(s[live])), F.B_OFF[c.dtype] * 2 * abs(H[k, 2]), e[live].min(), e[live].max()))
    _check(c, 'all_mobile_n130', [('state %d' % k, s, ut[k][p.cand], H[k]) for k, s in enumerate((s0, s1))], p.unit)
    for k, s in enumerate((s0, s1)):
        live = np.isfinite(s)
        assert np.max(np.abs(s[live])) <= F.B_OFF[c.dtype] * 2 * abs(H[k, 2])


@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('key', ['full_new_n300', 'full_mixed_n300'])
def test_full_rank1_lists(ctxs, key, dt):
    """MAX_APPEND = 128 forced picks: 128 new sites fill the complement's list and the pool's (signs at H + 3 and
    H + 3 + MAX_APPEND), 96 new and 32 mobile-sampled sites fill the pool's with both signs.  Utilities at picks 1, 2, 64,
    127 and 128; the 129th commit is refused; after a fresh solve the context scores the first state again."""
    c = ctxs[np.dtype(dt)]
    p = F.problem(key)
    forced = F.forced_picks(p)
    assert len(forced) == MAX_APPEND and p.case.check == (0, 1, 63, 126, 127)
    ut, H = F.case_reference(p)
    _load(c, p)
    _forced_run(c, p, key)
    s_end = c.scores(MI, S_STD, M_STD)
    left = p.cand[np.isfinite(s_end)]
    assert len(left) == len(p.cand) - MAX_APPEND
    with pytest.raises(ValueError, match='append capacity exhausted'):
        c.commit_pick(int(left[0]), S_STD, M_STD)
    assert np.array_equal(c.scores(MI, S_STD, M_STD), s_end)
    c.solve_candidates()
    _check(c, key + ' after a fresh solve', [('pick 1', c.scores(MI, S_STD, M_STD), ut[0][p.cand], H[0])], p.unit)


# ------------------------------------------------------------------ 2. candidate subsets and masks
def _subset_problem():
    p = F.problem('edges_n300')
    if 'subset' not in p.memo:
        sub = p.cand[::3]
        rng = np.random.RandomState(5)
        new_in = [q for q in sub if not p.mobile[q]]
        unit_in = [q for q in sub if p.mobile[q]]
        new_out = [q for q in p.cand if not p.mobile[q] and q not in sub]
        unit_out = [q for q in p.cand if p.mobile[q] and q not in sub]
        forced = [int(rng.choice(g)) for g in (new_in, new_out, unit_in, unit_out)]
        forced.append(int(rng.choice([q for q in new_in if q not in forced])))       # the state after the fourth pick is scored too
        alive = rng.uniform(size=len(sub)) < 0.7
        alive[np.isin(sub, forced)] = True
        ref = F.reference(p.C, p.static, p.mobile, S_STD, M_STD, forced)
        p.memo['subset'] = (sub, forced, alive, ref)
    return (p,) + p.memo['subset']


def _stepwise(c, sub, forced, ncommit):
    """scores before every pick of `forced`, the first `ncommit` of them committed"""
    out = []
    for k, f in enumerate(forced):
        out.append(c.scores(MI, S_STD, M_STD))
        if k < ncommit:
            c.commit_pick(f, S_STD, M_STD)
    return out


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_candidate_subset_with_picks_from_outside_it_and_masked_rows(ctxs, dt):
    """Candidates: every third site that is not static.  Picks: a new site of the list, a new site outside it
    (algp_commit_pick's remote-row route), a mobile-sampled site of the list, one outside it.  The listed rows against the
    reference; then the same with an alive mask: masked rows -inf, the others the unmasked run's bits."""
    c = ctxs[np.dtype(dt)]
    p, sub, forced, alive, (ut, H) = _subset_problem()
    _load(c, p, cand=sub)
    plain = _stepwise(c, sub, forced, 4)
    _check(c, 'subset', [('state %d' % k, s, ut[k][sub], H[k]) for k, s in enumerate(plain)], p.mobile[sub])
    _load(c, p, cand=sub, alive=alive)
    masked = _stepwise(c, sub, forced, 4)
    for s, m in zip(plain, masked):
        assert np.all(np.isneginf(m[~alive]))
        assert np.array_equal(m[alive], s[alive])


# ------------------------------------------------------------------ 3. state
@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_other_noise_levels_rebuild_the_state(ctxs, dt):
    """Scores under (0.1, 1.0), then under (0.2, 0.5) with nothing committed: the second equals a fresh context's bits, and
    going back gives the first again."""
    c = ctxs[np.dtype(dt)]
    p = F.problem('edges_n300')
    ut, H = F.case_reference(p)
    _load(c, p)
    s1 = c.scores(MI, S_STD, M_STD)
    s2 = c.scores(MI, 0.2, 0.5)
    s1b = c.scores(MI, S_STD, M_STD)
    f = _hip.Context(dt)
    try:
        _load(f, p)
        want2 = f.scores(MI, 0.2, 0.5)
    finally:
        f.close()
    _check(c, 'noise levels', [('(0.1, 1.0)', s1, ut[0][p.cand], H[0])], p.unit)
    assert not np.array_equal(s1, s2)
    assert np.array_equal(s2, want2)
    assert np.array_equal(s1b, s1)


@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('key', ['edges_n300', 'edges_n650'])
def test_entropy_picks_before_the_first_mi_scoring(ctxs, key, dt):
    """The first four tile-edge picks committed under the entropy criterion, so that mi_build meets picks (a new site at
    complement row 0, pool site 127, a new site at row 127, pool site 128); the other four folded on top one by one."""
    c = ctxs[np.dtype(dt)]
    p = F.problem(key)
    forced = F.forced_picks(p)
    ut, H = F.case_reference(p)
    _load(c, p)
    c.greedy(ENT, S_STD, M_STD, 4, forced_picks=forced[:4])
    rows = []
    for k in range(4, 8):
        rows.append(('pick %d' % (k + 1), c.scores(MI, S_STD, M_STD), ut[k][p.cand], H[k]))
        c.commit_pick(forced[k], S_STD, M_STD)
    _check(c, key + ' built with four picks', rows, p.unit)


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_train_set_extended_by_an_incremental_update(ctxs, dt):
    """A planning step: MI scores on a train set without five of its mobile-sampled sites, two new sites picked, then the
    picks and the five sites appended (factorize(incremental=True), solve_candidates(incremental=True) with the picks
    masked).  Both states against the reference; the second also against a fresh context, to the same bars."""
    c = ctxs[np.dtype(dt)]
    p = F.problem('pool_n513')
    rng = np.random.RandomState(11)
    late = rng.permutation(np.where(p.mobile & ~p.static)[0])[:5]
    mobile0 = p.mobile.copy()
    mobile0[late] = False
    picks = [int(q) for q in rng.permutation(p.Abar)[:2]]
    A0 = np.setdiff1d(p.A, late)
    var0 = F._noise(p.static, mobile0, SS, SM)[A0]
    ut0, H0 = F.reference(p.C, p.static, mobile0, S_STD, M_STD, picks)
    static1 = p.static.copy()
    static1[picks] = True
    A1 = np.r_[A0, picks, late]
    var1 = F._noise(static1, p.mobile, SS, SM)[A1]
    ut1, H1 = F.reference(p.C, static1, p.mobile, S_STD, M_STD, [int(p.Abar[~np.isin(p.Abar, picks)][0])])
    alive = ~static1[p.cand]
    _pool(c, p)
    c.set_train(A0, np.zeros(len(A0)), var0)
    c.factorize()
    c.set_candidates(p.cand, prior_includes_noise=True)
    c.solve_candidates(incremental=True)
    got, gut = c.greedy(MI, S_STD, M_STD, 2, forced_picks=picks, want_utilities=True)
    c.set_train(A1, np.zeros(len(A1)), var1)
    kept = c.factorize(incremental=True)
    assert kept == len(A0) // 128 * 128
    c.solve_candidates(incremental=True, alive=alive)
    s = c.scores(MI, S_STD, M_STD)
    f = _hip.Context(dt)
    try:
        _pool(f, p)
        f.set_train(A1, np.zeros(len(A1)), var1)
        f.factorize()
        f.set_candidates(p.cand, prior_includes_noise=True)
        f.solve_candidates(alive=alive)
        sf = f.scores(MI, S_STD, M_STD)
    finally:
        f.close()
    unit0 = mobile0[p.cand]
    _check(c, 'incremental, before', [('pick %d' % (k + 1), gut[k], ut0[k][p.cand], H0[k]) for k in range(2)], unit0)
    _check(c, 'incremental, after', [('updated', s, ut1[0][p.cand], H1[0]), ('fresh', sf, ut1[0][p.cand], H1[0]),
                                     ('updated against fresh', s, sf, H1[0])], p.unit)


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_a_train_set_with_repeats_is_refused(ctxs, dt):
    c = ctxs[np.dtype(dt)]
    p = F.problem('pool_n128')
    _pool(c, p)
    A = np.r_[p.A, p.A[:1]]
    c.set_train(A, np.zeros(len(A)), np.r_[p.var, p.var[:1]])
    c.factorize()
    c.set_candidates(p.cand, prior_includes_noise=True)
    c.solve_candidates()
    with pytest.raises(ValueError, match='the train set lists a site more than once; fuse its readings first'):
        c.scores(MI, S_STD, M_STD)
    _load(c, p)                                              # and the context goes on
    ut, H = F.case_reference(p)
    _check(c, 'after the refusal', [('pick 1', c.scores(MI, S_STD, M_STD), ut[0][p.cand], H[0])], p.unit)


# ------------------------------------------------------------------ 4. the dealt form
@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('key', ['edges_n300', 'edges_n650'])
def test_dealt_over_two_ranks_every_utility_of_every_shard(key, dt):
    """World of 2 on one card (host all-gather), the complement's inverse on rank 0 and the pool's on rank 1: after four
    algp_greedy_sharded picks every rank scores its shard from the whole diagonals it holds; each shard against the
    reference along those picks."""
    p = F.problem(key)

    def body(r, gather):
        c = _hip.Context(dt)
        try:
            _load(c, p, cand=p.cand[r::2])
            c.comm_init_host(2, r, gather)
            c.comm_set_mi_groups(1)
            picks = [int(q) for q in c.greedy_sharded(MI, S_STD, M_STD, 4)]
            return picks, c.scores(MI, S_STD, M_STD)
        finally:
            c.close()
    res = run_world(2, body)
    picks = res[0][0]
    assert res[1][0] == picks and len(set(picks)) == 4
    left = [int(q) for q in p.cand if q not in picks]
    ut, H = F.reference(p.C, p.static, p.mobile, S_STD, M_STD, picks + left[:1])
    c = type('dtype_only', (), dict(dtype=np.dtype(dt)))
    for r in range(2):
        shard = p.cand[r::2]
        _check(c, '%s rank %d' % (key, r), [('after 4 picks', res[r][1], ut[4][shard], H[4])], p.mobile[shard])
