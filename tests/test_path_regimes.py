"""algp_score_paths, algp_score_paths_mi and algp_score_paths_vr against the fp64 NumPy helpers of tests/path_forms.py, PER PATH, on
every route the three entry points can take (api_paths.hip, api_paths_vr.hip): the LDS kernels up to 64 distinct sites, the batched
2 x 2 tiled factorisations at ppad = 128 and 256, and for the variance reduction both of them inside one group and more than one
batch of long paths.  The problems, the site arrays and the route each case must take are the table path_forms.CASES;
tests/test_path_forms_host.py proves on the host that cond(S_A) and cond of every path's block stay below 1e3, that the routes
follow from the lengths, that the batching case exceeds one batch, and the margins the assertions here rely on.

Cases (each under RBF and Matern-3/2, coordinate pool and -- on the 576- and 900-site problems -- the explicit covariance pool,
fp64 and fp32; Matern-1/2 and Matern-5/2 once each through the batched routes):
  len1 .. len256         every length at a route edge, each a call of its own: 1, 2, 63, 64 | 65, 127, 128 | 129, 255, 256
  shape_*                maxlen 5; 64; 70 holding 64 distinct sites; 262 holding a 130-site path; a leading -1; a site three times;
                         an empty path in an LDS call and in a batched call (exactly 0.0, for MI every term)
  mixed_*                [7, 65], [64, 65, 3], [30, 129, 128, 1]: every path against its own bound
  rm_*                   second readings pinned: train row 0 and train row N - 1 (alone, together, among new sites, in LDS and in
                         batched calls), paths of nothing but second readings (3, 64 | 65 | 130: knew = 0 in the MI scorer), second
                         readings at packed positions 127, 128, 129 of a 200-site path
  wide_*                 N = 2100 (Npad > 2048): second readings of train rows >= 2048, three paths (3, 65 and 130 sites), entropy
                         and variance reduction
  full_1_5_40            every site sampled (MI's mb == 0 branch): paths only re-measure; the variance reduction has no target
                         there and returns zeros (sum over an empty T; include/algp_hip.h documents no refusal)
  vr_weights_40_70_200   target weights attached (a quarter of them zero)
  vr_batches             481 paths (fp64) / 961 paths (fp32), one of 129 sites: ppad = 256 and two batches (sync_count()), scored
                         again with max_union = 256
and the bits: two identical calls, a path alone and among 20 others, the context's posterior and entropy scores before and after.

Routes are asserted from sync_count() where it tells them apart: algp_score_paths synchronises once on the LDS route and once
more per batch on the batched one; algp_score_paths_mi (second call, the inverses resident) adds one per batch of its own;
algp_score_paths_vr synchronises once per batch of long paths (once per group without any) and once at the end.  The padding
(128 or 256) is taken from the table the host file proved.

Bounds, per path and never over the call:
    entropy          |got - want| <= tol max(1, |want_p|)        fp64 1e-9    fp32 2e-3
    each MI term     |got - want| <= tol max(1, |term_p|)        fp64 1e-7    fp32 3e-3     (and their sum against its own)
    VR               |got - want| <= tol |want_p|                fp64 1e-9    fp32 1e-3
These are the project's bars (tests/test_hip_greedy.py, tests/test_mi_paths.py, tests/test_paths_vr.py) on the path's own scale.
No fp32 bar had to be widened, so none carries a float32 NumPy figure.  In fp64 the argmax of every multi-path case equals the
helper's.

A path scored alone and among 20 others returns the same bits on every route (measured on the first run, then asserted).

Seeded into a scratch build, one at a time, each of these value-only faults turns the file red (nothing of them is kept):
  L[lp, k] read for every k instead of k <= lp in path_score_kernel and gather_rows_kernel: every case with a second reading, first
      rm_row0_rowN_lds / rm_row0_rowN_batched (all but wide_3_row2090, whose row's tail of the last tile happens to hold zeros);
  0 instead of 1 on path_assemble_kernel's padding diagonal: every batched case whose length is no multiple of 128 (len65, len127,
      len129, len255, mixed_*, rm_only_65_3, rm_only_130_64, shape_maxlen262_130sites, wide_65 / wide_130), as NaN;
  the second batch's path ids copied without the batch's offset in score_paths_vr: test_variance_reduction_in_two_batches, both dtypes,
      and nothing else;
  delta = sm for a re-measured site in score_paths_mi: every MI case with a second reading, first rm_only_3_64 and full_1_5_40;
  sm added off the diagonal in pvr_gather_kernel: every case with a long path under VR (len65 .. len256, mixed_*, rm_*_batched,
      vr_weights_40_70_200, vr_batches).

Measured on an MI355X, the worst per-path error per entry point, route and dtype over this file (220 tests in 12 s; the slowest,
the fp64 batching case with its 481 + 961 refits, 2.2 s; every other below 0.5 s):

                 entropy                          MI (terms and sum)               VR
          lds      batched128 batched256   lds      batched128 batched256   lds      batched128 batched256
    fp64  3.6e-16  7.4e-16    5.3e-16      2.7e-13  2.1e-13    2.2e-13      1.4e-12  4.5e-15    1.0e-14
    fp32  1.1e-07  3.9e-07    2.4e-07      4.5e-05  2.9e-05    5.2e-05      8.8e-06  3.1e-06    3.3e-06

    vr_batches: fp64 8.3e-15 over 481 paths, fp32 1.3e-06 over 961; max_union = 256 (94 groups) against one group 3.2e-16.
No bug was found in the library: every route meets the fp64 bars with five orders of magnitude to spare, and fp32 stays 25 times
and more below the project's bars even on a single path's own scale.
"""
import functools

import numpy as np
import pytest

import matern_forms as MF
import path_forms as PF
from algp_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float64, id='f64'), pytest.param(np.float32, id='f32')]
TOL = {'ent': {np.float64: 1e-9, np.float32: 2e-3}, 'mi': {np.float64: 1e-7, np.float32: 3e-3},
       'vr': {np.float64: 1e-9, np.float32: 1e-3}}
WORST = {}
SYNCS = {'ent': {'lds': 1, 'batched128': 2, 'batched256': 2}, 'mi': {'lds': 2, 'batched128': 3, 'batched256': 3}}


def _grid():
    out = []
    for name, case in PF.CASES.items():
        if name in ('vr_batches', 'vr_weights_40_70_200'):
            continue
        for kid in PF.kernels_of(name):
            pools = ['coords', 'cov'] if case.problem in ('small', 'mid') and kid in PF.KERNELS_EVERYWHERE else ['coords']
            out += [pytest.param(name, kid, pool, id='%s-%s-%s' % (name, PF.KNAMES[kid], pool)) for pool in pools]
    return out


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for (dt, entry, route), e in sorted(WORST.items()):
        print('\nworst per-path error  %s %-3s %-10s %.2e' % (dt, entry, route, e))


def context(p, dtype, pool, weights=None):
    c = _hip.Context(dtype)
    c.set_hypers(p.log_ls, p.log_os, p.log_noise, p.kid)
    if pool == 'cov':
        c.set_pool_cov(p.C)
    else:
        c.set_pool(p.X)
    if weights is not None:
        c.set_target_weights(weights)
    c.set_train(p.A, np.zeros(p.N), p.var)
    c.factorize()
    c.set_candidates(p.cand, prior_includes_noise=True)
    c.solve_candidates()
    return c


def _note(dtype, entry, route, err):
    key = (np.dtype(dtype).name, entry, route)
    WORST[key] = max(WORST.get(key, 0.0), err)


def check(entry, dtype, got, want, routes, what):
    """every path against its own bound; a reference of exactly 0 (an empty path) must be met with exactly 0; returns the worst"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got)), (what, got)
    tol, worst = TOL[entry][dtype], 0.0
    flat_routes = routes if got.ndim == 1 else np.repeat(routes, got.shape[1])
    for i, (g, w, rt) in enumerate(zip(got.ravel(), want.ravel(), flat_routes)):
        if rt == 'none':
            assert g == 0.0 and w == 0.0, (what, i, g)
            continue
        err = abs(g - w) / (abs(w) if entry == 'vr' else max(1.0, abs(w)))
        worst = max(worst, err)
        _note(dtype, entry, rt, err)
        assert err <= tol, (what, 'path or term %d' % i, g, w, err, tol)
    return worst


def _state(c):
    mu, var = c.posterior()
    return mu, var, c.scores(_hip.CRIT_ENTROPY, PF.STATIC_STD, PF.MOBILE_STD)


def _same_state(a, b):
    """NaN equal to NaN: the static-only train rows among the candidates are not switched off here, and the entropy score of a
    unit row assumes a mobile-sampled site (log1p(delta s_cc) with delta < 0), which is NaN for some of them before and after"""
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _call(c, entry, sites, **kw):
    if entry == 'ent':
        return c.score_paths(sites, PF.MOBILE_STD)
    if entry == 'mi':
        return c.score_paths_mi(sites, PF.STATIC_STD, PF.MOBILE_STD, want_terms=True)
    return c.score_paths_vr(sites, PF.MOBILE_STD, **kw)


def _score(c, entry, sites):
    """(result, the same call again, synchronisations of the second call)"""
    first = _call(c, entry, sites)
    n0 = c.sync_count()
    again = _call(c, entry, sites)
    return first, again, c.sync_count() - n0


def _vr_routes(case, rows):
    return ['none' if not PF.distinct(r) else rt for r, rt in zip(rows, case.routes['vr'])]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,kid,pool', _grid())
def test_every_path_meets_its_own_bound(name, kid, pool, dtype):
    case = PF.CASES[name]
    p = PF.problem(case.problem, kid)
    sites, rows = PF.sites_of(name)
    ref = PF.reference(name, kid)
    empty = [not PF.distinct(r) for r in rows]
    line = []
    c = context(p, dtype, pool)
    try:
        before = _state(c)
        if 'ent' in case.entries:
            got, again, syncs = _score(c, 'ent', sites)
            assert np.array_equal(got, again), 'two identical calls must return identical bits'
            assert syncs == SYNCS['ent'][case.routes['ent']], (syncs, case.routes['ent'])
            assert _same_state(before, _state(c))
            rts = ['none' if e else case.routes['ent'] for e in empty]
            line.append('entropy %.2e' % check('ent', dtype, got, ref['ent'], rts, name))
            if dtype is np.float64 and case.argmax and len(rows) > 1:
                assert int(np.argmax(got)) == int(np.argmax(ref['ent']))
        if 'mi' in case.entries:
            (got, terms), (again, terms2), syncs = _score(c, 'mi', sites)
            assert np.array_equal(got, again) and np.array_equal(terms, terms2), 'two identical calls must return identical bits'
            assert syncs == SYNCS['mi'][case.routes['mi']], (syncs, case.routes['mi'])
            assert _same_state(before, _state(c))
            rts = ['none' if e else case.routes['mi'] for e in empty]
            want = ref['mi']
            line.append('mi terms %.2e' % check('mi', dtype, terms, want, rts, name))
            line.append('mi %.2e' % check('mi', dtype, got, want[:, 0] + want[:, 1] - want[:, 2], rts, name))
            if dtype is np.float64 and case.argmax and len(rows) > 1 and len(p.free):
                assert int(np.argmax(got)) == int(np.argmax(want[:, 0] + want[:, 1] - want[:, 2]))
        if 'vr' in case.entries:
            got, again, syncs = _score(c, 'vr', sites)
            assert np.array_equal(got, again), 'two identical calls must return identical bits'
            assert syncs == 2, syncs                             # one group: one batch of long paths (or none), the read-back
            assert _same_state(before, _state(c))
            line.append('vr %.2e' % check('vr', dtype, got, ref['vr'], _vr_routes(case, rows), name))
            if dtype is np.float64 and case.argmax and len(rows) > 1:
                assert int(np.argmax(got)) == int(np.argmax(ref['vr']))
    finally:
        c.close()
    print('%s %s %s %s: %s' % (name, PF.KNAMES[kid], pool, np.dtype(dtype).name, '  '.join(line)))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kid', PF.KERNELS_EVERYWHERE, ids=['rbf', 'matern15'])
def test_without_a_target_the_variance_reduction_is_zero(kid, dtype):
    """every site of `full` is sampled: T is empty, Phi = 0 and the sum over no target is 0 for every path"""
    p = PF.problem('full', kid)
    sites, rows = PF.sites_of('full_1_5_40')
    c = context(p, dtype, 'coords')
    try:
        got = c.score_paths_vr(sites, PF.MOBILE_STD)
    finally:
        c.close()
    assert got.shape == (3,) and np.all(got == 0.0), got


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kid', PF.KERNELS_EVERYWHERE, ids=['rbf', 'matern15'])
def test_variance_reduction_with_target_weights(kid, dtype):
    name = 'vr_weights_40_70_200'
    case = PF.CASES[name]
    p = PF.problem(case.problem, kid)
    sites, rows = PF.sites_of(name)
    w = PF.weights_of(name)
    assert np.sum(w[p.free] == 0.0) > 50 and np.array_equal(PF.f32(w), w)
    c = context(p, dtype, 'coords', weights=w)
    try:
        got, again, syncs = _score(c, 'vr', sites)
    finally:
        c.close()
    assert np.array_equal(got, again) and syncs == 2
    worst = check('vr', dtype, got, PF.reference(name, kid)['vr'], _vr_routes(case, rows), name)
    print('%s %s %s: vr %.2e' % (name, PF.KNAMES[kid], np.dtype(dtype).name, worst))
    if dtype is np.float64:
        assert int(np.argmax(got)) == int(np.argmax(PF.reference(name, kid)['vr']))


@pytest.mark.parametrize('dtype', DTYPES)
def test_variance_reduction_in_two_batches(dtype):
    """More long paths than one batch holds (476 in fp64, 953 in fp32 at ppad = 256; the host file derives the counts from
    api_paths_vr.hip): the p0 += bmax loop runs twice -- d_pid + p0, d_upos reused after the batch's synchronisation, the four
    bmax-strided blocks of the scratch.  About 1 GB of the library's own scratch, freed with the context."""
    name = 'vr_batches'
    npaths = 481 if dtype is np.float64 else 961
    case = PF.CASES[name]
    p = PF.problem(case.problem, MF.RBF)
    sites, rows = PF.sites_of(name)
    sites, rows = sites[:npaths], rows[:npaths]
    want = PF.reference(name, MF.RBF)['vr'][:npaths]
    c = context(p, dtype, 'coords')
    try:
        got, again, syncs = _score(c, 'vr', sites)
        assert syncs == 3, syncs                                 # two batches and the read-back
        assert np.array_equal(got, again)
        worst = check('vr', dtype, got, want, case.routes['vr'][:npaths], name)
        print('%s %s: vr %.2e over %d paths' % (name, np.dtype(dtype).name, worst, npaths))
        if dtype is np.float64:
            assert int(np.argmax(got)) == int(np.argmax(want))
            n0 = c.sync_count()
            cut = c.score_paths_vr(sites, PF.MOBILE_STD, max_union=256)
            groups, union = 1, set()                             # the library's rule: consecutive paths while the union fits
            for r in rows:
                if union and len(union | set(r)) > 256:
                    groups, union = groups + 1, set()
                union |= set(r)
            assert groups > 50 and c.sync_count() - n0 == groups + 1       # one batch of long paths per group
            check('vr', dtype, cut, want, case.routes['vr'][:npaths], name + ' max_union=256')
            err = float(np.max(np.abs(cut - got) / np.abs(got)))
            print('%s: max_union = 256 against one group %.2e' % (name, err))
            assert err < 1e-12
    finally:
        c.close()


# ---- bits -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _among(k):
    """a k-site path (new sites and second readings) alone, and as row 7 of a call with 20 others that keep the call's route"""
    p = PF.problem('mid', MF.RBF)
    rng = np.random.RandomState(900 + k)
    lo = 1 if k <= 64 else 65 if k <= 128 else 129
    others = [PF._mixed(p, rng, int(m), int(m) // 5) for m in rng.randint(lo, k + 1, 20)]
    target = PF._mixed(p, rng, k, k // 5)
    rows = others[:7] + [target] + others[7:]
    sites = np.full((21, k), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        sites[i, :len(r)] = r
    return np.array([target], dtype=np.int64), sites


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k', [30, 100, 200], ids=['lds', 'batched128', 'batched256'])
def test_a_path_alone_and_among_others(k, dtype):
    """On the LDS route a workgroup owns a path: the same bits whatever else the call holds.  On the batched routes (and for the
    MI scorer's P and Q blocks, which are batched on every route) the first run on an MI355X showed the same bits as well, for all
    three entry points and both dtypes -- a batch entry's tiles are computed by the same code whatever its neighbours, and a
    union site's Gamma and Phi entries are the same dot products wherever the site sits in the union -- so that is asserted."""
    p = PF.problem('mid', MF.RBF)
    alone, among = _among(k)
    rt = PF.route(k)
    c = context(p, dtype, 'coords')
    try:
        for entry in ('ent', 'mi', 'vr'):
            a, b = _call(c, entry, alone), _call(c, entry, among)
            if entry == 'mi':
                a, b = np.c_[a[0], a[1]], np.c_[b[0], b[1]]
            a, b = np.asarray(a, np.float64).reshape(1, -1)[0], np.asarray(b, np.float64)[7].ravel()
            same = bool(np.array_equal(a, b))
            print('alone and among others: %s %s %s same bits: %s (largest difference %.2e)'
                  % (np.dtype(dtype).name, entry, rt, same, float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(a))))))
            assert same, (entry, rt, a, b)
    finally:
        c.close()
