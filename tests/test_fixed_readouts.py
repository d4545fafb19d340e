"""The read-outs that carry the estimated fixed effects -- algp_genotype_posterior_fixed, algp_group_posterior_fixed,
algp_posterior_mean_fixed, algp_sample_posterior_fixed (Context.genotype_posterior / group_posterior / sample_posterior with
fixed=True, Context.posterior_mean_fixed) and the GPR methods on them -- against tests/fixed_readout_forms.py computed in fp64
from the same inputs, both dtypes.

Inputs are tests/test_fixed_effects.py's _case (test_fit_regimes._draw, reml_forms.basis, a planted H beta; cond(S) <= 1e3 and the
scaled cond(H_A' S^-1 H_A) <= 1e2 asserted on the host) and, for the genotype counts and the separable kernel, cases built the
same way here and in tests/test_separable_kernel.py (ai_case), under the same two assertions.

Bounds: 1e-5 (fp64) | 1e-3 (fp32); vectors and sample matrices relative to max(1, max |reference|), covariances
per entry relative to sqrt(c_aa c_bb), the Q x M cross relative to sqrt(cov_qq Sigma_jj).

Shapes: N = p + 1; 63 | 64 | 65; 127 | 128 | 129; 513.  p = 1, 3, 16.  Q = 1; 15 | 16 | 17; 63 | 64 | 65; 129.  M = 1, 64, 65, 129,
300.  Groupings: one group of all rows, singletons (= algp_get_posterior_fixed), rows in no group, explicit weights with an empty
group, a group that spans the member chunks of both segmented sums.  Samples: S = 1, 127, 129.
"""
import functools
import os
import re

import numpy as np
import pytest

import ai_forms as AI
import fixed_readout_forms as FO
import group_forms as GF
import matern_forms as MF
import pathwise_forms as PF
import relationship_forms as RF
import reml_forms as RM
import separable_forms as SF
import test_average_information as TA
import test_fit_regimes as FR
import test_fixed_effects as FE
import test_separable_kernel as TS
from algp_amd import _hip
from algp_amd.models import GPR

pytestmark = pytest.mark.gpu

DTYPES = FR.DTYPES
TOL = FE.TOL
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, 'algp_amd', 'csrc', 'vecops.h')) as _f:
    _h = _f.read()
GROUP_CHUNK = int(re.search(r'constexpr int GROUP_CHUNK = (\d+);', _h).group(1))
GROUP_ROWCHUNK = int(re.search(r'constexpr int GROUP_ROWCHUNK = (\d+);', _h).group(1))
TWO_PART = ('additive', 'relationship')

vec_err = FE._vec_err
f64 = lambda a: np.asarray(a, np.float64)           # (np.float64(a) turns a 1 x 1 matrix into a scalar)
cov_err = TA._error


def cross_err(got, want, cov_g, cov_c):
    scale = np.sqrt(np.outer(np.diag(cov_g), np.diag(cov_c)))
    assert np.all(np.asarray(got)[scale == 0] == 0)
    return float(np.max(np.where(scale > 0, np.abs(got - want) / np.where(scale > 0, scale, 1.0), 0.0)))


def _args(case):
    i = case['idx']
    return (case['family'], case['spec'], case['theta'], case['x'][i], case['y'], case['H'][i]), (case['var'], None, case['mean'])


@functools.lru_cache(maxsize=None)
def _post(key):
    """The universal-kriging posterior at the candidates of FE._case(*key), with its full covariance: shared, never written to."""
    case = FE._case(*key)
    a, kw = _args(case)
    post = RM.posterior_fixed(*a, case['x'][case['cand']], case['H'][case['cand']], *kw)
    for v in post.values():
        v.setflags(write=False)
    return post


@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in (np.float64, np.float32)}
    yield c
    for v in c.values():
        v.close()


def _with(ctxs, dtype, case, body, solve=True):
    c = ctxs[np.dtype(dtype)]
    try:
        FE._load(c, case, solve=solve)
        return body(c)
    finally:
        c.set_constant_mean(None)
        c.set_fixed_effects(None)


# ---- the genotype effects --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _geno_case(Q, N, p, table=True):
    """FE._case's recipe with Q genotypes: a marker relationship (table) or the identity.  The two conditions are asserted."""
    x, y, var, log_ls = FR._draw(N, 2, None, seed=0)
    rng = np.random.RandomState(N + Q + p)
    x = np.c_[x, rng.randint(0, Q, N).astype(np.float64)]
    spec = (MF.MATERN15, RF.marker_relationship(Q=Q, m=Q + 28) if table else None, Q)
    H = RM.basis(x[:, :2], p)
    y = y + H @ RM.planted_beta(p)
    theta = AI.pack(log_ls, (TA.LOG_OS, TA.LOG_OS2), TA.LOG_NOISE)
    ev = np.linalg.eigvalsh(AI.train_matrix('relationship', spec, theta, x, var))
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e3, 'the inputs are worse conditioned than the tolerances were set for'
    assert RM.scaled_cond(RM.gram('relationship', spec, theta, x, H, var)) <= 1e2, 'the basis is worse conditioned than the tolerances were set for'
    case = dict(model='rel', family='relationship', spec=spec, theta=theta, x=x, y=y, var=var, idx=np.arange(N), cand=np.arange(0), mean=None,
                H=H, p=p)
    for a in (x, y, var, theta, H):
        a.setflags(write=False)
    return case


def _check_geno(c, case):
    a, kw = _args(case)
    mean_w, cov_w = FO.genotype_posterior_fixed(*a, *kw)
    mean, var, cov = c.genotype_posterior(want_var=True, want_cov=True, fixed=True)
    known = c.genotype_posterior(want_var=True, want_cov=True)
    err = dict(mean=vec_err(mean, mean_w), var=vec_err(var, np.diag(cov_w)), cov=cov_err(f64(cov), cov_w))
    print('%s genotype effects Q=%d N=%d p=%d: %s' % (c.dtype.name, len(mean), len(case['idx']), case['p'],
                                                   '  '.join('%s %.2e' % kv for kv in sorted(err.items()))))
    for k, v in err.items():
        assert v <= TOL[c.dtype], (k, err)
    assert np.array_equal(cov, cov.T)
    again = c.genotype_posterior(want_var=True, want_cov=True, fixed=True)
    assert all(np.array_equal(u, v) for u, v in zip((mean, var, cov), again))
    assert np.array_equal(c.genotype_posterior(want_var=False, want_cov=False, fixed=True)[0], mean)
    # beta's uncertainty is there: never below the known-mean variances; the known-mean sibling is what it was
    assert np.all(var >= known[1] * (1 - 1e-6) - 1e-6)
    assert all(np.array_equal(u, v) for u, v in zip(known, c.genotype_posterior(want_var=True, want_cov=True)))
    return mean


GENO_SIZES = [(2, 1), (4, 3), (63, 3), (64, 16), (65, 3), (127, 16), (128, 3), (129, 16), (513, 3)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,p', GENO_SIZES, ids=['N%d-p%d' % s for s in GENO_SIZES])
def test_genotype_effects_every_size(ctxs, dtype, N, p):
    case = _geno_case(TA.NGEN, N, p)                       # at N = 2 and 4 most genotypes have no plot
    _with(ctxs, dtype, case, lambda c: _check_geno(c, case), solve=False)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Q', [1, 15, 16, 17, 63, 64, 65, 129])
def test_genotype_effects_every_count(dtype, Q):
    case = _geno_case(Q, 129, 3, table=Q % 2 == 1 and Q < 100)
    c = _hip.Context(dtype)                                # its own context: a resident pool's ids are checked against the new Q
    try:
        FE._load(c, case, solve=False)
        _check_geno(c, case)
    finally:
        c.close()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model,variant', [('rel_table', 'plain'), ('rel_identity', 'plain'), ('rel_table', 'permuted'), ('rel_identity', 'mean_given')])
def test_genotype_effects_every_kernel(ctxs, dtype, model, variant):
    case = FE._case(model, 129, 16, 2, variant)

    def body(c):
        mean = _check_geno(c, case)
        # component 1 of the mean at a site is the effect of its id
        sites = np.r_[case['cand'], case['idx'][:9]]
        share = c.posterior_mean_fixed(1, sites)
        assert vec_err(share, f64(mean)[case['x'][sites, -1].astype(int)]) <= TOL[c.dtype]
    _with(ctxs, dtype, case, body)


@pytest.mark.parametrize('dtype', DTYPES)
def test_genotype_effects_separable_kernel(dtype):
    case = TS.ai_case(('marker', 1, 3, 4, 129), 3)
    spec, i = case['spec'], case['idx']
    mean_w, cov_w = FO.genotype_posterior_fixed(SF.FAMILY, spec, case['theta'], case['x'][i], case['y'], case['H'][i], case['var'])
    c = _hip.Context(dtype)
    try:
        TS._load(c, case)
        c.factorize()
        mean, var, cov = c.genotype_posterior(want_var=True, want_cov=True, fixed=True)
        err = dict(mean=vec_err(mean, mean_w), var=vec_err(var, np.diag(cov_w)), cov=cov_err(f64(cov), cov_w))
        print('%s separable: %s' % (c.dtype.name, err))
        assert max(err.values()) <= TOL[c.dtype] and np.array_equal(cov, cov.T)
        sites = np.r_[case['cand'][:11], i[:9]]
        assert vec_err(c.posterior_mean_fixed(1, sites), f64(mean)[case['x'][sites, -1].astype(int)]) <= TOL[c.dtype]
        want = FO.mean_fixed(SF.FAMILY, spec, case['theta'], case['x'][i], case['y'], case['H'][i], case['x'][sites], case['H'][sites], -1, case['var'])
        assert vec_err(c.posterior_mean_fixed(-1, sites), want) <= TOL[c.dtype]
    finally:
        c.close()


# ---- the mean at pool sites ------------------------------------------------------------------------------------------------------
def _check_mean(c, case):
    a, kw = _args(case)
    sites = np.r_[case['cand'], case['idx'][:7]]
    comps = (-1, 0, 1, 2) if case['family'] in TWO_PART else (-1, 2)
    got = {k: c.posterior_mean_fixed(k, sites) for k in comps}
    for k in comps:
        want = FO.mean_fixed(*a, case['x'][sites], case['H'][sites], k, *kw)
        e = vec_err(got[k], want)
        print('%s %s mean component %d: %.2e' % (c.dtype.name, case['model'], k, e))
        assert e <= TOL[c.dtype], (k, e)
        assert np.array_equal(c.posterior_mean_fixed(k, sites), got[k])
    if len(comps) == 4:
        ybar = case['y'].mean() if case['mean'] is None else case['mean']
        assert vec_err(f64(got[-1]), ybar + f64(got[0]) + f64(got[1]) + f64(got[2])) <= TOL[c.dtype]
    else:
        for k in (0, 1):
            with pytest.raises(ValueError):
                c.posterior_mean_fixed(k, sites)
    # at the candidates: algp_get_posterior_fixed's mu
    assert vec_err(got[-1][:len(case['cand'])], f64(c.posterior_fixed()[0])) <= TOL[c.dtype]
    assert len(c.posterior_mean_fixed(-1, np.arange(0))) == 0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', sorted(TA.MODELS))
def test_mean_every_kernel_form(ctxs, dtype, model):
    case = FE._case(model, 129, 16)
    _with(ctxs, dtype, case, lambda c: _check_mean(c, case))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,p', GENO_SIZES, ids=['N%d-p%d' % s for s in GENO_SIZES])
def test_mean_every_size(ctxs, dtype, N, p):
    case = FE._case('matern' if N % 2 else 'rbf', N, p)
    _with(ctxs, dtype, case, lambda c: _check_mean(c, case))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model,variant', [('rbf', 'permuted'), ('rbf', 'mean_given')])
def test_mean_gathered_and_given(ctxs, dtype, model, variant):
    case = FE._case(model, 129, 16, 2, variant)
    _with(ctxs, dtype, case, lambda c: _check_mean(c, case))


# ---- the group aggregates --------------------------------------------------------------------------------------------------------
def _grouping(which, M, Q=None):
    """(labels, weights or None, Q)."""
    rng = np.random.RandomState(M + 31)
    if which == 'all':
        return np.zeros(M, np.int32), None, 1
    if which == 'singletons':
        return np.arange(M, dtype=np.int32), None, M
    if which == 'dealt':                                   # Q groups of near-equal size over all but a few rows, which carry no label
        n = max(1, (M - min(3, M - Q)) // Q)
        return GF.deal([n] * Q, M, 5), None, Q
    if which == 'weights_empty':                           # explicit weights, group 1 of 4 without members, some rows unlabelled
        lab = GF.deal([M // 4, 0, M // 3, M // 5], M, 6)
        return lab, PF.f32(rng.uniform(-1.0, 1.0, M)), 4
    if which == 'span':                                    # the first group spans the chunks of both segmented sums
        big = max(GROUP_CHUNK, GROUP_ROWCHUNK) + 3
        return GF.deal([big, 5, M - big - 9], M, 7), None, 3
    raise ValueError(which)


def _check_group(c, key, which, Q=None):
    case, post = FE._case(*key), _post(key)
    M = len(case['cand'])
    lab, w, Q = _grouping(which, M, Q)
    A = GF.coefficients(lab, w, Q)
    want = dict(mean=A @ post['mu'], cov=A @ post['cov'] @ A.T, cross=A @ post['cov'])
    mean, cov, cross = c.group_posterior(lab, weight=w, n_groups=Q, want_cov=True, want_cross=True, fixed=True)
    mean2, cov2, _ = c.group_posterior(lab, weight=w, n_groups=Q, want_cov=True, want_cross=False, fixed=True)
    mean3, _, _ = c.group_posterior(lab, weight=w, n_groups=Q, want_cov=False, want_cross=False, fixed=True)
    err = dict(mean=vec_err(mean, want['mean']), cov=cov_err(f64(cov), want['cov']), cov_alone=cov_err(f64(cov2), want['cov']),
               cross=cross_err(f64(cross), want['cross'], want['cov'], post['cov']))
    print('%s %s N=%d M=%d %s Q=%d: %s' % (c.dtype.name, case['model'], len(case['idx']), M, which, Q,
                                          '  '.join('%s %.2e' % kv for kv in sorted(err.items()))))
    for k, v in err.items():
        assert v <= TOL[c.dtype], (k, err)
    assert np.array_equal(cov, cov.T) and np.array_equal(cov2, cov2.T)
    assert np.array_equal(mean, mean2) and np.array_equal(mean, mean3)
    again = c.group_posterior(lab, weight=w, n_groups=Q, want_cov=True, want_cross=True, fixed=True)
    assert all(np.array_equal(u, v) for u, v in zip((mean, cov, cross), again))
    return mean, cov, cross


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('M', [1, 64, 65, 129, 300])
@pytest.mark.parametrize('which', ['all', 'singletons'])
def test_groups_every_candidate_count(ctxs, dtype, M, which):
    key = ('matern', 129, 3, 2, 'plain', M)

    def body(c):
        mean, cov, cross = _check_group(c, key, which)
        if which == 'singletons':                          # = algp_get_posterior_fixed and the covariance it describes
            mu, var, proj = c.posterior_fixed(want_var=True, want_proj=True)
            full = f64(c.posterior_cov()[0]) + f64(proj) @ f64(proj).T
            assert vec_err(mean, f64(mu)) <= TOL[c.dtype] and vec_err(np.diag(cov), f64(var)) <= TOL[c.dtype]
            assert cov_err(f64(cov), full) <= TOL[c.dtype] and cov_err(f64(cross), full) <= TOL[c.dtype]
    _with(ctxs, dtype, FE._case(*key), body)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Q', [1, 15, 16, 17, 63, 64, 65, 129])
def test_groups_every_group_count(ctxs, dtype, Q):
    key = ('rbf', 129, 16, 2, 'plain', 300)
    _with(ctxs, dtype, FE._case(*key), lambda c: _check_group(c, key, 'dealt', Q))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,p', GENO_SIZES, ids=['N%d-p%d' % s for s in GENO_SIZES])
def test_groups_every_size(ctxs, dtype, N, p):
    key = ('matern' if N % 2 else 'rbf', N, p)
    key = key + (2, 'plain', 40)
    _with(ctxs, dtype, FE._case(*key), lambda c: _check_group(c, key, 'weights_empty'))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', sorted(TA.MODELS))
def test_groups_every_kernel_form(ctxs, dtype, model):
    key = (model, 129, 16, 2, 'plain', 40)
    _with(ctxs, dtype, FE._case(*key), lambda c: _check_group(c, key, 'weights_empty'))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', ['permuted', 'mean_given'])
def test_groups_gathered_and_given(ctxs, dtype, variant):
    key = ('rbf', 129, 16, 2, variant, 40)
    _with(ctxs, dtype, FE._case(*key), lambda c: _check_group(c, key, 'dealt', 7))


@pytest.mark.parametrize('dtype', DTYPES)
def test_groups_spanning_member_chunks(ctxs, dtype):
    key = ('matern', 129, 3, 2, 'plain', max(GROUP_CHUNK, GROUP_ROWCHUNK) + 40)
    _with(ctxs, dtype, FE._case(*key), lambda c: _check_group(c, key, 'span'))


# ---- joint draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('S', [1, 127, 129])
def test_samples_from_prior_values(ctxs, dtype, S):
    """Values mode, entrywise against sample_rule fed the same draws: a deterministic comparison."""
    key = ('matern', 129, 16, 2, 'plain', 65)
    case = FE._case(*key)
    a, kw = _args(case)
    rng = np.random.RandomState(S)
    prior, eps = PF.f32(rng.standard_normal((S, len(case['x'])))), PF.f32(rng.standard_normal((S, len(case['idx']))))
    want = FO.sample_rule(*a, case['x'][case['cand']], case['H'][case['cand']], prior[:, case['idx']], prior[:, case['cand']], eps, *kw)

    def body(c):
        got = c.sample_posterior(eps, prior=prior, fixed=True)
        e = vec_err(got, want)
        print('%s S=%d samples: %.2e' % (c.dtype.name, S, e))
        assert got.shape == want.shape and e <= TOL[c.dtype]
        assert np.array_equal(c.sample_posterior(eps, prior=prior, fixed=True), got)
        # without randomness the draw is the universal-kriging mean; the known-mean sibling differs by the trend
        zero = c.sample_posterior(np.zeros((1, len(case['idx']))), prior=np.zeros((1, len(case['x']))), fixed=True)[0]
        assert vec_err(zero, f64(c.posterior_fixed()[0])) <= TOL[c.dtype]
    _with(ctxs, dtype, case, body)


@pytest.mark.parametrize('dtype', DTYPES)
def test_samples_from_random_features(ctxs, dtype):
    key = ('rbf', 129, 3, 2, 'permuted', 129)
    case = FE._case(*key)
    a, kw = _args(case)
    F, S = 100, 5
    omega, phase, weights, eps = PF.draws(11, F, S, 2, len(case['idx']))
    log_ls, log_os, _ = AI.unpack(case['family'], case['theta'], case['x'])
    G = weights @ PF.features(omega, phase, case['x'] * np.exp(-log_ls)[None, :], np.exp(log_os)).T
    want = FO.sample_rule(*a, case['x'][case['cand']], case['H'][case['cand']], G[:, case['idx']], G[:, case['cand']], eps, *kw)

    def body(c):
        got = c.sample_posterior(eps, weights=weights, omega=omega, phase=phase, fixed=True)
        e = vec_err(got, want)
        print('%s features samples: %.2e' % (c.dtype.name, e))
        assert e <= TOL[c.dtype]
    _with(ctxs, dtype, case, body)


# ---- state and hygiene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_nothing_else_moves(ctxs, dtype):
    """alpha, log det, the posterior, the gradient and the known-mean siblings' outputs bit for bit around the four calls; the
    device bytes unchanged by a repeated call; one synchronisation per call (the sampler: one for the rank flag and one per tile of 128 samples)."""
    key = ('rel_table', 513, 16, 2, 'permuted', 40)
    case = FE._case(*key)
    lab, w, Q = _grouping('weights_empty', 40)
    rng = np.random.RandomState(3)
    prior, eps = rng.standard_normal((130, len(case['x']))), rng.standard_normal((130, 513))
    sites = case['cand']

    def body(c):
        state = lambda: (c.alpha(), np.array(c.logdet()), c.mll_grad(), *c.posterior(), *c.posterior_fixed(want_var=True, want_proj=True),
                         *c.genotype_posterior(want_var=True, want_cov=True), *c.group_posterior(lab, weight=w, n_groups=Q, want_cross=True),
                         c.posterior_mean_component(1, sites), c.sample_posterior(eps, prior=prior))
        calls = [lambda: c.genotype_posterior(want_var=True, want_cov=True, fixed=True),
                 lambda: c.group_posterior(lab, weight=w, n_groups=Q, want_cov=True, want_cross=True, fixed=True),
                 lambda: (c.posterior_mean_fixed(-1, sites),), lambda: (c.posterior_mean_fixed(1, sites),),
                 lambda: (c.sample_posterior(eps, prior=prior, fixed=True),)]
        before = state()
        first = [f() for f in calls]
        for u, v in zip(before, state()):
            assert np.array_equal(u, v)
        nbytes = c.device_bytes()
        for f, out, nsync in zip(calls, first, (1, 1, 1, 1, 3)):
            n0 = c.sync_count()
            again = f()
            assert c.sync_count() == n0 + nsync
            assert all(np.array_equal(u, v) for u, v in zip(out, again))
        assert c.device_bytes() == nbytes
        for u, v in zip(before, state()):
            assert np.array_equal(u, v)
    _with(ctxs, dtype, case, body)


@pytest.mark.parametrize('dtype', DTYPES)
def test_refusals_leave_the_context_usable(dtype):
    case = FE._case('rel_table', 65, 3)
    a, kw = _args(case)
    M, N = len(case['cand']), len(case['idx'])
    lab = np.zeros(M, np.int32)
    eps, prior = np.zeros((1, N)), np.zeros((1, len(case['x'])))
    c = _hip.Context(dtype)
    try:
        TA._set_hypers(c, case)
        c.set_pool(case['x'])
        c.set_train(case['idx'], case['y'], case['var'])
        c.factorize()
        c.set_candidates(case['cand'], prior_includes_noise=False)
        c.solve_candidates()
        calls = [lambda: c.genotype_posterior(fixed=True), lambda: c.group_posterior(lab, fixed=True),
                 lambda: c.posterior_mean_fixed(-1, case['cand']), lambda: c.sample_posterior(eps, prior=prior, fixed=True)]
        for call in calls:                                                # no basis attached
            with pytest.raises(ValueError, match='fixed effects'):
                call()
        H = np.array(case['H'])
        c.set_fixed_effects(np.c_[H, H[:, 1]])                            # a dependent column: NOT_PD naming it (1-based)
        for call in calls:
            with pytest.raises(np.linalg.LinAlgError) as e:
                call()
            assert e.value.pivot == 4 and 'column 4' in str(e.value)
        c.set_fixed_effects(H)
        with pytest.raises(ValueError):
            c.posterior_mean_fixed(3, case['cand'])
        with pytest.raises(ValueError):
            c.posterior_mean_fixed(-1, [len(case['x'])])
        assert c.lib.algp_genotype_posterior_fixed(c.h, None, None, None) == _hip.ERR_BAD_ARG
        c.commit_pick(int(case['cand'][3]), 0.1, 1.0)                     # picks since the solve
        for call in (calls[0], calls[1], calls[3]):
            with pytest.raises(ValueError, match='pick'):
                call()
        c.set_train(case['idx'][:3], case['y'][:3], case['var'][:3])      # more effects than train rows can determine
        c.factorize()
        c.set_candidates(case['cand'], prior_includes_noise=False)
        c.solve_candidates()
        for call in calls[:3] + [lambda: c.sample_posterior(eps[:, :3], prior=prior, fixed=True)]:
            with pytest.raises(ValueError, match='determine'):
                call()
        c.set_train(case['idx'], case['y'], case['var'])
        for call in (calls[0], calls[2]):
            with pytest.raises(ValueError, match='factorize'):
                call()
        c.factorize()
        for call in (calls[1], calls[3]):
            with pytest.raises(ValueError, match='solve_candidates'):
                call()
        c.set_candidates(np.r_[case['idx'][:2], case['cand']], prior_includes_noise=True)
        c.solve_candidates()
        with pytest.raises(ValueError, match='unit row'):
            c.group_posterior(np.zeros(M + 2, np.int32), fixed=True)
        c.set_candidates(case['cand'], prior_includes_noise=False)
        c.solve_candidates()
        assert vec_err(c.genotype_posterior(fixed=True)[0], FO.genotype_posterior_fixed(*a, *kw)[0]) <= TOL[c.dtype]
        assert vec_err(c.group_posterior(lab, fixed=True)[0], np.mean(_post(('rel_table', 65, 3))['mu'], keepdims=True)) <= TOL[c.dtype]
        # the group call at the ABI: every output may be NULL on its own; cov alone is the cov of the full call
        full = c.group_posterior(lab, want_cov=True, want_cross=True, fixed=True)
        cov = np.empty((1, 1), c.dtype)
        labp = lab.ctypes.data_as(_hip.C.POINTER(_hip.C.c_int32))
        assert c.lib.algp_group_posterior_fixed(c.h, labp, None, 1, None, _hip._ptr(cov), None) == _hip.OK
        assert vec_err(cov, f64(full[1])) <= TOL[c.dtype]
        cross = np.empty((1, M), c.dtype)
        assert c.lib.algp_group_posterior_fixed(c.h, labp, None, 1, None, None, _hip._ptr(cross)) == _hip.OK
        assert np.array_equal(cross, full[2])
        assert c.lib.algp_group_posterior_fixed(c.h, labp, None, 0, None, None, None) == _hip.ERR_BAD_ARG
        # an explicit pool covariance has no coordinates to evaluate a kernel row or read an id from
        S = AI.train_matrix(case['family'], case['spec'], case['theta'], case['x'][case['idx']])
        c.set_pool_cov(S)
        c.set_fixed_effects(H[case['idx']])
        c.set_train(np.arange(N), case['y'], case['var'])
        c.factorize()
        for call in (calls[0], lambda: c.posterior_mean_fixed(-1, np.arange(4))):
            with pytest.raises(ValueError, match='coordinate pool'):
                call()
        # no genotype term in force: the effects' call is refused at the ABI (the binding has a check of its own before it)
        c.set_hypers(case['theta'][:2], TA.LOG_OS, TA.LOG_NOISE)
        c.set_pool(case['x'][:, :2])
        c.set_fixed_effects(H)
        c.set_train(case['idx'], case['y'], case['var'])
        c.factorize()
        mean = np.empty(TA.NGEN, c.dtype)
        assert c.lib.algp_genotype_posterior_fixed(c.h, _hip._ptr(mean), None, None) == _hip.ERR_STATE
        assert b'genotype term' in c.lib.algp_last_error(c.h)
        for k in (0, 1):                                                  # nor has a single kernel shares
            with pytest.raises(ValueError, match='single kernel'):
                c.posterior_mean_fixed(k, case['cand'])
        assert np.all(np.isfinite(c.posterior_mean_fixed(-1, case['cand'])))
    finally:
        c.close()


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def _gpr_problem():
    rng = np.random.RandomState(12)
    N, M, Q = 120, 30, 6
    x = np.c_[rng.uniform(0, 8, (N + M, 2)), rng.randint(0, Q, N + M)]
    y = np.sin(x[:N, 0]) + 0.4 * x[:N, 1] + 0.3 * rng.standard_normal(Q)[x[:N, 2].astype(int)] + 0.1 * rng.standard_normal(N)
    return x[:N], y, rng.uniform(0.005, 0.05, N), x[N:], Q


def _gpr(fixed_effects, G=None):
    xt, y, var, xs, Q = _gpr_problem()
    kp = {'type': 'genotype', 'spatial': {'type': 'matern', 'nu': 1.5}, 'relationship': G, 'n_genotypes': Q}
    gp = GPR(max_iterations=0, kernel_params=kp, fixed_effects=fixed_effects)
    gp.reset(xt, y, var)
    return gp, (xt, y, var, xs, Q)


def test_gpr_read_outs_carry_the_fixed_effects():
    """GPR(fixed_effects='linear') under the genotype kernel: the four read-outs against the forms at the model's parameters."""
    gp, (xt, y, var, xs, Q) = _gpr('linear', RF.marker_relationship(Q=6))
    log_ls, log_os, log_noise, kid = gp.hypers()
    G, Qm = gp.model.relationship
    a = ('relationship', (kid[1], G, Qm), AI.pack(log_ls, log_os, log_noise), xt, y, gp.fixed_basis(xt))
    Hs = gp.fixed_basis(xs)
    mean, v = gp.genotype_effects()
    mean_w, cov_w = FO.genotype_posterior_fixed(*a, var)
    assert vec_err(mean, mean_w) <= 1e-5 and vec_err(v, np.diag(cov_w)) <= 1e-5
    assert cov_err(gp.genotype_effects(return_cov=True)[1], cov_w) <= 1e-5
    # the adjustment is no rounding matter here: the known-mean BLUPs are elsewhere
    assert vec_err(FO.genotype_posterior_known(*a[:5], var)[0], mean_w) >= 1e-3
    ma, mb = gp.predict_components(xs)
    tr = gp.predict_trend(xs)
    for got, k in ((ma, 0), (mb, 1), (tr, 2)):
        assert vec_err(got, FO.mean_fixed(*a, xs, Hs, k, var)) <= 1e-5
    assert vec_err(ma + mb + tr + y.mean(), gp.predict(xs)) <= 1e-5
    lab = xs[:, 2].astype(np.int32)
    want = FO.group_posterior_fixed(*a, xs, Hs, GF.coefficients(lab, None, Q), var)
    gm, gc, gx = gp.group_posterior(xs, lab, n_groups=Q, return_cross=True)
    assert vec_err(gm, want['mean']) <= 1e-5 and cov_err(gc, want['cov']) <= 1e-5
    assert cross_err(gx, want['cross'], want['cov'], RM.posterior_fixed(*a, xs, Hs, var)['cov']) <= 1e-5
    # the draws are utils.posterior_samples' (its order of draws) through the rule with the effects
    from algp_amd.utils import relationship_prior_draws
    rng = np.random.RandomState(5)
    pool = np.vstack([xt, xs])
    prior = relationship_prior_draws(kid[1], log_ls, np.exp(log_os[0]), np.exp(log_os[1]), G, Qm, pool, 3, 64, rng)
    eps = rng.standard_normal((3, len(xt)))
    want_s = FO.sample_rule(*a, xs, Hs, prior[:, :len(xt)], prior[:, len(xt):], eps, var)
    assert vec_err(gp.sample_posterior(xs, n_samples=3, n_features=64, rng=5), want_s) <= 1e-5


def test_gpr_without_fixed_effects_is_what_it_was():
    """Without a basis the four methods return the bits of the known-mean entry points called directly."""
    gp, (xt, y, var, xs, Q) = _gpr(None)
    N, M = len(xt), len(xs)
    pool, idx = np.vstack([xt, xs]), np.arange(len(xt), len(xt) + len(xs))
    lab = xs[:, 2].astype(np.int32)
    c = _hip.Context(np.float64)
    try:
        gp.push_hypers(c)
        c.set_pool(xt)
        c.set_train(np.arange(N), y, var)
        c.factorize()
        g = c.genotype_posterior(want_var=True, want_cov=True)
        assert np.array_equal(gp.genotype_effects()[0], g[0]) and np.array_equal(gp.genotype_effects()[1], g[1])
        assert np.array_equal(gp.genotype_effects(return_cov=True)[1], g[2])
        c.set_pool(pool)
        c.set_train(np.arange(N), y, var)
        c.factorize()
        got = gp.predict_components(xs)
        assert np.array_equal(got[0], c.posterior_mean_component(0, idx)) and np.array_equal(got[1], c.posterior_mean_component(1, idx))
        c.set_candidates(idx, prior_includes_noise=False)
        c.fit_and_solve()
        want = c.group_posterior(lab, n_groups=Q, want_cov=True, want_cross=True)
        assert all(np.array_equal(u, v) for u, v in zip(gp.group_posterior(xs, lab, n_groups=Q, return_cross=True), want))
        from algp_amd.utils import relationship_prior_draws
        log_ls, log_os, _, kid = gp.hypers()
        rng = np.random.RandomState(5)
        prior = relationship_prior_draws(kid[1], log_ls, np.exp(log_os[0]), np.exp(log_os[1]), None, Q, pool, 3, 64, rng)
        eps = rng.standard_normal((3, N))
        assert np.array_equal(gp.sample_posterior(xs, n_samples=3, n_features=64, rng=5), c.sample_posterior(eps, prior=prior))
        with pytest.raises(ValueError, match='fixed_effects'):
            gp.predict_trend(xs)
    finally:
        c.close()
