"""algp_get_mll_ai (Context.mll_ai) against tests/ai_forms.average_information computed in fp64 from the same inputs, for the
four single forms, the additive and the relationship kernel and both dtypes, in

* every size at which a stage takes another path: N = 1, 2; 63 | 64 | 65 (the 64-row groups of mll_ai_u_kernel and its 64-column
  tiles); 127 | 128 | 129 (the 128-row tiles of the solve); 512 | 513 (its 512-column blocks); 1025;
* every instantiation of mll_ai_u_kernel<T, DP, Form>: D = 1, 2 (DP = 2), 3, 4 (DP = 4), 5, 8 (DP = 8) -- with D < DP the
  padded slots must add nothing, with D = DP the last slot must count;
* an index list that is a permutation into a larger pool, a site listed twice in different 64-row groups and thrice inside one
  (the reference is told which rows are one site), Matern-1/2 with a site listed twice (r = 0 under the sqrt), no per-site
  noise, a constant mean that is given;
* and what the call leaves behind: the same bits after fit_step and after factorize + mll_grad, the same bits twice, a
  symmetric and positive semi-definite matrix, alpha / log det / gradient / a candidate solve with two picks unmoved, the
  device bytes unchanged by a second call, one synchronisation, the refusals.

Inputs are test_fit_regimes.py's (_draw, _side: x ~ U(0, side)^D, y = sin(x_0) + 0.1 randn, var ~ U(0.005, 0.05), length-scales
~ U(0.8, 2.1), outputscale 0.9, noise 0.05; the second outputscale of the two-part kernels 0.3, and (0.1, 0.9) where part a has
one coordinate only), and cond(S) <= 1e3 is asserted
on the host's S.  Errors are per entry relative to sqrt(AI_aa AI_bb) of the reference; the bounds are that file's TOL, 1e-8
(fp64) and 2e-2 (fp32): the same inputs and conditioning, and AI is two solves against S where the gradient is one.

Where fit_step and factorize take different launches (from N = 897, the identity panel: alpha comes from another kernel, as
test_fit_regimes.py describes) the two states give AI matrices equal to rounding, not bit for bit; below it the bits are equal.

Measured on an MI355X (largest error over the cases of this file):

    model              fp64      fp32            model              fp64      fp32
    rbf                7.1e-15   3.8e-06         add_m15_rbf_2of3   1.8e-14   4.9e-06
    matern (nu 3/2)    1.0e-14   3.3e-06         add_rbf_m25_1of4   4.5e-15   1.6e-06
    matern05           2.2e-15   4.9e-07         rel_table          1.2e-14   3.0e-06
    matern25           6.2e-15   4.8e-06         rel_identity       1.5e-14   4.5e-06
"""
import functools

import numpy as np
import pytest

import ai_forms as AI
import matern_forms as MF
import relationship_forms as RF
import test_fit_regimes as FR
from algp_amd import _hip

pytestmark = pytest.mark.gpu

TOL = FR.TOL
DTYPES = FR.DTYPES
LOG_OS, LOG_OS2, LOG_NOISE = np.log(FR.OUTPUTSCALE), np.log(0.3), np.log(FR.NOISE)
NGEN = 12
# name -> (family, spec, D or None: the width is the case's)
MODELS = {
    'rbf': ('single', MF.RBF, None), 'matern': ('single', MF.MATERN15, None),
    'matern05': ('single', MF.MATERN05, None), 'matern25': ('single', MF.MATERN25, None),
    'add_m15_rbf_2of3': ('additive', (MF.MATERN15, MF.RBF, 2), 3),
    'add_rbf_m25_1of4': ('additive', (MF.RBF, MF.MATERN25, 1), 4),
    'rel_table': ('relationship', (MF.MATERN15, RF.marker_relationship(Q=NGEN), NGEN), 3),
    'rel_identity': ('relationship', (MF.RBF, None, NGEN), 3),
}
# the part over ONE coordinate piles the N sites onto a line (a rank-few part with eigenvalues ~ N os_a): 0.1 keeps cond(S) <= 1e3
TWO_PART_LOG_OS = {'add_rbf_m25_1of4': (np.log(0.1), LOG_OS)}
WORST = {}                                         # (dtype, model) -> largest error


@functools.lru_cache(maxsize=None)
def _case(model, N, D=2, variant='plain'):
    """Inputs and reference of one case: computed once, shared by both dtypes and every test that uses it, never written to.
    variant: 'plain' (the train sites are the pool), 'permuted' (N of a pool of 2 N, in random order), 'site_twice' (one of them
    listed again in another 64-row group), 'site_thrice_in_one_group', 'no_var', 'mean_given' (0.3) -- test_fit_regimes.py's
    _gather_case, for every model."""
    family, spec, Dm = MODELS[model]
    D = Dm or D
    nsp = D - 1 if family == 'relationship' else D          # the coordinates _draw gives; the id column comes behind them
    gathered = variant != 'plain'
    x, y, var, log_ls = FR._draw(N, nsp, 2 * N if gathered else None, seed=1 if gathered else 0)
    rng = np.random.RandomState(N + D)
    if family == 'relationship':
        x = np.c_[x, rng.randint(0, NGEN, len(x)).astype(np.float64)]
    idx = np.arange(N)
    if gathered:
        x = x[rng.permutation(2 * N)]
        idx = rng.permutation(2 * N)[:N]
    if variant == 'site_twice':                              # the noisiest row of the first group and of the others (cond(S))
        idx[64 + int(np.argmax(var[64:]))] = idx[int(np.argmax(var[:64]))]
    if variant == 'site_thrice_in_one_group':
        a, b, c3 = np.argsort(var[:64])[-3:]
        idx[b] = idx[c3] = idx[a]
    if variant == 'no_var':
        var = None
    mean = 0.3 if variant == 'mean_given' else None
    sites = idx if variant.startswith('site_') else None
    theta = AI.pack(log_ls, LOG_OS if family == 'single' else TWO_PART_LOG_OS.get(model, (LOG_OS, LOG_OS2)), LOG_NOISE)
    ev = np.linalg.eigvalsh(AI.train_matrix(family, spec, theta, x[idx], var, sites))
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e3, 'the inputs are worse conditioned than the tolerances were set for'
    want = AI.average_information(family, spec, theta, x[idx], y, var, sites, mean)
    for a in (x, y, idx, theta, want) + (() if var is None else (var,)):
        a.setflags(write=False)
    return dict(model=model, family=family, spec=spec, theta=theta, x=x, y=y, var=var, idx=idx, mean=mean, want=want)


@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in (np.float64, np.float32)}
    yield c
    for v in c.values():
        v.close()
    for (dt, model), e in sorted(WORST.items()):
        print('\nmax AI error vs the forms  %s %-17s %.2e' % (dt, model, e))


def _set_hypers(c, case):
    family, spec = case['family'], case['spec']
    log_ls, log_os, log_noise = AI.unpack(family, case['theta'], case['x'])
    if family == 'single':
        c.set_hypers(log_ls, log_os, log_noise, spec)
    elif family == 'additive':
        c.set_hypers_additive(log_ls, spec[2], log_os[0], log_os[1], log_noise, spec[0], spec[1])
    else:
        c.set_hypers_relationship(log_ls, log_os[0], log_os[1], log_noise, kernel_a=spec[0], G=spec[1], n_genotypes=spec[2])


def _load(c, case):
    c.set_constant_mean(case['mean'])
    _set_hypers(c, case)
    c.set_pool(case['x'])
    c.set_train(case['idx'], case['y'], case['var'])


def _error(ai, want):
    """Per entry relative to sqrt(want_aa want_bb); where that is 0 (N = 1: y - ybar = 0) the entry has to be 0 itself."""
    s = np.sqrt(np.diag(want))
    scale = np.outer(s, s)
    assert np.all(ai[scale == 0] == 0)
    return float(np.max(np.where(scale > 0, np.abs(ai - want) / np.where(scale > 0, scale, 1.0), 0.0)))


def _check(c, case, what=''):
    """The matrix after a fit_step: against the reference, symmetric bit for bit, positive semi-definite, the same bits twice."""
    P = len(case['theta'])
    c.fit_step()
    ai = c.mll_ai()
    assert ai.shape == (P, P) and ai.dtype == np.float64 and np.all(np.isfinite(ai))
    err = _error(ai, case['want'])
    key = (c.dtype.name, case['model'])
    WORST[key] = max(WORST.get(key, 0.0), err)
    print('%s %s N=%d %s: AI error %.3e' % (c.dtype.name, case['model'], len(case['idx']), what, err))
    assert err <= TOL[c.dtype], (what, ai, case['want'])
    assert np.array_equal(ai, ai.T)
    ev = np.linalg.eigvalsh(ai)
    assert ev[0] >= -TOL[c.dtype] * ev[-1]
    assert np.array_equal(c.mll_ai(), ai)
    return ai


def _run(ctxs, dtype, case, what=''):
    c = ctxs[np.dtype(dtype)]
    try:
        _load(c, case)
        return _check(c, case, what)
    finally:
        c.set_constant_mean(None)


SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 512, 513, 1025]
WIDTHS = [(N, D, ('rbf', 'matern')[(i + j) % 2]) for i, N in enumerate((129, 513)) for j, D in enumerate((1, 3, 4, 5, 8))]
TWO_PART = [(m, N) for m in ('add_m15_rbf_2of3', 'add_rbf_m25_1of4') for N in (65, 129, 513)] + \
           [(m, N) for m in ('rel_table', 'rel_identity') for N in (129, 513)]
GATHER = [('rbf', 'permuted'), ('matern', 'permuted'), ('rbf', 'site_twice'), ('matern', 'site_twice'), ('matern05', 'site_twice'),
          ('rbf', 'site_thrice_in_one_group'), ('matern', 'site_thrice_in_one_group'), ('rel_table', 'site_twice'),
          ('add_m15_rbf_2of3', 'site_thrice_in_one_group'), ('matern', 'no_var'), ('rbf', 'mean_given')]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', ['rbf', 'matern'])
@pytest.mark.parametrize('N', SIZES)
def test_every_size_at_which_a_stage_changes_path(ctxs, dtype, model, N):
    _run(ctxs, dtype, _case(model, N))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,D,model', WIDTHS, ids=['N%d-D%d-%s' % w for w in WIDTHS])
def test_every_coordinate_width(ctxs, dtype, N, D, model):
    _run(ctxs, dtype, _case(model, N, D))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', ['rbf', 'matern', 'matern05', 'matern25'])
def test_the_four_single_forms(ctxs, dtype, model):
    _run(ctxs, dtype, _case(model, 129))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model,N', TWO_PART, ids=['%s-N%d' % t for t in TWO_PART])
def test_additive_and_relationship_kernels(ctxs, dtype, model, N):
    _run(ctxs, dtype, _case(model, N))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model,variant', GATHER, ids=['%s-%s' % g for g in GATHER])
def test_train_set_gathered_from_a_larger_pool(ctxs, dtype, model, variant):
    _run(ctxs, dtype, _case(model, 129, 2, variant), variant)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model,N', [('rbf', 129), ('matern', 513), ('rel_table', 129), ('rbf', 1025)])
def test_same_matrix_after_fit_step_and_after_factorize(ctxs, dtype, model, N):
    """fit_step leaves alpha current, factorize + mll_grad computes it on demand: the same launches below 897 rows and so the
    same bits; from there on alpha comes from the identity panel's X after fit_step and from the substitution after factorize,
    and the two matrices agree to rounding (test_fit_regimes.py's bounds between two device routes: 1e-10 | 2e-3)."""
    case = _case(model, N)
    c = ctxs[np.dtype(dtype)]
    _load(c, case)
    c.fit_step()
    a = c.mll_ai()
    c.factorize()
    c.mll_grad()
    b = c.mll_ai()
    c.factorize()                                        # and with alpha not computed by anybody before the call
    b2 = c.mll_ai()
    assert np.array_equal(b, b2)
    if N < FR.PANEL_FROM:
        assert np.array_equal(a, b)
    else:
        assert _error(a, b) <= (1e-10 if c.dtype == np.float64 else 2e-3)
    assert _error(b, case['want']) <= TOL[c.dtype]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', ['matern', 'rel_table'])
def test_nothing_else_moves(ctxs, dtype, model):
    """alpha, log det and the gradient; a resident candidate solve with two committed picks (posterior and scores); the device
    bytes and the synchronisation count of a repeated call."""
    N, M = 513, 40
    case = _case(model, N, 2, 'permuted')
    c = ctxs[np.dtype(dtype)]
    _load(c, case)
    c.factorize()
    cand = np.setdiff1d(np.arange(len(case['x'])), case['idx'])[:M]
    c.set_candidates(cand, prior_includes_noise=True)
    c.solve_candidates()
    c.commit_pick(int(cand[3]), 0.1, 1.0)
    c.commit_pick(int(cand[17]), 0.1, 1.0)
    state = lambda: (c.alpha(), np.float64(c.logdet()), c.mll_grad(), *c.posterior(), c.scores(_hip.CRIT_ENTROPY, 0.1, 1.0))
    before = state()
    ai = c.mll_ai()
    after = state()
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
    assert _error(ai, case['want']) <= TOL[c.dtype]
    nbytes, nsync = c.device_bytes(), c.sync_count()
    assert np.array_equal(c.mll_ai(), ai)
    assert c.device_bytes() == nbytes and c.sync_count() == nsync + 1
    for u, v in zip(before, state()):
        assert np.array_equal(u, v)


@pytest.mark.parametrize('dtype', DTYPES)
def test_refusals_leave_the_context_usable(dtype):
    case = _case('rbf', 65)
    c = _hip.Context(dtype)
    try:
        out = np.full((4, 4), np.nan)
        call = lambda p=out.ctypes.data_as(_hip._dblp): c.lib.algp_get_mll_ai(c.h, p)
        _set_hypers(c, case)
        c.set_pool(case['x'])
        c.set_train(case['idx'], case['y'], case['var'])
        assert call() == _hip.ERR_STATE                                 # no factorisation yet
        assert b'factorize' in c.lib.algp_last_error(c.h) and np.all(np.isnan(out))
        with pytest.raises(ValueError):
            c.mll_ai()
        c.factorize()
        assert call(None) == _hip.ERR_BAD_ARG                           # ai_out == NULL
        assert call() == _hip.OK and _error(out, case['want']) <= TOL[c.dtype]
        c.set_hypers(np.zeros(2), 0.0, 0.0)                             # new hyper-parameters: the factor is not current
        assert call() == _hip.ERR_STATE
        # an explicit covariance has no coordinates to differentiate
        S = AI.train_matrix(case['family'], case['spec'], case['theta'], case['x'])
        c.set_pool_cov(S)
        c.set_train(case['idx'], case['y'], case['var'])
        c.factorize()
        assert call() == _hip.ERR_BAD_ARG
        assert b'coordinate pool' in c.lib.algp_last_error(c.h)
        assert c.logdet() == pytest.approx(np.linalg.slogdet(S + np.diag(case['var']))[1], rel=1e-9 if c.dtype == np.float64 else 1e-3)
        # and back: the same context serves the call again
        _set_hypers(c, case)
        c.set_pool(case['x'])
        c.set_train(case['idx'], case['y'], case['var'])
        c.fit_step()
        assert _error(c.mll_ai(), case['want']) <= TOL[c.dtype]
        # an empty train set is legal: a zero matrix
        c.set_train(np.zeros(0, np.int64), np.zeros(0))
        c.factorize()
        assert np.array_equal(c.mll_ai(), np.zeros((4, 4)))
    finally:
        c.close()
