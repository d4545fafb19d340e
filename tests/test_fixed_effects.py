"""The fixed effects' entry points (algp_set_fixed_effects, algp_get_gls, algp_get_posterior_fixed, algp_get_reml_grad,
algp_get_reml_ai, algp_reml_step; Context.set_fixed_effects, gls, posterior_fixed, reml_grad, reml_ai, reml_step) against
tests/reml_forms.py computed in fp64 from the same inputs, both dtypes, in

* every size at which a stage takes another path: N = p + 1; 63 | 64 | 65; 127 | 128 | 129 (the 128-row tiles of the solve);
  513; 897 (test_fit_regimes.PANEL_FROM); 1025;  p = 1, 3, 15, 16;  M = 1, 15 | 16 | 17 (one MFMA row group), 63 | 64 | 65 (the 64
  rows of a wave), 127 | 129, 300;  D = 1, 3, 5, 8;
* the four single forms, the additive and the relationship kernels; an index list that is a permutation into a larger pool, a
  site listed twice in different 64-row groups, a constant mean that is given;
* and what the calls leave behind: the same bits twice, alpha / log det / gradient / AI / a candidate solve with two picks
  unmoved, the device bytes unchanged by a second call, one synchronisation per call, the refusals.

Inputs are test_fit_regimes.py's (_draw, _side) with the hyper-parameters of test_average_information.py and a planted H beta
added to y; the bases are reml_forms.basis (p = 1: the constant; 3: + scaled coordinates; 16: + eleven indicators of twelve random
blocks + two quadratic terms).  Asserted on the host, as conditions of the bounds: cond(S) <= 1e3 and cond of A = H_A' S^-1 H_A
scaled to a unit diagonal <= 1e2.

Bounds: 1e-5 (fp64) | 1e-3 (fp32) for beta, mu, var and proj relative to max(1, max |reference|) and for
cov beta per entry relative to sqrt(cov_aa cov_bb); 1e-9 | 1e-3 relative for l_R (the log-determinant's bound);
test_fit_regimes.TOL (1e-8 | 2e-2) for the gradient relative to max(1, max |reference|) and for AI_R per entry relative to
sqrt(AI_aa AI_bb).

Measured on an MI355X (largest error over the accuracy cases of this file and over all eight quantities; the run prints the
table per quantity at its end):

    model              fp64      fp32            model              fp64      fp32
    rbf                1.5e-14   3.2e-06         add_m15_rbf_2of3   1.5e-14   2.9e-06
    matern (nu 3/2)    1.4e-14   2.9e-06         add_rbf_m25_1of4   6.9e-15   1.8e-06
    matern05           4.1e-15   8.8e-07         rel_table          9.3e-15   2.6e-06
    matern25           8.6e-15   4.1e-06         rel_identity       3.6e-14   5.3e-06

Every bar holds in fp32 at p = 16 with two orders to spare.
"""
import functools

import numpy as np
import pytest

import ai_forms as AI
import reml_forms as RM
import test_average_information as TA
import test_fit_regimes as FR
from algp_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = FR.DTYPES
TOL = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}
TOL_REML = {np.dtype(np.float64): 1e-9, np.dtype(np.float32): 1e-3}
WORST = {}                                         # (dtype, model) -> {quantity: largest error}


@functools.lru_cache(maxsize=None)
def _case(model, N, p, D=2, variant='plain', M=40):
    """Inputs and reference of one case: computed once, shared by both dtypes and every test that uses it, never written to.
    variant: 'plain' (the first N pool sites are the train set, the next M the candidates), 'permuted' (both drawn from a
    shuffled pool of 2 N + M), 'site_twice' (and one train site listed again in another 64-row group), 'mean_given' (0.3)."""
    family, spec, Dm = TA.MODELS[model]
    D = Dm or D
    nsp = D - 1 if family == 'relationship' else D
    gathered = variant in ('permuted', 'site_twice')
    npool = (2 * N if gathered else N) + M
    x, y, var, log_ls = FR._draw(N, nsp, npool, seed=1 if gathered else 0)
    rng = np.random.RandomState(N + D + p)
    if family == 'relationship':
        x = np.c_[x, rng.randint(0, TA.NGEN, len(x)).astype(np.float64)]
    idx, cand = np.arange(N), np.arange(N, N + M)
    if gathered:
        x = x[rng.permutation(npool)]
        order = rng.permutation(npool)
        idx, cand = order[:N], order[N:N + M]
    sites = None
    if variant == 'site_twice':
        idx[64 + int(np.argmax(var[64:]))] = idx[int(np.argmax(var[:64]))]
        sites = idx
    mean = 0.3 if variant == 'mean_given' else None
    H = RM.basis(x[:, :nsp], p)
    beta = RM.planted_beta(p)
    y = y + H[idx] @ beta
    theta = AI.pack(log_ls, TA.LOG_OS if family == 'single' else TA.TWO_PART_LOG_OS.get(model, (TA.LOG_OS, TA.LOG_OS2)), TA.LOG_NOISE)
    ev = np.linalg.eigvalsh(AI.train_matrix(family, spec, theta, x[idx], var, sites))
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e3, 'the inputs are worse conditioned than the tolerances were set for'
    assert RM.scaled_cond(RM.gram(family, spec, theta, x[idx], H[idx], var, sites)) <= 1e2, 'the basis is worse conditioned than the tolerances were set for'
    args = (family, spec, theta, x[idx], y, H[idx])
    b, cov = RM.gls(*args, var, sites, mean)
    post = RM.posterior_fixed(*args, x[cand], H[cand], var, sites, mean)
    known = RM.posterior_known_mean(family, spec, theta, x[idx], y, x[cand], var, sites, mean)
    want = dict(beta=b, cov=cov, reml=RM.reml(*args, var, sites, mean), mu=post['mu'], var=post['var'], proj=post['proj'],
                var_known=np.diag(known[1]).copy(), grad=RM.reml_grad(*args, var, sites, mean), ai=RM.reml_ai(*args, var, sites, mean))
    for a in (x, y, var, idx, cand, theta, H) + tuple(want[k] for k in ('beta', 'cov', 'mu', 'var', 'proj', 'var_known', 'grad', 'ai')):
        a.setflags(write=False)
    return dict(model=model, family=family, spec=spec, theta=theta, x=x, y=y, var=var, idx=idx, cand=cand, mean=mean, H=H, p=p,
                planted=beta, want=want)


@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in (np.float64, np.float32)}
    yield c
    for v in c.values():
        v.close()
    for (dt, model), e in sorted(WORST.items()):
        print('\nmax error vs the forms  %s %-17s %s' % (dt, model, '  '.join('%s %.1e' % kv for kv in sorted(e.items()))))


def _load(c, case, solve=True):
    c.set_constant_mean(case['mean'])
    TA._set_hypers(c, case)
    c.set_pool(case['x'])
    c.set_fixed_effects(case['H'])
    c.set_train(case['idx'], case['y'], case['var'])
    c.factorize()
    if solve:
        c.set_candidates(case['cand'], prior_includes_noise=False)
        c.solve_candidates()


def _vec_err(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / max(1.0, float(np.max(np.abs(want)))))


def _errors(c, case):
    """Every quantity's error against the reference, printed; the outputs."""
    want, p, M = case['want'], case['p'], len(case['cand'])
    beta, cov, reml = c.gls()
    grad, ai = c.reml_grad(), c.reml_ai()
    P = len(case['theta'])
    assert grad.shape == (P,) and ai.shape == (P, P) and np.all(np.isfinite(grad)) and np.all(np.isfinite(ai))
    mu, var, proj = c.posterior_fixed(want_var=True, want_proj=True)
    assert beta.shape == (p,) and cov.shape == (p, p) and mu.shape == (M,) and var.shape == (M,) and proj.shape == (M, p)
    assert all(np.all(np.isfinite(a)) for a in (beta, cov, mu, var, proj)) and np.isfinite(reml)
    err = dict(beta=_vec_err(beta, want['beta']), cov=TA._error(cov, want['cov']), mu=_vec_err(mu, want['mu']),
               var=_vec_err(var, want['var']), proj=_vec_err(proj, want['proj']), reml=abs(reml - want['reml']) / abs(want['reml']),
               grad=_vec_err(grad, want['grad']), ai=TA._error(ai, want['ai']))
    w = WORST.setdefault((c.dtype.name, case['model']), {})
    for k, v in err.items():
        w[k] = max(w.get(k, 0.0), v)
    print('%s %s N=%d p=%d M=%d: %s' % (c.dtype.name, case['model'], len(case['idx']), p, M,
                                       '  '.join('%s %.2e' % kv for kv in sorted(err.items()))))
    return err, (beta, cov, reml, mu, var, proj, grad, ai)


def _check(c, case):
    err, out = _errors(c, case)
    for k in ('beta', 'cov', 'mu', 'var', 'proj'):
        assert err[k] <= TOL[c.dtype], (k, err)
    assert err['reml'] <= TOL_REML[c.dtype], err
    assert err['grad'] <= FR.TOL[c.dtype] and err['ai'] <= FR.TOL[c.dtype], err
    assert np.array_equal(out[1], out[1].T) and np.array_equal(out[7], out[7].T)
    ev = np.linalg.eigvalsh(out[7])
    assert ev[0] >= -FR.TOL[c.dtype] * ev[-1]
    # the universal-kriging term is there: never below the known-mean variance, and far above rounding somewhere
    assert np.all(out[4] >= c.posterior()[1] * (1 - 1e-6) - 1e-6)
    return out


def _run(ctxs, dtype, case):
    c = ctxs[np.dtype(dtype)]
    try:
        _load(c, case)
        return _check(c, case)
    finally:
        c.set_constant_mean(None)
        c.set_fixed_effects(None)


SIZES = [(2, 1), (4, 3), (63, 3), (64, 16), (65, 3), (127, 16), (128, 3), (129, 16), (513, 3), (513, 16), (897, 16), (1025, 3), (1025, 16)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,p', SIZES, ids=['N%d-p%d' % s for s in SIZES])
def test_every_size_at_which_a_stage_changes_path(ctxs, dtype, N, p):
    _run(ctxs, dtype, _case('matern' if N % 2 else 'rbf', N, p))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('p', [1, 3, 15, 16])
def test_every_basis_width(ctxs, dtype, p):
    _run(ctxs, dtype, _case('rbf', 129, p))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('M', [1, 15, 16, 17, 63, 64, 65, 127, 129, 300])
def test_every_candidate_count(ctxs, dtype, M):
    _run(ctxs, dtype, _case('matern', 129, 3, M=M))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', [1, 3, 5, 8])
def test_every_coordinate_width(ctxs, dtype, D):
    _run(ctxs, dtype, _case('rbf', 129, 3, D))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', sorted(TA.MODELS))
def test_every_kernel_form(ctxs, dtype, model):
    _run(ctxs, dtype, _case(model, 129, 16))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model,variant', [('rbf', 'permuted'), ('matern', 'site_twice'), ('rel_table', 'site_twice'), ('rbf', 'mean_given')])
def test_train_set_gathered_from_a_larger_pool(ctxs, dtype, model, variant):
    _run(ctxs, dtype, _case(model, 129, 16, 2, variant))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model,N', [('rbf', 129), ('matern', 513), ('rel_table', 129), ('rbf', 1025)])
def test_reml_step_is_the_three_separate_calls(ctxs, dtype, model, N):
    """reml_step against factorize + gls + reml_grad: the same launches below test_fit_regimes.PANEL_FROM rows and so the same
    bits; from there on X = L^-T and S^-1 come out of the factorisation's launch and the two agree to rounding
    (test_average_information.py's bounds between its two routes: 1e-10 | 2e-3)."""
    case = _case(model, N, 16)
    c = ctxs[np.dtype(dtype)]
    try:
        _load(c, case, solve=False)
        value, grad = c.gls()[2], c.reml_grad()
        v2, g2 = c.reml_step()
        g3 = c.reml_grad()                                         # the state it leaves serves the separate call (from
        tol = 1e-10 if c.dtype == np.float64 else 2e-3             # PANEL_FROM on its z is the launch's own: to rounding)
        assert np.array_equal(g3, grad) if N < FR.PANEL_FROM else _vec_err(g3, grad) <= tol
        v3, _ = c.reml_step(want_grad=False)
        print('%s %s N=%d: l_R separate %.12f step %.12f step without gradient %.12f reference %.12f' %
              (c.dtype.name, model, N, value, v2, v3, case['want']['reml']))
        if N < FR.PANEL_FROM:
            assert v2 == value and v3 == value and np.array_equal(g2, grad)
        else:
            assert abs(v2 - value) <= tol * abs(value) and abs(v3 - value) <= tol * abs(value) and _vec_err(g2, grad) <= tol
        assert _vec_err(g2, case['want']['grad']) <= FR.TOL[c.dtype]
        assert abs(v2 - case['want']['reml']) <= TOL_REML[c.dtype] * abs(case['want']['reml'])
    finally:
        c.set_fixed_effects(None)


def test_the_variance_term_is_no_rounding_matter():
    """On these inputs the term a read-out without fixed effects drops is far above every bound of this file."""
    want = _case('rbf', 129, 16)['want']
    assert np.max(want['var'] - want['var_known']) >= 1e-2


@pytest.mark.parametrize('dtype', DTYPES)
def test_estimates_cover_the_planted_effects(ctxs, dtype):
    """The block indicators and quadratic terms are no part of sin(x_0): their estimates lie within 4 standard errors."""
    case = _case('rbf', 513, 16)
    beta, cov = _run(ctxs, dtype, case)[:2]
    se = np.sqrt(np.diag(cov))
    assert np.all(np.abs(beta - case['planted'])[3:] <= 4.0 * se[3:])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('model', ['matern', 'rel_table'])
def test_nothing_else_moves(ctxs, dtype, model):
    """alpha, log det, the gradient and the AI matrix; a resident candidate solve (posterior, then two committed picks and the
    scores); the device bytes and the synchronisation count of a repeated call; the same bits twice."""
    case = _case(model, 513, 16, 2, 'permuted')
    c = ctxs[np.dtype(dtype)]
    try:
        _load(c, case)
        state = lambda: (c.alpha(), np.float64(c.logdet()), c.mll_grad(), c.mll_ai(), *c.posterior())
        before = state()
        out = _check(c, case)
        for u, v in zip(before, state()):
            assert np.array_equal(u, v)
        nbytes, nsync = c.device_bytes(), c.sync_count()
        again = c.gls()
        assert c.sync_count() == nsync + 1
        post = c.posterior_fixed(want_var=True, want_proj=True)
        assert c.sync_count() == nsync + 2
        fit = (c.reml_grad(), c.reml_ai())
        assert c.device_bytes() == nbytes and c.sync_count() == nsync + 4
        for u, v in zip(out, again + post + fit):
            assert np.array_equal(u, v)
        for u, v in zip(before, state()):
            assert np.array_equal(u, v)
        # picks committed since the solve: refused as algp_get_posterior_cov refuses, nothing moved; a fresh solve serves again
        c.set_candidates(case['cand'], prior_includes_noise=True)
        c.solve_candidates()
        c.commit_pick(int(case['cand'][3]), 0.1, 1.0)
        c.commit_pick(int(case['cand'][17]), 0.1, 1.0)
        picked = lambda: (*c.posterior(), c.scores(_hip.CRIT_ENTROPY, 0.1, 1.0))
        held = picked()
        with pytest.raises(ValueError, match='pick'):
            c.posterior_fixed()
        assert np.array_equal(c.gls()[0], out[0])
        for u, v in zip(held, picked()):
            assert np.array_equal(u, v)
    finally:
        c.set_fixed_effects(None)


@pytest.mark.parametrize('dtype', DTYPES)
def test_refusals_leave_the_context_usable(dtype):
    case = _case('rbf', 65, 3)
    c = _hip.Context(dtype)
    try:
        TA._set_hypers(c, case)
        H = np.array(case['H'])
        with pytest.raises(ValueError, match='pool'):
            c.set_fixed_effects(H)                                       # no pool yet
        c.set_pool(case['x'])
        c.set_train(case['idx'], case['y'], case['var'])
        c.factorize()
        c.set_candidates(case['cand'], prior_includes_noise=False)
        c.solve_candidates()
        for call in (c.gls, c.posterior_fixed, c.reml_grad, c.reml_ai, c.reml_step):   # no basis attached
            with pytest.raises(ValueError, match='fixed effects'):
                call()
        with pytest.raises(ValueError):
            c.set_fixed_effects(H[:-1])                                  # rows != n_pool
        with pytest.raises(ValueError):
            c.set_fixed_effects(np.ones((len(H), 17)))                   # p > 16
        bad = H.copy()
        bad[5, 1] = np.inf
        with pytest.raises(ValueError, match='finite'):
            c.set_fixed_effects(bad)
        c.set_fixed_effects(H)
        assert _vec_err(c.gls()[0], case['want']['beta']) <= TOL[c.dtype]
        beta = np.empty(3)
        assert c.lib.algp_get_gls(c.h, None, None, None) == _hip.ERR_BAD_ARG
        # a duplicated column: NOT_PD naming it (1-based)
        c.set_fixed_effects(np.c_[H, H[:, 1]])
        with pytest.raises(np.linalg.LinAlgError) as e:
            c.gls()
        assert e.value.pivot == 4 and 'column 4' in str(e.value)
        with pytest.raises(np.linalg.LinAlgError) as e:
            c.posterior_fixed()
        assert e.value.pivot == 4
        # more effects than train rows can determine
        c.set_fixed_effects(H)
        c.set_train(case['idx'][:3], case['y'][:3], case['var'][:3])
        c.factorize()
        with pytest.raises(ValueError, match='determine'):
            c.gls()
        c.set_train(case['idx'], case['y'], case['var'])
        with pytest.raises(ValueError, match='factorize'):
            c.gls()                                                      # the factor is not current
        c.factorize()
        with pytest.raises(ValueError, match='solve_candidates'):
            c.posterior_fixed()                                          # a new factor: the solve is gone
        # a train site among the candidates under prior_includes_noise = 1 is a unit row
        c.set_candidates(np.r_[case['idx'][:2], case['cand']], prior_includes_noise=True)
        c.solve_candidates()
        with pytest.raises(ValueError, match='unit row'):
            c.posterior_fixed()
        c.set_candidates(case['cand'], prior_includes_noise=False)
        c.solve_candidates()
        assert _vec_err(c.posterior_fixed()[0], case['want']['mu']) <= TOL[c.dtype]
        assert c.lib.algp_get_gls(c.h, beta.ctypes.data_as(_hip._dblp), None, None) == _hip.OK
        # detaching restores the refusal; a new pool drops the basis
        c.set_fixed_effects(None)
        with pytest.raises(ValueError, match='fixed effects'):
            c.gls()
        c.set_fixed_effects(H)
        c.set_pool(case['x'])
        c.set_train(case['idx'], case['y'], case['var'])
        c.factorize()
        with pytest.raises(ValueError, match='fixed effects'):
            c.gls()
        # an explicit pool covariance carries a basis as well
        S = AI.train_matrix(case['family'], case['spec'], case['theta'], case['x'][case['idx']])
        c.set_pool_cov(S)
        c.set_fixed_effects(H[case['idx']])
        c.set_train(np.arange(len(S)), case['y'], case['var'])
        c.factorize()
        assert _vec_err(c.gls()[0], case['want']['beta']) <= TOL[c.dtype]
        for call in (c.reml_grad, c.reml_ai, c.reml_step):              # which has no coordinates to differentiate
            with pytest.raises(ValueError, match='coordinate pool'):
                call()
    finally:
        c.close()
