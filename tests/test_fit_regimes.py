"""algp_fit_step and algp_factorize + algp_get_mll + algp_get_mll_grad (the device work of one Adam iteration of GPR.fit,
reference models.py:145-158) against the fp64 closed form O.mll_and_grad computed from the same fp64 inputs, for both
kernels and both dtypes, in

* every instantiation of mll_grad_kernel<T, DP> (fit.hip): D = 1, 2 (DP = 2), 3, 4 (DP = 4), 5, 8 (DP = 8) -- with D < DP the
  padded coordinate slots must add nothing, with D = DP the last slot must be summed;
* every size at which a stage takes another path: N = 1, 2; 63 | 64 | 65 and 128 | 129 (the 64 x 64 tiles of the pairwise
  reduction, whose block index comes from a sqrt); 512 | 513 (trinv_upper's column blocks); 640; 896 | 897 (below / from
  DAG_MIN_TILES = 8 tiles: the launch sequence / the identity panel with y - ybar as tile row Npad and alpha from
  upper_gemv_kernel); 1024 | 1025 (no padding rows / one row into the next tile); 1537;
* with NULL for either output (api_fit.hip: prow = Npad, no inv_out, no z_row), an index list that is a permutation into a
  larger pool, a site listed twice (r = 0 under Matern's sqrt), no per-site noise, a constant mean that is given;
* and the state a fit_step leaves behind: alpha, log det, a following candidate solve, new hyper-parameters.

Inputs (seeded per case): x ~ U(0, side)^D at the point density of test_fold.py's N = 1400 case, y = sin(x_0) + 0.1 randn,
var ~ U(0.005, 0.05), length-scales ~ U(0.8, 2.1), outputscale 0.9, noise 0.05; cond(S) <= 1e3 is asserted on the oracle's S
(a condition on the inputs).  Tolerances against the oracle are test_fold.py's: 1e-8 (fp64) and 2e-2 (fp32), the MLL relative
to |MLL|, the gradient elementwise relative to max(1, |want|).

Measured on an MI355X (largest error over the cases of this file, fit_step and the three calls alike):

    fp64  rbf     MLL 2.0e-15   gradient 2.0e-13        fp32  rbf     MLL 1.8e-06   gradient 7.5e-05
    fp64  matern  MLL 1.0e-15   gradient 1.8e-13        fp32  matern  MLL 1.1e-06   gradient 1.9e-04

A site listed twice: algp_set_train documents that the two rows' cross entry is C(i,i) = k(0) + sigma_n^2 (the likelihood
noise belongs to the site, var to the measurement), so the oracle is told which rows are one site (sites=).  Against an
oracle without that entry the device's MLL is 1.4e-3 .. 1.1e-1 of |MLL| away, by that model and not by rounding; with it the
log_noise entry of the gradient has those cross entries too.  The rows of one site lie in different 64-row tiles of the
reduction (site_twice) or all in its first, diagonal, tile (site_thrice_in_one_tile).
"""
import functools

import numpy as np
import pytest
from scipy.linalg import cho_solve

from algp_amd import _hip
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

OUTPUTSCALE, NOISE = 0.9, 0.05
PANEL_FROM = 897                                   # DAG_MIN_TILES = 8 tiles of 128: Npad = 1024
KERNELS = {'rbf': (_hip.KERNEL_RBF, O.KERNEL_RBF), 'matern': (_hip.KERNEL_MATERN15, O.KERNEL_MATERN15)}
DTYPES = [pytest.param(np.float64, id='f64'), pytest.param(np.float32, id='f32')]
TOL = {np.dtype(np.float64): 1e-8, np.dtype(np.float32): 2e-2}

SWEEP_N = [1, 2, 63, 64, 65, 128, 129, 512, 513, 640, 896, 897, 1024, 1025, 1537]
BOUNDARY_N = [65, 129, 513, 897, 1025]
OTHER_D = [1, 3, 4, 5, 8]
# D = 2 over the whole size list under both kernels; at the stage boundaries every other width as well, the kernel
# alternating so that each width and each boundary meets both
SWEEP = [(N, 2, k) for N in SWEEP_N for k in ('rbf', 'matern')] + \
        [(N, D, ('rbf', 'matern')[(i + j) % 2]) for i, N in enumerate(BOUNDARY_N) for j, D in enumerate(OTHER_D)]

WORST = {}                                         # (dtype, kernel) -> [mll error, gradient error]


def _side(N, D):
    return 2.0 * (N / 4.0) ** (1.0 / D) if D <= 2 else (27000.0 * N / 1400.0) ** (1.0 / D)


def _draw(N, D, pool=None, seed=0):
    """x (pool x D; the train sites are the first N unless the caller picks others), y, var, log length-scales."""
    rng = np.random.RandomState(100000 * seed + 10 * N + D)
    x = rng.uniform(0, _side(N, D), (N, D))
    y = np.sin(x[:, 0]) + 0.1 * rng.standard_normal(N)
    var = rng.uniform(0.005, 0.05, N)
    log_ls = np.log(rng.uniform(0.8, 2.1, D))
    if pool is not None and pool > N:
        x = np.vstack([x, rng.uniform(0, _side(N, D), (pool - N, D))])
    return x, y, var, log_ls


def _hyp(log_ls, kname):
    return O.Hypers(log_ls, np.log(OUTPUTSCALE), np.log(NOISE), KERNELS[kname][1])


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


def _oracle(hyp, x, y, var, mean=None, sites=None):
    """MLL and gradient of the whole train set (the oracle's are per point), alpha, log det; asserts cond(S) <= 1e3."""
    N = len(y)
    f0, go = O.mll_and_grad(hyp, x, y, var, mean=mean, sites=sites)
    S = O.kernel_matrix(hyp, x) + hyp.noise * O.same_site(sites, N) + (np.diag(var) if var is not None else 0.0)
    ev = np.linalg.eigvalsh(S)
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e3, 'the inputs are worse conditioned than the tolerances were set for'
    L = np.linalg.cholesky(S)
    alpha = cho_solve((L, True), y - (y.mean() if mean is None else mean))
    return _frozen(mll=f0 * N, grad=np.r_[go['log_lengthscale'], go['log_outputscale'], go['log_noise']] * N,
                   alpha=alpha, logdet=2.0 * float(np.sum(np.log(np.diag(L)))))


@functools.lru_cache(maxsize=None)
def _case(N, D, kname):
    """Inputs and oracle of a case whose train sites are the first N pool points: computed once, shared by both dtypes and
    by every test that uses the case, never written to."""
    x, y, var, log_ls = _draw(N, D)
    hyp = _hyp(log_ls, kname)
    return dict(_frozen(x=x, y=y, var=var, log_ls=log_ls), hyp=hyp, idx=np.arange(N), **_oracle(hyp, x, y, var))


@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in (np.float64, np.float32)}
    yield c
    for v in c.values():
        v.close()
    for (dt, kname), (em, eg) in sorted(WORST.items()):
        print('\nmax error vs oracle  %s %-6s  mll %.2e  grad %.2e' % (dt, kname, em, eg))


def _load(c, case, kname, idx=None, var='case', log_ls=None):
    c.set_hypers(case['log_ls'] if log_ls is None else log_ls, np.log(OUTPUTSCALE), np.log(NOISE), KERNELS[kname][0])
    c.set_pool(case['x'])
    c.set_train(case['idx'] if idx is None else idx, case['y'], case['var'] if isinstance(var, str) else var)


def _profiled(c, call):
    """call() with profiling on: (its result, launches of the one-launch task list with a panel)."""
    c.prof_enable(True)
    try:
        c.prof_reset()
        out = call()
        return out, c.prof_get('dag_panel')['launches']
    finally:
        c.prof_enable(False)


def _grad_err(g, want):
    return float(np.max(np.abs(g - want) / np.maximum(1.0, np.abs(want))))


def _against_oracle(c, kname, want, mll=None, g=None, what=''):
    tol = TOL[c.dtype]
    w = WORST.setdefault((c.dtype.name, kname), [0.0, 0.0])
    if mll is not None:
        em = abs(mll - want['mll']) / abs(want['mll'])
        w[0] = max(w[0], em)
        print('%s %s %s: mll error %.3e' % (c.dtype.name, kname, what, em))
        assert em <= tol, (what, mll, want['mll'])
    if g is not None:
        assert g.shape == want['grad'].shape
        eg = _grad_err(g, want['grad'])
        w[1] = max(w[1], eg)
        print('%s %s %s: grad error %.3e' % (c.dtype.name, kname, what, eg))
        assert eg <= tol, (what, g, want['grad'])


def _same_to_rounding(c, mll_a, g_a, mll_b, g_b):
    """test_fold.py's bounds between two device routes of the same products."""
    f64 = c.dtype == np.float64
    if mll_a is not None and mll_b is not None:
        assert abs(mll_a - mll_b) <= (1e-12 if f64 else 1e-6) * abs(mll_b)
    if g_a is not None and g_b is not None:
        assert np.max(np.abs(g_a - g_b) / np.maximum(1.0, np.abs(g_b))) <= (1e-10 if f64 else 2e-3)


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,D,kname', SWEEP, ids=['N%d-D%d-%s' % s for s in SWEEP])
def test_fit_step_and_the_three_calls_against_the_oracle(ctxs, dtype, N, D, kname):
    case = _case(N, D, kname)
    c = ctxs[np.dtype(dtype)]
    _load(c, case, kname)
    (mll, g), panels = _profiled(c, c.fit_step)
    assert panels == (1 if N >= PANEL_FROM else 0), 'fit_step took the other route'
    _against_oracle(c, kname, case, mll, g, 'fit_step')
    mll_b, g_b = c.fit_step()
    assert mll_b == mll and np.array_equal(g_b, g)                     # fixed-order reductions: the same bits
    c.factorize()
    mll3, g3 = c.mll(), c.mll_grad()
    _against_oracle(c, kname, case, mll3, g3, 'factorize + mll + mll_grad')
    _same_to_rounding(c, mll3, g3, mll, g)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kname', ['rbf', 'matern'])
@pytest.mark.parametrize('N', [129, 897, 1025])
def test_state_after_fit_step_serves_alpha_logdet_and_a_candidate_solve(ctxs, dtype, kname, N):
    """On the panel route alpha = X z comes from upper_gemv_kernel, not from the backward substitution, and z from the
    panel's tile row: alpha, log det and the posterior of 40 further pool points (utils.py:293-319 as O.posterior_chol) at
    test_hip_kernels.py's bounds."""
    M = 40
    case = _case(N, 2, kname)
    case = dict(case, x=_draw(N, 2, N + M)[0])        # the same train sites, 40 more pool points behind them
    assert np.array_equal(case['x'][:N], _case(N, 2, kname)['x'])
    c = ctxs[np.dtype(dtype)]
    f64 = c.dtype == np.float64
    _load(c, case, kname)
    mll, g = c.fit_step()
    _against_oracle(c, kname, case, mll, g, 'fit_step')
    assert _relerr(c.alpha(), case['alpha']) < (1e-8 if f64 else 5e-2)
    t = 1e-9 if f64 else 1e-3
    assert c.logdet() == pytest.approx(case['logdet'], rel=t, abs=t)
    c.set_candidates(np.arange(N, N + M), prior_includes_noise=False)
    c.solve_candidates()
    mu, pv = c.posterior()
    ref = O.posterior_chol(case['hyp'], case['x'][:N], case['y'], case['x'][N:], case['var'])
    assert _relerr(mu, ref['mu']) < t and _relerr(pv, ref['var']) < t


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kname', ['rbf', 'matern'])
@pytest.mark.parametrize('N', [129, 897, 1024])
def test_fit_step_with_null_for_either_output(ctxs, dtype, kname, N):
    """algp_fit_step(ctx, mll, NULL) factors without the row that carries y - ybar and without S^-1;
    algp_fit_step(ctx, NULL, grad) skips nothing but the MLL's store.  After the MLL-only call the gradient and alpha are
    still to be had from the factor it left."""
    case = _case(N, 2, kname)
    c = ctxs[np.dtype(dtype)]
    f64 = c.dtype == np.float64
    _load(c, case, kname)
    mll, g = c.fit_step()
    (mll_only, none), panels = _profiled(c, lambda: c.fit_step(want_grad=False))
    assert none is None and panels == (1 if N >= PANEL_FROM else 0)
    _against_oracle(c, kname, case, mll=mll_only, what='fit_step(mll, NULL)')
    _same_to_rounding(c, mll_only, None, mll, None)
    g_after = c.mll_grad()
    _against_oracle(c, kname, case, g=g_after, what='mll_grad after fit_step(mll, NULL)')
    assert _relerr(c.alpha(), case['alpha']) < (1e-8 if f64 else 5e-2)
    (none, g_only), panels = _profiled(c, lambda: c.fit_step(want_mll=False))
    assert none is None and panels == (1 if N >= PANEL_FROM else 0)
    _against_oracle(c, kname, case, g=g_only, what='fit_step(NULL, grad)')
    _same_to_rounding(c, None, g_only, None, g)


@functools.lru_cache(maxsize=None)
def _gather_case(N, D, kname, variant):
    """A pool of 2 N points of which N, in random order, are the train set.  'site_twice': one of them is listed a second
    time (in another 64-row tile, under its own noise); 'site_thrice_in_one_tile': one is listed three times within the first
    64 rows; 'no_var': no per-site noise; 'mean_given': constant mean 0.3.
    The oracle runs on x[idx].  Where a site repeats it is told which rows are one site: algp_set_train documents that their
    cross entry is C(i,i) = k(0) + sigma_n^2 -- the likelihood noise belongs to the site -- so dS/dlog sigma_n^2 has that
    entry as well.  (Without it the oracle's MLL is another model's: 1e-3 .. 1e-1 of |MLL| away on these inputs.)"""
    x, y, var, log_ls = _draw(N, D, 2 * N, seed=1)
    rng = np.random.RandomState(N + D)
    x = x[rng.permutation(2 * N)]                     # the pool, shuffled: its density is that of 2 N points in N's box,
    idx = rng.permutation(2 * N)[:N]                  # the train set's that of N
    if variant == 'site_twice':
        # the noisiest row of the reduction's first 64-row tile and the noisiest of the others: the difference of the two rows
        # is close to an eigenvector of S with eigenvalue (var_i + var_j) / 2, which has to stay inside cond(S) <= 1e3
        idx[64 + int(np.argmax(var[64:]))] = idx[int(np.argmax(var[:64]))]
    if variant == 'site_thrice_in_one_tile':
        # three rows of the first tile (its three noisiest, for the same reason): their pairs lie inside a diagonal tile of the
        # reduction, beside the j > i skip and the i == j entry
        a, b, c3 = np.argsort(var[:64])[-3:]
        idx[b] = idx[c3] = idx[a]
    if variant == 'no_var':
        var = None
    mean = 0.3 if variant == 'mean_given' else None
    hyp = _hyp(log_ls, kname)
    return dict(_frozen(x=x, y=y, log_ls=log_ls, idx=idx), var=var, hyp=hyp, mean=mean,
                **_oracle(hyp, x[idx], y, var, mean, sites=idx if variant.startswith('site_') else None))


GATHER = [(N, D, k, v) for N in (65, 897) for D in (2, 5) for k in ('rbf', 'matern') for v in ('permuted', 'site_twice')] + \
         [(65, 2, 'rbf', 'site_thrice_in_one_tile'), (65, 2, 'matern', 'site_thrice_in_one_tile'),
          (897, 5, 'rbf', 'site_thrice_in_one_tile'), (897, 2, 'matern', 'no_var'), (897, 5, 'rbf', 'mean_given')]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,D,kname,variant', GATHER, ids=['N%d-D%d-%s-%s' % s for s in GATHER])
def test_train_set_gathered_from_a_larger_pool(ctxs, dtype, N, D, kname, variant):
    case = _gather_case(N, D, kname, variant)
    c = ctxs[np.dtype(dtype)]
    c.set_constant_mean(case['mean'])
    try:
        _load(c, case, kname, var=case['var'])
        mll, g = c.fit_step()
        _against_oracle(c, kname, case, mll, g, 'fit_step, ' + variant)
        c.factorize()
        mll3, g3 = c.mll(), c.mll_grad()
        _against_oracle(c, kname, case, mll3, g3, 'three calls, ' + variant)
        _same_to_rounding(c, mll3, g3, mll, g)
        assert _relerr(c.alpha(), case['alpha']) < (1e-8 if c.dtype == np.float64 else 5e-2)
    finally:
        c.set_constant_mean(None)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kname', ['rbf', 'matern'])
@pytest.mark.parametrize('N', [129, 897])
def test_fit_step_after_new_hyperparameters_equals_a_fresh_context(dtype, kname, N):
    """set_hypers between two fit_steps: the second one equals the oracle at the new values and, bit for bit, a context that
    was given them from the start (the scaled coordinates, the factor, z and alpha all belong to the old values)."""
    case = _case(N, 2, kname)
    new_ls = np.log(np.random.RandomState(N).uniform(0.8, 2.1, 2))
    assert np.min(np.abs(new_ls - case['log_ls'])) > 1e-3
    want = _oracle(_hyp(new_ls, kname), case['x'], case['y'], case['var'])
    a, b = _hip.Context(dtype), _hip.Context(dtype)
    try:
        _load(a, case, kname)
        _against_oracle(a, kname, case, *a.fit_step(), what='fit_step at the first values')
        a.set_hypers(new_ls, np.log(OUTPUTSCALE), np.log(NOISE), KERNELS[kname][0])
        mll_a, g_a = a.fit_step()
        _against_oracle(a, kname, want, mll_a, g_a, 'fit_step after set_hypers')
        _load(b, case, kname, log_ls=new_ls)
        mll_b, g_b = b.fit_step()
        assert mll_a == mll_b and np.array_equal(g_a, g_b)
        assert np.array_equal(a.alpha(), b.alpha()) and a.logdet() == b.logdet()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('dtype', DTYPES)
def test_refusals_and_the_empty_train_set(dtype):
    x, y, var, log_ls = _draw(20, 2)
    c = _hip.Context(dtype)
    try:
        out, g = _hip.C.c_double(), np.full(4, np.nan)
        step = lambda: c.lib.algp_fit_step(c.h, _hip.C.byref(out), g.ctypes.data_as(_hip._dblp))
        c.set_hypers(log_ls, np.log(OUTPUTSCALE), np.log(NOISE))
        c.set_pool(x)
        assert step() == _hip.ERR_STATE                                 # no train set yet
        assert b'set_train' in c.lib.algp_last_error(c.h)
        # an empty train set is legal (algp_factorize: 0 x 0 slogdet = 0): MLL = 0 and a zero gradient, on either route's
        # branch (the identity panel is never asked for), with either output NULL as well
        c.set_train(np.zeros(0, np.int64), np.zeros(0))
        assert step() == _hip.OK
        assert out.value == 0.0 and np.array_equal(g, np.zeros(4))
        assert c.fit_step(want_grad=False) == (0.0, None)
        none, g0 = c.fit_step(want_mll=False)
        assert none is None and np.array_equal(g0, np.zeros(4))
        assert c.mll() == 0.0 and np.array_equal(c.mll_grad(), np.zeros(4)) and c.logdet() == 0.0
        # an explicit covariance has no coordinates to differentiate
        S = O.kernel_matrix(_hyp(log_ls, 'rbf'), x) + NOISE * np.eye(20)
        c.set_pool_cov(S)
        c.set_train(np.arange(20), y, var)
        assert step() == _hip.ERR_BAD_ARG
        assert b'coordinate pool' in c.lib.algp_last_error(c.h)
        c.factorize()                                                   # the pool itself is fine
        assert c.logdet() == pytest.approx(np.linalg.slogdet(S + np.diag(var))[1], rel=1e-9 if c.dtype == np.float64 else 1e-3)
    finally:
        c.close()
