"""algp_sample_posterior and its Python surface: joint draws of the latent field at the candidates by pathwise conditioning.

The library draws no random numbers, so every test is a comparison with tests/pathwise_forms.py (NumPy fp64, independent of the
library; held to the posterior's moments by tests/test_pathwise_forms_host.py) on identical inputs, never with the library.
Inputs come from fixed seeds and are rounded to fp32-exact values, so both precisions see the same numbers; omega is drawn from
N(0, I) for every kernel (the ABI does not care about the distribution, and the cosine's argument stays below about 60).

Tolerance: the project's bars against the fp64 oracle on identical inputs, max|a - b| / max|b| <= 1e-5 in fp64
and <= 1e-3 in fp32.  A plain float32 NumPy run of the whole formula stays at <= 1e-5 of the fp64 one on these problems for
all four kernels (cond(S) between 8e1 and 9e2), so the fp32 bar has two orders of margin.

The problems (tests/pathwise_forms.py): a 24 x 24 unit grid, lengthscales (3, 3), os = 1, sigma_n^2 = 1e-2, N = 200 train sites
(Npad = 256, the last tile ragged), M = 300 candidates (Mpad = 384; 290 unsampled sites and 10 train sites under
prior_includes_noise = 0); the same on 576 random sites in 3 and 5 dimensions (DP = 4, 8)."""
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
import pathwise_forms as PF                          # noqa: E402
from algp_amd import _hip, utils                     # noqa: E402

pytestmark = pytest.mark.gpu

DT = [np.float64, np.float32]
DIDS = ['f64', 'f32']
BAR = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}
ENT, VRC = _hip.CRIT_ENTROPY, _hip.CRIT_VARIANCE_REDUCTION
S_STD, M_STD = 0.1, 1.0

kernels = pytest.mark.parametrize('kid', PF.KIDS, ids=PF.KNAMES)
dtypes = pytest.mark.parametrize('dt', DT, ids=DIDS)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def close(got, want, dt, what=''):
    e = relerr(got, want)
    print('%s relerr %.3g (bar %g)' % (what, e, BAR[np.dtype(dt)]))
    assert np.all(np.isfinite(got))
    assert e <= BAR[np.dtype(dt)], (what, e)


def context(dt, p, kid, cand=None, prior_noise=False, cov_pool=False, solve=True, A=None, src=None):
    c = _hip.Context(dt)
    c.set_hypers(p.log_ls, p.log_os, p.log_noise, kid)
    if cov_pool:
        c.set_pool_cov(MF.kernel_matrix(kid, p.log_ls, p.log_os, p.X) + np.exp(p.log_noise) * np.eye(len(p.X)))
    else:
        c.set_pool(p.X)
    if A is None:
        c.set_train(p.A, p.y, p.var)
    else:
        c.set_train(*A)
    if src is None:
        c.factorize()
    else:
        c.factorize_from(src)
    c.set_candidates(p.cand if cand is None else cand, prior_includes_noise=prior_noise)
    if solve:
        c.solve_candidates()
    return c


def problem(D):
    return PF.grid_problem() if D == 2 else PF.random_problem(D)


@functools.lru_cache(maxsize=None)
def feature_case(D, kid, F, S):
    """(omega, phase, weights, eps, the reference's draws), computed once and shared by both precisions."""
    p = problem(D)
    om, ph, W, eps = PF.draws(100 * kid + F + S + D, F, S, D, len(p.A))
    ref = PF.problem_draws(p, kid, F, S, weights=W, eps=eps, omega=om, phase=ph)
    for a in (om, ph, W, eps, ref):
        a.setflags(write=False)
    return om, ph, W, eps, ref


@functools.lru_cache(maxsize=None)
def values_case(kid, S):
    p = PF.grid_problem()
    prior = PF.exact_prior(p, kid, S, 300 + kid)
    eps = PF.f32(np.random.RandomState(400 + kid).standard_normal((S, len(p.A))))
    ref = PF.problem_draws(p, kid, 0, S, eps=eps, prior=prior)
    for a in (prior, eps, ref):
        a.setflags(write=False)
    return prior, eps, ref


# ---------------------------------------------------------------------------------------------------- 1. features mode
@kernels
@dtypes
@pytest.mark.parametrize('F,S', PF.FS, ids=['F1-S1', 'F100-S5', 'F257-S130'])
def test_features_mode(kid, dt, F, S):
    p = PF.grid_problem()
    om, ph, W, eps, ref = feature_case(2, kid, F, S)
    c = context(dt, p, kid)
    got = c.sample_posterior(eps, weights=W, omega=om, phase=ph)
    assert got.shape == (S, len(p.cand)) and got.dtype == np.dtype(dt)
    close(got, ref, dt, 'features kernel %d F %d S %d' % (kid, F, S))
    c.close()


@dtypes
@pytest.mark.parametrize('D,kid', [(3, MF.MATERN25), (5, MF.RBF)], ids=['D3-matern25', 'D5-rbf'])
def test_features_mode_wider_coordinates(D, kid, dt):
    p = PF.random_problem(D)
    F, S = PF.FS[-1]
    om, ph, W, eps, ref = feature_case(D, kid, F, S)
    c = context(dt, p, kid)
    close(c.sample_posterior(eps, weights=W, omega=om, phase=ph), ref, dt, 'features D %d' % D)
    c.close()


# ---------------------------------------------------------------------------------------------------- 2. values mode
@kernels
@dtypes
def test_values_mode_both_pool_kinds(kid, dt):
    """An exact prior draw chol(K_pool + 1e-10 I) xi on the coordinate pool and on the same pool handed over as an explicit
    covariance (sigma_n^2 on its diagonal): both equal the reference, and each other.  An explicit covariance takes
    prior_includes_noise = 1 only (algp_set_candidates), under which a train site is a unit row, so that context holds the 290
    unsampled candidates -- the first 290 columns of the coordinate pool's 300."""
    p = PF.grid_problem()
    S = 5
    prior, eps, ref = values_case(kid, S)
    a = context(dt, p, kid)
    b = context(dt, p, kid, cand=p.free, prior_noise=True, cov_pool=True)
    fa, fb = a.sample_posterior(eps, prior=prior), b.sample_posterior(eps, prior=prior)
    assert fa.shape == (S, 300) and fb.shape == (S, 290) and np.array_equal(p.cand[:290], p.free)
    close(fa, ref, dt, 'values, coordinates')
    close(fb, ref[:, :290], dt, 'values, explicit covariance')
    close(fb, fa[:, :290], dt, 'values, explicit covariance against coordinates')
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------- 3. mean recovery
@kernels
@dtypes
def test_zero_draws_give_the_posterior_mean(kid, dt):
    p = PF.grid_problem()
    F, S = 100, 5
    om, ph, _, _, _ = feature_case(2, kid, F, S)
    c = context(dt, p, kid)
    got = c.sample_posterior(np.zeros((S, len(p.A))), weights=np.zeros((S, F)), omega=om, phase=ph)
    mu = c.posterior(want_var=False)
    want = MF.posterior(kid, p.log_ls, p.log_os, p.log_noise, p.X[p.A], p.y, p.var, p.X[p.cand])[0]
    for s in range(S):
        close(got[s], mu, dt, 'row %d against algp_get_posterior' % s)
        close(got[s], want, dt, 'row %d against the reference' % s)
    c.close()


# ---------------------------------------------------------------------------------------------------- 4. state untouched
@dtypes
def test_state_untouched(dt):
    """Posterior, entropy scores, variance-reduction scores with the criterion's product resident: the same bits before and
    after a sampling call; a following greedy run returns what a context that never sampled returns."""
    p, kid = PF.grid_problem(), MF.MATERN15
    F, S = PF.FS[-1]
    om, ph, W, eps, _ = feature_case(2, kid, F, S)
    c = context(dt, p, kid, cand=p.free, prior_noise=True)
    fresh = context(dt, p, kid, cand=p.free, prior_noise=True)
    for x in (fresh, c):                                  # the two differ by the sampling calls alone
        mu0, v0 = x.posterior()
        e0 = x.scores(ENT, S_STD, M_STD)
        r0 = x.scores(VRC, S_STD, M_STD)                  # the criterion's sums are resident from here on
    got = c.sample_posterior(eps, weights=W, omega=om, phase=ph)
    assert got.shape == (S, len(p.free)) and np.all(np.isfinite(got))
    mu1, v1 = c.posterior()
    assert np.array_equal(mu0, mu1) and np.array_equal(v0, v1)
    assert np.array_equal(e0, c.scores(ENT, S_STD, M_STD))
    assert np.array_equal(r0, c.scores(VRC, S_STD, M_STD))
    c.sample_posterior(eps[:3], prior=np.zeros((3, len(p.X))))
    pk, ut = c.greedy(ENT, S_STD, M_STD, 3, want_utilities=True)
    pk2, ut2 = fresh.greedy(ENT, S_STD, M_STD, 3, want_utilities=True)
    assert np.array_equal(pk, pk2) and np.array_equal(ut, ut2)
    c.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------- 5. independence
@dtypes
def test_draws_are_independent_of_their_batch(dt):
    """130 draws in one call against the same draws in two calls of 65: equal to the bars (not bit for bit: the solve's route
    may depend on the row count)."""
    p, kid = PF.grid_problem(), MF.RBF
    F, S = PF.FS[-1]
    om, ph, W, eps, ref = feature_case(2, kid, F, S)
    c = context(dt, p, kid)
    one = c.sample_posterior(eps, weights=W, omega=om, phase=ph)
    two = np.vstack([c.sample_posterior(eps[h], weights=W[h], omega=om, phase=ph) for h in (slice(0, 65), slice(65, 130))])
    close(two, one, dt, 'two calls against one')
    close(two, ref, dt, 'two calls against the reference')
    c.close()


# ---------------------------------------------------------------------------------------------------- 6. shards
@dtypes
def test_shards(dt):
    """The candidate list split 137 + 163 over two contexts on the one card, the second taking the factor with
    algp_factorize_from: their rows, side by side, are the one-context result."""
    p, kid = PF.grid_problem(), MF.MATERN25
    F, S = PF.FS[-1]
    om, ph, W, eps, ref = feature_case(2, kid, F, S)
    whole = context(dt, p, kid)
    a = context(dt, p, kid, cand=p.cand[:137])
    b = context(dt, p, kid, cand=p.cand[137:], src=a)
    one = whole.sample_posterior(eps, weights=W, omega=om, phase=ph)
    parts = np.hstack([x.sample_posterior(eps, weights=W, omega=om, phase=ph) for x in (a, b)])
    assert parts.shape == one.shape
    close(parts, one, dt, 'shards against one context')
    close(parts, ref, dt, 'shards against the reference')
    for x in (whole, a, b):
        x.close()


# ---------------------------------------------------------------------------------------------------- 7. edges and refusals
def _raw(c, S, F, om, ph, W, prior, eps, out):
    dp = lambda a: None if a is None else a.ctypes.data_as(_hip._dblp)
    return c.lib.algp_sample_posterior(c.h, S, F, dp(om), dp(ph), dp(W), dp(prior), dp(eps), _hip._ptr(out))


def test_refusals_and_edges():
    p, kid, dt = PF.grid_problem(), MF.RBF, np.float64
    F, S = 100, 5
    om, ph, W, eps, ref = feature_case(2, kid, F, S)
    om, ph, W, eps = (np.ascontiguousarray(a) for a in (om, ph, W, eps))
    prior = np.zeros((S, len(p.X)))
    out = np.full((S, len(p.cand)), np.nan)
    good = (S, F, om, ph, W, None, eps, out)
    err = lambda c: c.lib.algp_last_error(c.h).decode()

    # no solve
    c = context(dt, p, kid, cand=p.free, prior_noise=True, solve=False)
    assert _raw(c, *good) == _hip.ERR_STATE
    c.solve_candidates()
    s0 = c.scores(ENT, S_STD, M_STD)

    def refused(code, args):
        before = out.copy()
        assert _raw(c, *args) == code, err(c)
        msg = err(c)
        assert np.array_equal(out, before, equal_nan=True)
        assert c.scores(ENT, S_STD, M_STD).tobytes() == s0.tobytes()       # the same bits (a unit row's utility may be NaN here)
        return msg

    # every bad combination of NULL and non-NULL, bad counts
    refused(_hip.ERR_BAD_ARG, (S, F, om, ph, W, prior, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, F, None, ph, W, None, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, F, om, None, W, None, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, F, om, ph, None, None, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, 0, None, None, None, None, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, 0, om, None, None, prior, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, 0, None, ph, None, prior, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, 0, None, None, W, prior, eps, out))
    refused(_hip.ERR_BAD_ARG, (0, F, om, ph, W, None, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, -1, om, ph, W, None, eps, out))
    refused(_hip.ERR_BAD_ARG, (S, F, om, ph, W, None, None, out))
    refused(_hip.ERR_BAD_ARG, (S, F, om, ph, W, None, eps, None))
    with pytest.raises(ValueError):
        c.sample_posterior(eps, weights=W, omega=om)
    with pytest.raises(ValueError):
        c.sample_posterior(eps, weights=W, omega=om, phase=ph, prior=prior)
    # one pick committed
    pick = c.greedy(ENT, S_STD, M_STD, 1)
    s0 = c.scores(ENT, S_STD, M_STD)
    assert 'pick' in refused(_hip.ERR_STATE, good) and len(pick) == 1
    c.close()

    # a unit row: a train-site candidate under prior_includes_noise = 1; the message names it
    c = context(dt, p, kid, prior_noise=True)
    s0 = c.scores(ENT, S_STD, M_STD)
    msg = refused(_hip.ERR_STATE, good)
    assert 'candidate 290 (pool index %d)' % p.cand[290] in msg and 'prior_includes_noise = 0' in msg
    with pytest.raises(ValueError, match='unit row'):
        c.sample_posterior(eps, weights=W, omega=om, phase=ph)
    c.close()

    # a train set with a repeated site
    A2 = (np.r_[p.A, p.A[:1]], np.r_[p.y, p.y[:1]], np.r_[p.var, p.var[:1]])
    c = context(dt, p, kid, cand=p.free, prior_noise=True, A=A2)
    s0 = c.scores(ENT, S_STD, M_STD)
    eps2 = np.zeros((S, len(p.A) + 1))
    assert 'more than one row' in refused(_hip.ERR_STATE, (S, F, om, ph, W, None, eps2, out))
    c.close()

    # features mode on an explicit covariance
    c = context(dt, p, kid, cand=p.free, prior_noise=True, cov_pool=True)
    s0 = c.scores(ENT, S_STD, M_STD)
    refused(_hip.ERR_BAD_ARG, good)
    c.close()

    # M = 0: OK, nothing written
    c = context(dt, p, kid, cand=np.zeros(0, np.int64))
    assert _raw(c, *good) == _hip.OK and np.all(np.isnan(out))
    assert c.sample_posterior(eps, weights=W, omega=om, phase=ph).shape == (S, 0)
    c.close()

    # N = 0 (a legal solve: tests/test_greedy_regimes.py picks from an empty train set): the prior draw
    empty = (np.zeros(0, np.int64), np.zeros(0), np.zeros(0))
    c = context(dt, p, kid, A=empty)
    got = c.sample_posterior(np.zeros((S, 0)), weights=W, omega=om, phase=ph)
    G = W @ PF.features(om, ph, p.X * np.exp(-p.log_ls)[None, :], 1.0).T
    close(got, G[:, p.cand], dt, 'empty train set, features')
    got = c.sample_posterior(np.zeros((S, 0)), prior=PF.f32(G))
    close(got, PF.f32(G)[:, p.cand], dt, 'empty train set, values')
    c.close()


# ---------------------------------------------------------------------------------------------------- 8. the Python surface
def _gp(p, kid, dt):
    import torch
    from algp_amd.models import GPR
    kp = {'type': 'rbf'} if kid == MF.RBF else {'type': 'matern', 'nu': MF.NU[kid]}
    gp = GPR(kernel_params=kp, max_iterations=0, dtype=dt)
    gp.reset(p.X[p.A], p.y, p.var)
    with torch.no_grad():
        gp.model.kernel_covar_module.base_kernel.log_lengthscale.copy_(torch.tensor(p.log_ls).reshape(1, 1, -1))
        gp.model.kernel_covar_module.log_outputscale.fill_(p.log_os)
        gp.likelihood.log_noise.fill_(p.log_noise)
    return gp


def _surface_reference(p, kid, test_x, y, var, S, F, seed):
    """The documented order of the draws: spectral_draws (z, c for Matern, phase), weights, eps."""
    rng = np.random.RandomState(seed)
    N = len(p.A)
    om, ph = utils.spectral_draws(kid, p.D, F, rng)
    W = rng.standard_normal((S, F))
    eps = rng.standard_normal((S, N))
    x = np.vstack([p.X[p.A], test_x])
    q = types.SimpleNamespace(X=x, A=np.arange(N), cand=np.arange(N, len(x)), y=y, var=var, log_ls=p.log_ls, log_os=p.log_os,
                              log_noise=p.log_noise)
    return PF.problem_draws(q, kid, F, S, weights=W, eps=eps, omega=om, phase=ph)


@dtypes
@pytest.mark.parametrize('kid', [MF.RBF, MF.MATERN25], ids=['rbf', 'matern25'])
def test_python_surface(kid, dt):
    p = PF.grid_problem()
    S, F = 7, 300
    test_x = p.X[p.free][:60]
    gp = _gp(p, kid, dt)
    want = _surface_reference(p, kid, test_x, p.y, p.var, S, F, 11)
    a = utils.posterior_samples(gp, p.X[p.A], p.y, test_x, p.var, n_samples=S, n_features=F, rng=11)
    assert a.shape == (S, 60) and a.dtype == np.dtype(dt)
    close(a, want, dt, 'utils.posterior_samples')
    b = gp.sample_posterior(test_x, n_samples=S, n_features=F, rng=np.random.RandomState(11))
    assert b.shape == (S, 60) and b.dtype == np.dtype(dt) and np.array_equal(a, b)        # reproducible under a seed
    other = gp.sample_posterior(test_x, n_samples=S, n_features=F, rng=12)
    assert other.shape == (S, 60) and not np.array_equal(a, other)
    assert gp.sample_posterior(test_x).shape == (1, 60)

    from algp_amd.agent import Agent
    ag = Agent.__new__(Agent)
    n = len(p.X)
    ag.env = types.SimpleNamespace(num_samples=n, X=p.X, test_X=test_x)
    ag.static_std, ag.mobile_std = 0.1, 1.0
    ag.static_data = [[] for _ in range(n)]
    ag.mobile_data = [[] for _ in range(n)]
    for i, yi in zip(p.A, p.y):
        ag.static_data[i].append(float(yi))
    ag.gp = gp
    ag._pool_key = ('x', 0)
    var = np.full(len(p.A), 0.1 ** 2)
    want = _surface_reference(p, kid, test_x, p.y, var, S, F, 13)
    d = ag.sample_posterior(n_samples=S, n_features=F, rng=13)
    assert d.shape == (S, 60) and d.dtype == np.dtype(dt) and ag._pool_key is None
    close(d, want, dt, 'Agent.sample_posterior')
    d2 = ag.sample_posterior(x=test_x[:9], n_samples=2, n_features=F, rng=13)
    assert d2.shape == (2, 9)
    assert np.array_equal(d, ag.sample_posterior(n_samples=S, n_features=F, rng=13))
    assert not np.array_equal(d, ag.sample_posterior(n_samples=S, n_features=F, rng=14))

    c = gp.ctx
    with pytest.raises(ValueError):
        c.sample_posterior(np.zeros((2, c.N + 1)), prior=np.zeros((2, c.n_pool)))
    with pytest.raises(ValueError):
        c.sample_posterior(np.zeros((2, c.N)), prior=np.zeros((3, c.n_pool)))
