"""algp_group_posterior and its Python surface: the joint posterior of group aggregates g_q = sum_{j in q} a_j f(x_j).

Every comparison is with tests/group_forms.py (NumPy fp64, independent of the library; held to the oracle by
tests/test_group_forms_host.py) on identical inputs, never with the library, except where a test says so.  Inputs come from
fixed seeds and are rounded to fp32-exact values, so both precisions see the same numbers.

Tolerance: the project's bars against the fp64 oracle on identical inputs, max|a - b| / max|b| <= 1e-5 in fp64
and <= 1e-3 in fp32, applied to the mean, to cov and to cross separately.  The whole formula in plain float32 NumPy on exactly
these problems (24 x 24 grid; 576 random sites in 3 and 5 dimensions; M = 300, N = 200; the three groupings, all four kernels,
cond(S) between 5e1 and 2.4e3) stays within 4.7e-5 of fp64 (worst: cross, RBF, D = 3), so the fp32 bar has a factor 20 of margin
and the fp64 bar is not in question; on the explicit-weights problem (64 x 64 grid, M = 2 600, N = 300) plain float32 NumPy
stays within 1.4e-6.

The problems: tests/pathwise_forms.py (M = 300, Mpad = 384, N = 200, the last tile ragged; 10 candidates are train sites under
prior_includes_noise = 0) and tests/group_forms.py (the groupings; the 64 x 64 grid; the duplicated candidates)."""
import functools
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import group_forms as GF                             # noqa: E402
import matern_forms as MF                            # noqa: E402
import pathwise_forms as PF                          # noqa: E402
from algp_amd import _hip, utils                     # noqa: E402

pytestmark = pytest.mark.gpu

DT = [np.float64, np.float32]
DIDS = ['f64', 'f32']
BAR = {np.dtype(np.float64): 1e-5, np.dtype(np.float32): 1e-3}
ENT = _hip.CRIT_ENTROPY
S_STD, M_STD = 0.1, 1.0

kernels = pytest.mark.parametrize('kid', GF.KIDS, ids=GF.KNAMES)
dtypes = pytest.mark.parametrize('dt', DT, ids=DIDS)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def close(got, want, dt, what=''):
    e = relerr(got, want)
    print('%s relerr %.3g (bar %g)' % (what, e, BAR[np.dtype(dt)]))
    assert got.shape == want.shape and got.dtype == np.dtype(dt), what
    assert np.all(np.isfinite(got))
    assert e <= BAR[np.dtype(dt)], (what, e)


def context(dt, p, kid, prior_noise=False, cov_pool=False, solve=True, cand=None):
    c = _hip.Context(dt)
    c.set_hypers(p.log_ls, p.log_os, p.log_noise, kid)
    if cov_pool:
        c.set_pool_cov(MF.kernel_matrix(kid, p.log_ls, p.log_os, p.X) + np.exp(p.log_noise) * np.eye(len(p.X)))
    else:
        c.set_pool(p.X)
    c.set_train(p.A, p.y, p.var)
    c.factorize()
    if cand is None:
        cand = p.free if cov_pool else p.cand
    c.set_candidates(cand, prior_includes_noise=prior_noise, extra_var=getattr(p, 'extra', None))
    if solve:
        c.solve_candidates()
    return c


PROBLEMS = {'grid': PF.grid_problem, 'random3': lambda: PF.random_problem(3), 'random5': lambda: PF.random_problem(5),
            'big': GF.big_problem, 'duplicates': GF.duplicate_problem}


@functools.lru_cache(maxsize=None)
def moments(name, kid):
    """(mu, Sigma) of a problem, computed once and shared by every case on it."""
    mu, Sigma = GF.problem_moments(PROBLEMS[name](), kid)
    mu.setflags(write=False)
    Sigma.setflags(write=False)
    return mu, Sigma


def want(name, kid, lab, weight, Q):
    mu, Sigma = moments(name, kid)
    return GF.aggregates(mu, Sigma, GF.coefficients(lab, weight, Q))


def check_both_routes(c, dt, ref, lab, weight, Q, what):
    """mean, cov and cross of a call with cross_out, and cov again from a call without (the route without the big product)."""
    mean, cov, cross = c.group_posterior(lab, weight=weight, n_groups=Q, want_cov=True, want_cross=True)
    close(mean, ref[0], dt, what + ' mean')
    close(cov, ref[1], dt, what + ' cov')
    close(cross, ref[2], dt, what + ' cross')
    mean2, cov2, none = c.group_posterior(lab, weight=weight, n_groups=Q)
    assert none is None and np.array_equal(mean, mean2)
    close(cov2, ref[1], dt, what + ' cov without cross')
    for m in (cov, cov2):
        assert np.array_equal(m, m.T)
    return mean, cov, cross


# ---------------------------------------------------------------------------------------------------- 1. the three groupings
@kernels
@dtypes
@pytest.mark.parametrize('which', GF.GROUPINGS)
def test_groupings(kid, dt, which):
    p = PF.grid_problem()
    lab, Q = GF.grouping(which)
    c = context(dt, p, kid)
    check_both_routes(c, dt, want('grid', kid, lab, None, Q), lab, None, Q, 'grouping %s kernel %d' % (which, kid))
    c.close()


# ---------------------------------------------------------------------------------------------------- 2. wider coordinates
@dtypes
@pytest.mark.parametrize('D,kid', [(3, MF.MATERN25), (5, MF.RBF)], ids=['D3-matern25', 'D5-rbf'])
def test_wider_coordinates(D, kid, dt):
    lab, Q = GF.grouping('a')
    c = context(dt, PF.random_problem(D), kid)
    check_both_routes(c, dt, want('random%d' % D, kid, lab, None, Q), lab, None, Q, 'D %d' % D)
    c.close()


# ---------------------------------------------------------------------------------------------------- 3. explicit weights
@dtypes
@pytest.mark.parametrize('kid', [MF.RBF, MF.MATERN05], ids=['rbf', 'matern05'])
def test_explicit_weights(kid, dt):
    """M = 2 600: several row blocks, several chunks of the member list with groups that span them; signed weights, labelled
    rows at 0, and an empty group, which is the zero functional."""
    lab, w, Q = GF.weighted_grouping()
    c = context(dt, GF.big_problem(), kid)
    mean, cov, cross = check_both_routes(c, dt, want('big', kid, lab, w, Q), lab, w, Q, 'weights kernel %d' % kid)
    e = GF.EMPTY_W
    assert mean[e] == 0 and not cov[e].any() and not cov[:, e].any() and not cross[e].any()
    c.close()


@dtypes
def test_one_group_of_every_row_of_the_large_problem(dt):
    """One group of all 2 600 rows: it fills whole chunks of the member list (a piece that neither starts nor ends in its
    chunk), which no other case does."""
    kid = MF.RBF
    lab = np.zeros(2600, np.int32)
    c = context(dt, GF.big_problem(), kid)
    check_both_routes(c, dt, want('big', kid, lab, None, 1), lab, None, 1, 'one group of 2600')
    c.close()


# ---------------------------------------------------------------------------------------------------- 4. extra_var, duplicates
@dtypes
@pytest.mark.parametrize('kid', [MF.RBF, MF.MATERN15], ids=['rbf', 'matern15'])
def test_extra_var_and_duplicate_sites(kid, dt):
    """cov = A (K + diag(extra) - ...) A^T: the extra variance is per row, two rows of one site are fully correlated."""
    lab, Q = GF.grouping('a')
    c = context(dt, GF.duplicate_problem(), kid)
    check_both_routes(c, dt, want('duplicates', kid, lab, None, Q), lab, None, Q, 'duplicates kernel %d' % kid)
    c.close()


# ---------------------------------------------------------------------------------------------------- 5. library against library
@dtypes
def test_singletons_reproduce_the_posterior(dt):
    """300 singleton groups: the mean is posterior()'s, cov and cross are posterior_cov()'s matrix (library against library,
    at the same bars), also with explicit unit weights."""
    p, kid = GF.duplicate_problem(), MF.MATERN25
    M = len(p.cand)
    c = context(dt, p, kid)
    mu = c.posterior(want_var=False)
    Sigma, _ = c.posterior_cov()
    for weight in (None, np.ones(M)):
        mean, cov, cross = check_both_routes(c, dt, (mu, Sigma, Sigma), np.arange(M), weight, M, 'singletons')
        assert np.array_equal(mean, mu)
    close(cov, moments('duplicates', kid)[1], dt, 'singletons against the reference')
    c.close()


# ---------------------------------------------------------------------------------------------------- 6. bits
@dtypes
def test_bits(dt):
    """Two calls return identical arrays, cov is its own transpose, and the posterior and the entropy scores are the same bits
    before and after (the scores need greedy semantics: the 2 590 unsampled candidates under prior_includes_noise = 1)."""
    p, kid = GF.big_problem(), MF.MATERN15
    lab, w, Q = GF.weighted_grouping()
    lab, w = lab[:len(p.free)], w[:len(p.free)]
    c = context(dt, p, kid, prior_noise=True, cand=p.free)
    mu0, v0 = c.posterior()
    e0 = c.scores(ENT, S_STD, M_STD)
    one = c.group_posterior(lab, weight=w, n_groups=Q, want_cross=True)
    two = c.group_posterior(lab, weight=w, n_groups=Q, want_cross=True)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    assert np.array_equal(one[1], one[1].T)
    a = c.group_posterior(lab, weight=w, n_groups=Q)
    b = c.group_posterior(lab, weight=w, n_groups=Q)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], a[1].T) and np.array_equal(a[0], one[0])
    mu1, v1 = c.posterior()
    assert np.array_equal(mu0, mu1) and np.array_equal(v0, v1)
    assert e0.tobytes() == c.scores(ENT, S_STD, M_STD).tobytes()
    c.close()


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals():
    p, kid, dt = PF.grid_problem(), MF.RBF, np.float64
    lab, Q = GF.grouping('a')
    ref = want('grid', kid, lab, None, Q)
    M = len(p.cand)

    def answers(c):
        """after a refusal the context still answers case 1a (where its state allows an answer at all)"""
        check_both_routes(c, dt, ref, lab, None, Q, 'after a refusal')

    def refused(c, code, word, labels, weight=None, n_groups=None):
        """the ABI's code and message, then the binding's exception for the same call"""
        labels = np.ascontiguousarray(labels, np.int32)
        w = None if weight is None else np.ascontiguousarray(weight, np.float64)
        out = np.full(n_groups, np.nan)
        rc = c.lib.algp_group_posterior(c.h, labels.ctypes.data_as(_hip.C.POINTER(_hip.C.c_int32)),
                                        None if w is None else w.ctypes.data_as(_hip._dblp), n_groups, _hip._ptr(out), None, None)
        msg = c.lib.algp_last_error(c.h).decode()
        assert rc == code and word in msg, (rc, msg)
        assert np.all(np.isnan(out))
        with pytest.raises(ValueError, match=re.escape(word)):
            c.group_posterior(labels, weight=weight, n_groups=n_groups)

    # no solve
    c = context(dt, p, kid, solve=False)
    refused(c, _hip.ERR_STATE, 'solve', lab, n_groups=Q)
    c.solve_candidates()
    answers(c)
    # labels, weights, Q
    bad = lab.copy()
    bad[17] = Q
    refused(c, _hip.ERR_BAD_ARG, 'candidate 17', bad, n_groups=Q)
    answers(c)
    bad[17] = -2
    refused(c, _hip.ERR_BAD_ARG, 'candidate 17', bad, n_groups=Q)
    answers(c)
    w = np.ones(M)
    w[5] = np.nan
    refused(c, _hip.ERR_BAD_ARG, 'candidate 5', lab, weight=w, n_groups=Q)
    w[5] = np.inf
    refused(c, _hip.ERR_BAD_ARG, 'candidate 5', lab, weight=w, n_groups=Q)
    answers(c)
    mean = np.zeros(Q)
    assert c.lib.algp_group_posterior(c.h, lab.ctypes.data_as(_hip.C.POINTER(_hip.C.c_int32)), None, 0, _hip._ptr(mean), None,
                                      None) == _hip.ERR_BAD_ARG                                    # Q = 0, through the ABI
    assert c.lib.algp_group_posterior(c.h, None, None, Q, _hip._ptr(mean), None, None) == _hip.ERR_BAD_ARG
    with pytest.raises(ValueError):
        c.group_posterior(lab, n_groups=0)
    answers(c)
    refused(c, _hip.ERR_BAD_ARG, 'group 6', lab, n_groups=Q + 1)                                   # an empty group, weight = NULL
    answers(c)
    mean, cov, _ = c.group_posterior(lab, weight=np.ones(M), n_groups=Q + 1)                       # ... is fine with weights
    assert mean[Q] == 0 and not cov[Q].any() and not cov[:, Q].any()
    # shapes are checked before the call
    with pytest.raises(ValueError):
        c.group_posterior(lab[:-1], n_groups=Q)
    with pytest.raises(ValueError):
        c.group_posterior(lab, weight=np.ones(M + 1), n_groups=Q)
    with pytest.raises(ValueError):
        c.group_posterior(lab.astype(np.float64), n_groups=Q)
    c.close()

    # a committed pick (greedy semantics: the unsampled candidates under prior_includes_noise = 1)
    c = context(dt, p, kid, prior_noise=True, cand=p.free)
    c.group_posterior(lab[:290], n_groups=Q)
    assert len(c.greedy(ENT, S_STD, M_STD, 1)) == 1
    refused(c, _hip.ERR_STATE, 'pick', lab[:290], n_groups=Q)
    c.set_candidates(p.cand, prior_includes_noise=False)
    c.solve_candidates()
    answers(c)
    c.close()

    # a unit row: a train-site candidate under prior_includes_noise = 1; the message names it
    c = context(dt, p, kid, prior_noise=True)
    refused(c, _hip.ERR_STATE, 'candidate 290 (pool index %d)' % p.cand[290], lab, n_groups=Q)
    c.set_candidates(p.cand, prior_includes_noise=False)
    c.solve_candidates()
    answers(c)
    c.close()

    # an explicit-covariance pool
    c = context(dt, p, kid, prior_noise=True, cov_pool=True)
    refused(c, _hip.ERR_BAD_ARG, 'coordinate pool', lab[:290], n_groups=Q)
    c.set_pool(p.X)
    c.set_train(p.A, p.y, p.var)
    c.factorize()
    c.set_candidates(p.cand, prior_includes_noise=False)
    c.solve_candidates()
    answers(c)
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


@dtypes
@pytest.mark.parametrize('kid', [MF.RBF, MF.MATERN25], ids=['rbf', 'matern25'])
def test_python_surface(kid, dt):
    p = PF.grid_problem()
    lab, Q = GF.grouping('a')
    ref = want('grid', kid, lab, None, Q)
    gp = _gp(p, kid, dt)
    test_x = p.X[p.cand]
    mean, cov = utils.group_posterior(gp, p.X[p.A], p.y, test_x, lab, train_var=p.var)
    close(mean, ref[0], dt, 'utils mean')
    close(cov, ref[1], dt, 'utils cov')
    out = gp.group_posterior(test_x, lab, n_groups=Q, return_cross=True)
    assert len(out) == 3
    for got, r, what in zip(out, ref, ('mean', 'cov', 'cross')):
        close(got, r, dt, 'GPR ' + what)
    # weights and a per-row extra variance go through
    d = GF.duplicate_problem()
    w = GF.f32(np.random.RandomState(3).uniform(-1, 1, len(d.cand)))
    mu, Sigma = moments('duplicates', kid)
    refw = GF.aggregates(mu, Sigma, GF.coefficients(lab, w, Q))
    out = utils.group_posterior(gp, d.X[d.A], d.y, d.X[d.cand], lab, train_var=d.var, test_var=d.extra, weight=w, return_cross=True)
    for got, r, what in zip(out, refw, ('mean', 'cov', 'cross')):
        close(got, r, dt, 'utils, weights and test_var: ' + what)


@dtypes
def test_agent_surface(dt):
    """Agent.group_posterior on a 12 x 12 SyntheticField, the field rows as groups over every site of the field, against the
    reference on the agent's sampled dataset."""
    from algp_amd.agent import Agent
    from algp_amd.field import SyntheticField
    kid = MF.RBF
    state = np.random.get_state()
    np.random.seed(5)
    env = SyntheticField(12, 12, num_test=24)
    np.random.set_state(state)
    p = PF.grid_problem()
    ag = Agent.__new__(Agent)
    ag.env = env
    ag.static_std, ag.mobile_std = 0.1, 1.0
    n = env.num_samples
    ag.static_data = [[] for _ in range(n)]
    ag.mobile_data = [[] for _ in range(n)]
    rng = np.random.RandomState(6)
    for i in rng.permutation(n)[:50]:
        ag.static_data[i].append(float(env.Y[i] + 0.1 * rng.standard_normal()))
    for i in rng.permutation(n)[:20]:
        ag.mobile_data[i].append(float(env.Y[i] + rng.standard_normal()))
    ag.gp = _gp(p, kid, dt)
    ag._pool_key = ('x', 0)
    ind, y, var = ag.get_sampled_dataset()
    x = env.all_x
    rows = x[:, 0].astype(np.int32)
    mu, Sigma = GF.moments(kid, p.log_ls, p.log_os, p.log_noise, env.X[ind], y, var, x)
    ref = GF.aggregates(mu, Sigma, GF.coefficients(rows, None, 12))
    out = ag.group_posterior(rows, x=x, return_cross=True)
    assert ag._pool_key is None and out[0].shape == (12,) and out[1].shape == (12, 12) and out[2].shape == (12, 144)
    for got, r, what in zip(out, ref, ('mean', 'cov', 'cross')):
        close(got, r, dt, 'Agent ' + what)
    # over env.test_X by default: the rows that hold a test site
    trow = env.test_X[:, 0].astype(np.int64)
    _, tlab = np.unique(trow, return_inverse=True)
    mu, Sigma = GF.moments(kid, p.log_ls, p.log_os, p.log_noise, env.X[ind], y, var, env.test_X)
    ref = GF.aggregates(mu, Sigma, GF.coefficients(tlab, None, tlab.max() + 1))
    mean, cov = ag.group_posterior(tlab)
    close(mean, ref[0], dt, 'Agent over test_X: mean')
    close(cov, ref[1], dt, 'Agent over test_X: cov')
