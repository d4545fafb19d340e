"""The joint posterior of group aggregates in NumPy fp64, independent of the library: what tests/test_group_posterior.py and
tests/test_group_forms_host.py compare against, and the problems and groupings both are run on (built here, without a device).

The latent field at the candidate rows X given the train data (sites A, targets y, per-row noise var, likelihood noise
sigma_n^2, constant mean ybar = mean(y)) has

    mu    = ybar + K_XA S^-1 (y - ybar),                      S = K_AA + diag(var + sigma_n^2)
    Sigma = K_XX + diag(extra) - K_XA S^-1 K_AX               (extra: per candidate ROW; two rows of one site share K(x, x))

and Q linear functionals g = A f, one row of coefficients per group, have mean A mu, covariance A Sigma A^T and cross-covariance
with the sites A Sigma.  A comes from one label per row (-1: in no group) and either explicit weights, used as given, or the
plain group means 1 / n_q.  Kernel values come from tests/matern_forms.py; the problems from tests/pathwise_forms.py.
"""
import functools
import types

import numpy as np
from scipy.linalg import cho_factor, cho_solve

import matern_forms as MF
import pathwise_forms as PF

KIDS, KNAMES, f32 = PF.KIDS, PF.KNAMES, PF.f32


def coefficients(group, weight, Q):
    """A (Q x M) from labels and weights; weight None: 1 / n_q (every group then needs a member)."""
    group = np.asarray(group)
    M = len(group)
    A = np.zeros((Q, M))
    lab = np.nonzero(group >= 0)[0]
    if weight is None:
        n = np.bincount(group[lab], minlength=Q)
        assert np.all(n > 0)
        A[group[lab], lab] = 1.0 / n[group[lab]]
    else:
        A[group[lab], lab] = np.asarray(weight, np.float64)[lab]
    return A


def moments(kid, log_ls, log_os, log_noise, x_train, y, var, x_test, extra=None):
    """(mu, Sigma) of the latent field at the rows x_test."""
    y = np.asarray(y, np.float64)
    S = MF.train_matrix(kid, log_ls, log_os, log_noise, x_train, var)
    K_XA = MF.kernel_matrix(kid, log_ls, log_os, x_test, x_train)
    cf = cho_factor(S, lower=True)
    mu = y.mean() + K_XA @ cho_solve(cf, y - y.mean())
    Sigma = MF.kernel_matrix(kid, log_ls, log_os, x_test) - K_XA @ cho_solve(cf, K_XA.T)
    if extra is not None:
        Sigma = Sigma + np.diag(np.asarray(extra, np.float64))
    return mu, Sigma


def problem_moments(p, kid):
    """(mu, Sigma) at the candidates of problem `p` (its per-row extra variance, if it carries one)."""
    return moments(kid, p.log_ls, p.log_os, p.log_noise, p.X[p.A], p.y, p.var, p.X[p.cand], getattr(p, 'extra', None))


def aggregates(mu, Sigma, A):
    """(A mu, A Sigma A^T, A Sigma)."""
    cross = A @ Sigma
    return A @ mu, cross @ A.T, cross


def reference(p, kid, group, weight, Q):
    mu, Sigma = problem_moments(p, kid)
    return aggregates(mu, Sigma, coefficients(group, weight, Q))


# ------------------------------------------------------------------------------------------------------------ the groupings
def deal(sizes, M, seed):
    """Labels for M rows: group q gets sizes[q] rows, the rest -1, dealt by a seeded permutation (no group is contiguous)."""
    assert sum(sizes) <= M
    lab = np.full(M, -1, np.int32)
    lab[:sum(sizes)] = np.repeat(np.arange(len(sizes)), sizes)
    return lab[np.random.RandomState(seed).permutation(M)]


SIZES_A = [1, 2, 37, 130, 64, 50]          # + 16 rows in no group: a singleton, a group wider than a 128-row tile


def grouping(which, M=300):
    """(labels, Q) of the three groupings of an M = 300 problem."""
    if which == 'a':
        return deal(SIZES_A, M, 7), len(SIZES_A)
    if which == 'b':
        return deal([2] * (M // 2), M, 8), M // 2                # Q = 150 crosses the 128 padding of the products
    if which == 'c':
        return np.zeros(M, np.int32), 1
    raise ValueError(which)


GROUPINGS = ['a', 'b', 'c']


# ------------------------------------------------------------------------------------------------------------ more problems
@functools.lru_cache(maxsize=None)
def big_problem():
    """64 x 64 unit grid, N = 300 train sites, M = 2 600 candidates (2 590 free sites and 10 train sites): several row blocks
    and several chunks of the member list."""
    rng = np.random.RandomState(2044)
    gi, gj = np.meshgrid(np.arange(64), np.arange(64), indexing='ij')
    X = np.c_[gi.ravel(), gj.ravel()].astype(np.float64)
    return PF._finish(rng, X, 2, N=300, n_free=2590, n_train_cand=10)


SIZES_W = [700, 1, 300, 0, 450, 2, 128, 129] + [3 + (7 * i) % 31 for i in range(32)]      # Q = 40, one group empty


@functools.lru_cache(maxsize=None)
def weighted_grouping():
    """(labels, weights, Q) on big_problem(): 40 groups of 1 .. 700 rows and an empty one, fp32-exact weights in [-1, 1] with
    eight labelled rows at 0."""
    M = len(big_problem().cand)
    lab = deal(SIZES_W, M, 9)
    rng = np.random.RandomState(10)
    w = f32(rng.uniform(-1.0, 1.0, M))
    w[rng.choice(np.nonzero(lab >= 0)[0], 8, replace=False)] = 0.0
    lab.setflags(write=False)
    w.setflags(write=False)
    return lab, w, len(SIZES_W)


EMPTY_W = SIZES_W.index(0)


@functools.lru_cache(maxsize=None)
def duplicate_problem():
    """The grid problem with five pool sites named twice in the candidate list (rows 100..104 repeat rows 0..4) and a per-row
    extra variance."""
    p = PF.grid_problem()
    cand = p.cand.copy()
    cand[100:105] = cand[0:5]
    q = types.SimpleNamespace(**vars(p))
    q.cand = cand
    q.extra = f32(np.random.RandomState(12).uniform(0.01, 0.1, len(cand)))
    return q
