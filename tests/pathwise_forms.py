"""Pathwise conditioning (Matheron's rule) in NumPy fp64, independent of the library: what tests/test_pathwise_samples.py
and tests/test_pathwise_forms_host.py compare against, and the problems both are run on (built here, without a device).

A prior draw g of the latent field becomes a posterior draw given the train data (sites A, targets y, per-row noise var,
likelihood noise sigma_n^2, constant mean ybar = mean(y)):

    f_s(j) = ybar + g_s(j) + K_jA S^-1 (y - ybar - g_s(A) - sqrt(v) o eps_s),     S = K_AA + diag(v),  v = var + sigma_n^2

The prior draw is either given (values at every pool site) or a random-Fourier-feature sum

    g_s = Phi w_s,     Phi[q, f] = sqrt(2 os / F) cos(Xs[q] . omega_f + phase_f),     Xs = x / lengthscale

whose covariance Phi Phi^T approaches k for omega drawn from the kernel's spectral density at unit lengthscale: N(0, I) for RBF,
the multivariate Student-t with 2 nu degrees of freedom for Matern-nu.  Kernel values come from tests/matern_forms.py.
"""
import functools
import types

import numpy as np
from scipy.linalg import cho_factor, cho_solve

import matern_forms as MF

KIDS = [MF.RBF, MF.MATERN15, MF.MATERN05, MF.MATERN25]
KNAMES = ['rbf', 'matern15', 'matern05', 'matern25']
FS = [(1, 1), (100, 5), (257, 130)]       # (features, samples); the last crosses the k-tile padding and the 128-sample tile


def f32(a):
    """Values both precisions hold exactly: rounded to float32, kept as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def features(omega, phase, xs, outputscale):
    """Phi (n x F) for scaled coordinates xs (n x D)."""
    omega = np.asarray(omega, np.float64)
    return np.sqrt(2.0 * outputscale / len(omega)) * np.cos(np.asarray(xs, np.float64) @ omega.T + np.asarray(phase, np.float64)[None, :])


def pathwise(K_XA, S, y, v, g_X, g_A, eps, mean=None):
    """f (S x M) from prior draws g_X (S x M) at the candidates and g_A (S x N) at the train sites; eps (S x N)."""
    y = np.asarray(y, np.float64)
    ybar = (y.mean() if len(y) else 0.0) if mean is None else mean
    if len(y) == 0:
        return ybar + np.asarray(g_X, np.float64)
    r = (y - ybar)[None, :] - g_A - np.sqrt(v)[None, :] * eps
    return ybar + g_X + cho_solve(cho_factor(S, lower=True), r.T).T @ K_XA.T


def problem_draws(p, kid, F, S, weights=None, eps=None, omega=None, phase=None, prior=None):
    """The reference for problem `p` under kernel `kid`: random features (omega, phase, weights) or prior values (S x n_pool)."""
    K = MF.kernel_matrix(kid, p.log_ls, p.log_os, p.X)
    v = p.var + np.exp(p.log_noise)
    Smat = K[np.ix_(p.A, p.A)] + np.diag(v)
    if prior is None:
        G = weights @ features(omega, phase, p.X * np.exp(-p.log_ls)[None, :], np.exp(p.log_os)).T
    else:
        G = np.asarray(prior, np.float64)
    return pathwise(K[np.ix_(p.cand, p.A)], Smat, p.y, v, G[:, p.cand], G[:, p.A], eps)


def draws(seed, F, S, D, N):
    """(omega, phase, weights, eps), fp32-exact; omega ~ N(0, I) whatever the kernel: the ABI does not care about the
    distribution, and the cosine's argument stays below about 60."""
    rng = np.random.RandomState(seed)
    return (f32(rng.standard_normal((F, D))), f32(rng.uniform(0, 2 * np.pi, F)), f32(rng.standard_normal((S, F))),
            f32(rng.standard_normal((S, N))))


def _finish(rng, X, D, N=200, n_free=290, n_train_cand=10):
    n = len(X)
    perm = rng.permutation(n)
    A = np.sort(perm[:N])
    free = np.sort(perm[N:N + n_free])
    cand = np.r_[free, np.sort(rng.choice(A, n_train_cand, replace=False))] if N else free
    y = f32(np.sin(X[A, 0] / 3.0) + 0.1 * rng.standard_normal(N))
    var = f32(rng.uniform(0.005, 0.05, N))
    return types.SimpleNamespace(X=X, D=D, A=A.astype(np.int64), y=y, var=var, cand=cand.astype(np.int64), free=free.astype(np.int64),
                                 log_ls=np.log(np.full(D, 3.0)), log_os=0.0, log_noise=np.log(1e-2))


@functools.lru_cache(maxsize=None)
def grid_problem():
    """24 x 24 unit grid, lengthscales (3, 3), os = 1, sigma_n^2 = 1e-2; N = 200 train sites (Npad = 256: two tiles, the last
    ragged), M = 300 candidates (Mpad = 384): 290 unsampled sites and 10 train sites."""
    rng = np.random.RandomState(2024)
    gi, gj = np.meshgrid(np.arange(24), np.arange(24), indexing='ij')
    X = np.c_[gi.ravel(), gj.ravel()].astype(np.float64)
    return _finish(rng, X, 2)


@functools.lru_cache(maxsize=None)
def random_problem(D):
    """576 random sites in [0, 10)^D (DP = 4 for D = 3, DP = 8 for D = 5), otherwise as the grid problem."""
    rng = np.random.RandomState(2030 + D)
    return _finish(rng, f32(rng.uniform(0, 10, (576, D))), D)


def train_matrix(p, kid):
    return MF.train_matrix(kid, p.log_ls, p.log_os, p.log_noise, p.X[p.A], p.var)


def all_problems():
    """(problem, kernel id) of every GPU case."""
    return [(grid_problem(), k) for k in KIDS] + [(random_problem(3), MF.MATERN25), (random_problem(5), MF.RBF)]


def exact_prior(p, kid, S, seed):
    """S exact prior draws at every pool site, chol(K_pool + 1e-10 I) xi, fp32-exact."""
    K = MF.kernel_matrix(kid, p.log_ls, p.log_os, p.X)
    L = np.linalg.cholesky(K + 1e-10 * np.eye(len(K)))
    return f32(np.random.RandomState(seed).standard_normal((S, len(K))) @ L.T)


def spectral_target(kid, xs, outputscale=1.0):
    """k at scaled coordinates xs (unit lengthscale): what Phi Phi^T of spectral draws approaches."""
    return MF.kernel_matrix(kid, np.zeros(xs.shape[1]), np.log(outputscale), xs)
