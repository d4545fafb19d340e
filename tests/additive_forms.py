"""The additive kernel of include/algp_hip.h (algp_set_hypers_additive) in NumPy fp64, built on tests/matern_forms.py and
independent of the library and of the oracle: what tests/test_additive_kernel.py and tests/test_additive_forms_host.py compare
against.

    k(x, x') = os_a kappa_a(r_a) + os_b kappa_b(r_b)

r_a over the first `split` coordinates, r_b over the others: the K of each part on its own columns, summed.  A kernel is
described by `spec` = (kernel_a, kernel_b, split); the parameters are log_ls (D entries, coordinate order), log_os = (a, b)
and log_noise.  The gradient has D + 3 entries: [log ls_0..D), log os_a, log os_b, log sigma_n^2].
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

import matern_forms as MF


def _cols(x, lo, hi):
    x = np.asarray(x, np.float64)
    return x.reshape(len(x), -1)[:, lo:hi]


def part_matrix(spec, part, log_ls, log_os, x1, x2=None):
    """os_c kappa_c(r_c): one part's kernel matrix, on its own columns."""
    ka, kb, split = spec
    log_ls = np.atleast_1d(np.asarray(log_ls, np.float64))
    D = len(log_ls)
    lo, hi, kid = (0, split, ka) if part == 0 else (split, D, kb)
    return MF.kernel_matrix(kid, log_ls[lo:hi], log_os[part], _cols(x1, lo, hi), None if x2 is None else _cols(x2, lo, hi))


def kernel_matrix(spec, log_ls, log_os, x1, x2=None):
    return part_matrix(spec, 0, log_ls, log_os, x1, x2) + part_matrix(spec, 1, log_ls, log_os, x1, x2)


def prior_var(log_os):
    return float(np.exp(log_os[0]) + np.exp(log_os[1]))


def train_matrix(spec, log_ls, log_os, log_noise, x, var=None, sites=None):
    """S = K + diag(var) + sigma_n^2 E, E_ij = 1 where rows i and j name the same pool site."""
    N = len(x)
    S = kernel_matrix(spec, log_ls, log_os, x) + np.exp(log_noise) * MF.same_site(sites, N)
    if var is not None:
        S = S + np.diag(np.asarray(var, np.float64))
    return S


def mll(spec, log_ls, log_os, log_noise, x, y, var=None, sites=None, mean=None):
    y = np.asarray(y, np.float64)
    y0 = y - (y.mean() if mean is None else mean)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x, var, sites))
    return float(-0.5 * y0 @ cho_solve((L, True), y0) - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2 * np.pi))


def mll_grad(spec, log_ls, log_os, log_noise, x, y, var=None, sites=None, mean=None):
    """d MLL / d (log ls_0..D, log os_a, log os_b, log sigma_n^2) = 1/2 tr(W dS/dtheta), W = alpha alpha' - S^-1."""
    ka, kb, split = spec
    y = np.asarray(y, np.float64)
    N = len(y)
    log_ls = np.atleast_1d(np.asarray(log_ls, np.float64))
    D = len(log_ls)
    y0 = y - (y.mean() if mean is None else mean)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x, var, sites))
    alpha = cho_solve((L, True), y0)
    W = np.outer(alpha, alpha) - cho_solve((L, True), np.eye(N))
    u2 = MF.scaled_sq(log_ls, x)
    g = []
    for part, (lo, hi, kid) in enumerate(((0, split, ka), (split, D, kb))):
        r = np.sqrt(sum(u2[lo:hi]))
        WdK = W * (np.exp(log_os[part]) * MF.dk_of_r(kid, r))
        g += [0.5 * np.sum(WdK * u2[d]) for d in range(lo, hi)]
    for part, (lo, hi, kid) in enumerate(((0, split, ka), (split, D, kb))):
        r = np.sqrt(sum(u2[lo:hi]))
        g.append(0.5 * np.sum(W * (np.exp(log_os[part]) * MF.k_of_r(kid, r))))
    g.append(0.5 * np.exp(log_noise) * np.sum(W * MF.same_site(sites, N)))
    return np.array(g)


def posterior(spec, log_ls, log_os, log_noise, x_train, y, var, x_test, sites=None):
    """(mean, variance of the latent field) at x_test by Cholesky, constant mean = mean(y)."""
    y = np.asarray(y, np.float64)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x_train, var, sites))
    Kx = kernel_matrix(spec, log_ls, log_os, x_test, x_train)
    mu = y.mean() + Kx @ cho_solve((L, True), y - y.mean())
    V = solve_triangular(L, Kx.T, lower=True)
    return mu, prior_var(log_os) - np.sum(V * V, axis=0)


def component_means(spec, log_ls, log_os, log_noise, x_train, y, var, x_test, sites=None):
    """(mu_a, mu_b): mu_c = K_c(x_test, x_train) alpha, without the constant mean; mu_a + mu_b + mean(y) = posterior mean."""
    y = np.asarray(y, np.float64)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x_train, var, sites))
    alpha = cho_solve((L, True), y - y.mean())
    return tuple(part_matrix(spec, c, log_ls, log_os, x_test, x_train) @ alpha for c in (0, 1))
