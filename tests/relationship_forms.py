"""The relationship kernel of include/algp_hip.h (algp_set_hypers_relationship) in NumPy fp64, built on tests/matern_forms.py and
independent of the library and of the oracle: what tests/test_relationship_kernel.py and tests/test_relationship_forms_host.py
compare against.

    k((s, g), (s', g')) = os_a kappa_a(r(s, s')) + os_g G[g, g']

The first D - 1 columns of x are spatial (ARD lengthscales log_ls, D - 1 entries), the last holds the integer genotype id.  A
kernel is described by `spec` = (kernel_a, G, Q) with G a (Q, Q) symmetric matrix or None for the identity; the parameters are
log_ls, log_os = (a, g) and log_noise.  The gradient has D + 2 entries: [log ls_0..D-1), log os_a, log os_g, log sigma_n^2].
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

import matern_forms as MF


def _split(x):
    x = np.asarray(x, np.float64)
    x = x.reshape(len(x), -1)
    ids = x[:, -1].astype(np.int64)
    assert np.array_equal(ids, x[:, -1]), 'the last column holds integer ids'
    return x[:, :-1], ids


def table(spec):
    """G as a dense (Q, Q) matrix (the identity for None)."""
    _, G, Q = spec
    return np.eye(Q) if G is None else np.asarray(G, np.float64)


def marker_relationship(Q=12, m=40, seed=5):
    """G = A A^T / m from a random Q x m marker matrix with allele counts {0, 1, 2} centred at 1 (entries -1, 0, 1): positive
    definite for m > Q, its diagonal not constant.  Symmetrised bit for bit and rounded to values both precisions hold exactly."""
    rng = np.random.RandomState(seed)
    A = rng.randint(0, 3, size=(Q, m)).astype(np.float64) - 1.0
    G = A @ A.T / m
    G = 0.5 * (G + G.T)
    return G.astype(np.float32).astype(np.float64)


def part_matrix(spec, part, log_ls, log_os, x1, x2=None):
    """Part 0: os_a kappa_a(r_a) on the spatial columns; part 1: os_g G[g, g']."""
    s1, g1 = _split(x1)
    s2, g2 = (s1, g1) if x2 is None else _split(x2)
    if part == 0:
        return MF.kernel_matrix(spec[0], log_ls, log_os[0], s1, None if x2 is None else s2)
    return np.exp(log_os[1]) * table(spec)[np.ix_(g1, g2)]


def kernel_matrix(spec, log_ls, log_os, x1, x2=None):
    return part_matrix(spec, 0, log_ls, log_os, x1, x2) + part_matrix(spec, 1, log_ls, log_os, x1, x2)


def prior_var(spec, log_os, x):
    """K_jj = os_a + os_g G[g_j, g_j], per site."""
    _, g = _split(x)
    return np.exp(log_os[0]) + np.exp(log_os[1]) * np.diag(table(spec))[g]


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
    """d MLL / d (log ls_0..D-1, log os_a, log os_g, log sigma_n^2) = 1/2 tr(W dS/dtheta), W = alpha alpha' - S^-1;
    dS/dlog os_g = os_g G[g_i, g_j]."""
    y = np.asarray(y, np.float64)
    N = len(y)
    log_ls = np.atleast_1d(np.asarray(log_ls, np.float64))
    s, _ = _split(x)
    y0 = y - (y.mean() if mean is None else mean)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x, var, sites))
    alpha = cho_solve((L, True), y0)
    W = np.outer(alpha, alpha) - cho_solve((L, True), np.eye(N))
    u2 = MF.scaled_sq(log_ls, s)
    r = np.sqrt(sum(u2))
    WdK = W * (np.exp(log_os[0]) * MF.dk_of_r(spec[0], r))
    g = [0.5 * np.sum(WdK * u2[d]) for d in range(len(log_ls))]
    g.append(0.5 * np.sum(W * (np.exp(log_os[0]) * MF.k_of_r(spec[0], r))))
    g.append(0.5 * np.sum(W * part_matrix(spec, 1, log_ls, log_os, x)))
    g.append(0.5 * np.exp(log_noise) * np.sum(W * MF.same_site(sites, N)))
    return np.array(g)


def posterior(spec, log_ls, log_os, log_noise, x_train, y, var, x_test, sites=None):
    """(mean, variance of the latent field) at x_test by Cholesky, constant mean = mean(y); the prior variance is the site's own."""
    y = np.asarray(y, np.float64)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x_train, var, sites))
    Kx = kernel_matrix(spec, log_ls, log_os, x_test, x_train)
    mu = y.mean() + Kx @ cho_solve((L, True), y - y.mean())
    V = solve_triangular(L, Kx.T, lower=True)
    return mu, prior_var(spec, log_os, x_test) - np.sum(V * V, axis=0)


def component_means(spec, log_ls, log_os, log_noise, x_train, y, var, x_test, sites=None):
    """(mu_a, mu_g): mu_c = K_c(x_test, x_train) alpha, without the constant mean; mu_a + mu_g + mean(y) = posterior mean."""
    y = np.asarray(y, np.float64)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x_train, var, sites))
    alpha = cho_solve((L, True), y - y.mean())
    return tuple(part_matrix(spec, c, log_ls, log_os, x_test, x_train) @ alpha for c in (0, 1))


def genotype_cross(spec, log_os, x_train):
    """B = os_g G[:, g_A]: cov(u, y_A), Q x N."""
    _, g = _split(x_train)
    return np.exp(log_os[1]) * table(spec)[:, g]


def genotype_posterior(spec, log_ls, log_os, log_noise, x_train, y, var, sites=None):
    """(mean, cov) of the Q genotype effects u ~ N(0, os_g G): mean = B S^-1 (y - mean(y)), cov = os_g G - B S^-1 B^T."""
    y = np.asarray(y, np.float64)
    S = train_matrix(spec, log_ls, log_os, log_noise, x_train, var, sites)
    B = genotype_cross(spec, log_os, x_train)
    return B @ np.linalg.solve(S, y - y.mean()), np.exp(log_os[1]) * table(spec) - B @ np.linalg.solve(S, B.T)
