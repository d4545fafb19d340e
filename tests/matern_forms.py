"""The four kernel forms of include/algp_hip.h in NumPy fp64, independent of the library and of the oracle: what
tests/test_matern_family.py and tests/test_matern_forms_host.py compare against.

With r^2 = sum_d ((x_d - x'_d) / ls_d)^2, r = sqrt(r^2), os = outputscale (gpytorch's ScaleKernel(RBFKernel | MaternKernel(nu))):

    id 0  RBF         k = os exp(-r^2 / 2)                               dk = k
    id 1  Matern-3/2  k = os (1 + a) exp(-a),           a = sqrt(3) r    dk = 3 os exp(-a)
    id 2  Matern-1/2  k = os exp(-r)                                     dk = os exp(-r) / r   (the term dk u_d^2 is 0 at r = 0)
    id 3  Matern-5/2  k = os (1 + a + a^2 / 3) exp(-a), a = sqrt(5) r    dk = 5/3 os (1 + a) exp(-a)

dk is the factor of the length-scale derivative, dk/dlog ls_d = dk u_d^2 with u_d = (x_d - x'_d) / ls_d, i.e. dk = -2 dk/dr^2.
"""
import numpy as np
from scipy.linalg import cho_solve

RBF, MATERN15, MATERN05, MATERN25 = 0, 1, 2, 3
NU = {MATERN05: 0.5, MATERN15: 1.5, MATERN25: 2.5}


def k_of_r(kernel_id, r):
    """k / os as a function of the scaled distance r >= 0."""
    r = np.asarray(r, np.float64)
    if kernel_id == RBF:
        return np.exp(-0.5 * r * r)
    if kernel_id == MATERN05:
        return np.exp(-r)
    if kernel_id == MATERN15:
        a = np.sqrt(3.0) * r
        return (1.0 + a) * np.exp(-a)
    if kernel_id == MATERN25:
        a = np.sqrt(5.0) * r
        return (1.0 + a + a * a / 3.0) * np.exp(-a)
    raise ValueError(kernel_id)


def dk_of_r(kernel_id, r):
    """dk / os; for id 2 the value at r = 0 is set to 0: it only ever multiplies u_d^2 = 0 there, and u_d^2 / r -> 0."""
    r = np.asarray(r, np.float64)
    if kernel_id == RBF:
        return np.exp(-0.5 * r * r)
    if kernel_id == MATERN05:
        safe = np.where(r > 0, r, 1.0)
        return np.where(r > 0, np.exp(-r) / safe, 0.0)
    if kernel_id == MATERN15:
        return 3.0 * np.exp(-np.sqrt(3.0) * r)
    if kernel_id == MATERN25:
        a = np.sqrt(5.0) * r
        return 5.0 / 3.0 * (1.0 + a) * np.exp(-a)
    raise ValueError(kernel_id)


def scaled_sq(log_ls, x1, x2=None):
    """[u_d^2 for every d]: the squared scaled coordinate differences, formed directly so that coincident points give 0."""
    x1 = np.asarray(x1, np.float64)
    x1 = x1.reshape(len(x1), -1)
    x2 = x1 if x2 is None else np.asarray(x2, np.float64).reshape(len(x2), -1)
    inv = np.exp(-np.atleast_1d(np.asarray(log_ls, np.float64)))
    return [np.square((x1[:, d][:, None] - x2[:, d][None, :]) * inv[d]) for d in range(x1.shape[1])]


def kernel_matrix(kernel_id, log_ls, log_os, x1, x2=None):
    r = np.sqrt(sum(scaled_sq(log_ls, x1, x2)))
    return np.exp(log_os) * k_of_r(kernel_id, r)


def same_site(sites, N):
    """E_ij = 1 where rows i and j name the same pool site (the identity without `sites`)."""
    if sites is None:
        return np.eye(N)
    s = np.asarray(sites)
    return (s[:, None] == s[None, :]).astype(np.float64)


def train_matrix(kernel_id, log_ls, log_os, log_noise, x, var=None, sites=None):
    """S = K + diag(var) + sigma_n^2 E."""
    N = len(x)
    S = kernel_matrix(kernel_id, log_ls, log_os, x) + np.exp(log_noise) * same_site(sites, N)
    if var is not None:
        S = S + np.diag(np.asarray(var, np.float64))
    return S


def mll(kernel_id, log_ls, log_os, log_noise, x, y, var=None, sites=None, mean=None):
    """-1/2 y0' S^-1 y0 - 1/2 log det S - N/2 log 2 pi of the whole train set (not per point), y0 = y - mean(y)."""
    y = np.asarray(y, np.float64)
    y0 = y - (y.mean() if mean is None else mean)
    L = np.linalg.cholesky(train_matrix(kernel_id, log_ls, log_os, log_noise, x, var, sites))
    return float(-0.5 * y0 @ cho_solve((L, True), y0) - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2 * np.pi))


def mll_grad(kernel_id, log_ls, log_os, log_noise, x, y, var=None, sites=None, mean=None):
    """d MLL / d (log ls_1..D, log os, log sigma_n^2) = 1/2 tr(W dS/dtheta), W = alpha alpha' - S^-1."""
    y = np.asarray(y, np.float64)
    N = len(y)
    y0 = y - (y.mean() if mean is None else mean)
    L = np.linalg.cholesky(train_matrix(kernel_id, log_ls, log_os, log_noise, x, var, sites))
    alpha = cho_solve((L, True), y0)
    W = np.outer(alpha, alpha) - cho_solve((L, True), np.eye(N))
    u2 = scaled_sq(log_ls, x)
    r = np.sqrt(sum(u2))
    os_ = np.exp(log_os)
    WdK = W * (os_ * dk_of_r(kernel_id, r))
    g = [0.5 * np.sum(WdK * u2[d]) for d in range(len(u2))]
    g.append(0.5 * np.sum(W * (os_ * k_of_r(kernel_id, r))))
    g.append(0.5 * np.exp(log_noise) * np.sum(W * same_site(sites, N)))
    return np.array(g)


def posterior(kernel_id, log_ls, log_os, log_noise, x_train, y, var, x_test, sites=None):
    """(mean, variance of the latent field) at x_test by Cholesky, constant mean = mean(y)."""
    y = np.asarray(y, np.float64)
    L = np.linalg.cholesky(train_matrix(kernel_id, log_ls, log_os, log_noise, x_train, var, sites))
    Kx = kernel_matrix(kernel_id, log_ls, log_os, x_test, x_train)
    mu = y.mean() + Kx @ cho_solve((L, True), y - y.mean())
    from scipy.linalg import solve_triangular
    V = solve_triangular(L, Kx.T, lower=True)
    return mu, np.exp(log_os) - np.sum(V * V, axis=0)


def factors_in_fp32(S):
    """Whether S, rounded to fp32 and factored by an fp32 Cholesky, meets no non-positive pivot."""
    try:
        np.linalg.cholesky(np.asarray(S, np.float32))
        return True
    except np.linalg.LinAlgError:
        return False
