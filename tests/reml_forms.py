"""Fixed effects in NumPy fp64 (include/algp_hip.h, algp_set_fixed_effects): the mean is mean + h(x)' beta with beta estimated
by generalised least squares.  Built on tests/ai_forms.py (train_matrix, derivative_matrices), independent of the library and
of the oracle, and written with the DENSE projector P where the library goes through the Cholesky factor: what
tests/test_reml_forms_host.py and tests/test_fixed_effects.py compare against.

    S = train_matrix,  y0 = y - mean,  A = H' S^-1 H,  beta = A^-1 H' S^-1 y0,  P = S^-1 - S^-1 H A^-1 H' S^-1
    l_R = -1/2 [ (N - p) log 2 pi + log|S| + log|A| + y0' P y0 ]           (Harville: no + 1/2 log|H'H|)
    dl_R/dtheta_a = 1/2 tr((P y0 y0' P - P) dS_a)         AI_R,ab = 1/2 y0' P dS_a P dS_b P y0
    candidates:  r_j = h_j - H' S^-1 k_j,  mu_j = mean + k_j' S^-1 y0 + r_j' beta,  cov = K_** - K_*A S^-1 K_A* + r A^-1 r'

A model is ai_forms' (family, spec) with theta in the gradient's order; H holds one row per train row.
"""
import numpy as np
from scipy.linalg import solve_triangular

import ai_forms as AI

LOG_2PI = 1.8378770664093453


def _parts(family, spec, theta, x, y, H, var=None, sites=None, mean=None):
    y = np.asarray(y, np.float64)
    H = np.asarray(H, np.float64).reshape(len(y), -1)
    S = AI.train_matrix(family, spec, theta, x, var, sites)
    Si = np.linalg.inv(S)
    A = H.T @ Si @ H
    Ai = np.linalg.inv(A)
    P = Si - Si @ H @ Ai @ H.T @ Si
    y0 = y - (y.mean() if mean is None else mean)
    return S, Si, A, Ai, P, y0, H


def gls(family, spec, theta, x, y, H, var=None, sites=None, mean=None):
    """(beta, cov beta)."""
    _, Si, _, Ai, _, y0, H = _parts(family, spec, theta, x, y, H, var, sites, mean)
    return Ai @ (H.T @ (Si @ y0)), Ai


def scaled_cond(A):
    """cond of A scaled to a unit diagonal."""
    d = 1.0 / np.sqrt(np.diag(A))
    return float(np.linalg.cond(A * np.outer(d, d)))


def gram(family, spec, theta, x, H, var=None, sites=None):
    """A = H' S^-1 H."""
    return _parts(family, spec, theta, x, np.zeros(len(x)), H, var, sites, 0.0)[2]


def reml(family, spec, theta, x, y, H, var=None, sites=None, mean=None):
    S, _, A, _, P, y0, H = _parts(family, spec, theta, x, y, H, var, sites, mean)
    N, p = H.shape
    return -0.5 * ((N - p) * LOG_2PI + np.linalg.slogdet(S)[1] + np.linalg.slogdet(A)[1] + y0 @ P @ y0)


def reml_grad(family, spec, theta, x, y, H, var=None, sites=None, mean=None):
    _, _, _, _, P, y0, _ = _parts(family, spec, theta, x, y, H, var, sites, mean)
    a = P @ y0
    W = np.outer(a, a) - P
    return np.array([0.5 * np.sum(W * dS) for dS in AI.derivative_matrices(family, spec, theta, x, sites)])


def reml_ai(family, spec, theta, x, y, H, var=None, sites=None, mean=None):
    _, _, _, _, P, y0, _ = _parts(family, spec, theta, x, y, H, var, sites, mean)
    a = P @ y0
    U = np.stack([dS @ a for dS in AI.derivative_matrices(family, spec, theta, x, sites)], axis=1)
    return 0.5 * U.T @ P @ U


def prior_blocks(family, spec, theta, x, xc, var=None, sites=None):
    """(S, K_*A, K_**) with K the noise-free kernel between the candidates xc and the train rows x."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    xc = np.asarray(xc, np.float64).reshape(len(xc), -1)
    N = len(x)
    noise = np.exp(AI.unpack(family, theta, x)[2])
    K = AI.train_matrix(family, spec, theta, np.vstack([x, xc])) - noise * np.eye(N + len(xc))
    return AI.train_matrix(family, spec, theta, x, var, sites), K[N:, :N], K[N:, N:]


def posterior_known_mean(family, spec, theta, x, y, xc, var=None, sites=None, mean=None):
    """(mu, cov) at xc for the constant mean alone: what algp_get_posterior / algp_get_posterior_cov return."""
    y = np.asarray(y, np.float64)
    S, Kca, Kcc = prior_blocks(family, spec, theta, x, xc, var, sites)
    m = y.mean() if mean is None else mean
    return m + Kca @ np.linalg.solve(S, y - m), Kcc - Kca @ np.linalg.solve(S, Kca.T)


def posterior_fixed(family, spec, theta, x, y, H, xc, Hc, var=None, sites=None, mean=None):
    """dict(mu, cov, var, proj) at xc: cov is the noise-free covariance with the universal-kriging term, var its diagonal, proj
    the rows r_j C with A^-1 = C C', C the inverse of A's upper Cholesky factor (cov = known-mean cov + proj proj')."""
    y = np.asarray(y, np.float64)
    S, Si, A, Ai, _, y0, H = _parts(family, spec, theta, x, y, H, var, sites, mean)
    _, Kca, Kcc = prior_blocks(family, spec, theta, x, xc, var, sites)
    Hc = np.asarray(Hc, np.float64).reshape(len(Kca), -1)
    beta = Ai @ (H.T @ (Si @ y0))
    R = Hc - Kca @ Si @ H
    C = np.linalg.inv(np.linalg.cholesky(A).T)
    proj = R @ C
    m = y.mean() if mean is None else mean
    cov = Kcc - Kca @ Si @ Kca.T + R @ Ai @ R.T
    return dict(mu=m + Kca @ (Si @ y0) + R @ beta, cov=cov, var=np.diag(cov).copy(), proj=proj, beta=beta)


def posterior_diffuse(family, spec, theta, x, y, H, xc, Hc, tau2, var=None, sites=None, mean=None):
    """(mu, cov) at xc of the GP with the prior beta ~ N(0, tau2 I) folded into the kernel: k + tau2 h(x)' h(x')."""
    y = np.asarray(y, np.float64)
    H = np.asarray(H, np.float64).reshape(len(y), -1)
    S, Kca, Kcc = prior_blocks(family, spec, theta, x, xc, var, sites)
    Hc = np.asarray(Hc, np.float64).reshape(len(Kca), -1)
    Sd = S + tau2 * H @ H.T
    kd = Kca + tau2 * Hc @ H.T
    m = y.mean() if mean is None else mean
    L = np.linalg.cholesky(Sd)
    V = solve_triangular(L, kd.T, lower=True)
    return m + V.T @ solve_triangular(L, y - m, lower=True), Kcc + tau2 * Hc @ Hc.T - V.T @ V


def contrast_likelihood(family, spec, theta, x, y, H, var=None, sites=None, mean=None):
    """The log-likelihood of the N - p error contrasts Q2' y0, Q2 an orthonormal basis of the complement of span(H)."""
    y = np.asarray(y, np.float64)
    H = np.asarray(H, np.float64).reshape(len(y), -1)
    N, p = H.shape
    Q2 = np.linalg.qr(H, mode='complete')[0][:, p:]
    S = AI.train_matrix(family, spec, theta, x, var, sites)
    w = Q2.T @ (y - (y.mean() if mean is None else mean))
    Sw = Q2.T @ S @ Q2
    return -0.5 * ((N - p) * LOG_2PI + np.linalg.slogdet(Sw)[1] + w @ np.linalg.solve(Sw, w))


# ---- the inputs of test_reml_forms_host.py and test_fixed_effects.py ------------------------------------------------------
def basis(x, p, seed=0):
    """(len(x), p) with linearly independent columns: p = 1 the constant; p = 3 the constant and the first two coordinates
    centred and scaled by their range (x with one coordinate: its square stands in for the second); p = 16 those, eleven
    indicators of twelve random blocks and two quadratic terms; any other p: the first p columns of the p = 16 basis."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    n = len(x)
    u = (x - x.mean(0)) / np.maximum(x.max(0) - x.min(0), 1e-12)
    u0 = u[:, 0]
    u1 = u[:, 1] if x.shape[1] > 1 else u0 ** 2 - np.mean(u0 ** 2)
    block = np.random.RandomState(1000 + seed).randint(0, 12, n)
    cols = [np.ones(n), u0, u1] + [(block == b).astype(np.float64) for b in range(11)] + [u0 * u1, u0 ** 2 - u1 ** 2]
    return np.stack(cols[:p], axis=1)


def planted_beta(p, seed=0):
    return np.random.RandomState(2000 + seed).uniform(-1.0, 1.0, p)
