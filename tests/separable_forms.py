"""The separable kernel of include/algp_hip.h (algp_set_hypers_separable) in NumPy fp64, built on tests/matern_forms.py and
independent of the library and of the oracle: what tests/test_separable_kernel.py and tests/test_separable_forms_host.py compare
against.

    k((x, g), (x', g')) = os kappa_a(r_a) kappa_b(r_b)  [ + os_g G[g, g'] ]

r_a runs over the first `split` columns of x, r_b over the other spatial ones, each factor at outputscale 1 with the ARD
lengthscales of its columns; with the genotype term the LAST column of x holds the integer genotype id.  A kernel is described by
`spec` = (kernel_a, kernel_b, split, G, Q): Q = 0 without the genotype term (G is then None), else G a (Q, Q) symmetric matrix or
None for the identity.  The parameters are log_ls (one per spatial column), log_os -- a float without the term, the pair (os, os_g)
with it -- and log_noise; theta packs them in the gradient's order [log ls..., log os, (log os_g,) log sigma_n^2], D + 2 entries
either way.

    dk/dlog ls_d = os kappa_b dk_a u_d^2 for d in part a (symmetric for b),  dk/dlog os = os kappa_a kappa_b,
    dk/dlog os_g = os_g G[g_i, g_j]

The restricted likelihood goes through tests/reml_forms.py, whose formulas take a model as ai_forms' (family, spec): _Family below
stands in for ai_forms there with the one family 'separable'.
"""
import contextlib

import numpy as np
from scipy.linalg import cho_solve, solve_triangular

import matern_forms as MF
import reml_forms as RM

FAMILY = 'separable'


def has_g(spec):
    return spec[4] > 0


def _split(spec, x):
    """(spatial columns, ids or None)."""
    x = np.asarray(x, np.float64)
    x = x.reshape(len(x), -1)
    if not has_g(spec):
        return x, None
    ids = x[:, -1].astype(np.int64)
    assert np.array_equal(ids, x[:, -1]), 'the last column holds integer ids'
    return x[:, :-1], ids


def table(spec):
    """G as a dense (Q, Q) matrix (the identity for None)."""
    return np.eye(spec[4]) if spec[3] is None else np.asarray(spec[3], np.float64)


def _os(spec, log_os):
    """(os, os_g or None)."""
    if has_g(spec):
        return np.exp(log_os[0]), np.exp(log_os[1])
    return np.exp(float(np.reshape(log_os, -1)[0])), None


def factors(spec, log_ls, x1, x2=None):
    """(kappa_a, kappa_b, r_a, r_b, u2): the two factor matrices at outputscale 1, their scaled distances, the squares per column."""
    ka, kb, split = spec[:3]
    s1, _ = _split(spec, x1)
    s2 = None if x2 is None else _split(spec, x2)[0]
    u2 = MF.scaled_sq(log_ls, s1, s2)
    ra, rb = np.sqrt(sum(u2[:split])), np.sqrt(sum(u2[split:]))
    return MF.k_of_r(ka, ra), MF.k_of_r(kb, rb), ra, rb, u2


def part_matrix(spec, part, log_ls, log_os, x1, x2=None):
    """Part 0: os kappa_a kappa_b on the spatial columns; part 1: os_g G[g, g'] (only with the genotype term)."""
    os_, osg = _os(spec, log_os)
    if part == 0:
        fa, fb = factors(spec, log_ls, x1, x2)[:2]
        return os_ * (fa * fb)
    assert has_g(spec), 'no genotype term'
    g1 = _split(spec, x1)[1]
    g2 = g1 if x2 is None else _split(spec, x2)[1]
    return osg * table(spec)[np.ix_(g1, g2)]


def kernel_matrix(spec, log_ls, log_os, x1, x2=None):
    K = part_matrix(spec, 0, log_ls, log_os, x1, x2)
    return K + part_matrix(spec, 1, log_ls, log_os, x1, x2) if has_g(spec) else K


def prior_var(spec, log_os, x):
    """K_jj = os (+ os_g G[g_j, g_j]), per site."""
    os_, osg = _os(spec, log_os)
    g = _split(spec, x)[1]
    return np.full(len(x), os_) if g is None else os_ + osg * np.diag(table(spec))[g]


def train_matrix(spec, log_ls, log_os, log_noise, x, var=None, sites=None):
    """S = K + diag(var) + sigma_n^2 E, E_ij = 1 where rows i and j name the same pool site."""
    N = len(x)
    S = kernel_matrix(spec, log_ls, log_os, x) + np.exp(log_noise) * MF.same_site(sites, N)
    if var is not None:
        S = S + np.diag(np.asarray(var, np.float64))
    return S


def derivative_matrices(spec, log_ls, log_os, log_noise, x, sites=None):
    """[dS/dtheta_a] in the gradient's order."""
    ka, kb, split = spec[:3]
    os_, _ = _os(spec, log_os)
    fa, fb, ra, rb, u2 = factors(spec, log_ls, x)
    ga, gb = os_ * fb * MF.dk_of_r(ka, ra), os_ * fa * MF.dk_of_r(kb, rb)
    d = [(ga if k < split else gb) * u2[k] for k in range(len(u2))]
    d.append(os_ * (fa * fb))
    if has_g(spec):
        d.append(part_matrix(spec, 1, log_ls, log_os, x))
    d.append(np.exp(log_noise) * MF.same_site(sites, len(x)))
    return d


def mll(spec, log_ls, log_os, log_noise, x, y, var=None, sites=None, mean=None):
    y = np.asarray(y, np.float64)
    y0 = y - (y.mean() if mean is None else mean)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x, var, sites))
    return float(-0.5 * y0 @ cho_solve((L, True), y0) - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2 * np.pi))


def mll_grad(spec, log_ls, log_os, log_noise, x, y, var=None, sites=None, mean=None):
    """d MLL / d theta = 1/2 tr(W dS/dtheta), W = alpha alpha' - S^-1."""
    y = np.asarray(y, np.float64)
    y0 = y - (y.mean() if mean is None else mean)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x, var, sites))
    alpha = cho_solve((L, True), y0)
    W = np.outer(alpha, alpha) - cho_solve((L, True), np.eye(len(y)))
    return np.array([0.5 * np.sum(W * dS) for dS in derivative_matrices(spec, log_ls, log_os, log_noise, x, sites)])


# ---- theta, and the quantities that take it ------------------------------------------------------------------------------------
def n_lengthscales(spec, x):
    D = np.asarray(x).reshape(len(x), -1).shape[1]
    return D - 1 if has_g(spec) else D


def unpack(spec, theta, x):
    """theta -> (log_ls, log_os, log_noise); log_os a float without the genotype term, else a pair."""
    theta = np.asarray(theta, np.float64)
    nl = n_lengthscales(spec, x)
    if not has_g(spec):
        return theta[:nl], float(theta[nl]), float(theta[nl + 1])
    return theta[:nl], (float(theta[nl]), float(theta[nl + 1])), float(theta[nl + 2])


def pack(log_ls, log_os, log_noise):
    return np.r_[np.atleast_1d(log_ls), np.atleast_1d(log_os), log_noise].astype(np.float64)


def mll_and_grad(spec, theta, x, y, var=None, sites=None, mean=None):
    p = unpack(spec, theta, x)
    return mll(spec, *p, x, y, var, sites, mean), mll_grad(spec, *p, x, y, var, sites, mean)


def average_information(spec, theta, x, y, var=None, sites=None, mean=None):
    """AI_ab = 1/2 alpha' dS_a S^-1 dS_b alpha by the Cholesky route."""
    y = np.asarray(y, np.float64)
    p = unpack(spec, theta, x)
    L = np.linalg.cholesky(train_matrix(spec, *p, x, var, sites))
    alpha = cho_solve((L, True), y - (y.mean() if mean is None else mean))
    U = np.stack([dS @ alpha for dS in derivative_matrices(spec, *p, x, sites)], axis=1)
    V = solve_triangular(L, U, lower=True)
    return 0.5 * V.T @ V


class _Family(object):
    """What reml_forms asks of ai_forms, for the family 'separable' with this spec."""

    def __init__(self, spec):
        self.spec = spec

    def unpack(self, family, theta, x):
        assert family == FAMILY
        return unpack(self.spec, theta, x)

    def train_matrix(self, family, spec, theta, x, var=None, sites=None):
        assert family == FAMILY
        return train_matrix(spec, *unpack(spec, theta, x), x, var, sites)

    def derivative_matrices(self, family, spec, theta, x, sites=None):
        assert family == FAMILY
        return derivative_matrices(spec, *unpack(spec, theta, x), x, sites)


@contextlib.contextmanager
def _in_reml_forms(spec):
    """reml_forms with a _Family in the place of ai_forms, for the calls made inside."""
    keep = RM.AI
    RM.AI = _Family(spec)
    try:
        yield
    finally:
        RM.AI = keep


def _reml_call(name):
    def call(spec, theta, *args, **kw):
        with _in_reml_forms(spec):
            return getattr(RM, name)(FAMILY, spec, theta, *args, **kw)
    call.__name__ = name
    call.__doc__ = 'reml_forms.%s for the separable kernel: (spec, theta, ...) in the place of (family, spec, theta, ...).' % name
    return call


gls = _reml_call('gls')
reml = _reml_call('reml')
reml_grad = _reml_call('reml_grad')
reml_ai = _reml_call('reml_ai')
posterior_fixed = _reml_call('posterior_fixed')


# ---- posteriors -------------------------------------------------------------------------------------------------------------
def posterior(spec, log_ls, log_os, log_noise, x_train, y, var, x_test, sites=None):
    """(mean, variance of the latent field) at x_test by Cholesky, constant mean = mean(y); the prior variance is the site's own."""
    y = np.asarray(y, np.float64)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x_train, var, sites))
    Kx = kernel_matrix(spec, log_ls, log_os, x_test, x_train)
    mu = y.mean() + Kx @ cho_solve((L, True), y - y.mean())
    V = solve_triangular(L, Kx.T, lower=True)
    return mu, prior_var(spec, log_os, x_test) - np.sum(V * V, axis=0)


def component_means(spec, log_ls, log_os, log_noise, x_train, y, var, x_test, sites=None):
    """(mu_s, mu_g): mu_c = K_c(x_test, x_train) alpha, without the constant mean (with the genotype term only)."""
    y = np.asarray(y, np.float64)
    L = np.linalg.cholesky(train_matrix(spec, log_ls, log_os, log_noise, x_train, var, sites))
    alpha = cho_solve((L, True), y - y.mean())
    return tuple(part_matrix(spec, c, log_ls, log_os, x_test, x_train) @ alpha for c in (0, 1))


def genotype_posterior(spec, log_ls, log_os, log_noise, x_train, y, var, sites=None):
    """(mean, cov) of the Q genotype effects u ~ N(0, os_g G): mean = B S^-1 (y - mean(y)), cov = os_g G - B S^-1 B^T with
    B = os_g G[:, g_A]."""
    y = np.asarray(y, np.float64)
    S = train_matrix(spec, log_ls, log_os, log_noise, x_train, var, sites)
    osg = _os(spec, log_os)[1]
    B = osg * table(spec)[:, _split(spec, x_train)[1]]
    return B @ np.linalg.solve(S, y - y.mean()), osg * table(spec) - B @ np.linalg.solve(S, B.T)


def fp32_product(spec, log_ls, log_os, x1, x2=None):
    """The spatial product as an fp32 evaluation rounds it at best: each factor rounded to fp32, then their product, then the
    product with os (the order common.h fixes), from fp64 factor values -- the rounding the product adds to a single form's."""
    fa, fb = factors(spec, log_ls, x1, x2)[:2]
    p = fa.astype(np.float32) * fb.astype(np.float32)
    return np.float32(_os(spec, log_os)[0]) * p
