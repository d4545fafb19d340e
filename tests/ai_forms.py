"""The average-information matrix of the MLL (include/algp_hip.h, algp_get_mll_ai) in NumPy fp64, built on tests/matern_forms.py,
tests/additive_forms.py and tests/relationship_forms.py and independent of the library and of the oracle: what
tests/test_ai_forms_host.py, tests/test_average_information.py and tests/test_fit_ai.py compare against.

    AI_ab = 1/2 alpha' dS/dtheta_a S^-1 dS/dtheta_b alpha,   alpha = S^-1 (y - mean)

theta are the log hyper-parameters in the gradient's order.  A model is (family, spec):

    'single'        spec = kernel id                 theta = [log ls_0..D), log os, log sigma_n^2]
    'additive'      spec = (kernel_a, kernel_b, split)       [log ls_0..D), log os_a, log os_b, log sigma_n^2]
    'relationship'  spec = (kernel_a, G or None, Q)          [log ls_0..D-1), log os_a, log os_g, log sigma_n^2]

(the last column of x is the genotype id under 'relationship').  dS/dlog ls_d = dk u_d^2 of the part that owns coordinate d,
dS/dlog os = the part's kernel matrix, dS/dlog sigma_n^2 = sigma_n^2 E with E_ij = 1 where rows i and j are one pool site.
"""
import functools

import numpy as np
from scipy.linalg import cho_solve, solve_triangular

import additive_forms as AF
import matern_forms as MF
import relationship_forms as RF


def n_lengthscales(family, x):
    D = np.asarray(x).reshape(len(x), -1).shape[1]
    return D - 1 if family == 'relationship' else D


def unpack(family, theta, x):
    """theta -> (log_ls, log_os, log_noise); log_os a float for 'single', else a pair."""
    theta = np.asarray(theta, np.float64)
    nl = n_lengthscales(family, x)
    if family == 'single':
        return theta[:nl], float(theta[nl]), float(theta[nl + 1])
    return theta[:nl], (float(theta[nl]), float(theta[nl + 1])), float(theta[nl + 2])


def pack(log_ls, log_os, log_noise):
    return np.r_[np.atleast_1d(log_ls), np.atleast_1d(log_os), log_noise].astype(np.float64)


def _forms(family):
    return {'single': MF, 'additive': AF, 'relationship': RF}[family]


def train_matrix(family, spec, theta, x, var=None, sites=None):
    log_ls, log_os, log_noise = unpack(family, theta, x)
    return _forms(family).train_matrix(spec, log_ls, log_os, log_noise, x, var, sites)


def mll_and_grad(family, spec, theta, x, y, var=None, sites=None, mean=None):
    """(MLL, gradient) of the whole train set; raises numpy.linalg.LinAlgError where S is not positive definite."""
    log_ls, log_os, log_noise = unpack(family, theta, x)
    F = _forms(family)
    return (F.mll(spec, log_ls, log_os, log_noise, x, y, var, sites, mean),
            F.mll_grad(spec, log_ls, log_os, log_noise, x, y, var, sites, mean))


def derivative_matrices(family, spec, theta, x, sites=None):
    """[dS/dtheta_a] in the gradient's order."""
    x = np.asarray(x, np.float64)
    x = x.reshape(len(x), -1)
    N = len(x)
    log_ls, log_os, log_noise = unpack(family, theta, x)
    if family == 'single':
        parts = [(0, x.shape[1], spec, log_os)]
    elif family == 'additive':
        ka, kb, split = spec
        parts = [(0, split, ka, log_os[0]), (split, x.shape[1], kb, log_os[1])]
    else:
        parts = [(0, x.shape[1] - 1, spec[0], log_os[0])]
    u2 = MF.scaled_sq(log_ls, x[:, :len(log_ls)])
    d_ls, d_os = [], []
    for lo, hi, kid, los in parts:
        r = np.sqrt(sum(u2[lo:hi]))
        dk = np.exp(los) * MF.dk_of_r(kid, r)
        d_ls += [dk * u2[d] for d in range(lo, hi)]
        d_os.append(np.exp(los) * MF.k_of_r(kid, r))
    if family == 'relationship':
        d_os.append(RF.part_matrix(spec, 1, log_ls, log_os, x))
    return d_ls + d_os + [np.exp(log_noise) * MF.same_site(sites, N)]


def alpha_of(family, spec, theta, x, y, var=None, sites=None, mean=None):
    """(S, L, alpha)."""
    y = np.asarray(y, np.float64)
    S = train_matrix(family, spec, theta, x, var, sites)
    L = np.linalg.cholesky(S)
    return S, L, cho_solve((L, True), y - (y.mean() if mean is None else mean))


def average_information(family, spec, theta, x, y, var=None, sites=None, mean=None):
    """AI by the Cholesky route: u_a = dS/dtheta_a alpha, V = L^-1 [u_a], AI = 1/2 V' V."""
    _, L, alpha = alpha_of(family, spec, theta, x, y, var, sites, mean)
    U = np.stack([dS @ alpha for dS in derivative_matrices(family, spec, theta, x, sites)], axis=1)
    V = solve_triangular(L, U, lower=True)
    return 0.5 * V.T @ V


def relative_error(ai, want):
    """The largest entry error relative to sqrt(want_aa want_bb)."""
    s = np.sqrt(np.diag(want))
    return float(np.max(np.abs(ai - want) / np.outer(s, s)))


# ---- the six N = 300 fits of test_ai_forms_host.py and test_fit_ai.py ------------------------------------------------------
NEWTON_N = 300
NEWTON_CASES = ['rbf', 'matern15', 'matern05', 'matern25', 'additive', 'relationship']


@functools.lru_cache(maxsize=None)
def newton_case(name):
    """dict(family, spec, x, y, var, theta_true, kernel_params): spatial x ~ U(0, 2 sqrt(N / 4))^2, var = 1e-5, y drawn from the
    model at theta_true with RandomState(0).  Single forms: lengthscales (1.3, 2.0), outputscale 0.9, noise 0.05.  Additive:
    Matern-3/2 over the two spatial columns plus RBF over a U(0, 6) covariate (lengthscale 1.0, outputscale 0.6).  Relationship:
    30 genotypes x 10 plots, marker_relationship(Q=30, m=80), lengthscales (1.5, 2.5), outputscales (0.6, 0.8), noise 0.1.
    Computed once, never written to.  kernel_params: what GPR takes for the same model."""
    N = NEWTON_N
    rng = np.random.RandomState(0)
    x = rng.uniform(0, 2.0 * np.sqrt(N / 4.0), (N, 2))
    if name == 'additive':
        family, spec = 'additive', (MF.MATERN15, MF.RBF, 2)
        x = np.c_[x, rng.uniform(0, 6.0, N)]
        theta = pack(np.log([1.3, 2.0, 1.0]), np.log([0.9, 0.6]), np.log(0.05))
        kp = {'type': 'additive', 'split': 2, 'parts': ({'type': 'matern', 'nu': 1.5}, {'type': 'rbf'})}
    elif name == 'relationship':
        G = RF.marker_relationship(Q=30, m=80)
        family, spec = 'relationship', (MF.MATERN15, G, 30)
        x = np.c_[x, rng.permutation(np.repeat(np.arange(30), 10)).astype(np.float64)]
        theta = pack(np.log([1.5, 2.5]), np.log([0.6, 0.8]), np.log(0.1))
        kp = {'type': 'genotype', 'spatial': {'type': 'matern', 'nu': 1.5}, 'relationship': G, 'n_genotypes': 30}
    else:
        kid, kp = {'rbf': (MF.RBF, {'type': 'rbf'}), 'matern15': (MF.MATERN15, {'type': 'matern', 'nu': 1.5}),
                   'matern05': (MF.MATERN05, {'type': 'matern', 'nu': 0.5}), 'matern25': (MF.MATERN25, {'type': 'matern', 'nu': 2.5})}[name]
        family, spec = 'single', kid
        theta = pack(np.log([1.3, 2.0]), np.log(0.9), np.log(0.05))
    var = np.full(N, 1e-5)
    y = np.linalg.cholesky(train_matrix(family, spec, theta, x, var)) @ rng.standard_normal(N)
    for a in (x, y, var, theta):
        a.setflags(write=False)
    return dict(family=family, spec=spec, x=x, y=y, var=var, theta_true=theta, kernel_params=kp)


@functools.lru_cache(maxsize=None)
def newton_host_fit(name):
    """(theta, info) of utils.ai_newton driven by the forms from theta = 0 on newton_case(name), 40 evaluations at most."""
    from algp_amd.utils import ai_newton
    c = newton_case(name)
    args = (c['family'], c['spec'])
    P = len(c['theta_true'])
    theta, info = ai_newton(np.zeros(P), lambda t: mll_and_grad(*args, t, c['x'], c['y'], c['var']),
                            lambda t: average_information(*args, t, c['x'], c['y'], c['var']),
                            max_evaluations=40, n=NEWTON_N)
    theta.setflags(write=False)
    return theta, info
