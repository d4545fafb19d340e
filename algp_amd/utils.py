"""Posterior / entropy helpers with the reference's names and return conventions
(reference utils.py:10, 188-194, 227-228, 293-319), computed by libalgp_hip.so.

`predictive_distribution` replaces the reference's explicit inverse (utils.py:300), its two dense
GEMMs (utils.py:300-305) and its slogdets (utils.py:314) with: one blocked Cholesky of
K_aa + diag(var) + sigma_n^2 I, one blocked triangular solve for all test points, fused row
reductions for mean and variance, and (only when asked) the full covariance and two log-dets.
"""
import numpy as np

from . import _hip

CONST = .5 * np.log(2 * np.pi * np.exp(1))                    # utils.py:10

_default_ctx = {}


def default_context(dtype=np.float64, device=0):
    """Lazily created module-level context for the free functions below."""
    key = (np.dtype(dtype).name, device)
    if key not in _default_ctx:
        _default_ctx[key] = _hip.Context(dtype, device)
    return _default_ctx[key]


def entropy_from_cov(cov, constant=CONST, ctx=None):
    """H = k*constant + 1/2 log det cov (utils.py:188-194) from a Cholesky factor on the GPU.
    A non positive definite `cov` raises LinAlgError (the reference silently drops slogdet's
    sign, utils.py:193)."""
    if constant is None:
        constant = CONST
    cov = np.asarray(cov)
    k = cov.shape[0]
    if k == 0:
        return 0.0
    dt = np.float32 if cov.dtype == np.float32 else np.float64
    c = ctx if ctx is not None else default_context(dt)
    return c.entropy_from_cov(cov) + k * (constant - CONST)


def predictive_distribution(gp, train_x, train_y, test_x, train_var=None, test_var=None, return_var=False,
                            return_cov=False, return_mi=False):
    """Exact GP posterior at `test_x` (utils.py:293-319), same return-tuple convention:
    mu | (mu, var) | (mu, cov) | (mu, mi) | (mu, cov, mi); `return_mi` overrides `return_var`."""
    c = gp.ctx
    gp.sync_hypers()
    train_x = np.asarray(train_x, dtype=np.float64)
    train_x = train_x.reshape(len(train_x), -1)
    test_x = np.asarray(test_x, dtype=np.float64)
    test_x = test_x.reshape(len(test_x), -1)
    N, M = len(train_x), len(test_x)
    c.set_pool(np.vstack([train_x, test_x]))
    fixed = getattr(gp, 'fixed_effects', None) is not None     # a gp with fixed effects: the trend-aware mean, variance and covariance
    if fixed:
        c.set_fixed_effects(gp.fixed_basis(np.vstack([train_x, test_x]), train_x))
    c.set_train(np.arange(N), train_y, train_var)              # mean-centring inside (utils.py:294)
    test_idx = np.arange(N, N + M)
    if fixed:                                                  # (mi stays the known-mean term)
        c.set_candidates(test_idx, prior_includes_noise=False, extra_var=test_var)
        c.fit_and_solve()
        mu, var, proj = c.posterior_fixed(want_var=return_var, want_proj=return_cov)
        cov = mi = None
        if return_cov or return_mi:
            cov, mi = c.posterior_cov(want_cov=return_cov, want_mi=return_mi)
            if return_cov:
                cov = cov + proj @ proj.T
        if return_cov and return_mi:
            return mu, cov, mi
        return (mu, mi) if return_mi else (mu, cov) if return_cov else (mu, var) if return_var else mu
    if not (return_var or return_cov or return_mi):
        c.factorize()                                          # replaces inv(cov_aa), utils.py:300
        return c.posterior_mean(test_idx)                      # mu only: no triangular solve needed
    c.set_candidates(test_idx, prior_includes_noise=False, extra_var=test_var)
    c.fit_and_solve()                                          # the factorisation and V^T = B^T L^-T (utils.py:300-301): ONE task-list
                                                               # launch up to 51 200 test sites, two phases beyond
    mu, var = c.posterior()
    res = None
    if return_var:
        res = (mu, var)
    cov = mi = None
    if return_cov or return_mi:
        cov, mi = c.posterior_cov(want_cov=return_cov, want_mi=return_mi)
    if return_cov:
        res = (mu, cov)
    if return_mi:
        res = (mu, mi)
    if return_cov and return_mi:
        res = (mu, cov, mi)
    return res


_MATERN_NU = {_hip.KERNEL_MATERN05: 0.5, _hip.KERNEL_MATERN15: 1.5, _hip.KERNEL_MATERN25: 2.5}


def _rng(rng):
    return rng if isinstance(rng, np.random.RandomState) else np.random.RandomState(rng)


def spectral_draws(kernel_id, D, n_features, rng):
    """(omega, phase): n_features random Fourier frequencies of the kernel's spectral density for UNIT lengthscale,
    (n_features, D) float64, and phases ~ U[0, 2 pi), (n_features,) float64, so that with x scaled by 1 / lengthscale
    E[2 os cos(omega . x + phase) cos(omega . x' + phase)] = k(x, x').  RBF: omega ~ N(0, I); Matern-nu: a multivariate
    Student-t with 2 nu degrees of freedom, omega = z sqrt(2 nu / c), z ~ N(0, I), c ~ chi^2(2 nu), one c per feature.
    Drawn from `rng` (a RandomState or a seed) in this order: z, c (Matern only), phase.
    The additive kernel: kernel_id = ('additive', split, id_a, id_b, os_a, os_b).  The normalised spectral density of a sum
    of kernels is the mixture of the parts' densities with weights os_c / (os_a + os_b), so every feature belongs to one
    part, chosen with that probability: its frequencies are that part's draw in the part's own coordinates and ZERO in the
    other's, and the amplitude is sqrt(2 (os_a + os_b) / F) (algp_sample_posterior).  Order: the parts' uniform draws (F),
    part a's z and c, part b's z and c, phase.
    The separable kernel: kernel_id = ('separable', split, id_a, id_b).  A product over disjoint coordinate groups has the
    product of the parts' spectral measures, so EVERY feature takes omega_a from part a's law in part a's coordinates and
    omega_b from part b's in the others, concatenated; the amplitude is sqrt(2 os / F) as for a single form.  Order: part a's
    z and c, part b's z and c, phase."""
    rng = _rng(rng)
    D, F = int(D), int(n_features)
    if isinstance(kernel_id, tuple) and kernel_id[0] == 'separable':
        _, split, id_a, id_b = kernel_id
        split = int(split)
        omega = np.empty((F, D))
        for ident, lo, hi in ((id_a, 0, split), (id_b, split, D)):
            w = rng.standard_normal((F, hi - lo))
            if ident != _hip.KERNEL_RBF:
                if ident not in _MATERN_NU:
                    raise NotImplementedError('spectral_draws: kernel id %r' % (ident,))
                w = w * np.sqrt(2.0 * _MATERN_NU[ident] / rng.chisquare(2.0 * _MATERN_NU[ident], size=F))[:, None]
            omega[:, lo:hi] = w
        phase = rng.uniform(0.0, 2.0 * np.pi, size=F)
        return np.ascontiguousarray(omega, dtype=np.float64), np.ascontiguousarray(phase, dtype=np.float64)
    if isinstance(kernel_id, tuple):
        _, split, id_a, id_b, os_a, os_b = kernel_id
        split = int(split)
        in_a = rng.uniform(size=F) < os_a / (os_a + os_b)
        omega = np.zeros((F, D))
        for ident, lo, hi, mine in ((id_a, 0, split, in_a), (id_b, split, D, ~in_a)):
            w = rng.standard_normal((F, hi - lo))
            if ident != _hip.KERNEL_RBF:
                if ident not in _MATERN_NU:
                    raise NotImplementedError('spectral_draws: kernel id %r' % (ident,))
                w = w * np.sqrt(2.0 * _MATERN_NU[ident] / rng.chisquare(2.0 * _MATERN_NU[ident], size=F))[:, None]
            omega[mine, lo:hi] = w[mine]
        phase = rng.uniform(0.0, 2.0 * np.pi, size=F)
        return np.ascontiguousarray(omega, dtype=np.float64), np.ascontiguousarray(phase, dtype=np.float64)
    omega = rng.standard_normal((F, D))
    if kernel_id != _hip.KERNEL_RBF:
        if kernel_id not in _MATERN_NU:
            raise NotImplementedError('spectral_draws: kernel id %r' % (kernel_id,))
        nu = _MATERN_NU[kernel_id]
        omega = omega * np.sqrt(2.0 * nu / rng.chisquare(2.0 * nu, size=F))[:, None]
    phase = rng.uniform(0.0, 2.0 * np.pi, size=F)
    return np.ascontiguousarray(omega, dtype=np.float64), np.ascontiguousarray(phase, dtype=np.float64)


def relationship_prior_draws(kernel_a, log_lengthscale, os_a, os_g, G, n_genotypes, x, n_samples, n_features, rng, chunk=4096):
    """(n_samples, len(x)) float64 draws of the PRIOR of the relationship kernel os_a kappa_a(r_a) + os_g G[g, g'] at the sites
    `x` (last column: the genotype ids; kernel_a = ('separable', split, id_a, id_b): the separable product as the spatial part), built on the host in NumPy -- the genotype part has no spectral density, so the device's
    features mode cannot draw it, and the result goes to algp_sample_posterior in values mode.
    Spatial part: n_features random Fourier features of kappa_a over the D - 1 spatial coordinates scaled by 1 / lengthscale,
    amplitude sqrt(2 os_a / F), evaluated in chunks of `chunk` sites.  Genotype part: u = sqrt(os_g) chol(G + jitter I) xi with
    jitter = 1e-10 max(diag G) (u = sqrt(os_g) xi for G None), gathered by id.  Drawn from `rng` in this order:
    spectral_draws(kernel_a, D - 1, n_features, rng), the weights standard_normal((n_samples, n_features)), xi
    standard_normal((n_samples, Q))."""
    rng = _rng(rng)
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(len(x), -1)
    S, F, Ds = int(n_samples), int(n_features), x.shape[1] - 1
    ids = x[:, -1].astype(np.int64)
    Q = int(n_genotypes) if G is None else int(np.shape(G)[0])
    omega, phase = spectral_draws(kernel_a, Ds, F, rng)
    weights = rng.standard_normal((S, F))
    xi = rng.standard_normal((S, Q))
    xs = x[:, :Ds] * np.exp(-np.asarray(log_lengthscale, dtype=np.float64).reshape(-1))
    out = np.empty((S, len(x)))
    amp = np.sqrt(2.0 * os_a / F)
    for i0 in range(0, len(x), int(chunk)):
        i1 = min(len(x), i0 + int(chunk))
        out[:, i0:i1] = amp * (weights @ np.cos(xs[i0:i1] @ omega.T + phase).T)
    if G is None:
        u = np.sqrt(os_g) * xi
    else:
        G = np.asarray(G, dtype=np.float64)
        Lg = np.linalg.cholesky(G + 1e-10 * np.max(np.diag(G)) * np.eye(Q))
        u = np.sqrt(os_g) * (xi @ Lg.T)
    out += u[:, ids]
    return out


def posterior_samples(gp, train_x, train_y, test_x, train_var=None, n_samples=1, n_features=2048, rng=None):
    """(n_samples, len(test_x)) joint draws of the latent field at `test_x` given the train data, by pathwise conditioning
    on the device (algp_sample_posterior): pool, train set and candidates exactly as predictive_distribution sets them
    (prior_includes_noise=False), the prior draw from `n_features` random Fourier features of the kernel.  Everything random
    comes from `rng` (a RandomState or a seed), in this order: spectral_draws(kernel, D, n_features, rng), the weights
    standard_normal((n_samples, n_features)), the train-noise draws standard_normal((n_samples, N)).
    Under the genotype kernel the prior is drawn on the host at every pool site (relationship_prior_draws, whose draws come
    first, in its own order) and passed in values mode; then the train-noise draws standard_normal((n_samples, N)).
    A model with fixed effects (GPR(fixed_effects=...)) gives draws of the total signal mean + h' beta + f with beta's
    uncertainty in them (algp_sample_posterior_fixed), from the same draws in the same order."""
    c = gp.ctx
    gp.sync_hypers()
    rng = _rng(rng)
    train_x = np.asarray(train_x, dtype=np.float64)
    train_x = train_x.reshape(len(train_x), -1)
    test_x = np.asarray(test_x, dtype=np.float64)
    test_x = test_x.reshape(len(test_x), -1)
    N, M = len(train_x), len(test_x)
    c.set_pool(np.vstack([train_x, test_x]))
    fixed = getattr(gp, 'fixed_effects', None) is not None
    if fixed:
        c.set_fixed_effects(gp.fixed_basis(np.vstack([train_x, test_x]), train_x))
    c.set_train(np.arange(N), train_y, train_var)
    c.set_candidates(np.arange(N, N + M), prior_includes_noise=False)
    c.fit_and_solve()
    hyp = gp.hypers()
    if isinstance(hyp[3], tuple) and hyp[3][0] == 'genotype':
        G, Q = gp.model.relationship
        prior = relationship_prior_draws(hyp[3][1], hyp[0], np.exp(hyp[1][0]), np.exp(hyp[1][1]), G, Q, np.vstack([train_x, test_x]),
                                         n_samples, n_features, rng)
        eps = rng.standard_normal((int(n_samples), N))
        return c.sample_posterior(eps, prior=prior, fixed=fixed)
    if isinstance(hyp[3], tuple) and hyp[3][0] == 'separable':
        kid = hyp[3]
    else:
        kid = hyp[3] + tuple(np.exp(hyp[1])) if isinstance(hyp[3], tuple) else hyp[3]  # additive: with the two outputscales
    omega, phase = spectral_draws(kid, train_x.shape[1], n_features, rng)
    weights = rng.standard_normal((int(n_samples), int(n_features)))
    eps = rng.standard_normal((int(n_samples), N))
    return c.sample_posterior(eps, weights=weights, omega=omega, phase=phase, fixed=fixed)


def group_posterior(gp, train_x, train_y, test_x, group, train_var=None, test_var=None, weight=None, n_groups=None,
                    return_cross=False):
    """(mean, cov) or (mean, cov, cross): the joint posterior of the aggregates g_q = sum_{j in q} a_j f(test_x_j) of the
    latent field over groups of test sites -- a genotype's plots, a field row -- on the device (algp_group_posterior): pool,
    train set and candidates exactly as predictive_distribution sets them (prior_includes_noise=False, extra_var=test_var).
    group, weight, n_groups: see Context.group_posterior; cov = A Sigma A^T for the Sigma predictive_distribution returns
    with return_cov, without that matrix being formed; cross = A Sigma.
    A model with fixed effects (GPR(fixed_effects=...)) gives the aggregates of the total signal mean + h' beta + f with the
    effects estimated (algp_group_posterior_fixed): Sigma then carries the universal-kriging term."""
    c = gp.ctx
    gp.sync_hypers()
    train_x = np.asarray(train_x, dtype=np.float64)
    train_x = train_x.reshape(len(train_x), -1)
    test_x = np.asarray(test_x, dtype=np.float64)
    test_x = test_x.reshape(len(test_x), -1)
    N, M = len(train_x), len(test_x)
    c.set_pool(np.vstack([train_x, test_x]))
    fixed = getattr(gp, 'fixed_effects', None) is not None
    if fixed:
        c.set_fixed_effects(gp.fixed_basis(np.vstack([train_x, test_x]), train_x))
    c.set_train(np.arange(N), train_y, train_var)
    c.set_candidates(np.arange(N, N + M), prior_includes_noise=False, extra_var=test_var)
    c.fit_and_solve()
    if fixed:
        mean, cov, cross = c.group_posterior(group, weight=weight, n_groups=n_groups, want_cov=True, want_cross=return_cross, fixed=True)
        return (mean, cov, cross) if return_cross else (mean, cov)
    mean, cov, cross = c.group_posterior(group, weight=weight, n_groups=n_groups, want_cov=True, want_cross=return_cross)
    return (mean, cov, cross) if return_cross else (mean, cov)


def ai_newton(theta0, value_and_grad, information, free=None, max_evaluations=60, gtol=1e-6, n=1):
    """Maximise a marginal log likelihood by damped Newton steps on its average-information matrix (AI-REML's iteration;
    Gilmour, Thompson & Cullis 1995).  Pure NumPy: the caller supplies the numbers.

    value_and_grad(theta) -> (MLL, gradient); it may raise numpy.linalg.LinAlgError or return a non-finite MLL where S is not
    positive definite.  information(theta) -> the AI matrix; it is only ever called for the point value_and_grad was last
    called for and accepted.  free: the entries of theta that are optimised (indices or a mask; default all) -- the others
    stay fixed and their rows and columns of AI are dropped.

    From lambda = 1e-2: the trial step is delta = solve(AI + lambda diag(diag AI), g), clipped elementwise to +-2 (log units).
    A trial whose MLL is finite and larger is accepted: lambda <- max(lambda / 10, 1e-8), and the trial's own gradient and the
    AI matrix at it are taken, so no point is evaluated twice.  Any other trial is rejected: lambda <- 10 lambda, again from the
    same point.  AI is positive semi-definite, so every step is an ascent direction.  It ends with reason 'gradient' when
    max|g_free| / n < gtol, 'stalled' when lambda passes 1e8, or 'max_evaluations' (calls of value_and_grad, the first included).

    Returns (theta, info): info has evaluations, iterations (accepted steps), reason, mll, grad_max (max|g_free| / n), damping
    (the last lambda) and trace (the MLL at the start and at every accepted point)."""
    theta = np.array(theta0, dtype=np.float64).reshape(-1)
    P = len(theta)
    if free is None:
        free = np.arange(P)
    else:
        free = np.asarray(free)
        free = np.flatnonzero(free) if free.dtype == bool else free.astype(np.int64).reshape(-1)
    f, g = value_and_grad(theta.copy())
    if not np.isfinite(f):
        raise np.linalg.LinAlgError('ai_newton: the MLL is not finite at the initial parameters')
    g = np.asarray(g, dtype=np.float64)
    A = np.asarray(information(theta.copy()), dtype=np.float64)
    evaluations, iterations, lam, trace = 1, 0, 1e-2, [float(f)]
    while True:
        grad_max = float(np.max(np.abs(g[free]))) / n if len(free) else 0.0
        if grad_max < gtol:
            reason = 'gradient'
            break
        if lam > 1e8:
            reason = 'stalled'
            break
        if evaluations >= max_evaluations:
            reason = 'max_evaluations'
            break
        Af = A[np.ix_(free, free)]
        try:
            delta = np.linalg.solve(Af + lam * np.diag(np.diag(Af)), g[free])
        except np.linalg.LinAlgError:
            delta = None
        if delta is None or not np.all(np.isfinite(delta)):
            lam *= 10.0                                        # a singular damped matrix: more damping, nothing to evaluate
            continue
        trial = theta.copy()
        trial[free] += np.clip(delta, -2.0, 2.0)
        evaluations += 1
        try:
            ft, gt = value_and_grad(trial.copy())
        except np.linalg.LinAlgError:                          # S is not positive definite there: a rejected trial
            ft, gt = np.nan, None
        if np.isfinite(ft) and ft > f:
            theta, f, g = trial, ft, np.asarray(gt, dtype=np.float64)
            A = np.asarray(information(theta.copy()), dtype=np.float64)
            lam = max(lam / 10.0, 1e-8)
            iterations += 1
            trace.append(float(f))
        else:
            lam *= 10.0
    return theta, dict(evaluations=evaluations, iterations=iterations, reason=reason, mll=float(f), grad_max=grad_max,
                       damping=lam, trace=trace)


def heritability(log_os_a, log_os_g, log_noise, gbar, cov3):
    """(h2, se) under the relationship kernel: h2 = gbar os_g / (gbar os_g + os_a + sigma_n^2), gbar the mean of diag G (1 for
    the identity table), with the delta-method standard error on the log parameters: d = dh2/d(log os_a, log os_g,
    log sigma_n^2) = (-h2 os_a / tot, h2 (1 - h2), -h2 sigma_n^2 / tot), se = sqrt(d' C d).  cov3 = C is the block of those
    three parameters of the INVERSE of the whole average-information matrix (the marginal covariance, not the inverse of the
    block); 2 x 2 -- (log os_a, log os_g) -- where the noise was not learned."""
    osa, osg, s2 = np.exp(log_os_a), np.exp(log_os_g), np.exp(log_noise)
    tot = gbar * osg + osa + s2
    h2 = gbar * osg / tot
    d = np.array([-h2 * osa / tot, h2 * (1.0 - h2), -h2 * s2 / tot])
    C = np.asarray(cov3, dtype=np.float64)
    if C.shape == (2, 2):
        d = d[:2]
    elif C.shape != (3, 3):
        raise ValueError('heritability: cov3 must be 3 x 3 (2 x 2 with the noise not learned), got %s' % (C.shape,))
    return float(h2), float(np.sqrt(max(d @ C @ d, 0.0)))


def compute_mae(true, pred):
    return np.mean(np.abs(true - pred))                        # utils.py:227-228


def generate_gaussian_data(num_rows, num_cols, k=5, min_var=10, max_var=100, algo='sum'):
    """Mixture-of-Gaussians field on an integer grid (utils.py:90-108); draws from the global
    np.random stream in the reference's order (row means, column means, variances)."""
    xx, yy = np.meshgrid(np.arange(num_cols), np.arange(num_rows))
    grid = np.vstack([yy.flatten(), xx.flatten()]).transpose()
    mr = np.random.uniform(0, num_rows, size=k)
    mc = np.random.uniform(0, num_cols, size=k)
    var = np.random.uniform(min_var, max_var, size=k)
    y = np.zeros(num_rows * num_cols)
    for i in range(k):
        bump = np.exp(-((grid[:, 0] - mr[i]) ** 2 + (grid[:, 1] - mc[i]) ** 2) / var[i])
        y = np.maximum(y, bump) if algo == 'max' else y + bump
    return grid, y


def find_shortest_path(paths_cost):
    """utils.py:365-368: random choice among the minimum-cost paths."""
    cost = np.asarray(paths_cost)
    return int(np.random.choice(np.where(cost == cost.min())[0]))


def find_equi_sample_path(paths_indices, idx):
    """utils.py:371-373: random choice among the paths that collect as many samples as path idx."""
    lens = np.array([len(p) for p in paths_indices])
    return int(np.random.choice(np.where(lens == lens[idx])[0]))
