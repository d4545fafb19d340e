"""The variance-reduction utility of whole paths (algp_score_paths_vr) on the host: its definition by brute force, the closed
form the library evaluates, and the problems, paths and references that tests/test_paths_vr.py runs on the GPU.

Definition (include/algp_hip.h): T = the candidates without a train row; path p reads each of its distinct sites once with
variance sm = mobile_std^2 -- a new site joins the train set with noise sm, a site with a train row of noise v ends with
v sm / (v + sm) --
    u_p = sum_{j in T} var(j | A) - sum_{j in T} var(j | A u path_p).
`brute_force` is that sentence in fp64 NumPy, one refit per path, on C = oracle.gp_oracle.kernel_matrix + sigma_n^2 I like
vr_reference of tests/test_variance_reduction.py.  `closed_form` is u_p = tr((Gamma_SS + sm I)^-1 Phi_SS) with Gamma the
posterior covariance of the union of the paths' sites and Phi = E E^T, E their cross covariance with the targets.

The two agree to 1e-9 |brute| + 64 eps sum_T var(j | A): the second term is the brute force's own cancellation (the difference
of two sums of |T| variances), which is all that is left of a utility below 1e-4 such as one re-measured static site's.

Nothing here needs a device.
"""
import os
import re

import numpy as np
import pytest

from oracle import gp_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS, SM = 0.1, 1.0                                    # static_std, mobile_std
SHAPES = [(100, 40, 2), (300, 130, 2), (400, 129, 6)]
SHAPE_IDS = ['n100-N40-D2', 'n300-N130-D2', 'n400-N129-D6']
# path lengths per shape: 64 is the LDS kernel's last size (and that union spans two ragged tiles); 65 .. 256 cover both
# block paddings of the batched route and the off-by-one on each side of 128
LENGTHS = {SHAPES[0]: (1, 5, 20), SHAPES[1]: (3, 40, 64), SHAPES[2]: (65, 128, 129, 200, 256)}
# one problem whose candidate rows pass the library's E chunk (PVR_CHUNK target columns per product), N = 128, D = 2
CHUNK_SHAPE = (16700, 128, 2)
CHUNK_LENGTHS = (7, 33, 64)
KERNELS = [O.KERNEL_RBF, O.KERNEL_MATERN15]
KIDS = ['rbf', 'matern']


class Problem(object):
    def cov(self, rows, cols):
        """C[rows, cols]: the pool covariance, sigma_n^2 where the pool indices coincide"""
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        return O.kernel_matrix(self.hyp, self.X[rows], self.X[cols]) + self.hyp.noise * (rows[:, None] == cols[None, :])


_PROBLEMS, _REFS = {}, {}


def problem(shape, kernel):
    """The generator of tests/test_variance_reduction.py: coordinates in [0, 12]^D, lengthscales in [2, 4], outputscale 1.3,
    noise 0.05; the first third of the train sites static, the rest mobile; every site a candidate."""
    key = (shape, kernel)
    if key not in _PROBLEMS:
        n, N, D = shape
        rng = np.random.RandomState(1000 * n + 10 * D + kernel)
        p = Problem()
        p.key, p.n, p.N, p.D = key, n, N, D
        p.X = rng.uniform(0.0, 12.0, size=(n, D))
        p.hyp = O.Hypers(np.log(rng.uniform(2.0, 4.0, size=D)), np.log(1.3), np.log(0.05), kernel)
        perm = rng.permutation(n)
        p.A = perm[:N]
        p.ns = N // 3
        p.noise = np.r_[np.full(p.ns, SS ** 2), np.full(N - p.ns, SM ** 2)]
        p.static = p.A[:p.ns]
        p.mobile = p.A[p.ns:]
        p.cand = np.arange(n)
        p.alive = np.ones(n, bool)
        p.alive[p.static] = False
        p.free = perm[N:]                            # the ordinary rows = the targets
        p.lengths = CHUNK_LENGTHS if shape == CHUNK_SHAPE else LENGTHS[shape]
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


def make_paths(p):
    """(sites, names): per length an all-new path and one mixing new and statically sampled sites, then one path of a
    single statically sampled site, an empty path and a path that lists a site twice; -1 padded rows of pool indices."""
    rng = np.random.RandomState(5 + p.n)
    rows, names = [], []
    for k in p.lengths:
        rows.append([int(v) for v in rng.choice(p.free, k, replace=False)])
        names.append('new%d' % k)
        m = min(max(1, k // 4), len(p.static))
        mixed = [int(v) for v in rng.choice(p.free, k - m, replace=False)] + [int(v) for v in rng.choice(p.static, m, replace=False)]
        rows.append([mixed[i] for i in rng.permutation(k)])
        names.append('mixed%d' % k)
    rows.append([int(p.static[1])])
    names.append('one-static')
    rows.append([])
    names.append('empty')
    a, b, c = (int(v) for v in p.free[:3])
    rows.append([a, b, a, c])
    names.append('twice')
    sites = np.full((len(rows), max(len(r) for r in rows)), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        sites[i, :len(r)] = r
    return sites, names


def distinct(row):
    return [int(j) for j in dict.fromkeys(int(v) for v in row) if j >= 0]


def closed_form(p, sites, sm=SM ** 2):
    """(utilities, sum_T var(j | A)) in fp64: Gamma and Phi over the union of the paths' sites, then one small solve per path"""
    paths = [distinct(r) for r in sites]
    L = np.linalg.cholesky(p.cov(p.A, p.A) + np.diag(p.noise))
    V = np.linalg.solve(L, p.cov(p.A, p.free))
    prior = p.hyp.outputscale + p.hyp.noise
    base = float(prior * len(p.free) - np.sum(V * V))
    U = sorted(set(j for pth in paths for j in pth))
    if not U:
        return np.zeros(len(paths)), base
    pos = {s: i for i, s in enumerate(U)}
    R = np.linalg.solve(L, p.cov(p.A, U))            # a train site's column is C[A, s] too: S e_l - v_l e_l
    Gam = p.cov(U, U) - R.T @ R
    E = p.cov(U, p.free) - R.T @ V
    Phi = E @ E.T
    out = np.zeros(len(paths))
    for i, pth in enumerate(paths):
        if pth:
            ix = np.ix_([pos[s] for s in pth], [pos[s] for s in pth])
            out[i] = np.trace(np.linalg.solve(Gam[ix] + sm * np.eye(len(pth)), Phi[ix]))
    return out, base


def brute_force(p, sites, sm=SM ** 2):
    """(utilities, sum_T var(j | A)) in fp64: one refit per path"""
    T = p.free
    prior = p.hyp.outputscale + p.hyp.noise

    def sumvar(train, nz):
        S = p.cov(train, train) + np.diag(nz)
        B = p.cov(train, T)
        return float(prior * len(T) - np.sum(B * np.linalg.solve(S, B)))

    train0, noise0 = [int(a) for a in p.A], [float(v) for v in p.noise]
    where = {s: i for i, s in enumerate(train0)}
    base = sumvar(train0, noise0)
    out = np.zeros(len(sites))
    for i, row in enumerate(sites):
        train, nz = list(train0), list(noise0)
        for s in distinct(row):
            if s in where:
                nz[where[s]] = nz[where[s]] * sm / (nz[where[s]] + sm)
            else:
                train.append(s)
                nz.append(sm)
        if len(train) > len(train0) or nz != noise0:
            out[i] = base - sumvar(train, nz)
    return out, base


def reference(shape, kernel):
    """(problem, sites, names, closed-form utilities), computed once per problem and shared"""
    key = (shape, kernel)
    if key not in _REFS:
        p = problem(shape, kernel)
        sites, names = make_paths(p)
        _REFS[key] = (p, sites, names, closed_form(p, sites)[0])
    return _REFS[key]


@pytest.mark.parametrize('shape,kernel',
                         [pytest.param(s, k, id=si + '-' + ki) for s, si in zip(SHAPES, SHAPE_IDS) for k, ki in zip(KERNELS, KIDS)] +
                         [pytest.param(CHUNK_SHAPE, O.KERNEL_RBF, id='chunk-rbf')])
def test_closed_form_equals_one_refit_per_path(shape, kernel):
    """every case of the GPU file: its three shapes under both kernels, and the chunk case (which runs under RBF there)"""
    p, sites, names, closed = reference(shape, kernel)
    brute, base = brute_force(p, sites)
    slack = 64 * np.finfo(np.float64).eps * base
    for nm, a, b in zip(names, closed, brute):
        print('%-10s closed %.12e brute %.12e diff %.2e (allowed %.2e)' % (nm, a, b, abs(a - b), 1e-9 * abs(b) + slack))
        assert abs(a - b) <= 1e-9 * abs(b) + slack, nm
    assert closed[names.index('empty')] == 0.0
    assert np.all(closed[[i for i, nm in enumerate(names) if nm != 'empty']] > 0.0)
    top = np.sort(closed)[-2:]
    assert (top[1] - top[0]) / top[1] > 1e-7       # the GPU file compares the argmax


def test_the_chunk_case_passes_the_library_chunk():
    text = open(os.path.join(REPO, 'algp_amd', 'csrc', 'api_paths_vr.hip')).read()
    m = re.search(r'constexpr int64_t PVR_CHUNK = (\d+);', text)
    assert m, 'PVR_CHUNK not found'
    chunk = int(m.group(1))
    n = CHUNK_SHAPE[0]
    assert chunk % 128 == 0 and n > chunk + 128      # a second chunk with targets of its own
    p = problem(CHUNK_SHAPE, O.KERNEL_RBF)
    assert np.any(p.free < chunk) and np.any(p.free >= chunk)
    sites, _ = make_paths(p)
    assert sites.shape[0] <= 9 and sites.shape[1] <= 64 and p.N == 128 and p.D == 2


def test_max_var_red_is_a_path_strategy():
    """run_ipp's strategy check takes 'MaxVarRed' (under any criterion) and still refuses an unknown name; under the
    variance-reduction criterion every other strategy keeps raising."""
    from algp_amd.agent import Agent
    with pytest.raises(AssertionError, match='Unknown criterion'):
        Agent.run_ipp(object(), criterion='no-such-criterion', strategy='MaxVarRed')
    with pytest.raises(AssertionError, match='Unknown strategy'):
        Agent.run_ipp(object(), criterion='entropy', strategy='no-such-strategy')
    for strategy in ('MaxEnt', 'Shortest', 'Equi-Sample'):
        with pytest.raises(NotImplementedError, match='MaxVarRed'):
            Agent.run_ipp(object(), criterion='variance_reduction', strategy=strategy)


def test_score_paths_vr_is_declared_and_bound():
    from algp_amd import _hip
    text = open(os.path.join(REPO, 'include', 'algp_hip.h')).read()
    assert re.search(r'\bint algp_score_paths_vr\(algp_ctx\* ctx, const int64_t\* sites, int npaths, int maxlen, double mobile_std,'
                     r'\s*int64_t max_union,\s*double\* dV_out\);', text)
    assert 'algp_score_paths_vr' in _hip.SIGNATURES
    assert hasattr(_hip.Context, 'score_paths_vr')
