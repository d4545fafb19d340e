"""The three utilities of whole paths (algp_score_paths, algp_score_paths_mi, algp_score_paths_vr) in NumPy fp64, independent of
the library: what tests/test_path_regimes.py compares every route against, the problems it runs on and the table of its cases
(built here, without a device; tests/test_path_forms_host.py holds the helpers to the oracle and proves the conditions the
bounds of the GPU file rest on).

Pool covariance C = k + sigma_n^2 where the pool indices coincide (greedy semantics, prior_includes_noise = 1).  The train set
A holds each sampled site once, row l with noise var_l (static-only: ss, mobile-only: sm).  A path reads each of its distinct
sites once with noise sm; -1 entries are no site.

  entropy_gain        k CONST + 1/2 (log det S_{A u P} - log det S_A); a site that is train row l already gets a SECOND row
                      (cross entry k + sigma_n^2, its own noise sm) -- tests/test_hip_greedy.py's definition, evaluated
                      through the Schur complement G = C_PP + sm I - V_P^T V_P of the fp64 Cholesky factor of S_A
  mi_terms            (dH_A, dH_Abar, dH_all) from log-determinants of the sets themselves, fused form: a re-measured train site
                      keeps its row, its noise v -> v sm / (v + sm)
  variance_reduction  sum_T w_j var(j | A) - sum_T w_j var(j | A u path), one refit per path (fused form), T = the candidates
                      without a train row

Every input is rounded to values fp32 holds exactly (coordinates, noises, weights; length-scales 2^k or 1.5 * 2^k), so both
precisions see the same numbers.  static_std = 0.5, mobile_std = 0.75, sigma_n^2 = 2^-5, outputscale 1: with these the train
matrix and every path's block stay below cond 1e3 (proved by the host file), so the bounds of the GPU file hold for the
reference alone and a miss is the library's.

CASES: name -> problem, the site rows, and the route each entry point must take for them (api_paths.hip, api_paths_vr.hip):
'lds' (at most 64 distinct sites: one workgroup per path), 'batched128', 'batched256' (2 x 2 tiled factorisations at ppad = 128
or 256).  For the entropy and MI scorers the call's longest path decides (under MI the route is that of its dH_A term; its P and
Q blocks are always batched, at ppad = 128 up to 128 sites); for VR every path has its own: the short ones take the LDS kernel,
the long ones the batches at the padding of the longest, 'none' for an empty path.
"""
import functools
import types

import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular

import matern_forms as MF

CONST = 0.5 * (1.0 + np.log(2.0 * np.pi))
STATIC_STD, MOBILE_STD = 0.5, 0.75
SS, SM = STATIC_STD ** 2, MOBILE_STD ** 2
LOG_NOISE = np.log(2.0 ** -5)
KNAMES = {MF.RBF: 'rbf', MF.MATERN15: 'matern15', MF.MATERN05: 'matern05', MF.MATERN25: 'matern25'}


def f32(a):
    """Values both precisions hold exactly: rounded to float32, kept as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- problems -----------------------------------------------------------------------------------------------------------
def _layout(name):
    """(X, log_ls, train sites in row order, how many of the first and last rows are static-only)"""
    if name == 'small':                                  # 24 x 24 unit grid; N = 129: Npad = 256, the last tile ragged
        gi, gj = np.meshgrid(np.arange(24), np.arange(24), indexing='ij')
        X = np.c_[gi.ravel(), gj.ravel()].astype(np.float64)
        return X, np.log([1.5, 2.0]), 129, (40, 40), 11
    if name == 'mid':                                    # D = 5 (DP = 8); N = 300, 270 of them static-only
        rng = np.random.RandomState(501)
        return f32(rng.uniform(0, 5, (900, 5))), np.log([2.0, 3.0, 2.0, 3.0, 2.0]), 300, (140, 130), 12
    if name == 'wide':                                   # N = 2100: Npad = 2176 > 2048, a second 2048-column block
        rng = np.random.RandomState(502)
        return f32(rng.uniform(0, 60, (2400, 2))), np.log([1.5, 2.0]), 2100, (1000, 1000), 13
    if name == 'full':                                   # every site sampled (static-only): paths only re-measure
        gi, gj = np.meshgrid(np.arange(5), np.arange(8), indexing='ij')
        X = np.c_[gi.ravel(), gj.ravel()].astype(np.float64)
        return X, np.log([1.5, 2.0]), 40, (20, 20), 14
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def problem(name, kid):
    """`name` is 'small', 'mid', 'wide', 'full', or 'mid400': mid with a candidate set of 400 rows (300 unsampled sites and 100
    static-only ones).  The train rows are [static-only ... | mobile-only ... | static-only ...]: rows 0 and N - 1 can be
    re-measured."""
    base = 'mid' if name == 'mid400' else name
    X, log_ls, N, (s0, s1), seed = _layout(base)
    rng = np.random.RandomState(seed)
    n = len(X)
    perm = rng.permutation(n)
    A = perm[:N].astype(np.int64)
    static = np.zeros(n, bool)
    mobile = np.zeros(n, bool)
    static[A[:s0]] = True
    static[A[N - s1:]] = True
    mobile[A[s0:N - s1]] = True
    var = np.where(static[A], SS, SM)
    cand = np.where(~mobile)[0].astype(np.int64)
    if name == 'mid400':
        free = np.where(~static & ~mobile)[0]
        cand = np.sort(np.r_[rng.permutation(free)[:300], rng.permutation(A[:s0])[:100]]).astype(np.int64)
    p = types.SimpleNamespace(name=name, kid=kid, X=X, D=X.shape[1], n=n, N=N, A=A, var=var, static=static, mobile=mobile,
                              log_ls=log_ls, log_os=0.0, log_noise=LOG_NOISE, noise=np.exp(LOG_NOISE), cand=cand,
                              prior_includes_noise=1)
    p.C = MF.kernel_matrix(kid, log_ls, 0.0, X) + p.noise * np.eye(n)
    p.row = np.full(n, -1, np.int64)
    p.row[A] = np.arange(N)
    in_cand = np.zeros(n, bool)
    in_cand[cand] = True
    p.free = np.where(in_cand & ~static & ~mobile)[0]           # the candidates without a train row: VR's targets
    p.st = A[static[A] & in_cand[A]]                            # re-measurable candidates, in train-row order
    p.SA = p.C[np.ix_(A, A)] + np.diag(var)
    p.L = np.linalg.cholesky(p.SA)
    return p


# ---- the helpers --------------------------------------------------------------------------------------------------------
def distinct(row):
    return [int(j) for j in dict.fromkeys(int(v) for v in row) if j >= 0]


def path_block(p, sites, sm=SM):
    """G = C_PP + sm I - V_P^T V_P of the path's distinct sites (second rows for train sites: C carries sigma_n^2 between them)"""
    u = distinct(sites)
    V = solve_triangular(p.L, p.C[np.ix_(p.A, u)], lower=True)
    return p.C[np.ix_(u, u)] + sm * np.eye(len(u)) - V.T @ V


def entropy_gain(p, sites, sm=SM):
    u = distinct(sites)
    if not u:
        return 0.0
    Lg = np.linalg.cholesky(path_block(p, sites, sm))
    return len(u) * CONST + float(np.sum(np.log(np.diag(Lg))))


def _logdet(M):
    return 2.0 * float(np.sum(np.log(np.diag(np.linalg.cholesky(M))))) if len(M) else 0.0


def _state(p, var):
    """[H(A), H(Abar), H(all)] of the state whose sampled sites are var < inf"""
    sampled = np.isfinite(var)
    a, b = np.where(sampled)[0], np.where(~sampled)[0]
    hA = len(a) * CONST + 0.5 * _logdet(p.C[np.ix_(a, a)] + np.diag(var[a]))
    hB = len(b) * CONST + 0.5 * _logdet(p.C[np.ix_(b, b)])
    hAll = p.n * CONST + 0.5 * _logdet(p.C + np.diag(np.where(sampled, var, 0.0)))
    return np.array([hA, hB, hAll])


_BASE = {}


def mi_terms(p, sites, ss=SS, sm=SM):
    """(dH_A, dH_Abar, dH_all) of changing the path's sites, each from log-determinants of the sets themselves"""
    assert ss == SS and np.all(p.var[p.static[p.A]] == ss)
    var = np.full(p.n, np.inf)
    var[p.A] = p.var
    key = (p.name, p.kid)
    if key not in _BASE:
        _BASE[key] = _state(p, var)
    after = var.copy()
    for s in distinct(sites):
        after[s] = sm if not np.isfinite(var[s]) else var[s] * sm / (var[s] + sm)
    if not distinct(sites):
        return np.zeros(3)
    return _state(p, after) - _BASE[key]


def _sumvar(p, train, nz, w):
    T = p.free
    B = p.C[np.ix_(train, T)]
    Z = cho_solve(cho_factor(p.C[np.ix_(train, train)] + np.diag(nz), lower=True), B)
    return float(np.sum(w * (np.diag(p.C)[T] - np.sum(B * Z, axis=0))))


def variance_reduction(p, sites, sm=SM, weights=None):
    """one refit per path; weights: one per pool site (the targets' are read)"""
    w = np.ones(len(p.free)) if weights is None else np.asarray(weights, np.float64)[p.free]
    u = distinct(sites)
    if not u or not len(p.free):
        return 0.0
    train, nz = [int(a) for a in p.A], [float(v) for v in p.var]
    key = (p.name, p.kid, None if weights is None else np.asarray(weights).tobytes())
    if key not in _BASE:
        _BASE[key] = _sumvar(p, train, nz, w)
    for s in u:
        if p.row[s] >= 0:
            nz[p.row[s]] = nz[p.row[s]] * sm / (nz[p.row[s]] + sm)
        else:
            train.append(s)
            nz.append(sm)
    return _BASE[key] - _sumvar(p, train, nz, w)


def fuse_constant(p, sites, sm=SM):
    """row form -> fused form: CONST + 1/2 log(v + sm) per re-measured site (include/algp_hip.h, algp_score_paths)"""
    return sum(CONST + 0.5 * np.log(p.var[p.row[s]] + sm) for s in distinct(sites) if p.row[s] >= 0)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def _new(p, rng, k):
    return [int(v) for v in rng.choice(p.free, k, replace=False)]


def _rm(p, rng, k):
    return [int(v) for v in rng.choice(p.st, k, replace=False)]


def _mixed(p, rng, k, krm):
    s = _new(p, rng, k - krm) + _rm(p, rng, krm)
    return [s[i] for i in rng.permutation(k)]


def route(k):
    """the rule of the code: used <= 64 -> LDS, <= 128 -> ppad 128, otherwise 256"""
    return 'none' if k == 0 else 'lds' if k <= 64 else 'batched128' if k <= 128 else 'batched256'


def _length_rows(k):
    def rows(p, rng):
        return [_new(p, rng, k), _mixed(p, rng, k, max(1, k // 4)) if k > 1 else _rm(p, rng, 1)]
    return rows


def _shape5(p, rng):
    a = _new(p, rng, 5)
    s = _rm(p, rng, 1)[0]
    return [a, [-1, a[0], a[1], -1, a[2]], [a[3], a[3], a[4], a[3], -1], [-1] * 5, [s, a[1], a[4], -1, -1]]


def _shape64(p, rng):
    return [_mixed(p, rng, 64, 9), _new(p, rng, 10) + [-1] * 54, _mixed(p, rng, 63, 5) + [-1]]


def _shape70(p, rng):
    """maxlen 70, at most 64 DISTINCT sites: the LDS route although the array is wider than its 64 slots"""
    a = _mixed(p, rng, 64, 6)
    b = _new(p, rng, 20)
    return [a[:30] + [-1] + a[30:50] + [a[3], a[3], -1] + a[50:] + [a[63], -1],
            [-1] * 40 + b + [b[0]] * 10,
            [-1] * 70]


def _shape262(p, rng):
    """maxlen 262 > ppad: a 130-site path behind -1 entries and repeats, an empty path in a batched call, a leading -1"""
    a = _mixed(p, rng, 130, 20)
    b = _new(p, rng, 5)
    return [[-1] * 60 + a[:100] + [a[0], a[99], -1] * 10 + a[100:] + [-1] * 42,
            [-1] * 262,
            [-1] + b + [-1] * 256,
            _new(p, rng, 70) + [-1] * 192]


def _mix(lengths):
    def rows(p, rng):
        return [_mixed(p, rng, k, k // 5) for k in lengths]
    return rows


def _rm_edges(long):
    """second readings of train row 0 and of train row N - 1, alone and among new sites (long: inside 70-site paths)"""
    def rows(p, rng):
        first, last = int(p.A[0]), int(p.A[-1])
        assert p.row[first] == 0 and p.row[last] == p.N - 1 and p.static[first] and p.static[last]
        k = 69 if long else 3
        return [_new(p, rng, k) + [first], [last] + _new(p, rng, k), [first], [last], [first, last]]
    return rows


def _rm_only(lengths):
    def rows(p, rng):
        return [_rm(p, rng, k) for k in lengths]
    return rows


def _rm_at_tile_edge(p, rng):
    """200 sites, second readings at packed positions 127, 128 and 129: both sides of the 128-row tile of the block"""
    a, r = _new(p, rng, 197), _rm(p, rng, 3)
    return [a[:127] + r + a[127:], _new(p, rng, 200)]


def _wide(k, rows_of):
    def rows(p, rng):
        rm = [int(p.A[r]) for r in rows_of(rng)]
        assert all(p.static[s] for s in rm)
        s = _new(p, rng, k - len(rm)) + rm
        return [[s[i] for i in rng.permutation(k)]]
    return rows


def _full(p, rng):
    return [_rm(p, rng, 1), _rm(p, rng, 5), _rm(p, rng, 40)]


def _vr_batches(p, rng):
    """one 129-site path, then 960 paths of 65 sites, all from the 400 candidate rows (second readings among them)"""
    pool = np.r_[p.free, p.st]
    return [[int(v) for v in rng.choice(pool, 129, replace=False)]] + \
           [[int(v) for v in rng.choice(pool, 65, replace=False)] for _ in range(960)]


def _case(prob, rows, seed, ent, mi, vr, entries=('ent', 'mi', 'vr'), argmax=True):
    return types.SimpleNamespace(problem=prob, rows=rows, seed=seed, routes={'ent': ent, 'mi': mi, 'vr': vr}, entries=entries,
                                 argmax=argmax)


CASES = {}
for _k in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256):
    CASES['len%d' % _k] = _case('small' if _k <= 64 else 'mid', _length_rows(_k), 100 + _k, route(_k), route(_k), [route(_k)] * 2)
CASES.update({
    'shape_maxlen5': _case('small', _shape5, 201, 'lds', 'lds', ['lds', 'lds', 'lds', 'none', 'lds']),
    'shape_maxlen64': _case('small', _shape64, 202, 'lds', 'lds', ['lds'] * 3),
    'shape_maxlen70_64distinct': _case('small', _shape70, 203, 'lds', 'lds', ['lds', 'lds', 'none']),
    'shape_maxlen262_130sites': _case('small', _shape262, 204, 'batched256', 'batched256', ['batched256', 'none', 'lds', 'batched256']),
    'mixed_7_65': _case('mid', _mix([7, 65]), 301, 'batched128', 'batched128', ['lds', 'batched128']),
    'mixed_64_65_3': _case('mid', _mix([64, 65, 3]), 302, 'batched128', 'batched128', ['lds', 'batched128', 'lds']),
    'mixed_30_129_128_1': _case('mid', _mix([30, 129, 128, 1]), 303, 'batched256', 'batched256',
                                ['lds', 'batched256', 'batched256', 'lds']),
    'rm_row0_rowN_lds': _case('small', _rm_edges(False), 401, 'lds', 'lds', ['lds'] * 5),
    'rm_row0_rowN_batched': _case('mid', _rm_edges(True), 402, 'batched128', 'batched128', ['batched128'] * 2 + ['lds'] * 3),
    'rm_only_3_64': _case('mid', _rm_only([3, 64]), 403, 'lds', 'lds', ['lds', 'lds']),
    'rm_only_65_3': _case('mid', _rm_only([65, 3]), 404, 'batched128', 'batched128', ['batched128', 'lds']),
    'rm_only_130_64': _case('mid', _rm_only([130, 64]), 405, 'batched256', 'batched256', ['batched256', 'lds']),
    'rm_at_127_128_129': _case('mid', _rm_at_tile_edge, 406, 'batched256', 'batched256', ['batched256'] * 2),
    'wide_3_row2090': _case('wide', _wide(3, lambda g: [2090 + g.randint(10)]), 501, 'lds', None, ['lds'], ('ent', 'vr'), False),
    'wide_65_rows5_2090': _case('wide', _wide(65, lambda g: [5, 2090 + g.randint(10)]), 502, 'batched128', None, ['batched128'],
                                ('ent', 'vr'), False),
    'wide_130_forty_rows_2048': _case('wide', _wide(130, lambda g: 2048 + g.permutation(52)[:40]), 503, 'batched256', None,
                                      ['batched256'], ('ent', 'vr'), False),
    'full_1_5_40': _case('full', _full, 601, 'lds', 'lds', ['lds'] * 3, ('ent', 'mi')),
    'vr_weights_40_70_200': _case('mid', _mix([40, 70, 200]), 701, None, None, ['lds', 'batched256', 'batched256'], ('vr',)),
    'vr_batches': _case('mid400', _vr_batches, 702, None, None, ['batched256'] * 961, ('vr',)),
})
# every case with more than one path and an argmax assertion: the host file proves the margin of the top two
KERNELS_EVERYWHERE = (MF.RBF, MF.MATERN15)
EXTRA_KERNELS = {'mixed_30_129_128_1': (MF.MATERN05,), 'mixed_64_65_3': (MF.MATERN25,)}     # once each, batched routes, on mid


@functools.lru_cache(maxsize=None)
def sites_of(name):
    """(sites array npaths x maxlen, -1 padded; the rows as lists): the same for every kernel"""
    case = CASES[name]
    p = problem(case.problem, MF.RBF)
    rows = case.rows(p, np.random.RandomState(case.seed))
    sites = np.full((len(rows), max(len(r) for r in rows)), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        sites[i, :len(r)] = r
    sites.setflags(write=False)
    return sites, rows


@functools.lru_cache(maxsize=None)
def weights_of(name):
    """fp32-exact target weights, a quarter of them zero"""
    p = problem(CASES[name].problem, MF.RBF)
    rng = np.random.RandomState(CASES[name].seed + 1)
    w = np.round(rng.uniform(0.25, 4.0, p.n) * 8) / 8
    w[rng.permutation(p.n)[:p.n // 4]] = 0.0
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(name, kid):
    """{'ent': (npaths,), 'mi': (npaths, 3), 'vr': (npaths,)} for the case's entry points: computed once, never written to"""
    case = CASES[name]
    p = problem(case.problem, kid)
    _, rows = sites_of(name)
    w = weights_of(name) if name.startswith('vr_weights') else None
    out = {}
    if 'ent' in case.entries:
        out['ent'] = np.array([entropy_gain(p, r) for r in rows])
    if 'mi' in case.entries:
        out['mi'] = np.array([mi_terms(p, r) for r in rows])
    if 'vr' in case.entries:
        out['vr'] = np.array([variance_reduction(p, r, weights=w) for r in rows])
    for v in out.values():
        v.setflags(write=False)
    return out


def kernels_of(name):
    """RBF and Matern-3/2 for every case but the batching one: that one is about the host's loop over batches, and its 961
    refits are paid once"""
    return (MF.RBF,) if name == 'vr_batches' else KERNELS_EVERYWHERE + EXTRA_KERNELS.get(name, ())
