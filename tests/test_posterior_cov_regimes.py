"""algp_get_posterior_cov (the device side of predictive_distribution, utils.py:293-319: the full M x M covariance and
mi = H(cov_xx) - H(cov)) behind every route the candidate solve can take, and its siblings on the same scratch
(algp_set_entropy / algp_set_inverse_diag) across tile, 512-column-block and task-list boundaries.

The call consumes ALL of the resident V^T -- the solved columns, the columns in [N, Npad), the rows in [M, Mpad) and
the padding row fit_and_solve borrows for y - ybar -- in one Mpad x Mpad x Npad product, and its two log-determinants
sum every pivot of the padded matrices.  mu / var never read the padding and never form an off-diagonal product, so
each route is held here to the full covariance and the MI term: the small sweep at its tile edges, the folded launch,
the solve-only task list, a narrow last tile behind both, and appended columns through the segments route.

Reference: the plain fp64 closed form (_reference below) on inputs that are exactly representable in float32, so one
reference serves both precisions (it IS the closed form on the inputs rounded to the context's dtype).  The sites are
a perturbed unit lattice with a lengthscale of 0.6 spacings: K_** is well conditioned (its Cholesky succeeds in fp64
and in fp32 without jitter), so every case asserts last_jitter() == 0.0.

Tolerances (tests/test_hip_kernels.py): cov 1e-9 / 1e-3 max-abs relative, mi 1e-8 / 5e-3, inverse diagonal
1e-10 / 1e-3, entropies 1e-11 / 1e-4 (fp64 / fp32).  For the largest case (N = 2113, M = 4100, mi = 176.84) the same
closed form evaluated in float32 NumPy is off the fp64 one by 6.9e-6 in cov and 1.0e-7 relative in mi: far inside
the fp32 figures, which therefore hold for every case unchanged.

Left out: the sweep with row statistics.  It needs more than 320 tile rows of candidates (40 961), whose covariance
alone is 13 GB in fp64.
"""
import functools

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from algp_amd import _hip
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

DT = [np.float64, np.float32]
IDS = ['f64', 'f32']
NB = 128                                        # tile of the factor and of V^T (common.h: NB)


def tol(dt, t64, t32):
    return t64 if np.dtype(dt) == np.float64 else t32


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in DT}
    yield c
    for v in c.values():
        v.close()


def _f32(a):
    """Values every context holds exactly: rounded to float32, kept as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _sites(n, D, rng):
    """n sites of a unit lattice (a line for D = 1, a square otherwise) moved by up to 0.2 per axis; further
    dimensions carry small offsets (a Hadamard factor with unit diagonal: it cannot lower K's smallest eigenvalue)."""
    if D == 1:
        base = rng.permutation(n).astype(np.float64)[:, None]
    else:
        side = int(np.ceil(np.sqrt(n)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing='ij'), -1).reshape(-1, 2)
        base = g[rng.permutation(len(g))[:n]].astype(np.float64)
    x = base + rng.uniform(-0.2, 0.2, base.shape)
    if D > 2:
        x = np.hstack([x, rng.uniform(0.0, 0.5, (n, D - 2))])
    return _f32(x)


def _hypers(D, kernel=O.KERNEL_RBF):
    ls = np.r_[np.full(min(D, 2), 0.6), np.full(max(D - 2, 0), 1.5)]
    return O.Hypers(np.log(ls), np.log(1.3), np.log(0.05), kernel)


def _reference(hyp, x, A, y, tvar, cand, extra):
    """utils.py:293-319 in closed form, fp64: S = K_AA + sigma_n^2 [same site] + diag(var), B = K_A*,
    cov = K_** + diag(extra) - B^T S^-1 B, mi = (logdet(K_** + diag(extra)) - logdet(cov)) / 2.  sigma_n^2 also sits on
    the cross entries of two train rows of one site (algp_set_train); two candidate rows of one site share K(x, x)
    without `extra`, which is per row."""
    A = np.asarray(A, np.int64)
    cand = np.asarray(cand, np.int64)
    S = O.kernel_matrix(hyp, x[A]) + hyp.noise * (A[:, None] == A[None, :])
    if tvar is not None:
        S = S + np.diag(tvar)
    L = np.linalg.cholesky(S)
    V = solve_triangular(L, O.kernel_matrix(hyp, x[A], x[cand]), lower=True)
    ybar = float(np.mean(y))
    z = solve_triangular(L, y - ybar, lower=True)
    Kxx = O.kernel_matrix(hyp, x[cand])
    if extra is not None:
        Kxx = Kxx + np.diag(extra)
    cov = Kxx - V.T @ V
    ld_xx = 2.0 * float(np.sum(np.log(np.diag(np.linalg.cholesky(Kxx)))))       # raises if K_** needed a jitter
    ld_cov = 2.0 * float(np.sum(np.log(np.diag(np.linalg.cholesky(cov)))))
    return dict(cov=cov, mi=0.5 * (ld_xx - ld_cov), mu=ybar + V.T @ z, var=np.diag(cov).copy())


def _load(c, hyp, x, A, y, tvar):
    c.set_hypers(hyp.log_lengthscale, hyp.log_outputscale, hyp.log_noise, hyp.kernel)
    c.set_pool(x)
    c.set_train(A, y, tvar)


def _launches(c, solve):
    """Run solve() under the profiler: launch counts of the three route markers."""
    c.prof_enable(True)
    c.prof_reset()
    try:
        solve()
        return {k: c.prof_get(k)['launches'] for k in ('tail_cols', 'dag_panel', 'gemm_trsm')}
    finally:
        c.prof_enable(False)


def _check(c, ref, what=''):
    """The assertions of every case; returns (cov, mi) of the context."""
    dt = c.dtype
    mu0, var0 = c.posterior()
    cov, mi = c.posterior_cov(want_cov=True, want_mi=True)
    assert c.last_jitter() == 0.0, (what, c.last_jitter())
    cov_only, none = c.posterior_cov(want_cov=True, want_mi=False)
    nocov, mi_only = c.posterior_cov(want_cov=False, want_mi=True)
    cov2, mi2 = c.posterior_cov(want_cov=True, want_mi=True)
    assert none is None and nocov is None
    assert np.array_equal(cov, cov_only) and np.array_equal(cov, cov2), what
    assert mi == mi_only == mi2, (what, mi, mi_only, mi2)
    mu1, var1 = c.posterior()
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1), what
    e_cov = relerr(cov, ref['cov'])
    e_mi = abs(mi - ref['mi']) / max(1.0, abs(ref['mi']))
    e_diag = float(np.max(np.abs(np.diag(cov) - var0))) / max(1e-300, float(np.max(np.abs(ref['cov']))))
    e_mu = float(np.max(np.abs(mu0 - ref['mu']))) / max(1.0, float(np.max(np.abs(ref['mu']))))
    print('%s %s: cov %.2e mi %.2e (%.6g) diag-var %.2e mu %.2e' % (what, dt.name, e_cov, e_mi, ref['mi'], e_diag, e_mu))
    assert np.array_equal(cov, cov.T), what
    assert e_cov < tol(dt, 1e-9, 1e-3), (what, e_cov)
    assert mi == pytest.approx(ref['mi'], rel=tol(dt, 1e-8, 5e-3), abs=tol(dt, 1e-8, 5e-3)), (what, mi, ref['mi'])
    assert e_diag < tol(dt, 1e-9, 1e-3), (what, e_diag)             # the same quantity by two summation orders
    assert e_mu < tol(dt, 1e-9, 1e-3), (what, e_mu)
    return cov, mi


# ------------------------------------------------------------------ the small sweep at its tile edges
EDGE = [1, 127, 128, 129, 257]


@functools.lru_cache(maxsize=None)
def _edge_problem(D, kernel):
    rng = np.random.RandomState(100 * D + kernel)
    x = _sites(2 * EDGE[-1], D, rng)
    y = _f32(np.sin(x[:, 0] / 2.0) + 0.1 * rng.standard_normal(len(x)))
    tvar = _f32(rng.choice([0.01, 1.0], len(x)))
    extra = _f32(rng.uniform(0.05, 0.2, len(x)))
    return x, y, tvar, extra


@functools.lru_cache(maxsize=None)
def _edge_reference(D, kernel, N, M, with_extra):
    x, y, tvar, extra = _edge_problem(D, kernel)
    A, cand = np.arange(N), np.arange(EDGE[-1], EDGE[-1] + M)
    return _reference(_hypers(D, kernel), x, A, y[A], tvar[A], cand, extra[cand] if with_extra else None)


@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('with_extra', [True, False], ids=['extra', 'noextra'])
@pytest.mark.parametrize('D', [1, 3, 8])
@pytest.mark.parametrize('kernel', [O.KERNEL_RBF, O.KERNEL_MATERN15], ids=['rbf', 'matern'])
def test_tile_edges_on_the_small_sweep(ctxs, dt, with_extra, D, kernel):
    """N and M one below, on and one above a tile and two tiles, every pair; the three padded coordinate widths
    (D = 1, 3, 8 -> 2, 4, 8); RBF and Matern-1.5; with and without extra_var.  One context serves all pairs in
    ascending and descending sizes, so a smaller problem sees the larger one's leftovers in every buffer."""
    c = ctxs[np.dtype(dt)]
    x, y, tvar, extra = _edge_problem(D, kernel)
    hyp = _hypers(D, kernel)
    pairs = [(N, M) for N in EDGE for M in EDGE[::-1]]
    for N, M in pairs:
        A, cand = np.arange(N), np.arange(EDGE[-1], EDGE[-1] + M)
        _load(c, hyp, x, A, y[A], tvar[A])
        c.factorize()
        c.set_candidates(cand, prior_includes_noise=False, extra_var=extra[cand] if with_extra else None)
        n = _launches(c, c.solve_candidates)
        assert n['tail_cols'] == 0 and n['dag_panel'] == 0, (N, M, n)
        _check(c, _edge_reference(D, kernel, N, M, with_extra), 'N=%d M=%d' % (N, M))


# ------------------------------------------------------------------ candidates that are train sites; an index twice
@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_candidates_in_the_train_set_are_ordinary_rows_without_prior_noise(ctxs, dt):
    """prior_includes_noise = 0: a candidate that is a train site is an ordinary point at the same location
    (cov_xx and cov_xa of utils.py:297-298 carry no noise), and the closed form holds for it."""
    c = ctxs[np.dtype(dt)]
    x, y, tvar, extra = _edge_problem(3, O.KERNEL_RBF)
    hyp = _hypers(3)
    A = np.arange(200)
    cand = np.r_[np.arange(150, 330)]                          # 50 train sites, 130 others
    _load(c, hyp, x, A, y[A], tvar[A])
    c.factorize()
    for e in (extra[cand], None):
        c.set_candidates(cand, prior_includes_noise=False, extra_var=e)
        c.solve_candidates()
        _check(c, _reference(hyp, x, A, y[A], tvar[A], cand, e), 'train-site candidates')


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_a_candidate_listed_twice(ctxs, dt):
    """Two rows of one site: extra_var is per ROW (kmat_kernel adds diag_add only on the row's own diagonal entry),
    so the cross entry of the two copies in cov_xx is K(x, x) = outputscale without it, and in cov it is
    outputscale - |V_j|^2: the site's latent variance.  With a positive extra_var the matrix is not singular."""
    c = ctxs[np.dtype(dt)]
    x, y, tvar, extra = _edge_problem(3, O.KERNEL_RBF)
    hyp = _hypers(3)
    A = np.arange(130)
    cand = np.r_[np.arange(300, 400), 305, 399, 305]           # 305 three times, 399 twice
    e = extra[:len(cand)]
    _load(c, hyp, x, A, y[A], tvar[A])
    c.factorize()
    c.set_candidates(cand, prior_includes_noise=False, extra_var=e)
    c.solve_candidates()
    ref = _reference(hyp, x, A, y[A], tvar[A], cand, e)
    cov, _ = _check(c, ref, 'duplicates')
    t = tol(dt, 1e-9, 1e-3)
    assert abs(cov[5, 100] - (cov[5, 5] - e[5])) < t and abs(cov[100, 102] - (cov[102, 102] - e[102])) < t
    assert abs(cov[99, 101] - (cov[99, 99] - e[99])) < t


# ------------------------------------------------------------------ the routes of the task list
@functools.lru_cache(maxsize=None)
def _big_problem():
    """One lattice for every case from 8 tiles of train rows on: 2 200 train sites, 4 100 candidates."""
    rng = np.random.RandomState(7)
    x = _sites(6300, 2, rng)
    y = _f32(np.sin(x[:, 0] / 3.0) + 0.1 * rng.standard_normal(len(x)))
    tvar = _f32(rng.choice([0.01, 1.0], len(x)))
    return x, y, tvar


BIG_CAND0 = 2200                                 # candidates are sites BIG_CAND0 .. of _big_problem


@functools.lru_cache(maxsize=3)                  # a 4 100 x 4 100 covariance is 134 MB: the dtypes of a case run back to back
def _big_reference(N, M):
    x, y, tvar = _big_problem()
    A, cand = np.arange(N), np.arange(BIG_CAND0, BIG_CAND0 + M)
    return _reference(_hypers(2), x, A, y[A], tvar[A], cand, None)


def _big_load(c, N, M):
    x, y, tvar = _big_problem()
    A = np.arange(N)
    _load(c, _hypers(2), x, A, y[A], tvar[A])
    c.set_candidates(np.arange(BIG_CAND0, BIG_CAND0 + M), prior_includes_noise=False)


N_FOLD = 7 * NB + 4                              # 8 tiles: the smallest train set panel_fits accepts (DAG_MIN_TILES)
M_TASKS = 32 * NB + 4                            # 33 tile rows: the smallest from-scratch solve on the task list


@pytest.mark.parametrize('M,dt', [(M, dt) for M in (200, 256) for dt in DT],
                         ids=['%s-%s' % (m, d) for m in ('z_in_the_last_tile', 'no_padding_row') for d in IDS])
def test_fit_and_solve_on_the_folded_route(ctxs, M, dt):
    """One launch factors S and solves the candidates.  M % 128 != 0: row M of V^T carries y - ybar through the
    launch and must be a zero padding row again afterwards -- it enters cov's padded block and both log-determinants.
    M % 128 == 0: no padding row, z by substitution."""
    c = ctxs[np.dtype(dt)]
    _big_load(c, N_FOLD, M)
    n = _launches(c, c.fit_and_solve)
    assert n == dict(tail_cols=0, dag_panel=1, gemm_trsm=0), n
    _check(c, _big_reference(N_FOLD, M), 'folded M=%d' % M)


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_solve_candidates_on_the_task_list_route(ctxs, dt):
    c = ctxs[np.dtype(dt)]
    _big_load(c, N_FOLD, M_TASKS)
    c.factorize()
    n = _launches(c, c.solve_candidates)
    assert n == dict(tail_cols=0, dag_panel=1, gemm_trsm=0), n
    _check(c, _big_reference(N_FOLD, M_TASKS), 'task list')


N_NARROW = 16 * NB                               # plan_route: narrow needs Npad - 128 >= 2048 full columns ...
M_NARROW = 15 * NB + 10                          # ... and Mpad >= 2048; M < Mpad: the z row's tile keeps every column


@pytest.mark.parametrize('route,r,dt', [(route, r, dt) for route in ('folded', 'tasklist') for r in (1, 16, 64, 65) for dt in DT],
                         ids=['%s-r%d-%s' % (route, r, d) for route in ('folded', 'tasklist') for r in (1, 16, 64, 65) for d in IDS])
def test_a_narrow_last_tile_behind_the_task_list(ctxs, monkeypatch, route, r, dt):
    """A train set that ends r <= 64 columns into its last tile: the launch leaves that column tile out and the tail
    kernel solves the r columns behind it (r = 65: no tail launch, every column in the launch).  The covariance reads
    those columns AND the untouched ones up to Npad; the same state built with $ALGP_TAIL_COLS=0 must agree."""
    c = ctxs[np.dtype(dt)]
    N, M = N_NARROW + r, (M_NARROW if route == 'folded' else M_TASKS)
    _big_load(c, N, M)

    def solve():
        if route == 'folded':
            c.fit_and_solve()
        else:
            c.factorize()
            c.solve_candidates()
    n = _launches(c, solve)
    assert n == dict(tail_cols=1 if r <= 64 else 0, dag_panel=1, gemm_trsm=0), n
    ref = _big_reference(N, M)
    cov, mi = _check(c, ref, '%s r=%d' % (route, r))
    monkeypatch.setenv('ALGP_TAIL_COLS', '0')
    n = _launches(c, solve)
    assert n == dict(tail_cols=0, dag_panel=1, gemm_trsm=0), n
    cov0, mi0 = _check(c, ref, '%s r=%d, no tail' % (route, r))
    assert relerr(cov, cov0) < tol(dt, 1e-9, 1e-3)
    assert mi == pytest.approx(mi0, rel=tol(dt, 1e-8, 5e-3), abs=tol(dt, 1e-8, 5e-3))


# ------------------------------------------------------------------ appended columns through the segments route
# plan_route: p0 >= 2048 unchanged leading train rows, Mpad >= 2048.
# (start, [(rows appended, tail launches, kept columns)]); no tail launch: the 128-column blocks
APPENDS = {
    # 2120: the 20 columns exactly.  2190: [2112, 2176) + [2176, 2192), two ranges of <= 64 in two blocks; Npad grows and
    # V^T moves.  2290: [2176, 2304) is more than 64 columns of one block: back to the 128-column blocks
    'inside_a_block_then_two_ranges_then_blocks': (2100, [(20, 1, 2100), (70, 2, 2112), (100, 0, 2176)]),
    'straddling_a_boundary': (2150, [(40, 1, 2150)]),                         # 2190 crosses 2176: a window of L; V^T moves
    'a_new_block': (17 * NB, [(10, 1, 17 * NB)]),                             # 2186: Npad grows, ldv changes, V^T moves
}


@pytest.mark.parametrize('with_alive', [False, True], ids=['noalive', 'alive'])
@pytest.mark.parametrize('name,dt', [(k, dt) for k in APPENDS for dt in DT], ids=['%s-%s' % (k, d) for k in APPENDS for d in IDS])
def test_appends_through_the_segments_route(ctxs, name, dt, with_alive):
    """factorize(incremental) + solve_candidates(incremental) after an append solve only the new columns of V^T: at
    most 64 of them exactly (the tail kernel; across a 128 boundary with the inverse of a window of L), more as one or
    two 16-aligned ranges of at most 64 columns, else as 128-column blocks.  The first solve is not incremental, so its row stride is exact and an append that grows
    Npad re-lays V^T out.  After every step: against the closed form and against a from-scratch context."""
    N0, steps = APPENDS[name]
    M = M_NARROW
    rng = np.random.RandomState(3)
    alive = (rng.uniform(size=M) < 0.7) if with_alive else None
    scratch = ctxs[np.dtype(dt)]
    c = _hip.Context(dt)
    try:
        _big_load(c, N0, M)
        c.factorize()
        c.solve_candidates()
        N = N0
        for add, tails, kept in steps:
            N += add
            x, y, tvar = _big_problem()
            c.set_train(np.arange(N), y[:N], tvar[:N])
            assert c.factorize(incremental=True) == (N - add) // NB * NB

            def solve():
                solve.kept = c.solve_candidates(incremental=True, alive=alive)
            n = _launches(c, solve)
            assert n['tail_cols'] == tails and n['dag_panel'] == 0 and solve.kept == kept, (n, solve.kept)
            assert (n['gemm_trsm'] > 0) == (tails == 0), n
            ref = _big_reference(N, M)
            cov, mi = _check(c, ref, '%s N=%d' % (name, N))
            _big_load(scratch, N, M)
            scratch.factorize()
            scratch.solve_candidates()
            cov_s, mi_s = scratch.posterior_cov(want_cov=True, want_mi=True)
            assert relerr(cov, cov_s) < tol(dt, 1e-9, 1e-3)
            assert mi == pytest.approx(mi_s, rel=tol(dt, 1e-8, 5e-3), abs=tol(dt, 1e-8, 5e-3))
    finally:
        c.close()


# ------------------------------------------------------------------ the shared scratch; refusals
@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_interleaving_on_the_shared_scratch(ctxs, dt):
    """auxA / auxW / auxInv also serve fit_step (which leaves L^-T in auxW), set_inverse_diag and set_entropy: called
    before and between posterior_cov calls they do not change its bits.  fit_step factors again, which invalidates the
    candidate solve: posterior_cov then refuses until the candidates are solved again."""
    c = ctxs[np.dtype(dt)]
    _big_load(c, N_FOLD, 200)
    c.fit_step()
    c.factorize()
    c.solve_candidates()
    cov, mi = _check(c, _big_reference(N_FOLD, 200), 'after fit_step')
    sub = np.arange(3000, 3300)
    c.set_inverse_diag(sub, np.full(len(sub), 0.3))
    cov1, mi1 = c.posterior_cov(want_cov=True, want_mi=True)
    c.set_entropy(sub[:140])
    cov2, mi2 = c.posterior_cov(want_cov=True, want_mi=True)
    assert np.array_equal(cov, cov1) and np.array_equal(cov, cov2) and mi == mi1 == mi2
    c.fit_step()
    assert c.lib.algp_get_posterior_cov(c.h, None, None) == _hip.ERR_STATE
    c.solve_candidates()
    cov3, mi3 = c.posterior_cov(want_cov=True, want_mi=True)
    assert np.array_equal(cov, cov3) and mi == mi3


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_refusals_and_the_empty_set(dt):
    """An explicit-covariance pool: ALGP_ERR_BAD_ARG.  No candidate solve: ALGP_ERR_STATE.  M = 0: an empty covariance,
    mi = 0, no jitter."""
    x, y, tvar, _ = _edge_problem(3, O.KERNEL_RBF)
    hyp = _hypers(3)
    A = np.arange(100)
    c = _hip.Context(dt)
    try:
        _load(c, hyp, x, A, y[A], tvar[A])
        c.factorize()
        c.set_candidates(np.arange(300, 340), prior_includes_noise=False)
        assert c.lib.algp_get_posterior_cov(c.h, None, None) == _hip.ERR_STATE
        with pytest.raises(ValueError, match='solve_candidates'):
            c.posterior_cov()
        c.set_candidates(np.zeros(0, np.int64), prior_includes_noise=False)
        c.solve_candidates()
        cov, mi = c.posterior_cov(want_cov=True, want_mi=True)
        assert cov.shape == (0, 0) and mi == 0.0 and c.last_jitter() == 0.0
        C = O.kernel_matrix(hyp, x[:340]) + hyp.noise * np.eye(340)
        c.set_pool_cov(C)
        c.set_train(A, y[A], tvar[A])
        c.factorize()
        c.set_candidates(np.arange(300, 340), prior_includes_noise=True)
        c.solve_candidates()
        assert c.lib.algp_get_posterior_cov(c.h, None, None) == _hip.ERR_BAD_ARG
        with pytest.raises(ValueError, match='coordinate pool'):
            c.posterior_cov()
    finally:
        c.close()


# ------------------------------------------------------------------ the two contract holes
@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_train_site_candidates_under_prior_noise_are_refused(ctxs, dt):
    """prior_includes_noise = 1 (greedy semantics): a candidate that is a train site is solved as the unit row e_pos,
    V_j = L^T e_pos, and cov_xx - V^T V is not its covariance (it gave -(sigma_n^2 + var) on that diagonal, zeros
    against ordinary rows, and ALGP_ERR_NOT_PD after the whole jitter ladder for the MI term): ALGP_ERR_STATE, naming
    the candidate.  Without such a candidate the call answers: cov_xx never carries sigma_n^2 (utils.py:297), so it is
    the closed form of the latent covariance and diag(cov) = posterior()'s variance - sigma_n^2."""
    c = ctxs[np.dtype(dt)]
    x, y, tvar, _ = _edge_problem(3, O.KERNEL_RBF)
    hyp = _hypers(3)
    A = np.arange(200)
    _load(c, hyp, x, A, y[A], tvar[A])
    c.factorize()
    c.set_candidates(np.arange(190, 330), prior_includes_noise=True)          # rows 0 .. 9 are train sites
    c.solve_candidates()
    _, var = c.posterior()
    assert c.lib.algp_get_posterior_cov(c.h, None, None) == _hip.ERR_STATE
    with pytest.raises(ValueError, match=r'candidate 0 \(pool index 190\) is a train site'):
        c.posterior_cov(want_cov=True, want_mi=True)
    assert np.array_equal(c.posterior()[1], var)
    cand = np.arange(200, 330)
    c.set_candidates(cand, prior_includes_noise=True)
    c.solve_candidates()
    _, var = c.posterior()
    cov, mi = c.posterior_cov(want_cov=True, want_mi=True)
    ref = _reference(hyp, x, A, y[A], tvar[A], cand, None)
    assert c.last_jitter() == 0.0
    assert relerr(cov, ref['cov']) < tol(dt, 1e-9, 1e-3)
    assert mi == pytest.approx(ref['mi'], rel=tol(dt, 1e-8, 5e-3), abs=tol(dt, 1e-8, 5e-3))
    assert np.max(np.abs(np.diag(cov) - (var - hyp.noise))) < tol(dt, 1e-9, 1e-3)


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_committed_picks_are_refused_until_the_next_solve(ctxs, dt):
    """After algp_greedy / algp_commit_pick, posterior()'s variances include the picks (columns Npad .. ncols of V^T),
    which the covariance's product does not read: the two getters disagreed.  The call now refuses with ALGP_ERR_STATE
    until the candidates are solved again, and then returns the bits it returned before."""
    c = ctxs[np.dtype(dt)]
    x, y, tvar, _ = _edge_problem(3, O.KERNEL_RBF)
    hyp = _hypers(3)
    A = np.arange(200)
    cand = np.arange(200, 330)
    _load(c, hyp, x, A, y[A], tvar[A])
    c.factorize()
    c.set_candidates(cand, prior_includes_noise=True)
    c.solve_candidates()
    _, var = c.posterior()
    cov, mi = c.posterior_cov(want_cov=True, want_mi=True)
    picks = c.greedy(_hip.CRIT_ENTROPY, 0.1, 1.0, 2)
    _, var_picked = c.posterior()
    others = ~np.isin(cand, picks)
    assert np.max(var[others] - var_picked[others]) > 1e-2         # the picks are in the variances ...
    assert c.lib.algp_get_posterior_cov(c.h, None, None) == _hip.ERR_STATE
    with pytest.raises(ValueError, match=r'2 pick\(s\) were committed'):
        c.posterior_cov()                                          # ... so a covariance without them is not handed out
    c.solve_candidates()
    c.commit_pick(int(cand[7]), 0.1, 1.0)
    with pytest.raises(ValueError, match=r'1 pick\(s\) were committed'):
        c.posterior_cov(want_cov=False, want_mi=True)
    c.solve_candidates()
    cov1, mi1 = c.posterior_cov(want_cov=True, want_mi=True)
    assert np.array_equal(cov, cov1) and mi == mi1


# ------------------------------------------------------------------ set_entropy / set_inverse_diag across tiles
SET_M = [1, 127, 128, 129, 300, 513, 1100]      # one tile; trinv_upper's 512-column block; 8 tiles: the one-launch factorisation


@functools.lru_cache(maxsize=None)
def _set_problem():
    rng = np.random.RandomState(11)
    x = _sites(1300, 2, rng)
    var = _f32(rng.uniform(0.01, 1.0, 1300))
    return x, var, rng.permutation(1300)


@functools.lru_cache(maxsize=None)
def _set_reference(m, with_var, twice):
    x, var, perm = _set_problem()
    hyp = _hypers(2)
    idx = _set_idx(m, twice)
    S = O.kernel_matrix(hyp, x[idx]) + hyp.noise * (idx[:, None] == idx[None, :])
    if with_var:
        S = S + np.diag(var[:m])
    return S, np.diag(np.linalg.inv(S)).copy(), m * O.CONST + 0.5 * np.linalg.slogdet(S)[1]


def _set_idx(m, twice):
    idx = _set_problem()[2][:m].copy()
    if twice and m > 1:
        idx[m - 1] = idx[0]                      # one site in two rows: sigma_n^2 on their cross entries, var per row
    return idx


@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('pool', ['coords', 'cov'])
@pytest.mark.parametrize('with_var,twice', [(True, False), (False, False), (True, True)], ids=['var', 'novar', 'var-twice'])
@pytest.mark.parametrize('m', SET_M)
def test_set_entropy_and_inverse_diag_across_tiles(dt, pool, with_var, twice, m, set_ctxs):
    """H(S) and diag(S^-1) of a listed subset, S = C[idx, idx] + diag(var), against slogdet / inv of the fp64 matrix:
    across one tile, trinv_upper's 512-column block (its push into the trailing block) and the 8-tile switch to the
    one-launch factorisation; a coordinate pool and an explicit covariance; an index listed twice (with var: without
    it the two rows are equal and S is singular)."""
    c = set_ctxs[(np.dtype(dt), pool)]
    x, var, perm = _set_problem()
    idx = _set_idx(m, twice)
    S, dinv, H = _set_reference(m, with_var, twice)
    v = var[:m] if with_var else None
    H1 = c.set_entropy(idx, v)
    d, H2 = c.set_inverse_diag(idx, v)
    print('m=%d %s: H %.2e diag %.2e' % (m, c.dtype.name, abs(H1 - H) / abs(H), relerr(d, dinv)))
    assert H1 == pytest.approx(H, rel=tol(dt, 1e-11, 1e-4))
    assert H2 == H1
    assert relerr(d, dinv) < tol(dt, 1e-10, 1e-3)


@pytest.fixture(scope='module')
def set_ctxs():
    x, var, perm = _set_problem()
    hyp = _hypers(2)
    out = {}
    for dt in DT:
        for pool in ('coords', 'cov'):
            c = _hip.Context(dt)
            c.set_hypers(hyp.log_lengthscale, hyp.log_outputscale, hyp.log_noise)
            if pool == 'coords':
                c.set_pool(x)
            else:
                c.set_pool_cov(O.kernel_matrix(hyp, x) + hyp.noise * np.eye(len(x)))
            out[(np.dtype(dt), pool)] = c
    yield out
    for c in out.values():
        c.close()
