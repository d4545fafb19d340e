"""The greedy picks (algp_scores / algp_best_candidate / algp_commit_pick / algp_greedy, agent.py:295-356) behind every
coordinate width, kernel, row length and route of lazy_refresh_kernel (vecops.hip).

Every pick after the first goes through that kernel: the full pass as mode 2 (flush_lazy), the picks-only route as modes
0 and 1, a remote commit on one row (the cooperative one-row instance, also mode 2 with M = 1).  It is compiled for the
padded coordinate widths DP = 2, 4, 8 and takes its cross covariance from pick_bprime (an RBF and a Matern-1.5 branch);
its dot products (row_dot_one_wave / row_dot_virtual_wave) start a second stride past 1024 16-byte vectors, i.e. beyond
2048 columns in fp64 and 4096 in fp32.

Two references, both fp64 NumPy, neither the code under test:
 - per pick, oracle.gp_oracle.greedy_fast on C = kernel_matrix + sigma_n^2 I (one Cholesky + rank-1 appends);
 - independent of that rank-1 algebra, after the last pick of every route ONE dense Cholesky of the train set A u picks
   (_dense: a new site carries the static noise, a mobile-sampled site that was picked the fused one): the posterior
   variance of every surviving ordinary row, [S^-1]_jj of every surviving unit row (directly, and through the utility
   1/2 log(1 + delta s_jj) where the row is alive).  posterior() / scores() flush first, so the check fails if the rows
   of V^T fall behind the picks.

Inputs: coordinates uniform on a cube of side 1.25 n^(1/D) (dense enough that far sites do not all sit at the prior and
tie), rounded to float32 so one reference serves both precisions; one length-scale per dimension from [1.5, 3.5];
outputscale 1, sigma_n^2 = 1e-2, static / mobile std 0.1 / 1.0.

Tolerances: fp64 utilities 1e-9 max(1, max|u|), variances 1e-9; fp32 utilities 1e-3 max|u|, variances and [S^-1]_jj
1e-3 (tests/test_hip_greedy.py).  The fp32 figures hold unchanged in the new regimes; measured
on an MI355X against the fp64 oracle: N = 4100 utilities off by 6.2e-5 (RBF) and 4.5e-5 (Matern) of max|u| 1.87 / 1.64,
variances by 1.3e-6; 128 picks utilities by 1.4e-5 of 1.92, variances by 2.9e-7.

Pick sequences of free runs are compared with the oracle's only where the oracle's top-two gap exceeds 1e-6 (fp64) or
1e-2 (fp32: ten times the utility tolerance) at EVERY pick; the seeds (SEEDS below; found with the oracle alone, see
_gap) are chosen so that no fp64 case is skipped, and every test asserts the skipped share of the file's fp32 cases
(_assert_skipped_share: at most one in four), so that a change of inputs cannot silently empty the comparison.
Utilities along the oracle's forced picks, the dense check and every bit-for-bit comparison run in every case.
"""
import functools
import types

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from algp_amd import _hip
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

DT = [np.float64, np.float32]
IDS = ['f64', 'f32']
KERNELS = [O.KERNEL_RBF, O.KERNEL_MATERN15]
KIDS = ['rbf', 'matern']
ENT = _hip.CRIT_ENTROPY
S_STD, M_STD = 0.1, 1.0
SS, SM = S_STD ** 2, M_STD ** 2
VF = 1.0 / (1.0 / SS + 1.0 / SM)
DELTA = VF - SM
GAP = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-2}
MAX_APPEND = 128                                 # common.h


def tol(dt, t64, t32):
    return t64 if np.dtype(dt) == np.float64 else t32


@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in DT}
    yield c
    for v in c.values():
        v.close()


def _f32(a):
    """Values every context holds exactly: rounded to float32, kept as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------ problems and the two references
def _problem(key, seed, n, D, kernel, n_static, n_mobile, overlap, explicit=False, side=None):
    """n sites on the cube; `n_static` static sites and `n_mobile` mobile-sampled ones of which `overlap` are both.
    Candidates are the sites that are not static (agent.py:318): the mobile-only ones are unit rows of B^T."""
    rng = np.random.RandomState(seed)
    X = _f32(rng.uniform(0.0, side or 1.25 * n ** (1.0 / D), (n, D)))
    hyp = O.Hypers(np.log(rng.uniform(1.5, 3.5, D)), 0.0, np.log(1e-2), kernel)
    perm = rng.permutation(n)
    static = np.zeros(n, bool)
    mobile = np.zeros(n, bool)
    static[perm[:n_static]] = True
    mobile[perm[n_static - overlap:n_static - overlap + n_mobile]] = True
    p = types.SimpleNamespace(key=key, n=n, D=D, X=X, hyp=hyp, static=static, mobile=mobile, explicit=explicit, rng=rng)
    p.C = O.kernel_matrix(hyp, X) + hyp.noise * np.eye(n)
    p.A = np.where(static | mobile)[0]
    p.var = np.where(static[p.A] & mobile[p.A], VF, np.where(static[p.A], SS, SM))
    p.pos_in_A = -np.ones(n, np.int64)
    p.pos_in_A[p.A] = np.arange(len(p.A))
    p.cand = np.where(~static)[0]
    p.memo = {}
    return p


def _oracle(p, k, forced=None):
    """greedy_fast on the whole pool, memoised per problem: (picks, utilities[k, n])."""
    key = ('oracle', k, None if forced is None else tuple(int(f) for f in forced))
    if key not in p.memo:
        p.memo[key] = O.greedy_fast(p.C, p.static, p.mobile, S_STD, M_STD, k, 'entropy', forced_picks=forced)
    return p.memo[key]


def _gap(ut):
    """The smallest top-two gap over the picks of an oracle run: how far every argmax is from a tie.  A pick from an
    empty train set is left out: every utility there is the prior's, the same bits in every row and precision, and the
    first maximum is the first row for np.argmax and for the device alike."""
    g = np.inf
    for row in ut:
        v = np.sort(row[np.isfinite(row)])
        if len(v) > 1 and v[-1] != v[0]:
            g = min(g, float(v[-1] - v[-2]))
    return g


def _dense(p, picks, cand):
    """One dense solve on A u picks: (ordinary rows, their posterior variance, unit rows, their [S^-1]_jj) for the
    rows of `cand` that are not picked."""
    key = ('dense', tuple(int(q) for q in picks), np.asarray(cand, np.int64).tobytes())
    if key in p.memo:
        return p.memo[key]
    picks = np.asarray(picks, np.int64)
    new = np.array([q for q in picks if p.pos_in_A[q] < 0], np.int64)
    A = np.r_[p.A, new]
    noise = np.r_[p.var, np.full(len(new), SS)]
    for q in picks:
        if p.pos_in_A[q] >= 0:
            assert p.mobile[q] and not p.static[q]
            noise[p.pos_in_A[q]] = VF
    pos = -np.ones(p.n, np.int64)
    pos[A] = np.arange(len(A))
    L = np.linalg.cholesky(p.C[np.ix_(A, A)] + np.diag(noise))
    left = ~np.isin(cand, picks)
    unit = left & p.mobile[cand]
    ordn = left & ~p.mobile[cand]
    B = np.zeros((len(A), len(cand)))             # columns of the ordinary rows: C[A, j]; of the unit rows: e_pos(j)
    B[:, ordn] = p.C[np.ix_(A, cand[ordn])]
    B[pos[cand[unit]], np.where(unit)[0]] = 1.0
    V = solve_triangular(L, B, lower=True)
    sq = np.sum(V * V, axis=0)
    p.memo[key] = (ordn, p.C[cand[ordn], cand[ordn]] - sq[ordn], unit, sq[unit])
    return p.memo[key]


def _load(c, p, cand=None, alive=None):
    """Pool, train set, factor, candidates and a fresh solve."""
    c.set_hypers(p.hyp.log_lengthscale, p.hyp.log_outputscale, p.hyp.log_noise, p.hyp.kernel)
    if p.explicit:
        c.set_pool_cov(p.C)
    else:
        c.set_pool(p.X)
    c.set_train(p.A, np.zeros(len(p.A)), p.var)
    c.factorize()
    c.set_candidates(p.cand if cand is None else cand, prior_includes_noise=True)
    c.solve_candidates(alive=alive)


def _fresh(c, alive=None):
    """Back to the state after the candidate solve: no picks, every row current."""
    c.solve_candidates(alive=alive)


def _ut_bound(dt, scale):
    return 1e-9 * max(1.0, scale) if np.dtype(dt) == np.float64 else 1e-3 * scale


def _check_utilities(c, got, want_full, cand, what):
    """Every finite utility of every pick against the oracle; the -inf pattern identical."""
    want = want_full[:, cand]
    got = np.asarray(got).reshape(want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    scale = float(np.max(np.abs(want[fin])))
    err = float(np.max(np.abs(got[fin] - want[fin])))
    print('%s %s: utilities %.2e of max|u| %.3f' % (what, c.dtype.name, err, scale))
    assert err < _ut_bound(c.dtype, scale), (what, err, scale)
    return err / scale


def _check_dense(c, p, picks, what, cand=None, alive=None):
    """The survivors of `picks` against the dense solve; returns (scores, variances) for bit-for-bit comparisons."""
    cand = p.cand if cand is None else cand
    ordn, pv, unit, sjj = _dense(p, picks, cand)
    s = c.scores(ENT, S_STD, M_STD)
    var = c.posterior()[1].astype(np.float64)
    live = ~np.isin(cand, picks) if alive is None else (~np.isin(cand, picks) & alive)
    assert np.array_equal(np.isfinite(s), live), what
    e_var = float(np.max(np.abs(var[ordn] - pv))) if ordn.any() else 0.0
    e_s = float(np.max(np.abs(var[unit] - sjj))) if unit.any() else 0.0
    u_ord = O.CONST + 0.5 * np.log(pv + SS)
    u_unit = 0.5 * np.log1p(DELTA * sjj)
    want = np.full(len(cand), -np.inf)
    want[ordn] = u_ord
    want[unit] = u_unit
    scale = float(np.max(np.abs(want[live]))) if live.any() else 1.0
    e_u = float(np.max(np.abs(s[live] - want[live]))) if live.any() else 0.0
    print('%s %s dense: var %.2e  s_jj %.2e  utilities %.2e of %.3f' % (what, c.dtype.name, e_var, e_s, e_u, scale))
    assert e_var < tol(c.dtype, 1e-9, 1e-3), (what, e_var)
    assert e_s < tol(c.dtype, 1e-9, 1e-3), (what, e_s)
    assert e_u < _ut_bound(c.dtype, scale), (what, e_u, scale)
    return s, c.posterior()[1]


def _profiled(c, call):
    """call() under the profiler: (its result, full score sweeps, launches of class `rows`).  Class `score` books a
    sweep over all rows with 4 M flop and an argmax with M, so sweeps = (flop / M - launches) / 3."""
    c.prof_enable(True)
    c.prof_reset()
    try:
        out = call()
        sc, rows = c.prof_get('score'), c.prof_get('rows')
    finally:
        c.prof_enable(False)
    sweeps = (sc['flops'] / c.M - sc['launches']) / 3.0
    assert sweeps == int(sweeps), (sc, c.M)
    return out, int(sweeps), rows['launches']


def _three_routes(c, p, k, what, alive=None, mask_pool=None, picks_o=None, ut_o=None):
    """Routes (a) full pass, (b) picks only, (c) stepwise, each from a fresh solve, each followed by the dense check.
    Returns (free-run picks, whether they were compared with the oracle's)."""
    dt = c.dtype
    cand = p.cand
    if picks_o is None:
        picks_o, ut_o = _oracle(p, k)
    # (a) along the oracle's picks: every utility; then free, which fixes picks and final bits for (b) and (c)
    _fresh(c, alive)
    (got, ut), sweeps, _ = _profiled(c, lambda: c.greedy(ENT, S_STD, M_STD, k, forced_picks=picks_o, want_utilities=True))
    assert [int(q) for q in got] == [int(q) for q in picks_o] and sweeps == k, (what, sweeps)
    _check_utilities(c, ut, ut_o, cand, what + ' (a)')
    _check_dense(c, p, picks_o, what + ' (a)', alive=alive)
    _fresh(c, alive)
    full, ut_free = c.greedy(ENT, S_STD, M_STD, k, want_utilities=True)
    full = [int(q) for q in full]
    s_full, var_full = _check_dense(c, p, full, what + ' (a, free)', alive=alive)
    compared = _gap(ut_o) > GAP[dt]
    if compared:
        assert full == [int(q) for q in picks_o], (what, full, picks_o)
    if mask_pool is not None:
        assert not np.any(np.isin(full, mask_pool)), what
        assert np.all(np.isneginf(ut_free[:, np.isin(cand, mask_pool)])), what
    # (b) picks only: after the first pick no sweep over all rows, the lazy chain instead
    _fresh(c, alive)
    lazy, sweeps, rows = _profiled(c, lambda: c.greedy(ENT, S_STD, M_STD, k))
    assert [int(q) for q in lazy] == full, (what, lazy, full)
    assert sweeps == 1 and rows >= 2 * (k - 1), (what, sweeps, rows)
    s_lazy, var_lazy = _check_dense(c, p, full, what + ' (b)', alive=alive)
    assert np.array_equal(s_lazy, s_full) and np.array_equal(var_lazy, var_full), what
    # (c) stepwise: the lazy best candidate, then the flushed scores of the same state
    _fresh(c, alive)
    for q in range(k):
        pos, w, val = c.best_candidate(ENT, S_STD, M_STD)
        s = c.scores(ENT, S_STD, M_STD)
        assert pos == int(np.argmax(s)) and w == int(cand[pos]) == full[q] and val == s[pos], (what, q, pos, w, val)
        c.commit_pick(w, S_STD, M_STD)
    s_step, var_step = _check_dense(c, p, full, what + ' (c)', alive=alive)
    assert np.array_equal(s_step, s_full) and np.array_equal(var_step, var_full), what
    return full, compared


# ------------------------------------------------------------------ seeds, checked with the oracle alone
# (group, D or N, kernel) -> seed, and the smallest top-two gap of its oracle run.  Searched over seeds 0, 1, 2, ... with the
# oracle alone: the first seed whose gap clears 1.2e-2 (for the two masked cells: also with the mask), else the widest
# found.  No fp32 run clears 1e-2 on a line of 500 length-scales (D = 1), over 128 picks, or from at most one train
# site: those are the skipped share, 8 of the file's 33 pick comparisons.
RBF, MATERN = KERNELS
SEEDS = {
    ('w', 1, RBF): 54, ('w', 1, MATERN): 49,            # 1.3e-3, 6.6e-4
    ('w', 2, RBF): 26, ('w', 2, MATERN): 42,            # 1.2e-2 (masked too), 1.5e-2
    ('w', 3, RBF): 3, ('w', 3, MATERN): 0,              # 1.4e-2, 1.6e-2 (masked too)
    ('w', 4, RBF): 1, ('w', 4, MATERN): 28,             # 1.9e-2, 1.3e-2
    ('w', 5, RBF): 31, ('w', 5, MATERN): 60,            # 1.5e-2, 1.6e-2
    ('w', 8, RBF): 50, ('w', 8, MATERN): 101,           # 1.7e-2, 1.3e-2
    ('cov', 2, RBF): 26,                                # the same field as ('w', 2, RBF)
    ('cap', 0, RBF): 4, ('cap', 100, RBF): 2,           # 1.2e-5, 5.6e-6 over 128 picks
    ('n', 0, RBF): 1, ('n', 0, MATERN): 33,             # 5.2e-3, 2.6e-3
    ('n', 1, RBF): 26, ('n', 1, MATERN): 49,            # 1.2e-3, 2.0e-3
    ('n', 127, RBF): 0, ('n', 127, MATERN): 9,          # 2.7e-2, 1.3e-2
    ('n', 128, RBF): 0, ('n', 128, MATERN): 2,          # 2.3e-2, 1.5e-2
    ('n', 129, RBF): 7, ('n', 129, MATERN): 12,         # 1.4e-2, 2.5e-2
    ('n', 2047, RBF): 4, ('n', 2047, MATERN): 8,        # 5.0e-2, 1.5e-2
    ('n', 2049, RBF): 3, ('n', 2049, MATERN): 7,        # 3.0e-2, 1.4e-2
    ('n', 4100, RBF): 4, ('n', 4100, MATERN): 2,        # 2.7e-2, 1.4e-2
}


def _seed(*key):
    return SEEDS[key]


WIDTHS = [1, 2, 3, 4, 5, 8]
N_POOL, K_WIDTHS = 400, 6


@functools.lru_cache(maxsize=None)
def _width_problem(D, kernel, explicit=False):
    key = ('cov' if explicit else 'w', D, kernel)
    return _problem(key, _seed(*key), N_POOL, D, kernel, 60, 100, 20, explicit)


SMALL_SIDE = 6.0                                 # cube of the cases that start from at most one train site: with the
                                                 # usual side every site far from the few sampled ones ties at the prior
ROW_N = [0, 1, 127, 128, 129, 2047, 2049, 4100]  # the last three pad to 2048, 2176, 4224 columns
ROW_KINDS = [(2, O.KERNEL_RBF), (3, O.KERNEL_MATERN15)]
K_ROWS = 5


@functools.lru_cache(maxsize=None)
def _row_problem(N, D, kernel):
    """N train sites, (N + 1) // 2 but at most 40 of them mobile-only (unit rows), 300 candidates in all."""
    n_unit = min(40, (N + 1) // 2)
    key = ('n', N, kernel)
    return _problem(key, _seed(*key), N + 300 - n_unit, D, kernel, N - n_unit, n_unit, 0, side=SMALL_SIDE if N <= 1 else None)


CAP_N = [0, 100]


@functools.lru_cache(maxsize=None)
def _cap_problem(N):
    key = ('cap', N, O.KERNEL_RBF)
    return _problem(key, _seed(*key), 300, 2, O.KERNEL_RBF, 80 if N else 0, 40 if N else 0, 20 if N else 0, side=SMALL_SIDE)


MASK_KINDS = [(2, O.KERNEL_RBF), (3, O.KERNEL_MATERN15)]


def _masked_oracle(p, k):
    """The oracle with the masked sites taken out of the candidate set: its utilities of pick q do not depend on what
    is forced at q, so the picks are resolved one at a time -- mask, then np.argmax."""
    if 'masked' in p.memo:
        return p.memo['masked']
    first = _oracle(p, 1)[0][0]
    rng = np.random.RandomState(17)
    mob_only = p.cand[p.mobile[p.cand]]
    others = np.setdiff1d(p.cand, np.r_[mob_only, first])
    third = len(p.cand) // 3
    mask_pool = np.r_[first, mob_only[::2], rng.permutation(others)[:third - 1 - len(mob_only[::2])]]
    picks = []
    for q in range(k):
        _, ut = _oracle(p, q + 1, picks + [int(others[-1])])
        row = ut[q].copy()
        row[mask_pool] = -np.inf
        picks.append(int(np.argmax(row)))
    _, ut = _oracle(p, k, picks)
    ut = ut.copy()
    ut[:, mask_pool] = -np.inf
    p.memo['masked'] = (mask_pool, picks, ut)
    return p.memo['masked']


def _pick_cases():
    """(problem builder, its oracle run) of every case whose free-run picks are compared with the oracle's."""
    out = [(lambda D=D, kn=kn: _oracle(_width_problem(D, kn), K_WIDTHS)[1]) for D in WIDTHS for kn in KERNELS]
    out += [lambda: _oracle(_width_problem(2, O.KERNEL_RBF, True), K_WIDTHS)[1]]
    out += [(lambda N=N, D=D, kn=kn: _oracle(_row_problem(N, D, kn), K_ROWS)[1]) for N in ROW_N for D, kn in ROW_KINDS]
    out += [(lambda N=N: _oracle(_cap_problem(N), MAX_APPEND)[1]) for N in CAP_N]
    out += [(lambda D=D, kn=kn: _masked_oracle(_width_problem(D, kn), K_WIDTHS)[2]) for D, kn in MASK_KINDS]
    return out


@functools.lru_cache(maxsize=None)
def _skipped_share():
    gaps = [_gap(ut()) for ut in _pick_cases()]
    return (sum(g <= GAP[np.dtype(np.float64)] for g in gaps) / len(gaps),
            sum(g <= GAP[np.dtype(np.float32)] for g in gaps) / len(gaps))


def _assert_skipped_share():
    s64, s32 = _skipped_share()
    assert s64 == 0.0 and s32 <= 0.25, (s64, s32)


# ------------------------------------------------------------------ 1. widths and kernels
@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('kernel', KERNELS, ids=KIDS)
@pytest.mark.parametrize('D', WIDTHS)
def test_widths_and_kernels(ctxs, D, kernel, dt):
    """D = 1 .. 8 reaches each padded width (2, 4, 8) from both ends; RBF and Matern-1.5; k = 6 picks on 400 sites
    (60 static, 100 mobile, 20 both: 80 unit rows among 340 candidates) through the three routes."""
    _assert_skipped_share()
    c = ctxs[np.dtype(dt)]
    p = _width_problem(D, kernel)
    _load(c, p)
    _three_routes(c, p, K_WIDTHS, 'D=%d %s' % (D, KIDS[kernel]))


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_explicit_covariance_pool(ctxs, dt):
    """The same three routes on algp_set_pool_cov: pick_bprime reads C(pick, j) from the matrix."""
    _assert_skipped_share()
    c = ctxs[np.dtype(dt)]
    p = _width_problem(2, O.KERNEL_RBF, True)
    _load(c, p)
    _three_routes(c, p, K_WIDTHS, 'explicit cov')


# ------------------------------------------------------------------ 2. winner kinds
@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('kernel', KERNELS, ids=KIDS)
@pytest.mark.parametrize('D', [2, 3, 8])
def test_new_and_mobile_sampled_winners_alternate(ctxs, D, kernel, dt):
    """With std 0.1 / 1.0 a free run never picks a mobile-sampled site (its gain is negative), so the sequence is
    forced: new site, mobile-sampled train site, ... over 6 picks -- an ordinary and a unit row each meet a new and an
    in-train pick (commit_finalize_kernel's two scales, pick_bprime's zero branch) at every width.  Utilities pick by
    pick through the full pass; then the same picks committed without scoring in between, so that one flush applies
    all six to every row: the same bits."""
    c = ctxs[np.dtype(dt)]
    p = _width_problem(D, kernel)
    rng = np.random.RandomState(D)
    mob_only = rng.permutation(p.cand[p.mobile[p.cand]])
    new = rng.permutation(p.cand[~p.mobile[p.cand]])
    forced = [int(v) for pair in zip(new[:3], mob_only[:3]) for v in pair]
    _, ut_o = _oracle(p, 6, forced)
    what = 'D=%d %s alternating' % (D, KIDS[kernel])
    _load(c, p)
    got, ut = c.greedy(ENT, S_STD, M_STD, 6, forced_picks=forced, want_utilities=True)
    assert [int(q) for q in got] == forced
    _check_utilities(c, ut, ut_o, p.cand, what)
    s_full, var_full = _check_dense(c, p, forced, what)
    _fresh(c)
    for q in forced:
        c.commit_pick(q, S_STD, M_STD)
    s, var = _check_dense(c, p, forced, what + ', one flush')
    assert np.array_equal(s, s_full) and np.array_equal(var, var_full)


# ------------------------------------------------------------------ 3. row lengths
@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('D,kernel', ROW_KINDS, ids=['D2-rbf', 'D3-matern'])
@pytest.mark.parametrize('N', ROW_N)
def test_row_lengths(ctxs, N, D, kernel, dt):
    """Train sizes around one tile and around the second stride of the dot products (2047 -> 2048 columns: the last
    length before it in fp64; 2049 -> 2176: the second stride in fp64; 4100 -> 4224: the second stride in fp32); the
    k = 5 picks make the column count Npad + q cover every 16-byte remainder in both precisions.  300 candidates, up to
    40 of them unit rows.  The routes are asserted with the profiler's launch counts (_three_routes): k sweeps over all
    rows on the full pass, one on the picks-only route."""
    _assert_skipped_share()
    c = ctxs[np.dtype(dt)]
    p = _row_problem(N, D, kernel)
    assert len(p.A) == N and len(p.cand) == 300
    _load(c, p)
    _three_routes(c, p, K_ROWS, 'N=%d %s' % (N, KIDS[kernel]))


# ------------------------------------------------------------------ 4. one row
@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('D,kernel', [(5, O.KERNEL_MATERN15), (2, O.KERNEL_RBF)], ids=['D5-matern', 'D2-rbf'])
@pytest.mark.parametrize('local', ['one_new', 'one_unit', '300'])
def test_remote_commits_on_one_row_and_on_many(ctxs, local, D, kernel, dt):
    """A candidate list of ONE site (an ordinary row; a unit row) takes the cooperative instance for mode 2; two remote
    commits -- a new site, then the mobile-sampled train site next to it -- outside the list, then scores() and
    posterior().  The one row is chosen next to both (see below), so that a missed or wrong refresh shows.  With
    300 local rows remote_row's own one-row launch has to catch the second pick's row up on the first.  The reference is
    the oracle over the whole candidate set, restricted to the local rows; scored after each commit and, from a fresh
    solve, only after both (one flush for two picks): the same bits."""
    c = ctxs[np.dtype(dt)]
    p = _width_problem(D, kernel)
    rng = np.random.RandomState(5)
    mob_only = rng.permutation(p.cand[p.mobile[p.cand]])
    new = rng.permutation(p.cand[~p.mobile[p.cand]])
    r0 = int(new[0])
    remote = [r0, int(mob_only[np.argmax(p.C[r0, mob_only])])]      # the mobile-sampled site closest to the new one
    _, ut_o = _oracle(p, 3, remote + [int(new[1])])
    if local == '300':
        cand = np.setdiff1d(p.cand, remote)[:300]
    else:
        # the one local row is the one BOTH commits move the most (by the oracle): a row far from the picks would
        # pass without ever being refreshed.  Each commit moves it by more than 4x the fp32 bound.
        pool = np.setdiff1d(new[2:] if local == 'one_new' else mob_only, remote)
        move = np.minimum(np.abs(ut_o[1, pool] - ut_o[0, pool]), np.abs(ut_o[2, pool] - ut_o[1, pool]))
        cand = pool[[int(np.argmax(move))]]
        assert move.max() > 4 * _ut_bound(np.float32, float(np.max(np.abs(ut_o[:, cand])))), move.max()
    assert not np.any(np.isin(remote, cand))
    what = 'D=%d %s local=%s' % (D, KIDS[kernel], local)
    _load(c, p, cand=cand)
    for q in range(3):
        s = c.scores(ENT, S_STD, M_STD)
        _check_utilities(c, s, ut_o[q:q + 1], cand, '%s after %d' % (what, q))
        if q < 2:
            c.commit_pick(remote[q], S_STD, M_STD)
    s_each, var_each = _check_dense(c, p, remote, what, cand=cand)
    _fresh(c)
    for q in remote:
        c.commit_pick(q, S_STD, M_STD)
    s, var = _check_dense(c, p, remote, what + ', one flush', cand=cand)
    assert np.array_equal(s, s_each) and np.array_equal(var, var_each)


# ------------------------------------------------------------------ 5. capacity
@pytest.mark.parametrize('route,dt', [('full', np.float64), ('picks', np.float64), ('full', np.float32)],
                         ids=['full-f64', 'picks-f64', 'full-f32'])
@pytest.mark.parametrize('N', CAP_N)
def test_128_picks_and_the_refusals_behind_them(ctxs, N, route, dt):
    """MAX_APPEND = 128 picks in one algp_greedy call on a 300-site pool, from an empty train set and from 100 sites
    (20 unit rows).  fp64: the picks equal the oracle's on both routes (the full pass's own argmax at every pick
    along the forced sequence; the picks-only route as a free run).  fp32: utilities and the dense check along the
    oracle's forced picks, NO pick comparison (no fp32 run of 128 picks clears the 1e-2 gap: it counts in the skipped
    share).  Then the 129th algp_commit_pick: ALGP_ERR_STATE;
    algp_greedy with k = 129: ALGP_ERR_BAD_ARG; scores() before and after either refusal: the same bits.  Last, what
    the header says of the two orders of checks: algp_greedy looks at k alone, so k = 128 behind one committed pick
    commits 127 and stops with ALGP_ERR_STATE; with 128 committed, a repeat meets the capacity check before the
    duplicate check."""
    _assert_skipped_share()
    c = ctxs[np.dtype(dt)]
    p = _cap_problem(N)
    k = MAX_APPEND
    picks_o, ut_o = _oracle(p, k)
    what = 'N=%d %d picks %s' % (N, k, route)
    assert len(p.A) == N and _gap(ut_o) > GAP[np.dtype(np.float64)]
    _load(c, p)
    if route == 'full':
        got, ut = c.greedy(ENT, S_STD, M_STD, k, forced_picks=picks_o, want_utilities=True)
        assert [int(q) for q in got] == picks_o                                     # forced: only that they were taken
        _check_utilities(c, ut, ut_o, p.cand, what)
        if np.dtype(dt) == np.float64:
            assert [int(p.cand[int(np.argmax(row))]) for row in ut] == picks_o      # its own argmax at every pick
    else:
        got, sweeps, _ = _profiled(c, lambda: c.greedy(ENT, S_STD, M_STD, k))
        assert sweeps == 1
        assert [int(q) for q in got] == picks_o                                     # a free run: the pick comparison
    s0, _ = _check_dense(c, p, picks_o, what)
    left = p.cand[np.isfinite(s0)]
    assert c.lib.algp_commit_pick(c.h, int(left[0]), S_STD, M_STD) == _hip.ERR_STATE
    with pytest.raises(ValueError, match='append capacity exhausted'):
        c.commit_pick(int(left[0]), S_STD, M_STD)
    assert np.array_equal(c.scores(ENT, S_STD, M_STD), s0)
    buf = np.empty(k + 1, np.int64)
    assert c.lib.algp_greedy(c.h, ENT, S_STD, M_STD, k + 1, None, buf.ctypes.data_as(_hip._i64p), None) == _hip.ERR_BAD_ARG
    with pytest.raises(ValueError, match='0 <= k <= 128'):
        c.greedy(ENT, S_STD, M_STD, k + 1)
    assert np.array_equal(c.scores(ENT, S_STD, M_STD), s0)
    _fresh(c)
    with pytest.raises(ValueError, match='0 <= k <= 128'):                      # also with nothing committed yet
        c.greedy(ENT, S_STD, M_STD, k + 1)
    assert len(c.greedy(ENT, S_STD, M_STD, 1)) == 1
    # only k is checked up front: with one pick committed, k = 128 commits the 127 that fit, then ALGP_ERR_STATE
    with pytest.raises(ValueError, match='append capacity exhausted'):
        c.greedy(ENT, S_STD, M_STD, k, want_utilities=route == 'full')
    s1 = c.scores(ENT, S_STD, M_STD)
    assert int(np.isfinite(s1).sum()) == len(p.cand) - k
    assert c.lib.algp_commit_pick(c.h, int(p.cand[np.isneginf(s1)][0]), S_STD, M_STD) == _hip.ERR_STATE  # a repeat: capacity first
    assert np.array_equal(c.scores(ENT, S_STD, M_STD), s1)


# ------------------------------------------------------------------ 6. alive masks
@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('D,kernel', MASK_KINDS, ids=['D2-rbf', 'D3-matern'])
def test_masked_rows(ctxs, D, kernel, dt):
    """algp_set_candidate_alive with a third of the rows off -- the unmasked run's first winner and every other unit
    row among them: -inf on every route, never picked, picks and utilities those of the oracle without these sites.
    Committing a masked row BY NAME is accepted (include/algp_hip.h: the mask removes a row from scoring and from the
    library's own picks, not from the sites algp_commit_pick takes): the other rows then follow the oracle with that
    pick forced, and the row stays at -inf."""
    _assert_skipped_share()
    c = ctxs[np.dtype(dt)]
    p = _width_problem(D, kernel)
    mask_pool, picks_o, ut_o = _masked_oracle(p, K_WIDTHS)
    alive = ~np.isin(p.cand, mask_pool)
    assert _oracle(p, 1)[0][0] in mask_pool and np.any(p.mobile[mask_pool]) and np.any(p.mobile[p.cand[alive]])
    assert abs(int((~alive).sum()) - len(p.cand) // 3) <= 1 and not np.any(np.isin(picks_o, mask_pool))
    what = 'masked D=%d %s' % (D, KIDS[kernel])
    _load(c, p, alive=alive)
    _three_routes(c, p, K_WIDTHS, what, alive=alive, mask_pool=mask_pool, picks_o=picks_o, ut_o=ut_o)
    # a masked ordinary row committed by name, after two picks of the library's own
    named = int(p.cand[~alive & ~p.mobile[p.cand]][3])
    seq = picks_o[:2] + [named]
    _, ut_n = _oracle(p, 4, seq + [picks_o[2]])
    ut_n = ut_n.copy()
    ut_n[:, mask_pool] = -np.inf
    _fresh(c, alive)
    c.greedy(ENT, S_STD, M_STD, 2, forced_picks=picks_o[:2])
    s_before = c.scores(ENT, S_STD, M_STD)
    assert np.isneginf(s_before[p.cand == named])
    assert c.lib.algp_commit_pick(c.h, named, S_STD, M_STD) == _hip.OK
    s_after = c.scores(ENT, S_STD, M_STD)
    _check_utilities(c, s_after, ut_n[3:4], p.cand, what + ', named')
    _check_dense(c, p, seq, what + ', named', alive=alive)
    with pytest.raises(ValueError, match='already static-sampled'):
        c.commit_pick(named, S_STD, M_STD)
