"""fit_and_solve's split (api_candidates.hip: plan_route, split_tiles; $ALGP_SPLIT_PANELS): the last p tile rows of the
candidates -- the tile whose padding row carries y - ybar among them -- ride the factorisation's one launch as its panel, the
rows in front of them go to the scheduled sweep, and no forward substitution is launched for z.  At the smallest shapes the route
can go wrong on: nine tiles of train columns (block 0, one full 512-column block, a ragged 128-wide one), 321 tile rows left to
the sweep (it is scheduled from 321 on), p = 1 (the z tile alone) and p = 14, five padding rows; a train set that fills its
last tile, one that ends 76 columns into it (not narrow), and one of 2 064 rows, whose 16 last columns go to the tail kernel
(the plan takes a narrow tile only behind 2 048 full columns).

Checked: posterior mean and variance on 192 sampled candidates of each part against the oracle (utils.py:293-319 as
O.posterior_chol) at tests/test_trsm_regimes.py's bars, 1e-9 / 2e-3 of max(1, max |ref|); every row, alpha and the
log-determinant against the same context with ALGP_SPLIT_PANELS=0 at that file's bars for two orders of the same sums, 2e-11 /
2e-4 (alpha and the log-determinant, which are not O(1), relative to max(1, max |unsplit|)); run against run bit for bit; four
greedy picks against the unsplit run's, on a problem where the CPU oracle's two best utilities differ by more than 1e-6 of
their size at every pick; the profile's marks (dag_panel and gemm_trsm launches in one call, no trsv launch), and -- the
launch log lists the products only, the profile counts products and finish launches -- that a sweep left with whole rounds
launches exactly what a solve of those rows alone launches, which has no finish launch."""
import numpy as np
import pytest

from algp_amd import _hip
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

HYP = O.Hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))
TOL = {np.float64: 1e-9, np.float32: 2e-3}
LOOSE = {np.float64: 2e-11, np.float32: 2e-4}
SEED = 11
SPLIT_P_MAX = 14                                   # api_impl.h: the rule's largest p (profiles/split_solve_parts.txt)


def _slots():
    """2 x the compute units of the GPU, as tests/test_trsm_scheduled.py reads them from the KFD topology"""
    import glob
    for path in sorted(glob.glob('/sys/class/kfd/kfd/topology/nodes/*/properties'), key=lambda q: int(q.split('/')[-2])):
        try:
            prop = dict(line.split() for line in open(path) if len(line.split()) == 2)
        except OSError:
            continue
        if int(prop.get('simd_count', 0)) > 0:
            return 2 * int(prop['simd_count']) // int(prop['simd_per_cu'])
    raise RuntimeError('no GPU node in the KFD topology')


def _problem(N, M, seed=SEED, side=40, static_var=False):
    """train sites on a grid, candidates scattered over it (tests/test_trsm_regimes.py); the first rows of a larger M are the same"""
    rng = np.random.RandomState(seed)
    xx, yy = np.meshgrid(np.arange(side), np.arange(side))
    grid = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    A = np.sort(rng.permutation(len(grid))[:N])
    var = np.full(N, 0.01) if static_var else rng.choice([0.01, 1.0], N)
    y = rng.uniform(0, 1, N)
    cand = np.random.RandomState(seed + 1000).uniform(0, side, (M, 2))
    pool = np.vstack([grid, cand])
    return pool, A, y, var, np.arange(len(grid), len(grid) + M)


def _context(dtype, pool, A, y, var):
    c = _hip.Context(dtype)
    c.set_hypers(HYP.log_lengthscale, HYP.log_outputscale, HYP.log_noise)
    c.set_pool(pool)
    c.set_train(A, y, var)
    return c


def _run(c, monkeypatch, flag):
    """one fit_and_solve under ALGP_SPLIT_PANELS = flag (None: unset): launches by class, posterior, alpha, log-determinant"""
    if flag is None:
        monkeypatch.delenv('ALGP_SPLIT_PANELS', raising=False)
    else:
        monkeypatch.setenv('ALGP_SPLIT_PANELS', str(flag))
    c.prof_enable(True)
    c.prof_reset()
    c.fit_and_solve()
    n = {k: c.prof_get(k)['launches'] for k in ('dag_panel', 'chol_dag', 'gemm_trsm', 'trsv', 'tail_cols')}
    c.prof_enable(False)
    monkeypatch.delenv('ALGP_SPLIT_PANELS', raising=False)
    mu, pv = c.posterior()
    return n, mu, pv, c.alpha(), c.logdet()


def _taken(n):
    return n['dag_panel'] > 0 and n['gemm_trsm'] > 0 and n['trsv'] == 0


def _parts(M, p, rng):
    """up to 192 sampled rows of the sweep's part, of the folded tile rows in front of the z tile, and of the z tile"""
    mpad = -(-M // 128) * 128
    ms = mpad - 128 * p
    parts = [np.arange(ms), np.arange(ms, mpad - 128), np.arange(mpad - 128, M)]
    return np.sort(np.concatenate([rng.permutation(q)[:192] for q in parts if len(q)]))


def _check_oracle(mu, pv, samp, ref, tol, var_shift, what):
    d_mu = np.max(np.abs(mu[samp] - ref['mu'])) / max(1.0, np.max(np.abs(ref['mu'])))
    d_pv = np.max(np.abs(pv[samp] - (ref['var'] + var_shift))) / max(1.0, np.max(np.abs(ref['var'] + var_shift)))
    print('%s vs oracle: mean %.3e variance %.3e (bar %.1e)' % (what, d_mu, d_pv, tol))
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(pv))
    assert d_mu <= tol and d_pv <= tol, what


def _check_unsplit(split, plain, loose, what):
    _, mu, pv, al, ld = split
    _, mu0, pv0, al0, ld0 = plain
    d = (np.max(np.abs(mu - mu0)), np.max(np.abs(pv - pv0)), np.max(np.abs(al - al0)) / max(1.0, np.max(np.abs(al0))),
         abs(ld - ld0) / max(1.0, abs(ld0)))
    print('%s vs unsplit: mean %.3e variance %.3e alpha %.3e logdet %.3e (bar %.1e)' % ((what,) + d + (loose,)))
    assert max(d) <= loose, (what, d)


def _split_case(monkeypatch, dtype, N, p, tiles, side=40, prior_noise=False, unit_rows=None, narrow=False):
    M = 128 * tiles - 5
    pool, A, y, var, cidx = _problem(N, M, side=side)
    cand = cidx.copy()
    if unit_rows is not None:
        cand[unit_rows[0]] = A[unit_rows[1]]
    c = _context(dtype, pool, A, y, var)
    c.set_candidates(cand, prior_includes_noise=prior_noise)
    split = _run(c, monkeypatch, p)
    assert _taken(split[0]), split[0]
    assert split[0]['tail_cols'] == (1 if narrow else 0), split[0]
    again = _run(c, monkeypatch, p)
    assert again[0] == split[0]
    assert np.array_equal(split[1], again[1]) and np.array_equal(split[2], again[2]) and np.array_equal(split[3], again[3])
    assert split[4] == again[4]
    plain = _run(c, monkeypatch, 0)
    assert not _taken(plain[0]), plain[0]
    samp = _parts(M, p, np.random.RandomState(SEED + p))
    if unit_rows is not None:
        samp = samp[~np.isin(samp, unit_rows[0])]                 # the oracle's rows are ordinary candidates
        assert np.all(np.isfinite(split[1][unit_rows[0]])) and np.all(np.isfinite(split[2][unit_rows[0]]))
    ref = O.posterior_chol(HYP, pool[A], y, pool[cand[samp]], var)
    shift = HYP.noise if prior_noise else 0.0
    _check_oracle(split[1], split[2], samp, ref, TOL[dtype], shift, 'split p = %d' % p)
    _check_oracle(plain[1], plain[2], samp, ref, TOL[dtype], shift, 'unsplit')
    _check_unsplit(split, plain, LOOSE[dtype], 'p = %d' % p)
    return c, cand


@pytest.mark.parametrize('p', [1, 14])
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_split_against_the_oracle_the_unsplit_route_and_itself(monkeypatch, dtype, p):
    c, _ = _split_case(monkeypatch, dtype, 1040, p, 321 + p)
    c.close()


@pytest.mark.parametrize('n_train,side,narrow', [(1152, 40, False), (1100, 40, False), (2064, 50, True)],
                         ids=['full_last_tile', 'r76_not_narrow', 'r16_tail_kernel'])
def test_split_with_every_kind_of_last_column_tile(monkeypatch, n_train, side, narrow):
    c, _ = _split_case(monkeypatch, np.float64, n_train, 14, 335, side=side, narrow=narrow)
    c.close()


def test_split_with_train_site_candidates_in_every_part(monkeypatch):
    """prior_includes_noise=True: candidates that are train sites are unit rows e_pos of B^T -- in the sweep's part (block 0's
    columns, the full block's, the ragged block's), in the folded tile rows and in the tile that carries z."""
    M = 128 * 335 - 5
    rows = np.r_[np.arange(5) * 37 + 11, 321 * 128 + np.arange(4) * 200 + 3, 334 * 128 + np.array([0, 60, 122])]
    pos = np.array([0, 511, 512, 1023, 1039, 5, 700, 1024, 1030, 17, 600, 1038])
    assert rows.max() < M and len(rows) == len(pos)
    c, _ = _split_case(monkeypatch, np.float64, 1040, 14, 335, prior_noise=True, unit_rows=(rows, pos))
    c.close()


def _oracle_greedy_gaps(pool, A, var, cand, ss, k):
    """gp_oracle.greedy_fast's recurrence for ordinary candidates (dH_j = CONST + 1/2 log(pv_j + ss), one appended row of V per
    pick) without the pool-wide covariance it takes: the picks and, per pick, the distance of the two best utilities over the size
    of the best."""
    from scipy.linalg import solve_triangular
    S = O.kernel_matrix(HYP, pool[A]) + np.diag(var + HYP.noise)
    V = solve_triangular(np.linalg.cholesky(S), O.kernel_matrix(HYP, pool[A], pool[cand]), lower=True)
    d = (np.exp(HYP.log_outputscale) + HYP.noise) - np.sum(V * V, axis=0)
    alive = np.ones(len(cand), bool)
    rows, picks, gaps = [], [], []
    for _ in range(k):
        ut = np.where(alive, O.CONST + 0.5 * np.log(d + ss), -np.inf)
        o = np.argsort(ut)[::-1]
        picks.append(int(cand[o[0]]))
        gaps.append((ut[o[0]] - ut[o[1]]) / abs(ut[o[0]]))
        b = O.kernel_matrix(HYP, pool[cand[o[0]]][None, :], pool[cand])[0]
        b[o[0]] += HYP.noise
        t = V[:, o[0]] @ V + sum(r[o[0]] * r for r in rows)
        r = (b - t) / np.sqrt(d[o[0]] + ss)
        rows.append(r)
        d = d - r * r
        alive[o[0]] = False
    return picks, gaps


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_split_gives_the_unsplit_routes_greedy_picks(monkeypatch, dtype):
    M = 128 * 335 - 5
    pool, A, y, var, cidx = _problem(1040, M, static_var=True)
    want, gaps = _oracle_greedy_gaps(pool, A, var, cidx, 0.1 ** 2, 4)
    print('oracle picks', want, 'relative gaps of the two best utilities', gaps)
    assert min(gaps) > 1e-6, gaps                                # the problem separates its picks (the seed was chosen so)
    c = _context(dtype, pool, A, y, var)
    c.set_candidates(cidx, prior_includes_noise=True)
    got = []
    for flag in (14, 0):
        n = _run(c, monkeypatch, flag)[0]
        assert _taken(n) == (flag == 14), (flag, n)
        got.append([int(q) for q in c.greedy(_hip.CRIT_ENTROPY, 0.1, 1.0, 4)])
    assert got[0] == got[1], got
    if dtype == np.float64:
        assert got[0] == want, (got[0], want)
    c.close()


def test_the_automatic_rule_and_whole_rounds_without_a_finish_launch(monkeypatch):
    """512 + 14 tile rows, more than the folded route's 400: on 256 CUs the sweep's leftover row panels are (526 mod 128) = 14,
    which the rule takes with the switch unset (1 <= p <= SPLIT_P_MAX; the expectation follows the device's CU count).  The
    split leaves the sweep 512 tile rows = four whole rounds: it launches exactly what a solve of those rows alone launches
    (whole rounds, no finish launch), fewer than the unsplit sweep with its finish launch per cut update product."""
    slots = _slots()
    tiles = 4 * (slots // 4) + 14
    M = 128 * tiles - 5
    pool, A, y, var, cidx = _problem(1040, M)
    c = _context(np.float64, pool, A, y, var)
    c.set_candidates(cidx, prior_includes_noise=False)
    left = tiles % (slots // 4)
    assert left == 14
    auto = _run(c, monkeypatch, None)
    assert _taken(auto[0]) == (1 <= left <= SPLIT_P_MAX), auto[0]
    split = _run(c, monkeypatch, left)
    plain = _run(c, monkeypatch, 0)
    assert _taken(split[0]) and not _taken(plain[0])
    assert plain[0]['dag_panel'] == 0 and plain[0]['chol_dag'] > 0 and plain[0]['trsv'] > 0
    _check_unsplit(split, plain, LOOSE[np.float64], 'p = %d of %d tile rows' % (left, tiles))
    samp = _parts(M, left, np.random.RandomState(3))
    ref = O.posterior_chol(HYP, pool[A], y, pool[cidx[samp]], var)
    _check_oracle(split[1], split[2], samp, ref, 1e-9, 0.0, 'split')
    # the sweep's rows alone: a multiple of slots / 4 tile rows
    ms = 128 * (tiles - left)
    c.set_candidates(cidx[:ms], prior_includes_noise=False)
    whole = _run(c, monkeypatch, left)                            # M = Mpad: not taken
    assert not _taken(whole[0]) and whole[0]['trsv'] > 0
    assert split[0]['gemm_trsm'] == whole[0]['gemm_trsm'], (split[0], whole[0])
    assert plain[0]['gemm_trsm'] > split[0]['gemm_trsm'], (plain[0], split[0])
    c.close()


def test_the_folded_routes_range_splits_only_when_forced(monkeypatch):
    """3 whole rounds + 7 tile rows (384 + 7 = 391 on 256 CUs: a rank's share of 100 000 candidates on 2 GPUs) fits the folded
    route's 400 tile rows: unset, the rule leaves it folded whole; forced, the 7 leftover tile rows ride the launch."""
    per = _slots() // 4
    tiles = 3 * per + 7
    if tiles > 400:
        tiles = 391
    left = tiles % per
    M = 128 * tiles - 5
    pool, A, y, var, cidx = _problem(1040, M)
    c = _context(np.float64, pool, A, y, var)
    c.set_candidates(cidx, prior_includes_noise=False)
    unset = _run(c, monkeypatch, None)
    assert not _taken(unset[0]) and unset[0]['gemm_trsm'] == 0 and unset[0]['dag_panel'] > 0, unset[0]      # folded whole
    auto = _run(c, monkeypatch, max(left, 1))
    assert _taken(auto[0]) == (tiles - max(left, 1) > 320), (auto[0], tiles, left)
    plain = _run(c, monkeypatch, 0)
    assert not _taken(plain[0]) and plain[0]['gemm_trsm'] == 0 and plain[0]['dag_panel'] > 0, plain[0]      # folded whole
    _check_unsplit(auto, plain, LOOSE[np.float64], '%d tile rows, forced' % tiles)
    samp = _parts(M, max(left, 1), np.random.RandomState(4))
    ref = O.posterior_chol(HYP, pool[A], y, pool[cidx[samp]], var)
    _check_oracle(auto[1], auto[2], samp, ref, 1e-9, 0.0, 'forced')
    c.close()


def test_the_split_is_not_taken(monkeypatch):
    """Today's route stays -- no call with task-list panel rows, sweep launches and no substitution launch at once -- where M fills
    its last tile (no padding row for z), where 320 or fewer tile rows would remain for the sweep, on an incremental call and on
    solve_candidates after factorize."""
    tiles = 335
    M = 128 * tiles - 5
    pool, A, y, var, cidx = _problem(1040, 128 * tiles)
    c = _context(np.float64, pool, A, y, var)
    c.set_candidates(cidx, prior_includes_noise=False)             # M a multiple of 128
    n = _run(c, monkeypatch, 14)[0]
    assert not _taken(n) and n['gemm_trsm'] == 0 and n['dag_panel'] > 0, n      # the folded route
    c.set_candidates(cidx[:M], prior_includes_noise=False)
    n = _run(c, monkeypatch, 15)[0]                                # 320 tile rows would remain
    assert not _taken(n) and n['gemm_trsm'] == 0 and n['dag_panel'] > 0, n
    ref = _run(c, monkeypatch, 14)
    assert _taken(ref[0])
    monkeypatch.setenv('ALGP_SPLIT_PANELS', '14')
    c.prof_enable(True)
    for call in (lambda: c.solve_candidates(incremental=True), lambda: c.solve_candidates()):
        c.prof_reset()
        c.factorize()
        call()
        n = {k: c.prof_get(k)['launches'] for k in ('dag_panel', 'chol_dag', 'gemm_trsm', 'trsv')}
        assert not _taken(n) and n['chol_dag'] > 0 and n['trsv'] > 0, n         # the factorisation alone, with its substitution
        mu, pv = c.posterior()
        assert np.max(np.abs(mu - ref[1])) <= 2e-11 and np.max(np.abs(pv - ref[2])) <= 2e-11
    c.prof_enable(False)
    c.close()
