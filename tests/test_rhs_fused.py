"""The scheduled candidate sweep forms the candidates' right-hand sides B^T = K(candidates, train) in the epilogues of its update
products (gemm.hip: GEN; potrf.hip: trsm_blocked with an RhsGen) instead of reading them from V^T, where a kernel-matrix launch
had written them.  ALGP_RHS_FUSED=0 (read per call) keeps the materialised form.  Both forms evaluate one definition of a B^T
entry (common.h: bt_entry / kmat_value) and run the same products in the same order, so every result must agree BIT FOR BIT:
posterior mean and variance, four entropy picks, their utilities and the picked rows of V^T -- here at 51 300 rows (68 leftover
tiles on 512 slots: cut along k, summed by the finish kernel, which generates its C term too; also: padding rows, 51 300 is no
multiple of 128) and 65 536 rows (no leftover), against train sets of 1 296 (block 0, a full block, a ragged 384-wide one),
1 400 (the same blocks, other padding), 1 536 (three full blocks) and 2 320 sites (four full blocks, a ragged 256-wide one and a
narrow last tile of 16 columns for the tail kernel: the narrow tile needs 2 048 columns in front of it, so 1 296 has none).
Run against run is bit-identical, both forms agree with the oracle's posterior (O.posterior_chol, 192 sampled rows; fp64 1e-9,
fp32 2e-3), and the bytes booked under `kmat` show which form ran.  Unit rows (candidates that are train sites), the Matern
kernel, three coordinates and an explicit pool covariance: whichever form the plan gives them, the results equal the
materialised form's."""
import numpy as np
import pytest

from algp_amd import _hip
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-9, np.float32: 2e-3}


def _hyp(D=2, kernel=O.KERNEL_RBF):
    return O.Hypers(np.log([3.0] * D), 0.0, np.log(1e-2), kernel)


def _setup(dtype, M, N, seed, side, hyp=None, D=2):
    """tests/test_trsm_scheduled.py's problem: train sites on a grid, candidates scattered over it."""
    hyp = hyp or _hyp(D)
    rng = np.random.RandomState(seed)
    xx, yy = np.meshgrid(np.arange(side), np.arange(side))
    grid = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    cand_x = rng.uniform(0, side, (M, 2))
    if D == 3:
        grid = np.c_[grid, rng.uniform(0, 2, len(grid))]
        cand_x = np.c_[cand_x, rng.uniform(0, 2, M)]
    A = np.sort(rng.permutation(len(grid))[:N])
    pool = np.vstack([grid, cand_x])
    var = rng.choice([0.01, 1.0], N)
    y = rng.uniform(0, 1, N)
    c = _hip.Context(dtype)
    c.set_hypers(hyp.log_lengthscale, hyp.log_outputscale, hyp.log_noise, hyp.kernel)
    c.set_pool(pool)
    c.set_train(A, y, var)
    c.factorize()
    cidx = np.arange(len(grid), len(grid) + M)
    samp = np.sort(rng.permutation(M)[:192])
    samp[-1] = M - 1                                   # a row of the last (cut) row panel is always among them
    ref = O.posterior_chol(hyp, pool[A], y, pool[cidx[samp]], var)
    return c, cidx, samp, ref, A


def _kmat_bytes(c):
    """bytes booked under `kmat` by one solve_candidates"""
    c.prof_enable(True)
    c.prof_reset()
    c.solve_candidates()
    b = c.prof_get('kmat')['bytes']
    c.prof_enable(False)
    return b


def _expected_bytes(M, N, es):
    mpad = -(-M // 128) * 128
    npad = -(-N // 128) * 128
    ldv = npad + 128
    r = N % 128
    narrow = 0 < r <= 64 and npad - 128 >= 2048 and mpad >= 2048
    sweep_end = npad - 128 if narrow else npad
    return mpad * ldv * es, mpad * (512 + ldv - sweep_end) * es


def _posteriors(c, monkeypatch):
    """(fused, fused again, materialised) posterior (mean, variance)"""
    out = []
    for flag in ('1', '1', '0'):
        monkeypatch.setenv('ALGP_RHS_FUSED', flag)
        c.solve_candidates()
        out.append(c.posterior())
    monkeypatch.delenv('ALGP_RHS_FUSED')
    return out


def _picks(c, monkeypatch, flag):
    monkeypatch.setenv('ALGP_RHS_FUSED', flag)
    c.solve_candidates()
    picks, util, rows = [], [], []
    for q in range(4):
        pos, site, val = c.best_candidate(_hip.CRIT_ENTROPY, 0.1, 1.0)
        c.commit_pick(site, 0.1, 1.0)
        picks.append(int(site))
        util.append(float(val))
        rows.append(c.debug_get_pick(q))
    monkeypatch.delenv('ALGP_RHS_FUSED')
    return picks, np.array(util), rows, c.posterior()


def _same_picks(a, b):
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1])
    for (ra, da), (rb, db) in zip(a[2], b[2]):
        assert np.array_equal(ra, rb) and da == db
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])


def _check_oracle(mu, pv, samp, ref, tol, var_shift=0.0, what=''):
    d_mu = np.max(np.abs(mu[samp] - ref['mu'])) / max(1.0, np.max(np.abs(ref['mu'])))
    d_pv = np.max(np.abs(pv[samp] - (ref['var'] + var_shift))) / max(1.0, np.max(np.abs(ref['var'] + var_shift)))
    print('%s vs oracle: mean %.3e variance %.3e (tolerance %.1e)' % (what, d_mu, d_pv, tol))
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(pv))
    assert d_mu <= tol and d_pv <= tol


def _whole_case(monkeypatch, dtype, M, N, side, seed):
    c, cidx, samp, ref, A = _setup(dtype, M, N, seed, side)
    es = np.dtype(dtype).itemsize
    c.set_candidates(cidx, prior_includes_noise=False)
    (mu, pv), (mu2, pv2), (mu0, pv0) = _posteriors(c, monkeypatch)
    _check_oracle(mu, pv, samp, ref, TOL[dtype], what='fused')
    _check_oracle(mu0, pv0, samp, ref, TOL[dtype], what='materialised')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)          # run against run
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)          # fused against materialised
    # which form ran: the kernel-matrix bytes of one solve
    full, fused_most = _expected_bytes(M, N, es)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    b1 = _kmat_bytes(c)
    monkeypatch.setenv('ALGP_RHS_FUSED', '0')
    b0 = _kmat_bytes(c)
    monkeypatch.delenv('ALGP_RHS_FUSED')
    print('kmat bytes: fused %d (at most %d), materialised %d (= %d)' % (b1, fused_most, b0, full))
    assert b0 == full
    assert 0 < b1 <= fused_most < full
    # the greedy picks, their utilities and rows of V^T
    c.set_candidates(cidx, prior_includes_noise=True)
    _same_picks(_picks(c, monkeypatch, '1'), _picks(c, monkeypatch, '0'))
    c.close()


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('N', [1296, 1400, 1536])
@pytest.mark.parametrize('M', [51300, 65536], ids=['68_left_cut', 'no_leftover'])
def test_fused_equals_materialised(monkeypatch, dtype, M, N):
    _whole_case(monkeypatch, dtype, M, N, 40, 31)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_narrow_last_tile_behind_a_ragged_block(monkeypatch, dtype):
    """2 320 train sites: full blocks to 2 048, a ragged 256-wide block, 16 columns for the tail kernel, whose right-hand sides
    a kernel-matrix window writes (with the padding behind them) while the sweep generates its own."""
    _whole_case(monkeypatch, dtype, 51300, 2320, 50, 32)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_unit_rows_in_every_kind_of_block(monkeypatch, dtype):
    """Candidates that are train sites under prior_includes_noise=True are unit rows e_pos of B^T: positions in block 0, in later
    full blocks, in the ragged block, in the narrow tile, and the last row of the cut row panels among them."""
    M, N = 51300, 2320
    c, cidx, samp, ref, A = _setup(dtype, M, N, 33, 50)
    pos = np.array([0, 5, 511, 512, 700, 1535, 2047, 2048, 2100, 2303, 2304, 2310, 2319])
    rows = np.r_[np.arange(7) * 37 + 11, 400 * 128 + np.arange(5) * 13, M - 1]     # the last ones in the cut row panels
    cand = cidx.copy()
    cand[rows] = A[pos]
    c.set_candidates(cand, prior_includes_noise=True)
    (mu, pv), (mu2, pv2), (mu0, pv0) = _posteriors(c, monkeypatch)
    keep = ~np.isin(samp, rows)                        # the oracle's rows are ordinary candidates
    _check_oracle(mu, pv, samp[keep], dict(mu=ref['mu'][keep], var=ref['var'][keep]), TOL[dtype], _hyp().noise, 'fused')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)
    assert np.all(np.isfinite(mu[rows])) and np.all(np.isfinite(pv[rows]))
    full, fused_most = _expected_bytes(M, N, np.dtype(dtype).itemsize)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    assert 0 < _kmat_bytes(c) <= fused_most
    monkeypatch.delenv('ALGP_RHS_FUSED')
    _same_picks(_picks(c, monkeypatch, '1'), _picks(c, monkeypatch, '0'))
    c.close()


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_matern_kernel(monkeypatch, dtype):
    M, N = 51300, 1400
    hyp = _hyp(2, O.KERNEL_MATERN15)
    c, cidx, samp, ref, A = _setup(dtype, M, N, 34, 40, hyp)
    c.set_candidates(cidx, prior_includes_noise=False)
    (mu, pv), (mu2, pv2), (mu0, pv0) = _posteriors(c, monkeypatch)
    _check_oracle(mu, pv, samp, ref, TOL[dtype], what='fused')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)
    full, fused_most = _expected_bytes(M, N, np.dtype(dtype).itemsize)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    assert 0 < _kmat_bytes(c) <= fused_most
    monkeypatch.delenv('ALGP_RHS_FUSED')
    c.set_candidates(cidx, prior_includes_noise=True)
    _same_picks(_picks(c, monkeypatch, '1'), _picks(c, monkeypatch, '0'))
    c.close()


def test_three_coordinates(monkeypatch):
    """D = 3 (four padded coordinates per site): whichever form the plan chooses, the materialised form's bits."""
    M, N = 51300, 1400
    c, cidx, samp, ref, A = _setup(np.float64, M, N, 35, 40, D=3)
    c.set_candidates(cidx, prior_includes_noise=False)
    (mu, pv), (mu2, pv2), (mu0, pv0) = _posteriors(c, monkeypatch)
    _check_oracle(mu, pv, samp, ref, 1e-9, what='switch on')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)
    full, fused_most = _expected_bytes(M, N, 8)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    b = _kmat_bytes(c)
    monkeypatch.delenv('ALGP_RHS_FUSED')
    assert b == full or 0 < b <= fused_most
    c.set_candidates(cidx, prior_includes_noise=True)
    _same_picks(_picks(c, monkeypatch, '1'), _picks(c, monkeypatch, '0'))
    c.close()


def test_explicit_pool_covariance(monkeypatch):
    """set_pool_cov: the right-hand sides are read from the pool covariance, not computed.  A pool of 3 000 sites (the matrix is
    the pool's square), the 51 300 candidate rows drawn from its non-train sites with repetition; posterior against the
    coordinate pool's, switch on against switch off."""
    M, N, side = 51300, 1400, 40
    hyp = _hyp()
    rng = np.random.RandomState(36)
    xx, yy = np.meshgrid(np.arange(side), np.arange(side))
    grid = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    pool = np.vstack([grid, rng.uniform(0, side, (1400, 2))])
    A = np.sort(rng.permutation(len(grid))[:N])
    var = rng.choice([0.01, 1.0], N)
    y = rng.uniform(0, 1, N)
    cand = len(grid) + rng.randint(0, 1400, M)
    cand[:1400] = len(grid) + np.arange(1400)
    c = _hip.Context(np.float64)
    c.set_hypers(hyp.log_lengthscale, hyp.log_outputscale, hyp.log_noise)
    c.set_pool_cov(O.kernel_matrix(hyp, pool) + hyp.noise * np.eye(len(pool)))
    c.set_train(A, y, var)
    c.factorize()
    c.set_candidates(cand, prior_includes_noise=True)
    (mu, pv), (mu2, pv2), (mu0, pv0) = _posteriors(c, monkeypatch)
    samp = np.arange(0, 1400, 8)
    ref = O.posterior_chol(hyp, pool[A], y, pool[cand[samp]], var)
    _check_oracle(mu, pv, samp, ref, 1e-9, hyp.noise, 'switch on')
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)
    full, fused_most = _expected_bytes(M, N, 8)
    monkeypatch.setenv('ALGP_RHS_FUSED', '1')
    b = _kmat_bytes(c)
    monkeypatch.delenv('ALGP_RHS_FUSED')
    assert b == full or 0 < b <= fused_most
    c.close()
