"""The candidate sweep beyond the task list's range (more than 400 tile rows) runs by default as SCHEDULED launches on one
stream (potrf.hip: trsm_blocked; gemm.hip: SCHED; gemm_sched.h): 2 x CUs workgroups walk a fixed work list, the leftover tiles of
an update product -- the last row panels -- are cut along k and summed by a finish kernel in ascending k.  An explicit
chunk count (set_trsm_chunks) or ALGP_TRSM_SCHED=0 keeps the row chunks on three streams.  Here: against the oracle's
posterior (utils.py:293-319 as O.posterior_chol) on sampled candidates, against the chunked route on all rows (bit-identical
above the leftover row panels, to rounding inside them), run against run (bit-identical), greedy picks, and the profile's
bookkeeping -- at shapes with 68 leftover tiles (4 slices at k = 512, 7 from k = 1 024 on), 364 (left whole), 256 in 2 slices,
and none (all on 256 CUs; the expectations follow the device's CU count)."""
import numpy as np
import pytest

from algp_amd import _hip
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

HYP = O.Hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))


def _slots():
    """2 x the compute units of the GPU (the scheduled launch's grid), from the KFD topology: the first readable node with SIMDs
    (the GPUs of one box are the same model)."""
    import glob
    for path in sorted(glob.glob('/sys/class/kfd/kfd/topology/nodes/*/properties'), key=lambda q: int(q.split('/')[-2])):
        try:
            prop = dict(line.split() for line in open(path) if len(line.split()) == 2)
        except OSError:                                # a GPU of the box that this process may not use
            continue
        if int(prop.get('simd_count', 0)) > 0:
            return 2 * int(prop['simd_count']) // int(prop['simd_per_cu'])
    raise RuntimeError('no GPU node in the KFD topology')


def _first_cut_row(M, N, G):
    """First row whose result may differ from the plain kernel's: the first row panel that holds a leftover tile of a launch
    that cuts them (S >= 2).  The launches of the sweep: 512 wide over k = 512 J for the full blocks J >= 1; for a ragged
    last block one update of its width over the columns before it, then 128-wide updates over 128 and 256 inside it."""
    tm = -(-M // 128)
    npad = -(-N // 128) * 128
    if N % 128 and N % 128 <= 64:
        npad -= 128                                    # a narrow last tile goes to the tail kernel
    launches = [(4, j0 // 128) for j0 in range(512, npad - npad % 512, 512)]
    if npad % 512:
        w = npad % 512 // 128
        launches += [(w, (npad - npad % 512) // 128)] + [(1, q) for q in range(1, w)]
    first = tm
    for tn, kb in launches:
        tiles = tm * tn
        g = min(tiles, G)
        full = tiles // g * g
        left = tiles - full
        if left and min(g // left, kb) >= 2:
            first = min(first, full // tn)
    return first * 128


def _setup(dtype, M, N, seed, side):
    rng = np.random.RandomState(seed)
    xx, yy = np.meshgrid(np.arange(side), np.arange(side))
    grid = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    A = np.sort(rng.permutation(len(grid))[:N])
    pool = np.vstack([grid, rng.uniform(0, side, (M, 2))])
    var = rng.choice([0.01, 1.0], N)
    y = rng.uniform(0, 1, N)
    c = _hip.Context(dtype)
    c.set_hypers(HYP.log_lengthscale, HYP.log_outputscale, HYP.log_noise)
    c.set_pool(pool)
    c.set_train(A, y, var)
    c.factorize()
    cidx = np.arange(len(grid), len(grid) + M)
    samp = np.sort(rng.permutation(M)[:192])
    samp[-1] = M - 1                                   # a row of the last (cut) row panel is always among them
    ref = O.posterior_chol(HYP, pool[A], y, pool[cidx[samp]], var)
    return c, cidx, samp, ref


def _scheduled_and_chunked(c):
    c.set_trsm_chunks(0)
    c.solve_candidates()
    s1 = c.posterior()
    c.solve_candidates()
    s2 = c.posterior()
    c.set_trsm_chunks(3)
    c.solve_candidates()
    ch = c.posterior()
    c.set_trsm_chunks(0)
    return s1, s2, ch


def _check_against_chunks(c, M, N, samp, ref, tol, loose, first):
    (mu, pv), (mu2, pv2), (mu3, pv3) = _scheduled_and_chunked(c)
    d_mu = np.max(np.abs(mu[samp] - ref['mu'])) / max(1.0, np.max(np.abs(ref['mu'])))
    d_pv = np.max(np.abs(pv[samp] - ref['var'])) / max(1.0, np.max(np.abs(ref['var'])))
    e_mu, e_pv = np.max(np.abs(mu - mu3)), np.max(np.abs(pv - pv3))
    print('M %d N %d: vs oracle %.3e %.3e, vs chunks %.3e %.3e, first cut row %d' % (M, N, d_mu, d_pv, e_mu, e_pv, first))
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(pv))
    assert d_mu <= tol and d_pv <= tol
    assert e_mu <= loose and e_pv <= loose
    assert np.array_equal(mu[:first], mu3[:first]) and np.array_equal(pv[:first], pv3[:first])
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)
    return (mu, pv), (mu3, pv3)


@pytest.mark.parametrize('dtype,tol,loose', [(np.float64, 1e-9, 2e-11), (np.float32, 2e-3, 2e-4)], ids=['f64', 'f32'])
@pytest.mark.parametrize('M', [51300, 128 * 475, 128 * 448], ids=['68_left_cut', '364_left_whole', '256_left_2_slices'])
def test_scheduled_sweep_against_oracle_chunks_and_itself(dtype, tol, loose, M):
    N = 1400
    c, cidx, samp, ref = _setup(dtype, M, N, 21, 40)
    c.set_candidates(cidx, prior_includes_noise=False)
    first = _first_cut_row(M, N, _slots())
    if _slots() == 512:
        assert first == {51300: 341, 128 * 475: 475, 128 * 448: 384}[M] * 128   # (the ragged 384-wide update cuts deeper than the 512-wide ones)
    _check_against_chunks(c, M, N, samp, ref, tol, loose, first)
    c.close()


@pytest.mark.parametrize('dtype,tol,loose', [(np.float64, 1e-9, 1e-10), (np.float32, 3e-3, 5e-4)], ids=['f64', 'f32'])
def test_five_full_blocks_and_a_ragged_one(monkeypatch, dtype, tol, loose):
    M, N = 51300, 3000
    c, cidx, samp, ref = _setup(dtype, M, N, 22, 60)
    c.set_candidates(cidx, prior_includes_noise=False)
    out = []
    for flag in ('1', '0'):
        monkeypatch.setenv('ALGP_TRSM_SCHED', flag)
        c.solve_candidates()
        mu, pv = c.posterior()
        d_mu = np.max(np.abs(mu[samp] - ref['mu'])) / max(1.0, np.max(np.abs(ref['mu'])))
        d_pv = np.max(np.abs(pv[samp] - ref['var']))
        print('sched', flag, 'vs oracle', d_mu, d_pv)
        assert d_mu <= tol and d_pv <= tol, (dtype, flag)
        out.append((mu, pv))
    monkeypatch.delenv('ALGP_TRSM_SCHED')
    e_mu = np.max(np.abs(out[0][0] - out[1][0])) / max(1.0, np.max(np.abs(out[1][0])))
    e_pv = np.max(np.abs(out[0][1] - out[1][1]))
    print('scheduled vs ALGP_TRSM_SCHED=0', e_mu, e_pv)
    assert e_mu <= loose and e_pv <= loose
    c.close()


def test_no_leftover_no_difference():
    """65 536 rows = 512 row tiles: on 512 slots every launch of the sweep is whole rounds of whole tiles -- the chunked
    route's bits everywhere.  (On another CU count: everywhere above the first cut row panel.)"""
    M, N = 65536, 1400
    c, cidx, samp, ref = _setup(np.float64, M, N, 23, 40)
    c.set_candidates(cidx, prior_includes_noise=False)
    first = _first_cut_row(M, N, _slots())
    if _slots() == 512:
        assert first == M
    _check_against_chunks(c, M, N, samp, ref, 1e-9, 2e-11, first)
    c.close()


def test_greedy_picks_and_the_posterior_after_them():
    M, N = 51300, 1400
    c, cidx, samp, ref = _setup(np.float64, M, N, 24, 40)
    c.set_candidates(cidx, prior_includes_noise=True)
    runs = []
    for chunks in (0, 3):
        c.set_trsm_chunks(chunks)
        c.solve_candidates()
        picks, util = [], []
        for _ in range(4):
            pos, site, val = c.best_candidate(_hip.CRIT_ENTROPY, 0.1, 1.0)
            c.commit_pick(site, 0.1, 1.0)
            picks.append(int(site))
            util.append(float(val))
        runs.append((picks, np.array(util), c.posterior()))
    c.set_trsm_chunks(0)
    assert runs[0][0] == runs[1][0]
    assert np.max(np.abs(runs[0][1] - runs[1][1])) <= 1e-9
    assert np.max(np.abs(runs[0][2][0] - runs[1][2][0])) <= 2e-11 and np.max(np.abs(runs[0][2][1] - runs[1][2][1])) <= 2e-11
    c.close()


def test_profile_books_the_same_flop_under_gemm_trsm():
    M, N = 51300, 1400
    c, cidx, samp, ref = _setup(np.float64, M, N, 25, 40)
    c.set_candidates(cidx, prior_includes_noise=False)
    c.prof_enable(True)
    got = []
    for chunks in (0, 3):
        c.set_trsm_chunks(chunks)
        c.prof_reset()
        c.solve_candidates()
        got.append((c.prof_get('gemm_trsm'), c.prof_get('rows'), c.prof_get('trsm')))
    c.set_trsm_chunks(0)
    c.prof_enable(False)
    (s, s_rows, s_span), (ch, ch_rows, ch_span) = got
    print('scheduled', s, 'chunked', ch)
    assert s['flops'] == ch['flops'] and s['flops'] > 0
    assert 0 < s['launches'] <= ch['launches']
    assert s_rows['bytes'] == ch_rows['bytes'] and s_rows['launches'] == ch_rows['launches']   # the finish kernel is not a row pass
    assert s_span['launches'] == ch_span['launches'] == 1 and s_span['ms'] > 0
    c.close()
