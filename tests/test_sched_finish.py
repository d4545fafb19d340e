"""The finish kernels of the scheduled candidate sweep (gemm.hip: gemm_finish_kernel, gemm_finish_gen_kernel) add the k-slice
partials of an update product's leftover tiles to beta * C: 16 workgroups per tile, 16-byte pieces, the slices loaded in
batches of 8 with a remainder of 4 + 2 + 1 -- and, per element, the sum in ascending slice order that the element-by-element
kernels before them made.  Here at slice counts S that take every batch path, through the whole sweep (on 512 slots; the
expectations follow the device's CU count):
  51 300 x 1 400   68 leftover tiles in 4 slices (k = 512), 179 in 2 (the ragged 384-wide update)
  65 664 x 3 000   513 tile rows: 4 leftover tiles of one row panel in 4, 8, 12 and 16 slices at the full blocks, 3 in 20 at the
                   ragged 384-wide update, 1 in 2 inside it (and a narrow last tile for the tail kernel)
  51 300 x 2 048   68 leftover tiles in 4, 7 and 7 slices: the remainder 4 + 2 + 1 alone
  67 328 x 2 048   526 tile rows: 56 leftover tiles in 4, 8 and 9 slices, as in the 100 000 x 10 000 run: a batch and a remainder of 1
Per shape, fp64 and fp32: the generating and the loading finish kernel agree bit for bit (ALGP_RHS_FUSED=1 against =0), run
against run is bit-identical, the chunked route (set_trsm_chunks(3): no scheduled launches, no finish kernel) has the same bits
above the first cut row panel and agrees inside the cut panels within the bars tests/test_trsm_scheduled.py holds its shapes to
(1 400 columns: 2e-11 / 2e-4 absolute; from 2 048 columns on those of its 3 000-column case: 1e-10 / 5e-4), and the posterior
agrees with the oracle's (O.posterior_chol) on 192 sampled rows, the last row among them, within 1e-9 (fp64) and 2e-3 (fp32).
At the first shape four greedy picks equal the chunked route's (fp64, as in tests/test_trsm_scheduled.py: in fp32 the two routes'
utilities differ by rounding inside the cut panels)."""
import numpy as np
import pytest

from algp_amd import _hip
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

HYP = O.Hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))
TOL = {np.float64: 1e-9, np.float32: 2e-3}
# M, N, side of the train grid, seed, bars against the chunked route inside the cut panels (fp64, fp32)
SHAPES = {
    '68_left_4': (51300, 1400, 40, 41, (2e-11, 2e-4)),
    '4_left_up_to_20': (65664, 3000, 60, 42, (1e-10, 5e-4)),
    '68_left_7': (51300, 2048, 50, 43, (1e-10, 5e-4)),
    '56_left_9': (67328, 2048, 50, 44, (1e-10, 5e-4)),
}
# (leftover tiles, slices) of the sweep's cut launches in launch order, on 512 slots
CUTS_512 = {
    '68_left_4': [(68, 4), (179, 2)],
    '4_left_up_to_20': [(4, 4), (4, 8), (4, 12), (4, 16), (3, 20), (1, 2)],
    '68_left_7': [(68, 4), (68, 7), (68, 7)],
    '56_left_9': [(56, 4), (56, 8), (56, 9)],
}


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


def _cuts(M, N, G):
    """The sweep's update launches that cut their leftover tiles (S >= 2) as (leftover tiles, S), in launch order, and the first
    row whose result may differ from the plain kernel's: the first row panel that holds a leftover tile of such a launch.  The
    launches: 512 wide over k = 512 J for the full blocks J >= 1; for a ragged last block one update of its width over the
    columns before it, then 128-wide updates over 128 and 256 inside it."""
    tm = -(-M // 128)
    npad = -(-N // 128) * 128
    if N % 128 and N % 128 <= 64:
        npad -= 128                                    # a narrow last tile goes to the tail kernel
    launches = [(4, j0 // 128) for j0 in range(512, npad - npad % 512, 512)]
    if npad % 512:
        w = npad % 512 // 128
        launches += [(w, (npad - npad % 512) // 128)] + [(1, q) for q in range(1, w)]
    first, cuts = tm, []
    for tn, kb in launches:
        tiles = tm * tn
        g = min(tiles, G)
        full = tiles // g * g
        left = tiles - full
        if left and min(g // left, kb) >= 2:
            cuts.append((left, min(g // left, kb)))
            first = min(first, full // tn)
    return cuts, first * 128


def _setup(dtype, M, N, seed, side):
    """tests/test_trsm_scheduled.py's problem: train sites on a grid, candidates scattered over it."""
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


def _solve(c, monkeypatch, fused, chunks=0):
    monkeypatch.setenv('ALGP_RHS_FUSED', fused)
    c.set_trsm_chunks(chunks)
    c.solve_candidates()
    out = c.posterior()
    c.set_trsm_chunks(0)
    monkeypatch.delenv('ALGP_RHS_FUSED')
    return out


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_finish_kernels_through_the_sweep(monkeypatch, dtype, shape):
    M, N, side, seed, loose = SHAPES[shape]
    loose = loose[0 if dtype == np.float64 else 1]
    tol = TOL[dtype]
    cuts, first = _cuts(M, N, _slots())
    print('%s: cut launches (leftover tiles, slices) %s, first cut row %d' % (shape, cuts, first))
    if _slots() == 512:
        assert cuts == CUTS_512[shape]
    c, cidx, samp, ref = _setup(dtype, M, N, seed, side)
    c.set_candidates(cidx, prior_includes_noise=False)
    mu, pv = _solve(c, monkeypatch, '1')               # the generating finish kernel
    mu2, pv2 = _solve(c, monkeypatch, '1')
    mu0, pv0 = _solve(c, monkeypatch, '0')             # the loading one
    mu3, pv3 = _solve(c, monkeypatch, '1', chunks=3)   # no finish kernel
    c.close()
    d_mu = np.max(np.abs(mu[samp] - ref['mu'])) / max(1.0, np.max(np.abs(ref['mu'])))
    d_pv = np.max(np.abs(pv[samp] - ref['var'])) / max(1.0, np.max(np.abs(ref['var'])))
    e_mu, e_pv = np.max(np.abs(mu - mu3)), np.max(np.abs(pv - pv3))
    print('vs oracle: mean %.3e variance %.3e (tolerance %.1e); vs chunks: mean %.3e variance %.3e (bar %.1e)' % (
        d_mu, d_pv, tol, e_mu, e_pv, loose))
    print('loading form differs in %d + %d entries, second run in %d + %d, chunks above row %d in %d + %d' % (
        np.sum(mu != mu0), np.sum(pv != pv0), np.sum(mu != mu2), np.sum(pv != pv2), first,
        np.sum(mu[:first] != mu3[:first]), np.sum(pv[:first] != pv3[:first])))
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(pv))
    assert np.array_equal(mu, mu0) and np.array_equal(pv, pv0)          # both forms agree
    assert np.array_equal(mu, mu2) and np.array_equal(pv, pv2)          # run against run
    assert np.array_equal(mu[:first], mu3[:first]) and np.array_equal(pv[:first], pv3[:first])
    assert e_mu <= loose and e_pv <= loose
    assert d_mu <= tol and d_pv <= tol


def test_greedy_picks_equal_the_chunked_route():
    M, N, side, seed, _ = SHAPES['68_left_4']
    c, cidx, samp, ref = _setup(np.float64, M, N, seed + 10, side)
    c.set_candidates(cidx, prior_includes_noise=True)
    runs = []
    for chunks in (0, 3):
        c.set_trsm_chunks(chunks)
        c.solve_candidates()
        picks = []
        for _ in range(4):
            pos, site, val = c.best_candidate(_hip.CRIT_ENTROPY, 0.1, 1.0)
            c.commit_pick(site, 0.1, 1.0)
            picks.append(int(site))
        runs.append(picks)
    c.set_trsm_chunks(0)
    c.close()
    assert runs[0] == runs[1]
