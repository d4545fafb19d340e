"""What the GEMM launchers book in the profile (gemm.hip: gemm_book, dispatch): the launch count, the flop and the bytes of class
gemm_other after prof_reset -- what a slip on the host side of a launch changes and no numerical test sees.  Per product of
tiles = tiles_m * tiles_n output tiles of 128 x 128 over k (everything padded to 128), s bytes per element:
    flop  = 2 * 128^2 * k * tiles
    bytes = s * (tiles * 128^2 * (1 + [beta != 0]) + k * 128 * (tiles_m + tiles_n))
Both are sums of exactly representable doubles and are compared exactly.

bench_gemm itself books nothing: algp_bench_gemm times its launches with the profiler switched off and switches it back on
(api.hip), so its warm-ups, repetitions and finish launches never reach the profile -- its four launch regimes (4 leftover
tiles in one k block; cut in two slices with a finish launch; the same with C generated; the unscheduled lower-only form) are
held to exactly that, and to leaving the profiler as it was.  The closed form is held on the entry points whose launches are
booked under gemm_other: gemm_nt (one product, beta = 0 and beta != 0, sizes that are no multiple of 128, more than one k
block) and trsm_right_lt (a short X takes the right-looking order: per 128-column block one product with beta = 0 against the
block inverse and, while columns remain, one update of all of them with beta = 1 and k = 128).

The scheduled route (launch_scheduled) is booked where the candidate sweep takes it, under gemm_trsm: the 51 300 x 1 400 solve
of tests/test_sched_finish.py, with the right-hand sides generated and loaded (ALGP_RHS_FUSED=1 / 0).  Its launches, written out
in _sweep below: the six batched products of the 512-block inverses; per full 512-column block J >= 1 an update product over
k = 512 J (no C bytes where C is generated) and one triangular product (kcut: tiles_m * 4 * 5 / 2 tile-steps, k = 512 in the
bytes); for the ragged last block an update of its width, then per 128 columns an update over the columns before them inside
the block and the product with the block inverse.  An update with `left` leftover tiles on G = min(tiles, 2 x CUs) workgroups
is cut into S = min(G // left, k / 128) slices, and where S >= 2 a finish launch follows: 0 flop and s * 128^2 * left * (S + 2)
bytes where C is loaded, (S + 1) where it is generated.  On 512 slots: 17 launches, 68 leftover tiles in 4 slices and 179 in 2,
111 174 221 824 flop, 2 657 484 800 bytes generated and 3 057 778 688 loaded in fp64 (profiles/gemm_launch_ab.txt)."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import test_sched_finish as SF                       # noqa: E402
from algp_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])


def _pad(x):
    return -(-x // 128) * 128


def _product(s, m, n, k, beta):
    """(flop, bytes) of one product of the padded sizes."""
    tm, tn = _pad(m) // 128, _pad(n) // 128
    tiles = tm * tn
    return (2.0 * 128 * 128 * _pad(k) * tiles,
            float(s * (tiles * 128 * 128 * (2 if beta != 0 else 1) + _pad(k) * 128 * (tm + tn))))


def _booked(c):
    p = c.prof_get('gemm_other')
    print('gemm_other:', p)
    return p['launches'], p['flops'], p['bytes']


@DTYPES
@pytest.mark.parametrize('m,n,k,beta', [(256, 256, 128, 1.0), (256, 256, 256, 1.0), (256, 256, 128, 0.0), (200, 130, 300, 0.5)])
def test_one_product(dtype, m, n, k, beta):
    rng = np.random.RandomState(1)
    A, B, Cm = rng.uniform(-1, 1, (m, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (m, n))
    c = _hip.Context(dtype)
    c.prof_enable(True)
    c.prof_reset()
    D = c.gemm_nt(A, B, alpha=-1.0, beta=beta, Cm=Cm if beta else None)
    got = _booked(c)
    c.close()
    want = -A.astype(dtype).astype(np.float64) @ B.astype(dtype).astype(np.float64).T + beta * Cm.astype(dtype)
    assert np.max(np.abs(D - want)) <= (1e-12 if dtype == np.float64 else 1e-4) * k
    assert got == (1,) + _product(np.dtype(dtype).itemsize, m, n, k, beta)


@DTYPES
@pytest.mark.parametrize('m,n', [(100, 128), (300, 500)])
def test_right_looking_solve(dtype, m, n):
    rng = np.random.RandomState(2)
    L = np.tril(rng.uniform(-1, 1, (n, n)) / n) + np.eye(n)
    B = rng.uniform(-1, 1, (m, n))
    c = _hip.Context(dtype)
    c.prof_enable(True)
    c.prof_reset()
    X = c.trsm_right_lt(L, B)
    got = _booked(c)
    c.close()
    assert np.max(np.abs(X @ L.astype(dtype).T - B)) <= (1e-12 if dtype == np.float64 else 1e-4)
    s, blocks = np.dtype(dtype).itemsize, _pad(n) // 128
    flops, nbytes = 0.0, 0.0
    for b in range(blocks):
        parts = [_product(s, m, 128, 128, 0.0)]
        if b + 1 < blocks:
            parts.append(_product(s, m, 128 * (blocks - b - 1), 128, 1.0))
        flops += sum(p[0] for p in parts)
        nbytes += sum(p[1] for p in parts)
    assert got == (2 * blocks - 1, flops, nbytes)


@DTYPES
@pytest.mark.parametrize('args', [dict(k=128, beta_one=True), dict(k=256, beta_one=True), dict(k=256, generated_c=True),
                                  dict(k=128, lower_only=True, beta_one=False)],
                         ids=['one_k_block', 'two_slices', 'two_slices_generated', 'lower_only'])
def test_bench_gemm_stays_out_of_the_profile(dtype, args):
    c = _hip.Context(dtype)
    c.prof_enable(True)
    c.prof_reset()
    assert c.bench_gemm(256, 256, reps=1, **args) > 0
    assert _booked(c) == (0, 0.0, 0.0)
    c.gemm_nt(np.ones((128, 128)), np.ones((128, 128)))                       # the profiler is on again
    got = _booked(c)
    c.close()
    assert got == (1,) + _product(np.dtype(dtype).itemsize, 128, 128, 128, 0.0)


def _sweep(s, M, N, slots, generated):
    """(flop, bytes) of every gemm_trsm launch of the scheduled sweep of M candidates against N train columns, in launch order,
    and the (leftover tiles, slices) of its finish launches."""
    tm, npad = -(-M // 128), _pad(N)
    nb = npad // 512
    out, cuts = [], []

    def plain(tn, k, batch=1):
        out.append((2.0 * 128 * 128 * k * tm * tn * batch, float(s * batch * (tm * tn * 128 * 128 + k * 128 * (tm + tn)))))

    def update(tn, k, gen):
        tiles = tm * tn
        out.append((2.0 * 128 * 128 * k * tiles, float(s * (tiles * 128 * 128 * (1 if gen else 2) + k * 128 * (tm + tn)))))
        g = min(tiles, slots)
        left = tiles - tiles // g * g
        S = min(g // left, k // 128) if left else 0
        if S >= 2:
            cuts.append((left, S))
            out.append((0.0, float(s * 128 * 128 * left * (S + (1 if gen else 2)))))

    for tn, k in [(1, 128)] * 4 + [(2, 256)] * 2:                 # the 512-block inverses: tiles_m = tiles_n, nb blocks a launch
        out.append((2.0 * 128 * 128 * k * tn * tn * nb, float(s * nb * (tn * tn * 128 * 128 + k * 128 * 2 * tn))))
    for j0 in range(0, nb * 512, 512):
        if j0:
            update(4, j0, generated)
        out.append((2.0 * 128 ** 3 * tm * 4 * 5 / 2, float(s * (tm * 4 * 128 * 128 + 512 * 128 * (tm + 4)))))
    w = npad % 512 // 128
    if w:
        update(w, nb * 512, generated)
        for q in range(w):
            if q:
                update(1, 128 * q, False)
            plain(1, 128)
    return out, cuts


@DTYPES
def test_scheduled_sweep(monkeypatch, dtype):
    M, N, side, seed, _ = SF.SHAPES['68_left_4']
    assert _pad(N) % 512 and not 0 < N % 128 <= 64               # a ragged last block, no narrow last tile for the tail kernel
    slots, s = SF._slots(), np.dtype(dtype).itemsize
    c, cidx, samp, ref = SF._setup(dtype, M, N, seed, side)
    c.set_candidates(cidx, prior_includes_noise=False)
    c.prof_enable(True)
    got = {}
    for fused in ('1', '0'):
        monkeypatch.setenv('ALGP_RHS_FUSED', fused)
        c.prof_reset()
        c.solve_candidates()
        p = c.prof_get('gemm_trsm')
        print('ALGP_RHS_FUSED=%s gemm_trsm: %s' % (fused, p))
        got[fused] = (p['launches'], p['flops'], p['bytes'])
    c.close()
    for fused in ('1', '0'):
        want, cuts = _sweep(s, M, N, slots, fused == '1')
        print('ALGP_RHS_FUSED=%s want %d launches, %.0f flop, %.0f bytes, cuts %s' % (
            fused, len(want), sum(f for f, _ in want), sum(b for _, b in want), cuts))
        if slots == 512:
            assert cuts == SF.CUTS_512['68_left_4']
            if dtype == np.float64:
                assert (len(want), sum(f for f, _ in want)) == (17, 111174221824.0)
                assert sum(b for _, b in want) == (2657484800.0 if fused == '1' else 3057778688.0)
        assert got[fused] == (len(want), sum(f for f, _ in want), sum(b for _, b in want))
