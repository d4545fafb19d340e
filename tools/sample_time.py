"""Times algp_sample_posterior at the project's size: N = 10 000 train rows, M = 100 000 candidates on a 332 x 332 field,
S = 128 draws from F = 2 048 random Fourier features, fp64 and fp32.

Per dtype, one JSON line on stdout (all of them in --out):
  wall_ms        host clock around the ABI call (it ends in a stream synchronise; the S x M result crosses to the host inside
                 it), after a warm-up call of the same shape; min / median / max over --repeats
  classes        the library's HIP events of one more call, profiling on: ms, flop and launches of ALGP_PROF_GEMM_OTHER (the two
                 feature products and the product against V^T) and ALGP_PROF_GEMM_TRSM (the solve of the S right-hand sides)
  feature_*      the two feature products alone (train rows and candidates, 2 (M + N) S F flop): ALGP_PROF_GEMM_OTHER of the
                 call minus that of the same call in values mode, which books only the product against V^T there; next to
                 algp_bench_gemm(m = M + N padded, n = 128, k = F) on the same card -- how far the cosines are hidden behind
                 the products

    python tools/sample_time.py --out profiles/sample_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from algp_amd import _hip  # noqa: E402

ROWS, COLS = 332, 332                                # 110 224 sites


def spread(v):
    v = sorted(v)
    return {'min': v[0], 'median': v[len(v) // 2], 'max': v[-1], 'n': len(v)}


def context(dt, X, A, y, var, cand):
    c = _hip.Context(dt)
    c.set_hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2), _hip.KERNEL_RBF)
    c.set_pool(X)
    c.set_train(A, y, var)
    c.factorize()
    c.set_candidates(cand, prior_includes_noise=False)
    c.solve_candidates()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10000)
    ap.add_argument('--M', type=int, default=100000)
    ap.add_argument('--S', type=int, default=128)
    ap.add_argument('--F', type=int, default=2048)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    xx, yy = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    X = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    perm = rng.permutation(len(X))
    A, cand = np.sort(perm[:a.N]), np.sort(perm[a.N:a.N + a.M])
    y = np.sin(X[A, 0] / 30.0) + 0.1 * rng.standard_normal(a.N)
    var = np.full(a.N, 0.01)
    om, ph = rng.standard_normal((a.F, 2)), rng.uniform(0, 2 * np.pi, a.F)
    W, eps = rng.standard_normal((a.S, a.F)), rng.standard_normal((a.S, a.N))
    results = []
    for dt in (np.float64, np.float32):
        c = context(dt, X, A, y, var, cand)
        call = lambda ctx, e: ctx.sample_posterior(e, weights=W, omega=om, phase=ph)
        call(c, eps)                                                   # warm-up: the scratch is allocated here
        wall = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            f = call(c, eps)
            wall.append((time.perf_counter() - t0) * 1e3)
        c.prof_enable(True)
        c.prof_reset()
        call(c, eps)
        classes = {k: c.prof_get(k) for k in ('gemm_other', 'gemm_trsm')}
        # the same call in values mode: everything but the two feature products
        prior = rng.standard_normal((a.S, len(X)))
        c.sample_posterior(eps, prior=prior)
        feat = []
        for _ in range(a.repeats):
            ms = []
            for kw in (dict(weights=W, omega=om, phase=ph), dict(prior=prior)):
                c.prof_reset()
                c.sample_posterior(eps, **kw)
                ms.append(c.prof_get('gemm_other')['ms'])
            feat.append(ms[0] - ms[1])
        c.prof_enable(False)
        mpad = (a.M + a.N + 127) // 128 * 128
        gemm_ms = c.bench_gemm(mpad, 128, a.F, beta_one=False, reps=5)
        scratch = c.device_bytes()
        c.close()
        flop = 2.0 * (a.M + a.N) * a.S * a.F
        r = dict(dtype=np.dtype(dt).name, N=a.N, M=a.M, S=a.S, F=a.F, wall_ms=spread(wall), classes=classes,
                 device_bytes=scratch, feature_ms=spread(feat), feature_tflops=flop / (min(feat) * 1e-3) / 1e12,
                 bench_gemm_ms=gemm_ms, bench_gemm_tflops=2.0 * mpad * 128 * a.F / (gemm_ms * 1e-3) / 1e12,
                 sample_std=float(np.std(f)))
        print(json.dumps(r))
        results.append(r)
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(results, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
