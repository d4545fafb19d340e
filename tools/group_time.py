"""Times algp_group_posterior at the project's size: N = 10 000 train rows, M = 100 000 candidates on a 332 x 332 field, fp64
and fp32, for two groupings -- Q = 1 000 groups of 100 sites scattered at random (replicated genotypes) and the 332 contiguous
field rows -- each with and without cross_out.

Per dtype and case, one JSON line on stdout (all of them in --out):
  wall_ms        host clock around the ABI call (it ends in a stream synchronise; the results cross to the host inside it),
                 after a warm-up call of the same shape; min / median / max over --repeats
  classes        the library's HIP events of one more call, profiling on: ms and launches of ALGP_PROF_KMAT (the kernel sums),
                 ALGP_PROF_ROWS (the grouped sums) and ALGP_PROF_GEMM_OTHER (the products)
  group_evals_per_s   M x (labelled rows) kernel evaluations over the ALGP_PROF_KMAT time of the call
and per dtype the yardstick, existing code on the same card, dtype and kernel:
  build_evals_per_s   n^2 over the ALGP_PROF_KMAT time of algp_kernel_matrix at n = 16 384 (the matrix build, which writes every
                      value it forms; the group sums write Q / M of that)

    python tools/group_time.py --out profiles/group_time.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10000)
    ap.add_argument('--M', type=int, default=100000)
    ap.add_argument('--Q', type=int, default=1000)
    ap.add_argument('--build-n', type=int, default=16384)
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
    genotypes = rng.permutation(a.M) % a.Q                            # Q groups of M / Q sites scattered at random
    rows = X[cand, 0].astype(np.int64)                                # cand is sorted: every field row is contiguous
    groupings = {'genotypes': (genotypes, a.Q), 'field_rows': (rows, ROWS)}
    results = []
    for dt in (np.float64, np.float32):
        c = _hip.Context(dt)
        c.set_hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2), _hip.KERNEL_RBF)
        c.prof_enable(True)
        c.prof_reset()
        xb = X[:a.build_n]
        c.kernel_matrix(xb, xb.copy())
        build = c.prof_get('kmat')
        build_rate = float(a.build_n) ** 2 / (build['ms'] * 1e-3)
        c.prof_enable(False)
        c.set_pool(X)
        c.set_train(A, y, var)
        c.factorize()
        c.set_candidates(cand, prior_includes_noise=False)
        c.solve_candidates()
        for name, (lab, Q) in groupings.items():
            for cross in (False, True):
                call = lambda: c.group_posterior(lab, n_groups=Q, want_cov=True, want_cross=cross)
                call()                                                # warm-up: the scratch is allocated here
                wall = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    mean, cov, _ = call()
                    wall.append((time.perf_counter() - t0) * 1e3)
                c.prof_enable(True)
                c.prof_reset()
                call()
                classes = {k: c.prof_get(k) for k in ('kmat', 'rows', 'gemm_other')}
                c.prof_enable(False)
                evals = float(a.M) * float(np.sum(lab >= 0))
                r = dict(dtype=np.dtype(dt).name, N=a.N, M=a.M, Q=int(Q), grouping=name, cross=cross, wall_ms=spread(wall),
                         classes=classes, device_bytes=c.device_bytes(), group_evals_per_s=evals / (classes['kmat']['ms'] * 1e-3),
                         build_n=a.build_n, build_kmat_ms=build['ms'], build_evals_per_s=build_rate,
                         mean_of_means=float(np.mean(mean)), min_group_std=float(np.sqrt(np.min(np.diag(cov)))))
                print(json.dumps(r))
                results.append(r)
        c.close()
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(results, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
