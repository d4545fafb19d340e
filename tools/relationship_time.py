"""Times the relationship kernel (algp_set_hypers_relationship) against the additive one at the project's sizes, fp64 and fp32,
D = 3 (row, col | genotype id) on a 332 x 332 field:

  build      the kernel-matrix build at --rows x --cols (10 000 x 100 000): the relationship form with Q = 1 000 (G = NULL and a
             dense G) and Q = 5 000 (dense), and the yardstick, the additive form Matern-3/2 (position) + RBF (id) at the same
             shape.  ms = the library's HIP events around the build's launches (ALGP_PROF_KMAT) of one algp_kernel_matrix call,
             after a warm-up call; min / median / max over --repeats.  A Q = 1 000 fp64 table is 8 MB, a Q = 5 000 one 200 MB.
  fit_step   one algp_fit_step at N = --N (10 000) for both forms: host clock around the call (it ends in a stream synchronise),
             after a warm-up; and the ALGP_PROF_KMAT share (the gradient kernel) of one more call
  genotype   algp_genotype_posterior at N = --N for Q = 1 000 and 5 000 (dense G), with and without cov: host clock, and the
             classes of one more call (ALGP_PROF_ROWS: the gathers and reductions, GEMM_TRSM: the solve, GEMM_OTHER: W W^T)

One JSON line per measurement on stdout, all of them in --out.

    python tools/relationship_time.py --out profiles/relationship_time.json
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
LS, OS_A, OS_G, NOISE = np.log([3.0, 3.0]), np.log(0.7), np.log(0.4), np.log(1e-2)


def spread(v):
    v = sorted(v)
    return {'min': v[0], 'median': v[len(v) // 2], 'max': v[-1], 'n': len(v)}


def dense_table(Q, rng):
    """G = A A^T / m from Q x 2Q random markers in {-1, 0, 1}: positive definite, bitwise symmetric."""
    A = rng.randint(0, 3, size=(Q, 2 * Q)).astype(np.float32) - 1.0
    G = (A @ A.T).astype(np.float64) / (2 * Q)
    return 0.5 * (G + G.T)


def set_form(c, form, Q, G):
    if form == 'additive':
        c.set_hypers_additive(np.r_[LS, np.log(1.0)], 2, OS_A, OS_G, NOISE, _hip.KERNEL_MATERN15, _hip.KERNEL_RBF)
    else:
        c.set_hypers_relationship(LS, OS_A, OS_G, NOISE, kernel_a=_hip.KERNEL_MATERN15, G=G, n_genotypes=Q)


def kmat_ms(c, x1, x2, repeats):
    c.kernel_matrix(x1, x2)                                           # warm-up
    ms = []
    for _ in range(repeats):
        c.prof_enable(True)
        c.prof_reset()
        c.kernel_matrix(x1, x2)
        ms.append(c.prof_get('kmat')['ms'])
        c.prof_enable(False)
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10000)
    ap.add_argument('--rows', type=int, default=10000)
    ap.add_argument('--cols', type=int, default=100000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    xx, yy = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    pos = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    perm = rng.permutation(len(pos))
    tables = {1000: dense_table(1000, rng), 5000: dense_table(5000, rng)}
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        c = _hip.Context(dt)
        # ---- the matrix build
        cases = [('additive', 1000, None, 'additive m15+rbf'), ('relationship', 1000, None, 'relationship Q=1000 identity'),
                 ('relationship', 1000, tables[1000], 'relationship Q=1000 dense'),
                 ('relationship', 5000, tables[5000], 'relationship Q=5000 dense')]
        base = None
        for form, Q, G, label in cases:
            ids = rng.randint(Q, size=len(pos)).astype(np.float64)
            X = np.column_stack([pos, ids])
            x1, x2 = X[perm[:a.rows]], X[perm[a.rows:a.rows + a.cols]]
            set_form(c, form, Q, G)
            ms = kmat_ms(c, x1, x2, a.repeats)
            if form == 'additive':
                base = ms['median']
            emit(dict(what='build', dtype=name, case=label, rows=a.rows, cols=a.cols, kmat_ms=ms, ratio_to_additive=ms['median'] / base,
                      entries_per_s=float(a.rows) * a.cols / (ms['median'] * 1e-3)))
        # ---- one fit iteration, then the genotype posterior from its factor
        A = np.sort(perm[:a.N])
        y = np.sin(pos[A, 0] / 30.0) + 0.1 * rng.standard_normal(a.N)
        var = np.full(a.N, 0.01)
        for form, Q, G, label in (cases[0], cases[2], cases[3]):
            ids = rng.randint(Q, size=a.N).astype(np.float64)
            set_form(c, form, Q, G)
            c.set_pool(np.column_stack([pos[A], ids]))
            c.set_train(np.arange(a.N), y, var)
            c.fit_step()                                                  # warm-up: buffers and task lists
            wall = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                c.fit_step()
                wall.append((time.perf_counter() - t0) * 1e3)
            c.prof_enable(True)
            c.prof_reset()
            c.fit_step()
            grad = c.prof_get('kmat')
            c.prof_enable(False)
            emit(dict(what='fit_step', dtype=name, case=label, N=a.N, wall_ms=spread(wall), kmat_class_ms=grad['ms']))
            if form != 'relationship':
                continue
            for cov in (False, True):
                call = lambda: c.genotype_posterior(want_var=True, want_cov=cov)
                call()                                                    # warm-up: the scratch is allocated here
                wall = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    mean, v, _ = call()
                    wall.append((time.perf_counter() - t0) * 1e3)
                c.prof_enable(True)
                c.prof_reset()
                call()
                classes = {k: c.prof_get(k) for k in ('rows', 'gemm_trsm', 'gemm_other')}
                c.prof_enable(False)
                emit(dict(what='genotype_posterior', dtype=name, Q=Q, N=a.N, cov=cov, wall_ms=spread(wall), classes=classes,
                          device_bytes=c.device_bytes(), max_abs_mean=float(np.max(np.abs(mean))), min_var=float(np.min(v))))
        c.close()
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(results, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
