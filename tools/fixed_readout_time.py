"""Times the read-outs that carry the estimated fixed effects against their known-mean siblings at the project's size: N = 10 000
train rows, M = 100 000 candidates on a 332 x 332 field, p = 16 basis columns, Q = 1 000 groups of 100 scattered sites, Q = 1 000
genotypes (a dense table), S = 128 samples, fp64 and fp32.

Per dtype and call, one JSON line on stdout (all of them in --out):
  wall_ms          host clock around the ABI call (it ends in a stream synchronise; results cross to the host inside it), the
                   _fixed call and its sibling alternating in one process after a warm-up of each: min / median / max over
                   --repeats, the ratio of the medians, and the sibling's repeat-to-repeat spread (max - min) / median
  rows_ms          the library's HIP events of one more call of each, profiling on: ALGP_PROF_ROWS (the row passes: the sibling's
                   own, and for the _fixed call also the panel pass, the fold and the gathers), with the launch counts
and per dtype, on device-resident operands with HIP events around --repeats launches after two warm-up launches
(algp_bench_fixed_fold, algp_bench_fixed_panel):
  fold             the rank-p fold on the Q x M cross and on a 128 x M_pad sample tile, beside a device-to-device copy of the
                   same matrix (the fold reads and writes each entry once): fold_ms, copy_ms and their ratio
  panel            the posterior pass over the panels T and W (Q rows padded to 128) and Z^T (128 rows) of N_pad columns with a
                   zero basis row, and over V^T (M rows) for scale: ms per launch

    python tools/fixed_readout_time.py --out profiles/fixed_readout_time.json
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


def basis(X, p, rng):
    """Constant, two scaled coordinates, p - 5 block indicators, two quadratic terms (tests/reml_forms.basis's recipe)."""
    u = (X - X.mean(0)) / (X.max(0) - X.min(0))
    block = rng.randint(0, p - 4, len(X))
    cols = [np.ones(len(X)), u[:, 0], u[:, 1]] + [(block == b).astype(np.float64) for b in range(p - 5)] + \
           [u[:, 0] * u[:, 1], u[:, 0] ** 2 - u[:, 1] ** 2]
    return np.stack(cols[:p], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10000)
    ap.add_argument('--M', type=int, default=100000)
    ap.add_argument('--Q', type=int, default=1000)
    ap.add_argument('--S', type=int, default=128)
    ap.add_argument('--p', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dtypes', default='float64,float32')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    xx, yy = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    X = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    X = np.c_[X, rng.randint(0, a.Q, len(X)).astype(np.float64)]
    H = basis(X[:, :2], a.p, rng)
    perm = rng.permutation(len(X))
    A, cand = np.sort(perm[:a.N]), np.sort(perm[a.N:a.N + a.M])
    y = np.sin(X[A, 0] / 30.0) + 0.1 * rng.standard_normal(a.N) + H[A] @ rng.uniform(-1, 1, a.p)
    var = np.full(a.N, 0.01)
    Z = rng.randint(0, 3, (a.Q, a.Q + 40)).astype(np.float64) - 1.0
    G = Z @ Z.T / Z.shape[1]
    G = (0.5 * (G + G.T)).astype(np.float32).astype(np.float64)
    lab = (rng.permutation(a.M) % a.Q).astype(np.int32)
    prior = rng.standard_normal((a.S, len(X)))
    eps = rng.standard_normal((a.S, a.N))
    results = []
    for name in a.dtypes.split(','):
        dt = np.dtype(name)
        c = _hip.Context(dt)
        c.set_hypers_relationship(np.log([3.0, 3.0]), 0.0, np.log(0.3), np.log(1e-2), kernel_a=_hip.KERNEL_MATERN15, G=G)
        c.set_pool(X)
        c.set_fixed_effects(H)
        c.set_train(A, y, var)
        c.factorize()
        c.set_candidates(cand, prior_includes_noise=False)
        c.solve_candidates()
        pairs = {
            'genotype_cov': lambda f: c.genotype_posterior(want_var=True, want_cov=True, fixed=f),
            'genotype_var': lambda f: c.genotype_posterior(want_var=True, want_cov=False, fixed=f),
            'group_cov': lambda f: c.group_posterior(lab, n_groups=a.Q, want_cov=True, want_cross=False, fixed=f),
            'group_cross': lambda f: c.group_posterior(lab, n_groups=a.Q, want_cov=True, want_cross=True, fixed=f),
            'group_mean': lambda f: c.group_posterior(lab, n_groups=a.Q, want_cov=False, want_cross=False, fixed=f),
            'mean': lambda f: c.posterior_mean_fixed(-1, cand) if f else c.posterior_mean(cand),
            'samples': lambda f: c.sample_posterior(eps, prior=prior, fixed=f),
        }
        for what, call in pairs.items():
            call(False)
            call(True)                                                # warm-up: the scratch is allocated here
            wall = {False: [], True: []}
            for _ in range(a.repeats):
                for f in (False, True):
                    t0 = time.perf_counter()
                    call(f)
                    wall[f].append((time.perf_counter() - t0) * 1e3)
            rows = {}
            for f in (False, True):
                c.prof_enable(True)
                c.prof_reset()
                call(f)
                rows['fixed' if f else 'sibling'] = {k: c.prof_get(k) for k in ('rows', 'gemm_other', 'gemm_trsm', 'kmat')}
                c.prof_enable(False)
            sib, fx = spread(wall[False]), spread(wall[True])
            r = dict(what=what, dtype=dt.name, N=a.N, M=a.M, Q=a.Q, S=a.S, p=a.p, sibling_wall_ms=sib, fixed_wall_ms=fx,
                     ratio=fx['median'] / sib['median'], sibling_spread=(sib['max'] - sib['min']) / sib['median'], classes=rows,
                     device_bytes=c.device_bytes())
            print(json.dumps(r), flush=True)
            results.append(r)
        Mpad, Npad, Qpad = (a.M + 127) // 128 * 128, (a.N + 127) // 128 * 128, (a.Q + 127) // 128 * 128
        for rows, cols, what in ((a.Q, a.M, 'cross'), (128, Mpad, 'sample_tile'), (a.Q, a.Q, 'cov')):
            fold_ms, copy_ms = c.bench_fixed_fold(rows, cols, a.p, reps=20)
            r = dict(what='fold', matrix=what, dtype=dt.name, rows=rows, cols=cols, p=a.p, fold_ms=fold_ms, copy_ms=copy_ms,
                     ratio=fold_ms / copy_ms, fold_gb_per_s=2.0 * rows * cols * dt.itemsize / (fold_ms * 1e-3) / 1e9)
            print(json.dumps(r), flush=True)
            results.append(r)
        for rows, what in ((Qpad, 'T, W'), (128, 'Z^T'), (a.M, 'V^T')):
            ms = c.bench_fixed_panel(rows, Npad, a.p, reps=20)
            r = dict(what='panel', panel=what, dtype=dt.name, rows=rows, ncols=Npad, p=a.p, ms=ms, workgroups=(rows + 63) // 64,
                     gb_per_s=rows * Npad * dt.itemsize / (ms * 1e-3) / 1e9)
            print(json.dumps(r), flush=True)
            results.append(r)
        c.close()
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(results, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
