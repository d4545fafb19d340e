#!/usr/bin/env python
"""Times the additive kernel beside Matern-3/2 on the same D = 4 inputs: the 10 000 x 10 000 fp64 kernel-matrix
build (the library's own event timer of the build inside algp_factorize), one fit iteration (algp_fit_step, wall time of the
call) and the variance-reduction criterion's first scoring of 100 000 candidates against 10 000 train rows (wall time of
algp_scores behind a fresh candidate solve).  Best of three each.  Needs an MI355X.

    python tools/additive_timing.py [--train 10000] [--cand 100000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from algp_amd import _hip      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--train', type=int, default=10000)
    ap.add_argument('--cand', type=int, default=100000)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    N, M = a.train, a.cand
    emb = rng.uniform(0, 4, (200, 2))
    X = np.hstack([rng.uniform(0, 100, (N + M, 2)), emb[rng.randint(200, size=N + M)]])
    y = np.sin(X[:N, 0] / 9.0) + 0.3 * np.cos(X[:N, 2]) + 0.1 * rng.standard_normal(N)
    var = np.full(N, 0.01)
    ls = np.log([3.0, 3.0, 1.0, 1.0])
    out = {}
    for name in ('matern15', 'additive'):
        c = _hip.Context(np.float64)
        if name == 'additive':
            c.set_hypers_additive(ls, 2, np.log(0.7), np.log(0.4), np.log(1e-2), _hip.KERNEL_MATERN15, _hip.KERNEL_RBF)
        else:
            c.set_hypers(ls, 0.0, np.log(1e-2), _hip.KERNEL_MATERN15)
        c.set_pool(X)
        c.set_train(np.arange(N), y, var)
        c.prof_enable(True)
        build, fit, score = [], [], []
        for _ in range(4):
            c.prof_reset()
            c.factorize()
            build.append(c.prof_get('kmat')['ms'])
        for _ in range(4):
            t0 = time.perf_counter()
            c.fit_step()
            fit.append(1e3 * (time.perf_counter() - t0))
        c.prof_enable(False)
        c.set_candidates(np.arange(N, N + M))
        for _ in range(3):
            c.factorize()
            c.solve_candidates()
            c.sync()
            t0 = time.perf_counter()
            c.scores(2, 0.1, 1.0)
            score.append(1e3 * (time.perf_counter() - t0))
        c.close()
        out[name] = dict(kmat_build_ms=min(build[1:]), fit_step_ms=min(fit[1:]), alc_first_scoring_ms=min(score))
    out['ratio'] = {k: out['additive'][k] / out['matern15'][k] for k in out['additive']}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
