"""Times algp_fit_and_solve on bench.py's workload (N = 10 000 train points on the 100 x 100 field, M = 100 000 candidates, fp64,
l = 3, sigma_n^2 = 1e-2) under each of the four kernel forms: median of 10 calls after 3 warm-ups, one line per form.

    python tools/kernel_forms_time.py [--limit SECONDS] [ids ...]

Every form runs in a process of its own under a time limit of its own (--limit, 120 s by default); a form whose process fails
or runs out of time ends the run with its status, and no further form is started."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: 'rbf', 1: 'matern15', 2: 'matern05', 3: 'matern25'}


def one(kid, warmup=3, reps=10, N=10000, M=100000):
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    from algp_amd import _hip
    rng = np.random.RandomState(1)
    R = int(round(np.sqrt(N)))
    grid, field = bench.mog_field(R, N // R, rng)
    var = np.where(rng.uniform(size=len(grid)) < 0.5, 0.01, 1.0)
    y = np.maximum(field + rng.standard_normal(len(grid)) * np.sqrt(var), 0.0)
    cand = bench.candidate_lattice(M, R, N // R, 0)
    c = _hip.Context(np.float64)
    c.set_hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2), kid)
    c.set_pool(np.vstack([grid, cand]))
    c.set_train(np.arange(len(grid)), y, var)
    c.set_candidates(np.arange(len(grid), len(grid) + M), prior_includes_noise=True)
    ts = []
    for i in range(warmup + reps):
        c.sync()
        t0 = time.perf_counter()
        c.fit_and_solve()
        c.sync()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    mu, pv = c.posterior()
    c.close()
    return dict(kernel=kid, name=NAMES[kid], N=len(grid), M=M, dtype='float64', fit_and_solve_ms_median=float(np.median(ts)),
                ms_min=float(np.min(ts)), ms_max=float(np.max(ts)), finite=bool(np.all(np.isfinite(mu)) and np.all(np.isfinite(pv))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--limit', type=float, default=120.0)
    ap.add_argument('--child', type=int, default=None)
    ap.add_argument('ids', nargs='*', type=int, default=[0, 1, 2, 3])
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(one(a.child)), flush=True)
        return 0
    for kid in a.ids:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(kid)], timeout=a.limit)
        except subprocess.TimeoutExpired:
            print('kernel %d: no result within %.0f s; stopping' % (kid, a.limit), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print('kernel %d: exit status %d; stopping' % (kid, r.returncode), file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
