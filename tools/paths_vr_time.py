"""Times the variance-reduction utility of whole paths (algp_score_paths_vr) at planning sizes: 1 000 paths of about 32 sites
and 1 000 paths of about 200 sites, N = 10 000 train rows, 100 224 candidates without a train row, fp64 and fp32.

The paths are those of one planning step on a 332 x 332 field: staircase routes from the vehicle's cell to one of eight
waypoints at the path's length in Manhattan distance, so they share most of their sites; the size of the union and the number
of groups it is cut into are reported with the times.

Two yardsticks on the same paths, same box, same process:
  entropy    algp_score_paths (the entropy block scorer: no targets, one log-determinant per path)
  refit      the definition by the calls that existed before this scorer: per path one factor update with the path's sites
             appended (mobile noise), one candidate solve, the posterior variances summed over the targets.  Timed on 8 paths
             and EXTRAPOLATED to 1 000 (x 125): labelled so in the output.  Its utilities are compared with the scorer's.

Every figure is a host clock around an ABI call that ends in a stream synchronise, after a warm-up call of the same shape;
min / median / max over --repeats.  The time of all matrix-core products of a call comes from the library's HIP events in a
separate call (profiling on), not from the timed ones; the share of the E product alone (step 4's launch) is read from a
kernel trace of a run of its own (rocprofv3 --kernel-trace --stats -- python tools/paths_vr_time.py --refit-paths 0 ...).
One JSON line per (dtype, length) on stdout, all of them in --out.

    python tools/paths_vr_time.py --out profiles/paths_vr_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from algp_amd import _hip  # noqa: E402

SS, SM = 0.1, 1.0
PROF_GEMM_OTHER = 7
ROWS, COLS = 332, 332                                # 110 224 sites


def field(N, rng):
    xx, yy = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    X = np.vstack([yy.ravel(), xx.ravel()]).T.astype(np.float64)
    n = len(X)
    A = np.sort(rng.permutation(n)[:N])
    return X, A


def staircase_paths(npaths, length, rng):
    """routes from one start cell to one of eight waypoints `length` steps away (Manhattan), moves in random order"""
    start = (ROWS // 2, COLS // 2)
    ways = []
    for q in range(8):
        dr = int(round(length * (q + 2) / 11.0))
        dc = length - dr
        ways.append((dr if q % 2 else -dr, dc if q % 4 < 2 else -dc))
    sites = np.full((npaths, length), -1, dtype=np.int64)
    for p in range(npaths):
        dr, dc = ways[p % 8]
        moves = np.r_[np.zeros(abs(dr), int), np.ones(abs(dc), int)]
        rng.shuffle(moves)
        r, c = start
        for a, mv in enumerate(moves):
            if mv == 0:
                r += 1 if dr > 0 else -1
            else:
                c += 1 if dc > 0 else -1
            r, c = min(max(r, 0), ROWS - 1), min(max(c, 0), COLS - 1)
            sites[p, a] = r * COLS + c
    return sites


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def spread(v):
    v = sorted(v)
    return {'min': v[0], 'median': v[len(v) // 2], 'max': v[-1], 'n': len(v)}


def refit_loop(c, A, var, n, T, sites, k):
    """u_p by its definition for the first k paths: (utilities, ms per path)"""
    def sumvar(joined=()):
        # a target that joined the train set with noise v is a unit row: its statistic is s = [S^-1]_jj, its variance v - v^2 s
        pv = c.posterior()[1].astype(np.float64)
        pv[list(joined)] = SM ** 2 - SM ** 4 * pv[list(joined)]
        return float(np.sum(pv[T]))
    c.set_train(A, np.zeros(len(A)), var)
    c.factorize(incremental=True)
    c.set_candidates(np.arange(n), prior_includes_noise=True)
    c.solve_candidates()
    base = sumvar()
    in_train = {int(s): i for i, s in enumerate(A)}
    out, ms = [], []
    for p in range(k):
        t0 = time.perf_counter()
        path = [int(j) for j in dict.fromkeys(int(v) for v in sites[p]) if j >= 0]
        v2 = var.copy()
        extra = []
        for s in path:
            if s in in_train:
                v2[in_train[s]] = v2[in_train[s]] * SM ** 2 / (v2[in_train[s]] + SM ** 2)
            else:
                extra.append(s)
        A2 = np.r_[A, np.array(extra, dtype=np.int64)]
        c.set_train(A2, np.zeros(len(A2)), np.r_[v2, np.full(len(extra), SM ** 2)])
        c.factorize(incremental=True)
        c.set_candidates(np.arange(n), prior_includes_noise=True)
        c.solve_candidates()
        out.append(base - sumvar(extra))
        ms.append((time.perf_counter() - t0) * 1e3)
    return np.array(out), ms


def measure(dtype, N, length, npaths, seed, reps, refit_paths):
    rng = np.random.RandomState(seed)
    X, A = field(N, rng)
    n = len(X)
    ns = N // 3
    var = np.r_[np.full(ns, SS ** 2), np.full(N - ns, SM ** 2)][rng.permutation(N)]
    sites = staircase_paths(npaths, length, rng)
    union = len(set(int(v) for v in sites.ravel() if v >= 0))
    c = _hip.Context(dtype)
    c.set_hypers(np.log([3.0, 3.0]), np.log(1.3), np.log(0.05))
    c.set_pool(X)
    c.set_train(A, np.zeros(N), var)
    c.factorize()
    c.set_candidates(np.arange(n), prior_includes_noise=True)
    c.solve_candidates()
    T = np.setdiff1d(np.arange(n), A)
    u = c.score_paths_vr(sites, SM)                   # warm-up, same shapes
    c.score_paths(sites, SM)
    vr, ent = [], []
    for rep in range(reps):                          # alternating, so that drift hits both alike
        c.sync()
        vr.append(timed(lambda: c.score_paths_vr(sites, SM))[1])
        c.sync()
        ent.append(timed(lambda: c.score_paths(sites, SM))[1])
    c.prof_enable(True)
    c.prof_reset()
    _, prof_call_ms = timed(lambda: c.score_paths_vr(sites, SM))
    gemm_ms = c.prof_get(PROF_GEMM_OTHER)['ms']
    gemm_flops = c.prof_get(PROF_GEMM_OTHER)['flops']
    c.prof_enable(False)
    row = {'dtype': np.dtype(dtype).name, 'N': N, 'candidates': n, 'targets': int(len(T)), 'npaths': npaths, 'length': length,
           'union_sites': union, 'repeats': reps,
           'score_paths_vr_ms': spread(vr), 'entropy_score_paths_ms': spread(ent),
           'profiled_call_ms': prof_call_ms, 'profiled_matrix_core_products_ms': gemm_ms,
           'profiled_matrix_core_products_tflops': gemm_flops / max(gemm_ms, 1e-9) / 1e9,
           'finite': bool(np.all(np.isfinite(u)))}
    if refit_paths:
        ref, ms = refit_loop(c, A, var, n, T, sites, refit_paths)
        row['refit_paths_timed'] = refit_paths
        row['refit_ms_per_path'] = spread(ms)
        row['refit_ms_EXTRAPOLATED_to_all_paths'] = float(np.median(ms)) * npaths
        row['scorer_vs_refit_max_rel'] = float(np.max(np.abs(u[:refit_paths] - ref) / np.abs(ref)))
    c.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10000)
    ap.add_argument('--lengths', type=int, nargs='+', default=[32, 200])
    ap.add_argument('--npaths', type=int, default=1000)
    ap.add_argument('--dtypes', nargs='+', default=['float64', 'float32'], choices=['float32', 'float64'])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--refit-paths', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rows = []
    for dt in a.dtypes:
        for length in a.lengths:
            rows.append(measure(np.dtype(dt).type, a.N, length, a.npaths, a.seed, a.repeats, a.refit_paths))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
