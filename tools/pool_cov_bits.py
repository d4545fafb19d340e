#!/usr/bin/env python3
"""Same bits from two builds of the library for everything that evaluates the pool covariance outside the matrix build.

    python tools/pool_cov_bits.py <first libalgp_hip.so> <second libalgp_hip.so> [report.txt]

Runs the same small problems through both builds ($ALGP_LIB, the hook of algp_amd/_hip.py), each build in a child process of its
own under its own time limit, and compares every array with np.array_equal:
  all four kernel forms x D = 2, 3, 5 (every padded width) x fp64, fp32 x coordinate pool, explicit covariance pool;
  per combination, pool 300 with 130 train sites: greedy, 6 picks, lazily (refresh modes 0 and 1, then the flush, mode 2) and
  with the utilities of every pick; posterior_mean (coordinate pool); score_paths and score_paths_vr with paths of 5 and 64
  sites; the variance-reduction scores before and after two commits (the product's epilogue, then two rank-1 folds);
  pool 400 with 129 train sites: score_paths and score_paths_vr with paths of 65 and 130 sites (both block paddings).
Exit status 0 where every array is equal.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS, SM = 0.1, 1.0
KERNELS = {'rbf': 0, 'matern15': 1, 'matern05': 2, 'matern25': 3}


def kernel_matrix(kid, ls, os_, x):
    d = (x[:, None, :] - x[None, :, :]) / ls
    r = np.sqrt(np.sum(d * d, axis=2))
    if kid == 0:
        return os_ * np.exp(-0.5 * r * r)
    if kid == 2:
        return os_ * np.exp(-r)
    a = np.sqrt(3.0 if kid == 1 else 5.0) * r
    return os_ * (1.0 + a + (a * a / 3.0 if kid == 3 else 0.0)) * np.exp(-a)


def problem(n, N, D, kid):
    """coordinates in [0, 12]^D, lengthscales in [2, 4], outputscale 1.3, noise 0.05 (the suite's generator: its train matrices
    factor in fp32); the first third of the train sites static, the rest mobile; every site a candidate"""
    rng = np.random.RandomState(1000 * n + 10 * D + kid)
    X = rng.uniform(0.0, 12.0, size=(n, D))
    ls = rng.uniform(2.0, 4.0, size=D)
    perm = rng.permutation(n)
    A, free = perm[:N], perm[N:]
    ns = N // 3
    var = np.r_[np.full(ns, SS ** 2), np.full(N - ns, SM ** 2)]
    alive = np.ones(n, bool)
    alive[A[:ns]] = False
    return dict(X=X, ls=ls, A=A, free=free, static=A[:ns], var=var, alive=alive, y=rng.standard_normal(N), rng=rng)


def paths(p, lengths):
    rows = []
    for k in lengths:
        rows.append([int(v) for v in p['rng'].choice(p['free'], k, replace=False)])
        m = max(1, k // 4)
        rows.append([int(v) for v in p['rng'].choice(p['free'], k - m, replace=False)] +
                    [int(v) for v in p['rng'].choice(p['static'], min(m, len(p['static'])), replace=False)])
    sites = np.full((len(rows), max(len(r) for r in rows)), -1, dtype=np.int64)
    for i, r in enumerate(rows):
        sites[i, :len(r)] = r
    return sites


def context(_hip, p, dtype, kid, pool, n):
    c = _hip.Context(dtype)
    c.set_hypers(np.log(p['ls']), np.log(1.3), np.log(0.05), kid)
    if pool == 'cov':
        c.set_pool_cov(kernel_matrix(kid, p['ls'], 1.3, p['X']) + 0.05 * np.eye(n))
    else:
        c.set_pool(p['X'])
    c.set_train(p['A'], p['y'], p['var'])
    c.factorize()
    c.set_candidates(np.arange(n), prior_includes_noise=True)
    c.solve_candidates(alive=p['alive'])
    return c


def worker(out_path):
    sys.path.insert(0, REPO)
    from algp_amd import _hip
    out = {}
    for kname, kid in KERNELS.items():
        for D in (2, 3, 5):
            for dtype in (np.float64, np.float32):
                for pool in ('coords', 'cov'):
                    tag = '%s-D%d-%s-%s' % (kname, D, np.dtype(dtype).name, pool)
                    p = problem(300, 130, D, kid)
                    sites = paths(p, (5, 64))
                    c = context(_hip, p, dtype, kid, pool, 300)
                    out[tag + '/paths'] = c.score_paths(sites, SM)
                    out[tag + '/paths_vr'] = c.score_paths_vr(sites, SM)
                    if pool == 'coords':
                        out[tag + '/posterior_mean'] = c.posterior_mean(np.arange(300))
                    out[tag + '/lazy_picks'] = c.greedy(_hip.CRIT_ENTROPY, SS, SM, 6)
                    out[tag + '/lazy_flushed_scores'] = c.scores(_hip.CRIT_ENTROPY, SS, SM)
                    c.solve_candidates(alive=p['alive'])
                    picks, ut = c.greedy(_hip.CRIT_ENTROPY, SS, SM, 6, want_utilities=True)
                    out[tag + '/greedy_picks'], out[tag + '/greedy_utilities'] = picks, ut
                    c.solve_candidates(alive=p['alive'])
                    out[tag + '/vr_scores_0'] = c.scores(_hip.CRIT_VARIANCE_REDUCTION, SS, SM)
                    for q in (1, 2):
                        c.commit_pick(c.best_candidate(_hip.CRIT_VARIANCE_REDUCTION, SS, SM)[1], SS, SM)
                        out[tag + '/vr_scores_%d' % q] = c.scores(_hip.CRIT_VARIANCE_REDUCTION, SS, SM)
                    c.close()
                    p = problem(400, 129, D, kid)
                    sites = paths(p, (65, 130))
                    c = context(_hip, p, dtype, kid, pool, 400)
                    out[tag + '/long_paths'] = c.score_paths(sites, SM)
                    out[tag + '/long_paths_vr'] = c.score_paths_vr(sites, SM)
                    c.close()
    np.savez(out_path, **out)


def main():
    if sys.argv[1] == '--worker':
        return worker(sys.argv[2])
    libs = [os.path.abspath(a) for a in sys.argv[1:3]]
    report = open(sys.argv[3], 'w') if len(sys.argv) > 3 else None

    def say(line):
        print(line)
        if report:
            report.write(line + '\n')

    tmp = tempfile.mkdtemp()
    res = []
    for i, lib in enumerate(libs):
        path = os.path.join(tmp, 'build%d.npz' % i)
        subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', path], env=dict(os.environ, ALGP_LIB=lib), check=True,
                       timeout=420)
        res.append(np.load(path))
    a, b = res
    assert sorted(a.files) == sorted(b.files)
    bad = 0
    for k in sorted(a.files):
        same = a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True)
        bad += not same
        nan = int(np.sum(np.isnan(a[k])))
        say('%-52s %-12s %s%s' % (k, a[k].shape, 'equal' if same else 'DIFFERENT: max |a - b| = %.3e' % np.nanmax(np.abs(a[k] - b[k])),
                                  ' (%d NaN)' % nan if nan else ''))
    say('%s\n%s\n%d arrays compared with np.array_equal, %d different' % (sys.argv[1], sys.argv[2], len(a.files), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
