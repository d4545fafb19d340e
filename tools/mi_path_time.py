"""Time Agent.best_path under the mutual-information criterion at pool sizes the per-path loop cannot reach
(algp_score_paths_mi against the loop of algp_amd/agent.py: one factor update + two pool-sized set entropies per path).

One pool size per process (`--n`; a driver script runs each under its own time limit), fp64, on a rows x cols grid:
  base      ~6 % of the sites static, ~6 % mobile, ~1 % both (fused train rows, static_std 0.1, mobile_std 1.0)
  paths     1000 row segments of <= 32 changing sites and 1000 of ~200, random starts; a segment crosses static sites
            (re-measured: the delta < 0 case) where it meets them, mobile-sampled sites are left out (no change)
  build     first call minus second call of the short set (the two pool-wide inverses, O(n^3))
  scoring   the second call of each set; the Gram products' rate from algp_prof_get (class gemm_other; the row
            gathers are booked under rows)
  loop      `--loop-paths` paths timed through the per-path loop, extrapolated to 1000 (printed as such); 0 skips it
Prints one JSON line per pool size (and appends it to `--out` if given)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from algp_amd import _hip  # noqa: E402

SHAPES = {5000: (50, 100), 20000: (100, 200), 50000: (200, 250), 110000: (275, 400)}
SSD, MSD = 0.1, 1.0


def segments(rng, rows, cols, mobile, npaths, length):
    """npaths row segments of `length` cells (a segment that reaches the row's end continues on the next row)."""
    n = rows * cols
    out = []
    for _ in range(npaths):
        s = int(rng.randint(n))
        cells = np.arange(s, s + length) % n
        out.append([int(j) for j in cells if not mobile[j]])
    return out


def pack(paths):
    sites = np.full((len(paths), max(1, max(len(p) for p in paths))), -1, dtype=np.int64)
    for k, p in enumerate(paths):
        sites[k, :len(p)] = p
    return sites


def loop_time(c, base, var_base, static, mobile, paths):
    """The per-path loop of Agent._path_utilities_fused(batched=False), seconds per path."""
    n = len(static)
    ss, sm = SSD ** 2, MSD ** 2
    in_base = np.zeros(n, bool)
    in_base[base] = True
    t0 = time.perf_counter()
    for path in paths:
        mob = mobile.copy()
        mob[path] = True
        sampled = static | mob
        extra = [j for j in path if not in_base[j]]
        A = np.r_[base, np.array(extra, dtype=np.int64)]
        var = np.where(static[A] & mob[A], 1.0 / (1.0 / ss + 1.0 / sm), np.where(static[A], ss, sm))
        c.set_train(A, np.zeros(len(A)), var)
        c.factorize(incremental=True)
        ut = c.entropy() + c.set_entropy(np.where(~sampled)[0])
        var_all = np.zeros(n)
        var_all[A] = var
        ut -= c.set_entropy(np.arange(n), var_all)
    return (time.perf_counter() - t0) / len(paths)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, required=True, choices=sorted(SHAPES))
    ap.add_argument('--loop-paths', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rows, cols = SHAPES[a.n]
    n = rows * cols
    rng = np.random.RandomState(a.n % 9973)
    X = np.stack(np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij'), -1).reshape(-1, 2).astype(np.float64)
    perm = rng.permutation(n)
    k = n // 16
    static = np.zeros(n, bool)
    mobile = np.zeros(n, bool)
    static[perm[:k]] = True
    mobile[perm[k - k // 6:2 * k]] = True
    base = np.where(static | mobile)[0]
    ss, sm = SSD ** 2, MSD ** 2
    var_base = np.where(static[base] & mobile[base], 1.0 / (1.0 / ss + 1.0 / sm), np.where(static[base], ss, sm))
    short = segments(rng, rows, cols, mobile, 1000, 34)
    short = [p[:32] for p in short]
    long_ = segments(rng, rows, cols, mobile, 1000, 216)
    long_ = [p[:200] for p in long_]
    rec = dict(n=n, field='%dx%d' % (rows, cols), dtype='f64', train=int(len(base)),
               short_sites_mean=float(np.mean([len(p) for p in short])),
               long_sites_mean=float(np.mean([len(p) for p in long_])),
               remeasured_share=float(np.mean([static[j] for p in long_ for j in p])))
    c = _hip.Context(np.float64)
    try:
        c.set_hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))
        c.set_pool(X)
        c.set_train(base, np.zeros(len(base)), var_base)
        c.factorize()
        cand = np.array(sorted(set(j for p in short + long_ for j in p)), dtype=np.int64)
        c.set_candidates(cand, prior_includes_noise=True)
        t0 = time.perf_counter()
        c.solve_candidates()
        rec['candidates'] = int(len(cand))
        rec['base_solve_s'] = time.perf_counter() - t0
        S, L = pack(short), pack(long_)
        try:
            t0 = time.perf_counter()
            first = c.score_paths_mi(S, SSD, MSD)
            t_first = time.perf_counter() - t0
        except MemoryError as e:
            rec['error'] = 'ALGP_ERR_OOM: %s' % e
            print(json.dumps(rec), flush=True)
            return 0
        for name, sites in (('short', S), ('long', L)):
            c.prof_enable(True)
            c.prof_reset()
            t0 = time.perf_counter()
            got = c.score_paths_mi(sites, SSD, MSD)
            rec['%s_score_s' % name] = time.perf_counter() - t0
            g = c.prof_get('gemm_other')
            rec['%s_gram_tflops' % name] = g['flops'] / (g['ms'] * 1e-3) / 1e12 if g['ms'] > 0 else None
            rec['%s_gram_tflop' % name] = g['flops'] / 1e12
            c.prof_enable(False)
            rec['%s_finite' % name] = bool(np.all(np.isfinite(got)))
            if name == 'short':
                rec['build_s'] = t_first - rec['short_score_s']
                rec['repeat_bit_identical'] = bool(np.array_equal(first, got))
        rec['device_gb'] = c.device_bytes() / 1e9 if hasattr(c, 'device_bytes') else None
    finally:
        c.close()
    if a.loop_paths > 0:
        # the per-path loop in a context of its own (the inverses above are released)
        c = _hip.Context(np.float64)
        try:
            c.set_hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))
            c.set_pool(X)
            c.set_train(base, np.zeros(len(base)), var_base)
            c.factorize()
            try:
                per = loop_time(c, base, var_base, static, mobile, long_[:a.loop_paths])
                rec['loop_s_per_path_measured'] = per
                rec['loop_paths_timed'] = a.loop_paths
                rec['loop_1000_paths_s_extrapolated'] = 1000 * per
            except MemoryError as e:
                rec['loop_error'] = 'ALGP_ERR_OOM: %s' % e
        finally:
            c.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    print('n = %d: build %.3f s; scoring 1000 x <=32 sites %.1f ms, 1000 x ~200 sites %.1f ms (Gram %.1f TFLOP/s)%s'
          % (n, rec['build_s'], 1e3 * rec['short_score_s'], 1e3 * rec['long_score_s'], rec['long_gram_tflops'] or 0,
             '' if 'loop_s_per_path_measured' not in rec else
             '; per-path loop %.3f s per path measured on %d paths -> %.0f s for 1000 (extrapolated)'
             % (rec['loop_s_per_path_measured'], a.loop_paths, rec['loop_1000_paths_s_extrapolated'])))
    return 0


if __name__ == '__main__':
    sys.exit(main())
