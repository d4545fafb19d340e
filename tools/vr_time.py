"""Times the variance-reduction criterion (ALGP_CRIT_VARIANCE_REDUCTION) at planning sizes: the first scoring after a
candidate solve (one fused product, 2 M^2 K flop), picks 2..4 (one rank-1 fold each) and, for the ratio, a scoring with
ALGP_VR_RANK1=0 at pick 2 (the full product again, over the appended column too).

Every figure is a host clock around an ABI call that ends in a stream synchronise (algp_scores / algp_commit_pick), after a
warm-up of every kernel involved at a small size in the same process; the product's own time is also read from the
library's HIP events (class ALGP_PROF_GEMM_OTHER).  The whole sequence (a new candidate solve, the first scoring, picks
2..4, and pick 2 again by the full product) runs --repeats times; min / median / max of each figure are reported, rates and
the ratio from the medians.  One JSON line per size on stdout, all of them in --out.  --weights rand attaches target
weights uniform in [0.25, 4] (algp_set_target_weights) before the timed sequence: the weighted epilogue and folds.

    python tools/vr_time.py --N 10000 --M 20000 100000 --out profiles/vr_time.json
    ALGP_LIB=ab_tmp/lib_v1.so python tools/vr_time.py --M 20000          # another build of the same ABI, for an A/B
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


def setup(c, N, M, rng):
    """N train sites (a third static, the rest mobile) and M candidates: 1 000 mobile-sampled sites (unit rows, fewer when
    the train set is small) and unsampled sites, uniform in a square with four sites per squared lengthscale."""
    units = min(1000, (N - N // 3) // 2, M // 2)
    n = N + M - units
    side = np.sqrt(n / 4.0) * 3.0
    X = rng.uniform(0.0, side, size=(n, 2))
    c.set_hypers(np.log([3.0, 3.0]), np.log(1.3), np.log(0.05))
    c.set_pool(X)
    ns = N // 3
    c.set_train(np.arange(N), np.zeros(N), np.r_[np.full(ns, SS ** 2), np.full(N - ns, SM ** 2)])
    cand = np.r_[np.arange(ns, ns + units), np.arange(N, n)]
    c.set_candidates(cand, prior_includes_noise=True)
    c.fit_and_solve()
    return cand


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def spread(v):
    v = sorted(v)
    return {'min': v[0], 'median': v[len(v) // 2], 'max': v[-1], 'n': len(v)}


def measure(dtype, N, M, seed, reps, weights='none'):
    os.environ.pop('ALGP_VR_RANK1', None)
    rng = np.random.RandomState(seed)
    c = _hip.Context(dtype)
    setup(c, 300, 600, rng)                          # warm-up: every kernel of both routes, small
    c.greedy(_hip.CRIT_VARIANCE_REDUCTION, SS, SM, 2)
    os.environ['ALGP_VR_RANK1'] = '0'
    c.scores(_hip.CRIT_VARIANCE_REDUCTION, SS, SM)
    os.environ.pop('ALGP_VR_RANK1')
    cand = setup(c, N, M, rng)
    if weights == 'rand':
        c.set_target_weights(np.random.RandomState(seed + 1).uniform(0.25, 4.0, size=c.n_pool))
    Npad = (N + 127) // 128 * 128
    flop = 2.0 * float(len(cand)) ** 2 * Npad
    first, product, full, picks, commits, agree = [], [], [], [[], [], []], [], []
    for rep in range(reps):                          # every repeat: a new solve, the first scoring, picks 2..4
        if rep:
            c.solve_candidates()
        c.prof_enable(True)
        c.prof_reset()
        u, ms = timed(lambda: c.scores(_hip.CRIT_VARIANCE_REDUCTION, SS, SM))
        first.append(ms)
        product.append(c.prof_get(PROF_GEMM_OTHER)['ms'])
        c.prof_enable(False)
        for k in range(3):                           # commit (the rows catch up at the scoring), then score: one fold
            site = int(cand[int(np.argmax(u))])
            commits.append(timed(lambda: c.commit_pick(site, SS, SM))[1])
            u, ms = timed(lambda: c.scores(_hip.CRIT_VARIANCE_REDUCTION, SS, SM))
            picks[k].append(ms)
            if k == 0:                               # the same scoring (pick 2) by the full product, for the ratio; the state
                os.environ['ALGP_VR_RANK1'] = '0'    # it leaves holds the same pick, so the next fold starts from it
                u_full, ms = timed(lambda: c.scores(_hip.CRIT_VARIANCE_REDUCTION, SS, SM))
                os.environ.pop('ALGP_VR_RANK1')
                full.append(ms)
                fin = np.isfinite(u)
                agree.append(float(np.max(np.abs(u[fin] - u_full[fin]) / np.abs(u_full[fin]))))
    c.close()
    med = lambda v: sorted(v)[len(v) // 2]
    return {'dtype': np.dtype(dtype).name, 'N': N, 'M': len(cand), 'repeats': reps, 'weights': weights, 'first_scoring_flop': flop,
            'first_scoring_ms': spread(first), 'first_scoring_product_event_ms': spread(product),
            'first_scoring_tflops': flop / (med(first) * 1e-3) / 1e12, 'product_tflops': flop / (med(product) * 1e-3) / 1e12,
            'commit_ms': spread(commits), 'pick2_scoring_ms': spread(picks[0]), 'pick3_scoring_ms': spread(picks[1]),
            'pick4_scoring_ms': spread(picks[2]), 'pick2_full_product_ms': spread(full),
            'full_over_rank1_at_pick2': med(full) / med(picks[0]), 'rank1_vs_full_max_rel': max(agree)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=10000)
    ap.add_argument('--M', type=int, nargs='+', default=[20000, 100000])
    ap.add_argument('--dtype', default='float64', choices=['float32', 'float64'])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--weights', default='none', choices=['none', 'rand'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rows = []
    for M in a.M:
        rows.append(measure(np.dtype(a.dtype).type, a.N, M, a.seed, a.repeats, a.weights))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
