"""Times the separable kernel (algp_set_hypers_separable) against the additive one at the project's sizes, fp64 and fp32, on a
332 x 332 field: D = 2 (row | col) without the genotype term, D = 3 (row | col | genotype id) with a dense Q = 1 000 table.

The forms: (Matern-1/2 x Matern-1/2) -- AR1 x AR1 -- and (Matern-3/2 x RBF), each beside the yardstick, the ADDITIVE form of the
same two forms over the same coordinates with split 1 (the id, where there is one, is part b's second coordinate), measured in
the same process right before it: two exponentials and a product should cost what two exponentials and a sum do.

  build      the kernel-matrix build at --rows x --cols (10 000 x 100 000).  ms = the library's HIP events around the build's
             launches (ALGP_PROF_KMAT) of one algp_kernel_matrix call, after a warm-up call; min / median / max over --repeats
  fit_step   one algp_fit_step at N = --N (10 000): host clock around the call (it ends in a stream synchronise), after a warm-up;
             and the ALGP_PROF_KMAT share (the gradient kernel) of one more call
  mll_ai     one algp_get_mll_ai on that factor: host clock, and its ALGP_PROF_KMAT share (the pass that builds U)
  reml_step  one algp_reml_step with an intercept and a linear trend (p = 3): host clock

Every line carries ratio_to_additive = median / the additive form's median and additive_spread = (max - min) / median of the
additive form's own repeats: a ratio within 1 +- additive_spread says nothing.  One JSON line per measurement on stdout, all of
them in --out.

    python tools/separable_time.py --out profiles/separable_time.json
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
LS, OS, OS_G, NOISE = np.log([3.0, 3.0]), np.log(0.7), np.log(0.4), np.log(1e-2)
PAIRS = [('m05 x m05', _hip.KERNEL_MATERN05, _hip.KERNEL_MATERN05), ('m15 x rbf', _hip.KERNEL_MATERN15, _hip.KERNEL_RBF)]
Q = 1000


def spread(v):
    v = sorted(v)
    return {'min': v[0], 'median': v[len(v) // 2], 'max': v[-1], 'n': len(v)}


def dense_table(q, rng):
    """G = A A^T / m from q x 2q random markers in {-1, 0, 1}: positive definite, bitwise symmetric."""
    A = rng.randint(0, 3, size=(q, 2 * q)).astype(np.float32) - 1.0
    G = (A @ A.T).astype(np.float64) / (2 * q)
    return 0.5 * (G + G.T)


def set_form(c, form, ka, kb, G):
    """form: 'additive' | 'separable'; G: the table, or None for D = 2 without ids."""
    if form == 'additive':
        c.set_hypers_additive(LS if G is None else np.r_[LS, np.log(1.0)], 1, OS, OS_G, NOISE, ka, kb)
    elif G is None:
        c.set_hypers_separable(LS, 1, OS, NOISE, kernel_a=ka, kernel_b=kb)
    else:
        c.set_hypers_separable(LS, 1, OS, NOISE, kernel_a=ka, kernel_b=kb, log_outputscale_g=OS_G, G=G)


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


def wall_ms(call, repeats):
    call()                                                            # warm-up: buffers and task lists
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def kmat_share(c, call):
    c.prof_enable(True)
    c.prof_reset()
    call()
    ms = c.prof_get('kmat')['ms']
    c.prof_enable(False)
    return ms


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
    table = dense_table(Q, rng)
    ids = rng.randint(Q, size=len(pos)).astype(np.float64)
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    def against(base, got):
        return dict(ratio_to_additive=got['median'] / base['median'], additive_spread=(base['max'] - base['min']) / base['median'])

    for dt in (np.float64, np.float32):
        name = np.dtype(dt).name
        c = _hip.Context(dt)
        for G in (None, table):
            X = pos if G is None else np.column_stack([pos, ids])
            shape = 'D=2' if G is None else 'D=3 dense Q=%d' % Q
            x1, x2 = X[perm[:a.rows]], X[perm[a.rows:a.rows + a.cols]]
            A = np.sort(perm[:a.N])
            y = np.sin(pos[A, 0] / 30.0) + 0.1 * rng.standard_normal(a.N)
            var = np.full(a.N, 0.01)
            H = np.c_[np.ones(a.N), pos[A] / float(ROWS) - 0.5]
            for label, ka, kb in PAIRS:
                base = {}
                for form in ('additive', 'separable'):
                    case = '%s %s %s' % (form, label, shape)
                    set_form(c, form, ka, kb, G)
                    ms = kmat_ms(c, x1, x2, a.repeats)
                    r = dict(what='build', dtype=name, case=case, rows=a.rows, cols=a.cols, kmat_ms=ms,
                             entries_per_s=float(a.rows) * a.cols / (ms['median'] * 1e-3))
                    if form == 'additive':
                        base['build'] = ms
                    else:
                        r.update(against(base['build'], ms))
                    emit(r)
                    c.set_pool(X[A])
                    c.set_fixed_effects(H)
                    c.set_train(np.arange(a.N), y, var)
                    for what, call in (('fit_step', c.fit_step), ('mll_ai', c.mll_ai), ('reml_step', c.reml_step)):
                        w = wall_ms(call, a.repeats)
                        r = dict(what=what, dtype=name, case=case, N=a.N, wall_ms=w)
                        if what != 'reml_step':
                            r['kmat_class_ms'] = kmat_share(c, call)
                        if form == 'additive':
                            base[what] = w
                        else:
                            r.update(against(base[what], w))
                        emit(r)
                    c.set_fixed_effects(None)
        c.close()
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(results, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
