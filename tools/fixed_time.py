"""Times the fixed effects' entry points at N train rows and M candidates (default 10 000 and 100 000), p = 1, 3, 16, fp64 and
fp32, Matern-3/2 D = 2.  x ~ U(0, 2 sqrt(N / 4))^2, y = sin(x_0) + 0.1 randn + a planted H beta, var ~ U(0.005, 0.05); the bases
are tests/reml_forms.basis.

  gls_ms, reml_step_ms, fit_step_ms, reml_ai_ms, mll_ai_ms, posterior_fixed_ms
                          host clock around the call (each ends in the library's stream synchronise), after two warm-up calls:
                          (median, min, max) of 7
  posterior_pass_ms       the posterior kernel alone: ALGP_PROF_ROWS of a profiled algp_get_posterior_fixed (the gather of the
                          16 x N panel rides in the same class: microseconds), median of 5
  rows_reduce_ms          the yardstick: rows_reduce_launch (sum v^2 and v . z) over the same V^T, ALGP_PROF_ROWS of a profiled
                          candidate solve under ALGP_ROW_STATS=0 (the variance pass), median of 3
  padded_product_ms       the route that needs no new kernel: V^T (Mpad x Npad) against F^T padded to one 128-row tile,
                          algp_bench_gemm on buffers of that shape, beta = 0

One JSON line per (dtype, p) on stdout, all of them in the file given as third argument (default fixed_time_N.json).

    python tools/fixed_time.py 10000 100000 profiles/fixed_time.json
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import reml_forms as RM          # noqa: E402
from algp_amd import _hip        # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
OUT = sys.argv[3] if len(sys.argv) > 3 else 'fixed_time_%d.json' % N


def med(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def profiled(c, f, klass, reps):
    c.prof_enable(True)
    out = []
    for _ in range(reps):
        c.prof_reset()
        f()
        out.append(c.prof_get(klass)['ms'])
    c.prof_enable(False)
    return float(np.median(out))


rng = np.random.RandomState(0)
x = rng.uniform(0, 2.0 * np.sqrt(N / 4.0), (N + M, 2))
var = rng.uniform(0.005, 0.05, N)
noise = 0.1 * rng.standard_normal(N)
results = []
for dtype in (np.float64, np.float32):
    c = _hip.Context(dtype)
    c.set_hypers(np.log([1.3, 2.0]), np.log(0.9), np.log(0.05), _hip.KERNEL_MATERN15)
    c.set_pool(x)
    npad, mpad = -(-N // 128) * 128, -(-M // 128) * 128
    padded = c.bench_gemm(mpad, 128, npad, beta_one=False, reps=5)
    for p in (1, 3, 16):
        H = RM.basis(x, p)
        y = np.sin(x[:N, 0]) + noise + H[:N] @ RM.planted_beta(p)
        r = dict(dtype=np.dtype(dtype).name, N=N, M=M, p=p, padded_product_ms=padded)
        c.set_fixed_effects(H)
        c.set_train(np.arange(N), y, var)
        c.set_candidates(np.arange(N, N + M), prior_includes_noise=False)
        os.environ['ALGP_ROW_STATS'] = '0'
        c.factorize()
        c.solve_candidates()
        r['rows_reduce_ms'] = profiled(c, c.solve_candidates, 'rows', 3)
        del os.environ['ALGP_ROW_STATS']
        for _ in range(2):
            c.gls()
            c.posterior_fixed(want_var=True)
        r['gls_ms'] = med(c.gls, 7)
        r['posterior_fixed_ms'] = med(lambda: c.posterior_fixed(want_var=True), 7)
        r['posterior_pass_ms'] = profiled(c, lambda: c.posterior_fixed(want_var=True), 'rows', 5)
        r['pass_over_rows_reduce'] = r['posterior_pass_ms'] / r['rows_reduce_ms'] if r['rows_reduce_ms'] > 0 else None
        for _ in range(2):
            c.fit_step()
            c.mll_ai()
            c.reml_step()
            c.reml_ai()
        r['fit_step_ms'] = med(c.fit_step, 7)
        r['mll_ai_ms'] = med(c.mll_ai, 7)
        r['reml_step_ms'] = med(c.reml_step, 7)
        r['reml_ai_ms'] = med(c.reml_ai, 7)
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(OUT, 'w') as f:
            json.dump(results, f, indent=1)
    c.close()
