"""Times algp_get_mll_ai beside algp_fit_step, and GPR.fit under both fit methods, at N train rows (default 10 000), fp64 and
fp32, for RBF D = 2, the additive form Matern-3/2 (position) + RBF (a covariate) and the relationship form Matern-3/2 + a dense
Q = 1 000 table.  x ~ U(0, 2 sqrt(N / 4))^2, var = 1e-5, y drawn on the host from the model at known parameters (the models of
tests/ai_forms.py, which this tool imports).

  fit_step_ms, mll_ai_ms   host clock around the call (each ends in the library's stream synchronise) at the true parameters,
                           after two warm-up calls: (median, min, max) of 7
  mll_ai_class_ms          ALGP_PROF_KMAT (the pair pass), GEMM_TRSM (the solve), GEMM_OTHER (the Gram product): medians of 5
                           profiled calls
  fit_ai, fit_adam         GPR.fit from the all-zero parameters: wall time of the whole call, device steps, how the Newton loop
                           ended, the final MLL of the whole train set

One JSON line per (model, dtype) on stdout, all of them in the file given as second argument (default ai_time_N.json).

    python tools/ai_time.py 10000 profiles/ai_time.json
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import ai_forms as AI            # noqa: E402
import matern_forms as MF        # noqa: E402
from algp_amd import _hip        # noqa: E402
from algp_amd.models import GPR  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
Q = 1000 if N >= 10000 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else 'ai_time_%d.json' % N


def med(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def models():
    rng = np.random.RandomState(0)
    x2 = rng.uniform(0, 2.0 * np.sqrt(N / 4.0), (N, 2))
    A = rng.randint(0, 3, size=(Q, 2 * Q)).astype(np.float64) - 1.0
    G = A @ A.T / (2 * Q)
    G = (0.5 * (G + G.T)).astype(np.float32).astype(np.float64)
    yield ('rbf', 'single', MF.RBF, x2, AI.pack(np.log([1.3, 2.0]), np.log(0.9), np.log(0.05)), {'type': 'rbf'})
    yield ('additive', 'additive', (MF.MATERN15, MF.RBF, 2), np.c_[x2, rng.uniform(0, 6.0, N)],
           AI.pack(np.log([1.3, 2.0, 1.0]), np.log([0.9, 0.6]), np.log(0.05)),
           {'type': 'additive', 'split': 2, 'parts': ({'type': 'matern', 'nu': 1.5}, {'type': 'rbf'})})
    yield ('relationship', 'relationship', (MF.MATERN15, G, Q), np.c_[x2, rng.randint(0, Q, N).astype(np.float64)],
           AI.pack(np.log([1.5, 2.5]), np.log([0.6, 0.8]), np.log(0.1)),
           {'type': 'genotype', 'spatial': {'type': 'matern', 'nu': 1.5}, 'relationship': G, 'n_genotypes': Q})


def set_hypers(c, family, spec, theta, x):
    log_ls, log_os, log_noise = AI.unpack(family, theta, x)
    if family == 'single':
        c.set_hypers(log_ls, log_os, log_noise, spec)
    elif family == 'additive':
        c.set_hypers_additive(log_ls, spec[2], log_os[0], log_os[1], log_noise, spec[0], spec[1])
    else:
        c.set_hypers_relationship(log_ls, log_os[0], log_os[1], log_noise, kernel_a=spec[0], G=spec[1], n_genotypes=spec[2])


results = []
for name, family, spec, x, theta, kp in models():
    var = np.full(N, 1e-5)
    t0 = time.time()
    y = np.linalg.cholesky(AI.train_matrix(family, spec, theta, x, var)) @ np.random.RandomState(1).standard_normal(N)
    print('%s: data drawn on the host in %.1f s' % (name, time.time() - t0), flush=True)
    for dtype in (np.float64, np.float32):
        r = dict(model=name, dtype=np.dtype(dtype).name, N=N)
        c = _hip.Context(dtype)
        set_hypers(c, family, spec, theta, x)
        c.set_pool(x)
        c.set_train(np.arange(N), y, var)
        for _ in range(2):
            c.fit_step()
            ai = c.mll_ai()
        r['fit_step_ms'] = med(c.fit_step, 7)
        r['mll_ai_ms'] = med(c.mll_ai, 7)
        c.prof_enable(True)
        per = {k: [] for k in ('kmat', 'gemm_trsm', 'gemm_other')}
        for _ in range(5):
            c.prof_reset()
            c.mll_ai()
            for k in per:
                per[k].append(c.prof_get(k)['ms'])
        c.prof_enable(False)
        r['mll_ai_class_ms'] = {k: float(np.median(v)) for k, v in per.items()}
        r['ai_min_eig_over_max'] = float(np.linalg.eigvalsh(ai)[0] / np.linalg.eigvalsh(ai)[-1])
        c.close()
        for method, iters in (('ai', 60), ('adam', 200)):
            gp = GPR(fit_method=method, max_iterations=iters, kernel_params=kp, dtype=dtype)
            gp.ctx                                   # the context exists before the clock starts
            t0 = time.perf_counter()
            losses = gp.fit(x, y, var)
            wall = time.perf_counter() - t0
            mll = gp.ctx.fit_step(want_grad=False)[0]
            info = gp.fit_info or {}
            r['fit_' + method] = dict(wall_s=wall, device_steps=info.get('evaluations', iters), reason=info.get('reason'), mll=mll,
                                      accepted=info.get('iterations'))
            gp.ctx.close()
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(OUT, 'w') as f:
            json.dump(results, f, indent=1)
