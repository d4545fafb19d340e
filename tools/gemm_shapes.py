"""This library's GEMM on the shapes tools/rocblas_yardstick.cpp gives the vendor's (the same card, the same minute), in both
forms of the launcher: one workgroup per tile (ALGP_TRSM_SCHED=0, "plain") and the candidate sweep's scheduled launches
(the default, "sched"), alternated in one process -- ROUNDS times each, so the spread of the plain form is on the table.

    python tools/gemm_shapes.py generated
times the sweep's update launch (m = 100 096, n = 512, beta = 1) with its C tile LOADED against GENERATED in the epilogue from
coordinates (fused right-hand sides, gemm.hip: GEN), alternated, at k = 512, 2 048, 9 728: what the generating epilogue costs or
saves per launch, apart from the kernel-matrix launch and the copy it makes unnecessary."""
import os
import sys

import numpy as np

from algp_amd import _hip

ROUNDS = 3
if sys.argv[1:] == ['generated']:
    for dt, name in ((np.float64, 'dgemm'), (np.float32, 'sgemm')):
        c = _hip.Context(dt)
        for k in (512, 2048, 9728):
            ms = {'loaded': [], 'generated': []}
            for _ in range(ROUNDS):
                for form in ('loaded', 'generated'):
                    ms[form].append(c.bench_gemm(100096, 512, k, beta_one=True, reps=5, generated_c=form == 'generated'))
            for form in ('loaded', 'generated'):
                print('algp %s sched C %-9s m 100096 n 512 k %5d: %s ms (spread %.3f)' % (
                    name, form, k, ' '.join('%8.3f' % v for v in ms[form]), max(ms[form]) - min(ms[form])))
            print('     generated - loaded (medians): %+.4f ms' % (float(np.median(ms['generated'])) - float(np.median(ms['loaded']))))
            sys.stdout.flush()
        c.close()
    sys.exit(0)
for dt, peak in ((np.float64, 78.6), (np.float32, 157.3)):
    c = _hip.Context(dt)
    shapes = [(33408, 512, 2048), (33408, 512, 5120), (33408, 512, 9728), (100096, 512, 2048), (100096, 512, 5120), (100096, 512, 9728),
              (4096, 4096, 4096), (8192, 8192, 8192)]
    if dt == np.float32:
        shapes = [(33408, 512, 5120), (100096, 512, 5120), (8192, 8192, 8192)]
    name = 'dgemm' if dt == np.float64 else 'sgemm'
    for (m, n, k) in shapes:
        ms = {'plain': [], 'sched': []}
        for _ in range(ROUNDS):
            for form in ('plain', 'sched'):
                os.environ['ALGP_TRSM_SCHED'] = '0' if form == 'plain' else '1'
                ms[form].append(c.bench_gemm(m, n, k, beta_one=True, reps=5))
        for form in ('plain', 'sched'):
            best = min(ms[form])
            tf = 2.0 * m * n * k / best / 1e9
            print('algp %s %s m %6d n %5d k %5d: %s ms (spread %.3f)  best %6.1f TFLOP/s = %5.1f %% of %.1f' % (
                name, form, m, n, k, ' '.join('%8.3f' % v for v in ms[form]), max(ms[form]) - min(ms[form]), tf, 100 * tf / peak, peak))
        print('     sched / plain (medians): %.4f' % (float(np.median(ms['sched'])) / float(np.median(ms['plain']))))
        sys.stdout.flush()
    c.close()
os.environ.pop('ALGP_TRSM_SCHED', None)
