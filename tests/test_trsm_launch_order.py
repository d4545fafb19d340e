"""The blocked triangular solve X <- X L^-T (potrf.hip) enqueues the same GEMM launches, in the same order, as the library that
recorded tests/golden/trsm_launch_order.json: every order of the solve (short, push, left-looking with each of its inner
forms and the row-chunk loop, kept columns in the left-looking and the short order) and the two L^-T sweeps of one context
(trinv_upper, trinv_upper_inplace).  By default the task list (chol_dag.hip) takes a from-scratch solve of 33 .. 400 tile rows, so
the cases of 33 and of 321 tile rows switch it off (ALGP_SOLVE_DAG=0) and one of 401 tile rows runs at the defaults.  mi_trinv_rows needs several contexts in one process, whose lines would interleave: it
stays with tests/test_mi_sharded.py.

The library's launch log ($ALGP_LAUNCH_LOG, gemm.hip) has one flushed line per GEMM launch, in enqueue order: class m n k
lower_only batch ktri element-size kcut -- none of them depends on the device's CU count.  The log file is opened once per
process, so the cases run in ONE fresh child process (this file as a script), which notes the log's length around the call
of each case; the switches are read per call, so the child sets os.environ between the cases.  The log does not show
streams, so the child also holds, in the same run, that the posteriors of 1 / 2 / 3 / 4 row chunks are bit-identical and
that the scheduled sweep agrees with ALGP_TRSM_SCHED=0 to test_trsm_scheduled.py's bound (2e-11, fp64).

    python tests/test_trsm_launch_order.py --record      rewrites the fixture from the library as built
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, 'tests', 'golden', 'trsm_launch_order.json')
SWITCHES = ('ALGP_SOLVE_DAG', 'ALGP_RHS_FUSED', 'ALGP_ROW_STATS', 'ALGP_TRSM_INV512', 'ALGP_TRSM_SCHED', 'ALGP_TAIL_COLS',
            'ALGP_TRSM_CHUNKS')
M_LEFT, M_PUSH, M_SHORT = 41088, 4224, 2000        # 321 tile rows: left-looking; 33: the push; 16: short
M_BEYOND = 51328                                   # 401 tile rows: beyond the task list, which by default takes 33 .. 400 of them
NO_DAG = {'ALGP_SOLVE_DAG': '0'}                   # ... so the 33 and the 321 tile rows reach the sweep with it switched off


def _child(out_path):
    sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
    from algp_amd import _hip
    from oracle import gp_oracle as O
    from test_trsm_regimes import _setup, N

    log_path = os.environ['ALGP_LAUNCH_LOG']
    cases = {}

    def log_lines():
        if not os.path.exists(log_path):               # the library opens it at its first GEMM launch
            return []
        with open(log_path) as f:
            return [ln.strip() for ln in f]

    def record(name, call, env=None):
        """run call() under the switches `env`; the log lines it adds are the case's"""
        for k, v in (env or {}).items():
            os.environ[k] = v
        at = len(log_lines())
        res = call()
        cases[name] = log_lines()[at:]
        for k in (env or {}):
            del os.environ[k]
        assert cases[name], name + ': no launch was logged'
        return res

    rng = np.random.RandomState(31)
    c, pool, A, y, var, cidx = _setup(np.float64, M_BEYOND, rng)

    # (a) the short order through the ABI's own entry: 300 x 500 against a 500 x 500 factor
    Lh = np.tril(rng.uniform(-1, 1, (500, 500))) + 25 * np.eye(500)
    record('a_short_300x500', lambda: c.trsm_right_lt(Lh, rng.uniform(-1, 1, (300, 500))))

    def solve():
        c.solve_candidates()
        return c.posterior()

    # (b) the push order on two streams
    c.set_candidates(cidx[:M_PUSH], prior_includes_noise=False)
    record('b_push_33_tile_rows', solve, NO_DAG)

    # (c) scheduled, generated right-hand sides, statistics; (d) every inner form of the left-looking order, the chunk loop
    c.set_candidates(cidx, prior_includes_noise=False)
    record('c_left_scheduled_401_tile_rows_defaults', solve)
    c.set_candidates(cidx[:M_LEFT], prior_includes_noise=False)
    sched = record('c_left_scheduled', solve, NO_DAG)
    for name in ('ALGP_RHS_FUSED', 'ALGP_ROW_STATS', 'ALGP_TRSM_INV512'):
        record('d_' + name + '=0', solve, dict(NO_DAG, **{name: '0'}))
    chunked = {3: record('d_ALGP_TRSM_SCHED=0', solve, dict(NO_DAG, ALGP_TRSM_SCHED='0'))}
    for chunks in (1, 2, 4):
        c.set_trsm_chunks(chunks)
        chunked[chunks] = record('d_set_trsm_chunks_%d' % chunks, solve, NO_DAG)
    c.set_trsm_chunks(0)
    for chunks in (2, 3, 4):
        assert np.array_equal(chunked[chunks][0], chunked[1][0]) and np.array_equal(chunked[chunks][1], chunked[1][1]), chunks
    assert np.max(np.abs(sched[0] - chunked[3][0])) <= 2e-11 and np.max(np.abs(sched[1] - chunked[3][1])) <= 2e-11

    # (e) kept columns: ten train rows appended behind 1 400 -> columns [0, 1280) stay, [1280, 1536) are solved
    os.environ['ALGP_TAIL_COLS'] = '0'
    more = np.setdiff1d(np.arange(40 * 40), A)[:10]
    A2, y2, var2 = np.r_[A, more], np.r_[y, rng.uniform(0, 1, 10)], np.r_[var, np.full(10, 0.01)]
    for M in (M_LEFT, M_SHORT):
        c.set_train(A, y, var)
        c.factorize()
        c.set_candidates(cidx[:M], prior_includes_noise=False)
        c.solve_candidates(incremental=True)
        c.set_train(A2, y2, var2)
        assert c.factorize(incremental=True) == 1280
        kept_cols = record('e_kept_columns_M%d' % M, lambda: c.solve_candidates(incremental=True))
        assert kept_cols == 1280, kept_cols
    del os.environ['ALGP_TAIL_COLS']

    # (f) trinv_upper: the fit iteration at N = 1 400 -- fit_step (whose task list forms L^-T itself: S^-1 = X X^T is what it
    # logs) and the gradient after a plain factorisation (the sweep, 1 408 = 512 + 512 + a ragged 384) --, and a 700-site set
    # (768 = 512 + a ragged 256)
    c.set_train(A, y, var)
    record('f_fit_step', lambda: c.fit_step())
    c.factorize()
    record('f_mll_grad_after_factorize', lambda: c.mll_grad())
    record('f_set_inverse_diag_700', lambda: c.set_inverse_diag(np.arange(700)))
    c.close()

    # (g) trinv_upper_inplace: one MI-criterion build over a 700-site pool (both pool-wide inverses)
    rng = np.random.RandomState(32)
    grid, _ = O.generate_gaussian_data(25, 28, k=5, rng=rng)
    X = grid.astype(np.float64)
    perm = rng.permutation(len(X))
    static = np.zeros(len(X), bool)
    mobile = np.zeros(len(X), bool)
    static[perm[:60]] = True
    mobile[perm[40:120]] = True
    S = np.where(static | mobile)[0]
    v = np.where(static[S] & mobile[S], 1.0 / (1.0 / 0.01 + 1.0), np.where(static[S], 0.01, 1.0))
    g = _hip.Context(np.float64)
    g.set_hypers(np.log([1.5, 1.5]), 0.0, np.log(1e-2))
    g.set_pool(X)
    g.set_train(S, np.zeros(len(S)), v)
    g.factorize()
    g.set_candidates(np.where(~static)[0], prior_includes_noise=True)
    g.solve_candidates()
    record('g_mi_build_700_sites', lambda: g.scores(_hip.CRIT_MUTUAL_INFORMATION, 0.1, 1.0))
    g.close()
    assert N == 1400
    with open(out_path, 'w') as f:
        json.dump(cases, f)


def _run_child():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'cases.json')
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env['ALGP_LAUNCH_LOG'] = os.path.join(tmp, 'launches.txt')
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', out], env=env, cwd=REPO, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, r.stdout[-4000:]
        with open(out) as f:
            return json.load(f)


def test_every_order_enqueues_the_recorded_launches():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = _run_child()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, '%s: launch %d is "%s", recorded "%s"' % (name, i, g, w)
        assert len(got[name]) == len(want[name]), '%s: %d launches, recorded %d' % (name, len(got[name]), len(want[name]))


if __name__ == '__main__':
    if sys.argv[1] == '--child':
        _child(sys.argv[2])
    elif sys.argv[1] == '--record':
        cases = _run_child()
        with open(FIXTURE, 'w') as f:                  # one case per line
            f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(cases[k])) for k in sorted(cases)) + '\n}\n')
        print('recorded', {k: len(v) for k, v in cases.items()})
