"""algp_factorize_update, algp_solve_candidates_update and algp_factorize_from against the fp64 NumPy description of the same state
(tests/incremental_forms.py), on every route Impl<T>::factorize (api_factor.hip) and plan_route / solve_prepare / solve_finish
(api_candidates.hip) can take at the sizes where the routes part: the 128-row blocks, the factor's and V^T's first re-allocation,
all below 470 rows and 300 candidates.  Each case is a scripted sequence of states (incremental_forms.SEQUENCES; the host test
tests/test_incremental_forms_host.py proves cond(S) <= 1e3 at every step and that the expected routes follow from the 128-row
rule).  After EVERY step the updated context is compared with the helper -- not with another context --

    factor() (lower triangle, relative to max |L|), logdet, mll, alpha, posterior() at the ordinary candidates,
    scores(CRIT_ENTROPY, 0.1, 1.0) of all candidates (-inf patterns equal, no NaN; greedy semantics -- under predictive
    semantics the call is refused, which is asserted), posterior_mean of 16 held-out sites,

at the last step of a sequence also mll_grad() and mll_ai() (tests/ai_forms.py), and every step asserts its route: the kept rows
and columns the calls report, algp_debug_counter 1 (rows placed from V^T), gemm_chol launches <= 8 where the gather replaced the
solve (tests/test_incremental.py's bound), no tail_cols launch (these sizes never reach the tail kernel).

All sequences but prefix_changes and short_* get a context of their own instead of one per module: the first allocations and the
re-allocations then happen where the table says, whatever ran before.

Sequences: nothing kept below one block and the first kept block; the triangular solve with the factor's re-allocation
(keep_height = p0 > keep_rows) and the u / w restart; the gather with p0 on a block boundary, in mid-block, a whole new tile and
exactly MAX_APPEND rows, from a factor and a V^T with headroom and from tight ones that grow in the same call; second and third
readings of a site whose first row is in block 0, at keep - 1 and in [keep, p0), the refusal k >= p0
(refusal_first_row_not_in_front_of_p0: no earlier check refuses, which the host test proves), two rows of a new site in one
step; the fall-backs (a site that is no candidate, another candidate list, V^T under other hyper-parameters); var, order and y
changes inside the kept prefix, shrinks and growth after them; the carried row sums (acc3 / acc_cols / uw_stable) over appends,
candidates that become unit rows behind the kept columns, a re-target in block 0, a shrink that makes unit rows ordinary,
alive masks, extra_var, under greedy and predictive semantics; a constant mean that is given; factorize_from from an incrementally
updated source into a destination that holds nothing, a shorter prefix, a longer factor of another tail; and the shortest
gather + solve sequence for D = 1, 3, 5, 8, Matern-1/2 and -5/2, the additive and relationship forms and an explicit pool covariance
(the update's kernel-matrix launches pass row and column offsets that the from-scratch call never does), these in ONE context
per dtype that keeps the buffers and state of the sequence before.  Both dtypes throughout.

Not here: the sharded exchange (several processes: tests/test_sharded_loop.py), the tail kernel's column ranges (from 2 048 kept
rows: tests/test_incremental.py::test_only_the_new_columns_are_solved_after_an_append).  $ALGP_FACTOR_FROM_VT=0 is read once per process: a child process runs
three sequences under it.  No pick is compared, only every candidate's utility.

Tolerances, relative to max(1, |reference|) (max norm): fp64 1e-8; fp32 3e-3 for factor, alpha, mean, variance and scores and five
times that for logdet and mll (tests/test_randomized_sweep.py); the gradient and the average-information matrix at
tests/test_fit_regimes.py's TOL, measured as there and as tests/test_average_information.py does.

Measured on an MI355X (largest error over this file; a sequence takes 0.01 - 0.5 s, the child process 1.2 s, the 57 tests of the file 5.7 s):

    fp64  factor 2.3e-15  logdet 9.3e-15  mll 5.2e-16  alpha 1.3e-14  mean 1.3e-15  variance 2.4e-15  scores 7.8e-15
          held mean 1.0e-15  gradient 8.4e-15  ai 1.9e-14
    fp32  factor 2.2e-05  logdet 1.8e-06  mll 2.4e-07  alpha 4.9e-05  mean 7.5e-06  variance 1.3e-05  scores 1.5e-05
          held mean 5.4e-06  gradient 4.9e-05  ai 1.0e-05

Found by this file: a second reading of a train site under predictive semantics was gathered from V^T without the sigma_n^2 the
two rows share (sequence second_reading_predictive_is_solved_not_gathered: factor error 2.6e-2 in both dtypes before the fix in
vt_rows_for_new_sites).  The file also fails, as it should, on four faults seeded into a scratch build: the `k <= lr` zero dropped
in gather_rows_kernel (second_readings, second_readings_scratch), zero_rows3_launch skipped for rows that became unit rows
(carried_sums, and every gather sequence whose sums are live), `ku` not reset when u and w are re-allocated (solve_route), the `k >= p0` refusal dropped from vt_rows_for_new_sites
(refusal_first_row_not_in_front_of_p0, by its counter: the values stay right, the guard is conservative).
"""
import functools
import time

import numpy as np
import pytest

import ai_forms as AIF
import incremental_forms as F
import test_fit_regimes as FR
from algp_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float64, id='f64'), pytest.param(np.float32, id='f32')]
TOL = {np.dtype(np.float64): 1e-8, np.dtype(np.float32): 3e-3}
WIDE = {np.dtype(np.float64): 1.0, np.dtype(np.float32): 5.0}          # logdet and mll
WORST, SECONDS = {}, {}


@functools.lru_cache(maxsize=None)
def _case(name):
    """[(state, expect, reference)] of a sequence: computed once, shared by both dtypes, never written to."""
    sq = F.SEQUENCES[name]
    _, x, _ = F.problem(sq['model'], sq['M'])
    held = np.arange(len(x) - F.HELD, len(x))
    return x, held, [(st, ex, F.reference(st['model'], x, st, held)) for st, ex in F.states(name)]


@pytest.fixture(scope='module')
def ctxs():
    c = {np.dtype(dt): _hip.Context(dt) for dt in (np.float64, np.float32)}
    yield c
    for v in c.values():
        v.close()
    for (dt, what), e in sorted(WORST.items()):
        print('\nmax error vs fp64 helper  %s %-10s %.2e' % (dt, what, e))
    for name, s in sorted(SECONDS.items()):
        print('\nseconds  %-32s %.2f' % (name, s))


def _err(c, what, got, want, tol, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and not np.any(np.isnan(got)), what
    if want.size == 0:
        return
    scale = max(1.0, float(np.max(np.abs(want)))) if scale is None else scale
    e = float(np.max(np.abs(got - want))) / scale
    key = (c.dtype.name, what)
    WORST[key] = max(WORST.get(key, 0.0), e)
    print('%s %s: error %.3e' % (c.dtype.name, what, e))
    assert e <= tol, (what, e, tol)


def _set_model(c, model, x=None):
    """Hyper-parameters, and with x the pool (as coordinates, or as the covariance K + sigma_n^2 I)."""
    if model.family == 'additive':
        ka, kb, split = model.spec
        c.set_hypers_additive(model.log_ls, split, model.log_os[0], model.log_os[1], model.log_noise, ka, kb)
    elif model.family == 'relationship':
        c.set_hypers_relationship(model.log_ls, model.log_os[0], model.log_os[1], model.log_noise, model.spec[0], G=model.spec[1])
    else:
        c.set_hypers(model.log_ls, model.log_os, model.log_noise, model.spec)
    if x is not None and model.explicit:
        c.set_pool_cov(model.K(x) + model.noise * np.eye(len(x)))
    elif x is not None:
        c.set_pool(x)


def _set_state(c, st):
    c.set_train(st['idx'], st['y'], st['var'])
    if st['cand'] is not None:
        c.set_candidates(st['cand'], prior_includes_noise=st['pin'], extra_var=st['extra'])


def _compare(c, st, ref, held, last, what):
    tol, wide = TOL[c.dtype], TOL[c.dtype] * WIDE[c.dtype]
    model = st['model']
    _err(c, 'factor', np.tril(c.factor()), ref['L'], tol, scale=float(np.max(np.abs(ref['L']))))
    _err(c, 'logdet', c.logdet(), ref['logdet'], wide)
    _err(c, 'mll', c.mll(), ref['mll'], wide)
    _err(c, 'alpha', c.alpha(), ref['alpha'], tol)
    if st['solve']:
        mu, pv = c.posterior()
        o = ref['kind'] < 0
        _err(c, 'mean', mu[o], ref['mu'][o], tol)
        _err(c, 'variance', pv[o], ref['var'][o], tol)
    if st['solve'] and not st['pin']:                                    # algp_scores serves greedy semantics only
        with pytest.raises(ValueError):
            c.scores(_hip.CRIT_ENTROPY, F.S_STD, F.M_STD)
    elif st['solve']:
        s = c.scores(_hip.CRIT_ENTROPY, F.S_STD, F.M_STD)
        assert not np.any(np.isnan(s)), what
        fin = np.isfinite(ref['scores'])
        assert np.array_equal(np.isneginf(s), ~fin), what
        _err(c, 'scores', s[fin], ref['scores'][fin], tol)
        if np.any(~o):                                               # the unit rows' utilities on their own as well
            _err(c, 'unit scores', s[fin & ~o], ref['scores'][fin & ~o], tol)
    if not model.explicit:
        _err(c, 'held mean', c.posterior_mean(held), ref['held'], tol)
    if last and not model.explicit:
        want = ref['grad']()
        g = c.mll_grad()
        assert g.shape == want.shape
        _err(c, 'gradient', g / np.maximum(1.0, np.abs(want)), want / np.maximum(1.0, np.abs(want)), FR.TOL[c.dtype], scale=1.0)
        ai, want = c.mll_ai(), ref['ai']()
        sd = np.sqrt(np.diag(want))
        _err(c, 'ai', ai / np.outer(sd, sd), want / np.outer(sd, sd), FR.TOL[c.dtype], scale=1.0)
        assert AIF.relative_error(ai, want) <= FR.TOL[c.dtype]


def _run(c, name, from_vt=True):
    """from_vt=False: the process runs with the gather switched off; every step that keeps rows must then report counter 1 == 0."""
    sq = F.SEQUENCES[name]
    x, held, case = _case(name)
    c.set_constant_mean(sq['mean'])
    try:
        first, _, ref = case[0]
        model = first['model']
        _set_model(c, model, x)
        _set_state(c, first)
        if sq['first'] == 'scratch':
            c.factorize()
            if first['solve']:
                c.solve_candidates()
        else:
            assert c.factorize(incremental=True) == 0
            if first['solve']:
                assert c.solve_candidates(incremental=True) == 0
        _compare(c, first, ref, held, False, (name, 0))
        for k, (st, expect, ref) in enumerate(case[1:], 1):
            what = (name, k, expect)
            if st['model'] is not model:
                model = st['model']
                _set_model(c, model)
            _set_state(c, st)
            c.prof_enable(True)
            try:
                c.prof_reset()
                kept = c.factorize(incremental=True)
                chol = c.prof_get('gemm_chol')['launches']
                cols = c.solve_candidates(incremental=True, alive=st['alive']) if st['solve'] else None
                tail = c.prof_get('tail_cols')['launches']
            finally:
                c.prof_enable(False)
            placed = c.counter(1)
            print('%s %s step %d: kept %d rows, %s columns, %d rows from V^T, %d gemm_chol launches' %
                  (c.dtype.name, name, k, kept, cols, placed, chol))
            _compare(c, st, ref, held, k == len(case) - 1, what)
            assert kept == expect['kept'], what
            assert cols == expect['cols'], what
            if expect['vt'] is not None:
                assert placed == (expect['vt'] if from_vt else 0), what
                # (a step that changes no train row places only padding rows: nothing to solve on either route)
                if placed > 0 and len(st['idx']) > F.first_changed_row(case[k - 1][0], st):
                    assert chol <= 8, what                         # the Schur product and the small tail factorisation only
            assert tail == 0, what
    finally:
        c.set_constant_mean(None)


OWN = sorted(n for n, s in F.SEQUENCES.items() if not s['shared'])
SHARED = sorted(n for n, s in F.SEQUENCES.items() if s['shared'])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', OWN)
def test_sequence_in_a_new_context(dtype, name):
    """The first allocations and the re-allocations happen where the table says."""
    t0 = time.perf_counter()
    c = _hip.Context(dtype)
    try:
        _run(c, name)
    finally:
        c.close()
    SECONDS[name] = max(SECONDS.get(name, 0.0), time.perf_counter() - t0)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', SHARED)
def test_sequence_in_the_shared_context(ctxs, dtype, name):
    """Other widths, kernels and pools, each on top of the buffers, the factor and the V^T the sequence before left behind."""
    t0 = time.perf_counter()
    _run(ctxs[np.dtype(dtype)], name)
    SECONDS[name] = max(SECONDS.get(name, 0.0), time.perf_counter() - t0)


@functools.lru_cache(maxsize=None)
def _from_case():
    x, held, steps = F.factorize_from_script()
    return x, held, [(what, st, kept, None if what == 'source' else F.reference(st['model'], x, st, held)) for what, st, kept in steps]


@pytest.mark.parametrize('dtype', DTYPES)
def test_factorize_from_an_incrementally_updated_source(dtype):
    """incremental_forms.factorize_from_script: the source grows 129 -> 257 -> 300 by updates (its targets are zero: the greedy
    context); the destination adopts its factor while it holds nothing (kept 0), a shorter prefix (129 rows: kept 128), and a
    longer factor whose tail differs from row 200 on (kept 128); then only the destination's y changes (kept 256).  Everything the
    destination then serves against the helper, under ITS targets."""
    t0 = time.perf_counter()
    x, held, steps = _from_case()
    a, b = _hip.Context(dtype), _hip.Context(dtype)
    try:
        for c in (a, b):
            _set_model(c, steps[0][1]['model'], x)
        for k, (what, st, kept, ref) in enumerate(steps):
            c = a if what == 'source' else b
            c.set_train(st['idx'], st['y'], st['var'])
            got = b.factorize_from(a) if what == 'adopt' else c.factorize(incremental=True)
            assert got == kept, (what, len(st['idx']), got)
            if ref is not None:
                _compare(b, st, ref, held, k == len(steps) - 1, ('factorize_from', what, len(st['idx'])))
    finally:
        a.close()
        b.close()
    SECONDS['factorize_from'] = max(SECONDS.get('factorize_from', 0.0), time.perf_counter() - t0)


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import test_incremental_regimes as T
for dt in (np.float64, np.float32):
    c = T._hip.Context(dt)
    for name in %r:
        T._run(c, name, from_vt=False)
    c.close()
print('__SOLVED_NOT_GATHERED__')
"""
SWITCHED_OFF = ('gather_update', 'second_readings', 'short_matern3')


def test_gather_switched_off_by_the_environment_takes_the_solve():
    """$ALGP_FACTOR_FROM_VT=0 is read once per process, so the sequences run in a child process that has it set: a gather
    sequence, the second readings and one of the short ones, both dtypes, every step against the fp64 helper as above, the kept
    rows and columns as in the table, and counter 1 == 0 at every step that keeps rows -- the solve took the gather's place."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ALGP_FACTOR_FROM_VT='0')
    r = subprocess.run([sys.executable, '-c', _CHILD % (here, os.path.dirname(here), SWITCHED_OFF)], env=env, capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and '__SOLVED_NOT_GATHERED__' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    for name in SWITCHED_OFF:
        assert '%s step 1: ' % name in r.stdout and ' 0 rows from V^T' in r.stdout
