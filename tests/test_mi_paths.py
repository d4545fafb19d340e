"""best_path under the mutual-information criterion, all paths at once (algp_score_paths_mi; reference agent.py:358-403,
ent_a + ent_abar - ent_all per path at :374-400): against the oracle's per-path utilities, each of the three terms against
NumPy log-determinants of the sets they stand for, the state rules of the entry point, and the agent against its own
per-path loop."""
import importlib.util
import os
import re

import numpy as np
import pytest

from algp_amd import _hip
from oracle import gp_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS, SM = 0.1 ** 2, 1.0 ** 2


def test_score_paths_mi_is_declared_bound_and_exported():
    """The entry point is part of the C ABI: declared in the header, bound in _hip.SIGNATURES, exported by the .so."""
    hdr = open(os.path.join(REPO, 'include', 'algp_hip.h')).read()
    assert re.search(r'\bint algp_score_paths_mi\(algp_ctx\* ctx, const int64_t\* sites, int npaths, int maxlen,\s*double '
                     r'static_std, double mobile_std,\s*double\* dMI_out, double\* terms_out\);', hdr)
    assert 'algp_score_paths_mi' in _hip.SIGNATURES
    lib = _hip.load()
    assert hasattr(lib, 'algp_score_paths_mi')
    assert hasattr(_hip.Context, 'score_paths_mi')


# ---- GPU: against explicit log-determinants ---------------------------------------------------------------------------
def _field(seed=0):
    rng = np.random.RandomState(seed)
    grid, _ = O.generate_gaussian_data(30, 40, k=5, rng=rng)
    X = grid.astype(np.float64)
    n = len(X)
    perm = rng.permutation(n)
    static = np.zeros(n, bool)
    mobile = np.zeros(n, bool)
    static[perm[:220]] = True
    mobile[perm[160:420]] = True                             # 60 sites with both readings
    return rng, X, static, mobile


def _paths(rng, static, mobile, lengths, rm_share=0.25):
    """Paths of `lengths` changing sites: new (unsampled) and re-measured (static-only) sites, some listed twice, some -1
    entries; a length of 0 is a path with nothing but -1.  Returns the site rows (npaths x width) and the lists of
    changing sites per path."""
    n = len(static)
    new_pool = np.where(~static & ~mobile)[0]
    rm_pool = np.where(static & ~mobile)[0]
    lists = []
    for p, L in enumerate(lengths):
        nrm = min(len(rm_pool), int(round(rm_share * L))) if p % 3 != 2 else 0
        s = list(rng.permutation(rm_pool)[:nrm]) + list(rng.permutation(new_pool)[:L - nrm])
        lists.append([int(v) for v in rng.permutation(s)])
    width = max(lengths) + 4
    rows = np.full((len(lengths), width), -1, dtype=np.int64)
    for p, s in enumerate(lists):
        row = list(s)
        if p % 2 == 0 and row:
            row.append(row[0])                                   # a site crossed twice counts once
        if len(row) + 1 <= width:
            row.insert(rng.randint(len(row) + 1), -1)            # an off-field pose
        rows[p, :len(row)] = row
    return rows, lists


def _slogdet(M):
    s, ld = np.linalg.slogdet(M)
    assert s > 0
    return ld


def _terms_want(Cm, static, mobile, S):
    """(dH_A, dH_Abar, dH_all) of changing the sites S, from NumPy log-determinants of the sets themselves."""
    n = len(Cm)
    S = np.array(sorted(set(S)), dtype=np.int64)

    def state(mob):
        sampled = static | mob
        var = np.zeros(n)
        var[static & mob] = 1.0 / (1.0 / SS + 1.0 / SM)
        var[static & ~mob] = SS
        var[~static & mob] = SM
        A = np.where(sampled)[0]
        hA = len(A) * O.CONST + 0.5 * _slogdet(Cm[np.ix_(A, A)] + np.diag(var[A]))
        B = np.where(~sampled)[0]
        hB = len(B) * O.CONST + 0.5 * _slogdet(Cm[np.ix_(B, B)]) if len(B) else 0.0
        hAll = n * O.CONST + 0.5 * _slogdet(Cm + np.diag(var))
        return np.array([hA, hB, hAll])
    mob1 = mobile.copy()
    mob1[S] = True
    return state(mob1) - state(mobile)


CASES = [('coords', 'rbf', 'f64'), ('cov', 'matern', 'f64'), ('coords', 'matern', 'f32'), ('cov', 'rbf', 'f32')]


@pytest.mark.gpu
@pytest.mark.parametrize('mode,kern,dtname', CASES)
def test_score_paths_mi_against_explicit_logdets(mode, kern, dtname):
    """dMI of ~40 paths (1..64 and 65..256 changing sites: both regimes of the block scorer; re-measured static sites, the
    delta < 0 case; a site twice; -1 entries; an empty path) equals the oracle's per-path MI utility minus the empty path's,
    and each term equals NumPy log-determinants of the sets it stands for."""
    dt = np.float64 if dtname == 'f64' else np.float32
    rng, X, static, mobile = _field(3 if dt == np.float64 else 4)
    n = len(X)
    kid = O.KERNEL_RBF if kern == 'rbf' else O.KERNEL_MATERN15
    hyp = O.Hypers(np.log([3.0, 3.5]), np.log(0.9), np.log(1e-2), kid)
    Cm = O.kernel_matrix(hyp, X) + hyp.noise * np.eye(n)
    c = _hip.Context(dt)
    try:
        c.set_hypers(hyp.log_lengthscale, hyp.log_outputscale, hyp.log_noise, kernel=kid)
        if mode == 'coords':
            c.set_pool(X)
        else:
            c.set_pool_cov(Cm)
        A = np.where(static | mobile)[0]
        var = np.where(static[A] & mobile[A], 1.0 / (1.0 / SS + 1.0 / SM), np.where(static[A], SS, SM))
        c.set_train(A, np.zeros(len(A)), var)
        c.factorize()
        c.set_candidates(np.where(~mobile)[0], prior_includes_noise=True)
        c.solve_candidates()
        rel = 1e-7 if dt == np.float64 else 3e-3
        short = [0, 1, 2, 3, 5, 8, 13, 17, 21, 26, 30, 34, 40, 47, 52, 58, 61, 64, 33, 9, 4, 44, 63, 12]
        long_ = [65, 70, 96, 127, 128, 129, 150, 200, 241, 256, 100, 180, 77, 130, 255, 20]
        for lengths in (short, long_):
            rows, lists = _paths(rng, static, mobile, lengths)
            got, terms = c.score_paths_mi(rows, 0.1, 1.0, want_terms=True)
            assert np.all(np.isfinite(got)), got
            assert np.allclose(got, terms[:, 0] + terms[:, 1] - terms[:, 2], rtol=0, atol=1e-12 * np.max(np.abs(got)))
            # the oracle's utilities (agent.py:374-400), relative to a path that changes nothing
            _, ut = O.best_path_ref(Cm, static, mobile, [[]] + lists, [], 0.1, 1.0, 'mutual_information')
            want = ut[1:] - ut[0]
            assert np.max(np.abs(got - want)) <= rel * np.max(np.abs(want)), (lengths, np.max(np.abs(got - want)))
            if 0 in lengths:
                assert got[lengths.index(0)] == 0.0 and np.all(terms[lengths.index(0)] == 0.0)
            # each term on its own
            for p in range(0, len(lists), 3 if dt == np.float32 else 2):
                tw = _terms_want(Cm, static, mobile, lists[p])
                scale = max(1.0, np.max(np.abs(want)))
                assert np.max(np.abs(terms[p] - tw)) <= rel * scale, (lengths[p], terms[p], tw)
    finally:
        c.close()


# ---- GPU: state handling -----------------------------------------------------------------------------------------------
def _rc(c, rows, ss=0.1, sm=1.0):
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.empty(rows.shape[0])
    return c.lib.algp_score_paths_mi(c.h, rows.ctypes.data_as(_hip._i64p), rows.shape[0], rows.shape[1], ss, sm,
                                     out.ctypes.data_as(_hip._dblp), None)


def _small_ctx(dt=np.float64):
    rng, X, static, mobile = _field(7)
    c = _hip.Context(dt)
    c.set_hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))
    c.set_pool(X)
    A = np.where(static | mobile)[0]
    var = np.where(static[A] & mobile[A], 1.0 / (1.0 / SS + 1.0 / SM), np.where(static[A], SS, SM))
    c.set_train(A, np.zeros(len(A)), var)
    c.factorize()
    return c, rng, static, mobile


@pytest.mark.gpu
def test_score_paths_mi_state_rules():
    c, rng, static, mobile = _small_ctx()
    try:
        free = np.where(~static & ~mobile)[0]
        rows = np.array([free[:5], free[5:10]], dtype=np.int64)
        assert _rc(c, rows) == _hip.ERR_STATE                          # no candidate solve
        c.set_candidates(np.where(~mobile)[0], prior_includes_noise=False)
        c.solve_candidates()
        assert _rc(c, rows) == _hip.ERR_STATE                          # predictive semantics
        c.set_candidates(free[:300], prior_includes_noise=True)
        c.solve_candidates()
        assert _rc(c, np.array([[free[400]]])) == _hip.ERR_STATE       # not a resident candidate
        too_long = np.full((1, 270), -1, dtype=np.int64)
        too_long[0, :257] = free[:257]
        assert _rc(c, too_long) == _hip.ERR_BAD_ARG                    # 257 changing sites
        assert _rc(c, rows) == _hip.OK
        c.commit_pick(int(free[50]), 0.1, 1.0)
        assert _rc(c, rows) == _hip.ERR_STATE                          # a pick committed since the solve
        # a train set that lists a site twice: the MI greedy's message
        A = np.r_[np.where(static)[0], np.where(static)[0][:3]]
        c.set_train(A, np.zeros(len(A)), np.full(len(A), SS))
        c.factorize()
        c.set_candidates(free[:300], prior_includes_noise=True)
        c.solve_candidates()
        assert _rc(c, rows) == _hip.ERR_STATE
        with pytest.raises(ValueError, match='lists a site more than once'):
            c.score_paths_mi(rows, 0.1, 1.0)
    finally:
        c.close()


@pytest.mark.gpu
def test_score_paths_mi_reports_the_scratch_it_needs():
    """A 200 000-site pool: the two pool-wide inverses (640 GB) do not fit; ALGP_ERR_OOM with the byte count up front, and
    the context still scores the entropy criterion afterwards."""
    rng = np.random.RandomState(1)
    n = 200000
    X = rng.uniform(0, 500, (n, 2))
    c = _hip.Context(np.float64)
    try:
        c.set_hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))
        c.set_pool(X)
        A = np.arange(200)
        c.set_train(A, np.zeros(200), np.full(200, 0.01))
        c.factorize()
        c.set_candidates(np.arange(200, 1200), prior_includes_noise=True)
        c.solve_candidates()
        rows = np.array([[200, 201, 202, 203], [300, 301, -1, 300]], dtype=np.int64)
        with pytest.raises(MemoryError) as ei:
            c.score_paths_mi(rows, 0.1, 1.0)
        assert 'bytes for n_pool' in str(ei.value) and str(n) in str(ei.value)
        s = c.scores(_hip.CRIT_ENTROPY, 0.1, 1.0)
        assert np.all(np.isfinite(s))
        assert np.all(np.isfinite(c.score_paths(rows, 1.0)))
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtname', ['f64', 'f32'])
def test_score_paths_mi_second_call_reuses_the_inverses(dtname):
    """A second call on the same state gives the same bits and builds nothing pool-wide: no kernel-matrix build, no
    factorisation launch (the profiler's launch counts)."""
    dt = np.float64 if dtname == 'f64' else np.float32
    c, rng, static, mobile = _small_ctx(dt)
    try:
        c.set_candidates(np.where(~mobile)[0], prior_includes_noise=True)
        c.solve_candidates()
        for lengths in ([3, 17, 40, 64, 1], [90, 200, 12]):
            rows, _ = _paths(rng, static, mobile, lengths)
            c.prof_enable(True)
            c.prof_reset()
            first = c.score_paths_mi(rows, 0.1, 1.0)
            c.prof_reset()
            second = c.score_paths_mi(rows, 0.1, 1.0)
            counts = {k: c.prof_get(k)['launches'] for k in ('kmat', 'chol_dag', 'gemm_chol', 'gemm_chol_update', 'cholesky')}
            gemm = c.prof_get('gemm_other')
            c.prof_enable(False)
            assert np.array_equal(first, second)
            assert all(v == 0 for v in counts.values()), counts
            assert gemm['launches'] > 0 and gemm['flops'] > 0 and gemm['bytes'] > 0
    finally:
        c.close()


# ---- GPU: the agent ----------------------------------------------------------------------------------------------------
def _mi_agent(seed, rows, cols):
    from algp_amd.agent import Agent
    from algp_amd.arguments import get_args
    from algp_amd.field import SyntheticField
    np.random.seed(seed)
    env = SyntheticField(rows, cols, num_test=40)
    args = get_args(['--eval_only', '--kernel', 'rbf', '--max_iterations', '10', '--fraction_pretrain', '0.1'])
    ag = Agent(env, args)
    ag._setup_ipp('mutual_information')
    return env, ag


@pytest.mark.gpu
def test_agent_best_path_mi_batched_equals_per_path_loop():
    """Agent.best_path (MI) on a 40 x 50 field with the greedy's waypoints as static_indices: the batched route's utilities
    equal the per-path loop's (each relative to its own path 0) and both choose the same path."""
    env, ag = _mi_agent(6, 40, 50)
    rng = np.random.RandomState(9)
    n = env.num_samples
    mob = [int(i) for i in rng.permutation(n)[:40]]
    ag._add_samples(mob, [ag.mobile_std] * len(mob))
    waypoints = ag.greedy(3)
    static, mobile = ag._masks()
    st = static.copy()
    st[waypoints] = True
    paths = []
    for k in range(30):
        L = rng.randint(2, 60) if k % 5 else rng.randint(70, 200)
        pth = [int(j) for j in rng.permutation(n)[:L]]
        pth[rng.randint(L)] = int(waypoints[k % 3])                        # re-measures a waypoint
        pth[rng.randint(L)] = int(rng.choice(np.where(static)[0]))         # and a static site
        pth[rng.randint(L)] = int(rng.choice(np.where(mobile)[0]))         # a mobile site: no change
        pth.append(pth[0])                                                 # a site crossed twice
        paths.append(pth)
    c = ag._load_pool()
    ub = ag._path_utilities_fused(c, paths, st, mobile, batched=True)
    ul = ag._path_utilities_fused(c, paths, st, mobile, batched=False)
    db, dl = ub - ub[0], ul - ul[0]
    assert np.all(np.isfinite(ub))
    assert np.max(np.abs(db - dl)) <= 1e-7 * np.max(np.abs(dl)), np.max(np.abs(db - dl))
    assert int(np.argmax(ub)) == int(np.argmax(ul)) == ag.best_path(paths, waypoints)


def _loops_module():
    spec = importlib.util.spec_from_file_location('_mi_agent_loops', os.path.join(REPO, 'tests', 'test_agent_loops.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_run_ipp_mi_chooses_the_paths_of_the_per_path_route():
    """run_ipp(criterion='mutual_information') with the batched path scoring follows the same paths as with the
    per-path loop (a subclass that always takes the loop)."""
    from algp_amd.agent import Agent
    loops = _loops_module()

    class LoopAgent(Agent):
        def _path_utilities_fused(self, c, paths, static, mobile0, batched=True):
            return super()._path_utilities_fused(c, paths, static, mobile0, batched=False)

    runs = []
    for cls in (Agent, LoopAgent):
        env, agent = loops._make(seed=2)
        agent.__class__ = cls
        out = agent.run_ipp(num_runs=2, criterion='mutual_information', strategy='MaxEnt', disp=False)
        runs.append((np.array(agent.path), [float(e) for e in out['error']]))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert len(runs[0][1]) == 2
