"""The variance-reduction utility of whole paths, algp_score_paths_vr, against the closed form of tests/test_paths_vr_host.py
(which that file holds to one refit per path): u_p = sum_{j in T} var(j | A) - sum_{j in T} var(j | A u path_p).

Problems (sites n, train N, D) and path lengths, generator as in tests/test_variance_reduction.py:
  (100, 40, 2): 1, 5, 20 sites; (300, 130, 2): 3, 40, 64 -- 64 is the LDS kernel's last size, the union spans two ragged tiles;
  (400, 129, 6): 65, 128, 129, 200, 256 -- both block paddings of the batched route and the off-by-one on each side.
Per length an all-new path and one mixing new and statically sampled sites; then one statically sampled site alone, an empty
path and a path listing a site twice.  RBF and Matern, fp64 and fp32, coordinate pool and explicit covariance pool.

Tolerances, per utility, relative to the reference's own value: fp64 1e-9, fp32 1e-3 (the project's bars; a NumPy float32
evaluation of the same closed form is off by at most 4.1e-6).  The argmax equals the reference's in fp64 (the host file
asserts that the reference's top two differ by more than 1e-7 relative).
Measured on an MI355X over all cases of this file: fp64 at most 5.3e-13, fp32 at most 1.3e-4 (on the single re-measured static
site of (300, 130, 2), a utility of 1.5e-4), so neither bar was widened; max_union = 256 against one group: at most 1.6e-16.
"""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import test_paths_vr_host as H                       # noqa: E402
from algp_amd import _hip                            # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

SS, SM = H.SS, H.SM
DTYPES = [np.float64, np.float32]
DIDS = ['f64', 'f32']
POOLS = ['coords', 'cov']
TOL = {np.float64: 1e-9, np.float32: 1e-3}


def context(p, dtype, pool, cand=None, prior_includes_noise=True):
    c = _hip.Context(dtype)
    c.set_hypers(p.hyp.log_lengthscale, p.hyp.log_outputscale, p.hyp.log_noise, p.hyp.kernel)
    if pool == 'cov':
        c.set_pool_cov(p.cov(np.arange(p.n), np.arange(p.n)))
    else:
        c.set_pool(p.X)
    c.set_train(p.A, np.zeros(p.N), p.noise)
    c.factorize()
    c.set_candidates(p.cand if cand is None else cand, prior_includes_noise=prior_includes_noise)
    c.solve_candidates(alive=p.alive if cand is None else None)
    return c


def compare(got, want, names, tol, what):
    """every utility within tol of the reference's (relative to the reference's own value); an empty path exactly 0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got)), (what, got)
    worst = 0.0
    for nm, g, w in zip(names, got, want):
        if w == 0.0:
            assert g == 0.0, (what, nm, g)
            continue
        err = abs(g - w) / abs(w)
        worst = max(worst, err)
        print('%s %-10s got %.12e want %.12e rel %.3e' % (what, nm, g, w, err))
        assert err < tol, (what, nm, err, tol)
    print('%s: worst relative error %.3e (bar %.1e)' % (what, worst, tol))
    return worst


def raw(c, sites, max_union=0):
    sites = np.ascontiguousarray(sites, dtype=np.int64)
    out = np.empty(sites.shape[0])
    return c.lib.algp_score_paths_vr(c.h, _hip._i64(sites.ravel()), sites.shape[0], sites.shape[1], SM, max_union,
                                     out.ctypes.data_as(_hip._dblp))


CASES = dict(argnames='dtype,kernel,shape,pool',
             argvalues=[pytest.param(dt, k, s, pl, id='-'.join([di, ki, si, pl]))
                        for dt, di in zip(DTYPES, DIDS) for k, ki in zip(H.KERNELS, H.KIDS)
                        for s, si in zip(H.SHAPES, H.SHAPE_IDS) for pl in POOLS])


@pytest.mark.parametrize(**CASES)
def test_utilities_equal_the_closed_form(dtype, kernel, shape, pool):
    p, sites, names, want = H.reference(shape, kernel)
    c = context(p, dtype, pool)
    got = c.score_paths_vr(sites, SM)
    again = c.score_paths_vr(sites, SM)
    c.close()
    compare(got, want, names, TOL[dtype], 'utilities')
    assert np.array_equal(got, again), 'two identical calls must return identical bits'
    if dtype is np.float64:
        assert int(np.argmax(got)) == int(np.argmax(want))


@pytest.mark.parametrize('kernel', H.KERNELS, ids=H.KIDS)
def test_grouping_changes_rounding_only(kernel):
    """max_union = 256 cuts the 13 paths of the largest problem into several groups (their union holds about 390 sites)"""
    p, sites, names, want = H.reference(H.SHAPES[2], kernel)
    assert len(set(int(v) for v in sites.ravel() if v >= 0)) > 256
    c = context(p, np.float64, 'coords')
    one = c.score_paths_vr(sites, SM)
    cut = c.score_paths_vr(sites, SM, max_union=256)
    c.close()
    compare(cut, want, names, TOL[np.float64], 'grouped')
    nz = want != 0.0
    err = float(np.max(np.abs(cut[nz] - one[nz]) / np.abs(one[nz])))
    print('grouped against one group: %.3e' % err)
    assert err < 1e-12 and np.array_equal(cut[~nz], one[~nz])


@pytest.mark.parametrize('dtype', DTYPES, ids=DIDS)
def test_targets_beyond_one_chunk(dtype):
    """16 700 candidate rows: the targets pass the E scratch's chunk of columns, Phi is summed over two products"""
    p, sites, names, want = H.reference(H.CHUNK_SHAPE, O.KERNEL_RBF)
    c = context(p, dtype, 'coords')
    got = c.score_paths_vr(sites, SM)
    c.close()
    compare(got, want, names, TOL[dtype], 'chunked')


@pytest.mark.parametrize('dtype', DTYPES, ids=DIDS)
def test_a_switched_off_candidate_stays_a_target(dtype):
    p, sites, names, want = H.reference(H.SHAPES[1], O.KERNEL_MATERN15)
    c = context(p, dtype, 'coords')
    before = c.score_paths_vr(sites, SM)
    alive = p.alive.copy()
    alive[p.free[::5]] = False                       # ordinary rows, some of them on the paths
    assert c.lib.algp_set_candidate_alive(c.h, _hip._ptr(np.ascontiguousarray(alive, dtype=np.uint8))) == _hip.OK
    after = c.score_paths_vr(sites, SM)
    c.close()
    assert np.array_equal(before, after)
    compare(after, want, names, TOL[dtype], 'switched off')


def test_refusals_leave_the_state_usable():
    p, sites, names, want = H.reference(H.SHAPES[2], O.KERNEL_RBF)
    c = context(p, np.float64, 'coords')
    too_long = np.arange(257, dtype=np.int64)[None, :]
    assert raw(c, too_long) == _hip.ERR_BAD_ARG
    assert raw(c, np.arange(256, dtype=np.int64)[None, :]) == _hip.OK
    assert raw(c, sites, max_union=100) == _hip.ERR_BAD_ARG          # below one path's 256 sites
    compare(c.score_paths_vr(sites, SM), want, names, 1e-9, 'after a refused call')
    # a site that is not a resident candidate
    sub = np.sort(np.r_[p.free[:150], p.static[:5]])
    c.set_candidates(sub, prior_includes_noise=True)
    c.solve_candidates()
    outside = int(p.free[200])
    assert raw(c, np.array([[int(sub[0]), outside]])) == _hip.ERR_BAD_ARG
    assert raw(c, np.array([[int(sub[0]), int(sub[1])]])) == _hip.OK
    # picks committed since the solve
    c.commit_pick(int(sub[3]), SS, SM)
    assert raw(c, np.array([[int(sub[0]), int(sub[1])]])) == _hip.ERR_STATE
    # predictive-semantics candidates
    c.set_candidates(p.cand, prior_includes_noise=False)
    c.solve_candidates()
    assert raw(c, sites) == _hip.ERR_STATE
    # a candidate set that lists a pool site twice
    twice = np.r_[p.free[:10], p.free[3]]
    c.set_candidates(twice, prior_includes_noise=True)
    c.solve_candidates()
    assert raw(c, np.array([[int(p.free[0]), int(p.free[1])]])) == _hip.ERR_STATE
    # and the state is usable: the full set again
    c.set_candidates(p.cand, prior_includes_noise=True)
    c.solve_candidates(alive=p.alive)
    compare(c.score_paths_vr(sites, SM), want, names, 1e-9, 'after the refusals')
    c.close()


# ---- the Agent ------------------------------------------------------------------------------------------------------
def _field_agent(incremental, criterion='entropy'):
    from algp_amd.agent import Agent
    from algp_amd.arguments import get_args
    from test_agent_loops import ManhattanField
    np.random.seed(7)
    env = ManhattanField(20, 20, num_test=40)
    args = get_args(['--eval_only', '--kernel', 'rbf', '--max_iterations', '10', '--fraction_pretrain', '0.25',
                     '--criterion', criterion])
    args.incremental = incremental
    return Agent(env, args)


def _agent_brute_force(ag, paths, static_indices):
    """one refit per path from agent.cov_matrix: fused noise per sampled site, the targets every unsampled site"""
    C = np.asarray(ag.cov_matrix, np.float64)
    static, mobile = ag._masks()
    static = static.copy()
    static[static_indices] = True
    ss, sm = ag.static_std ** 2, ag.mobile_std ** 2
    A = np.where(static | mobile)[0]
    T = np.where(~(static | mobile))[0]

    def sumvar(st, mo):
        tr = np.where(st | mo)[0]
        S = C[np.ix_(tr, tr)] + np.diag(ag._fused_var(st[tr], mo[tr]))
        B = C[np.ix_(tr, T)]
        return float(np.sum(np.diag(C)[T]) - np.sum(B * np.linalg.solve(S, B)))

    base = sumvar(static, mobile)
    out = []
    for path in paths:
        mo = mobile.copy()
        mo[[j for j in path if j != -1]] = True
        out.append(base - sumvar(static, mo))
    assert len(A) and len(T)
    return np.array(out)


@pytest.mark.parametrize('incremental', [True, False], ids=['rows', 'fused'])
def test_agent_path_variance_reduction(incremental):
    """Both train forms (a row per reading while the factor is kept across steps; one fused row per site otherwise)."""
    ag = _field_agent(incremental)
    ag.run_greedy_ipp(num_runs=1, criterion='entropy', strategy='Shortest', disp=False)
    assert ag._use_rows() == incremental
    static, mobile = ag._masks()
    assert static.any() and (mobile & ~static).any()
    rng = np.random.RandomState(3)
    free = np.where(~(static | mobile))[0]
    st = np.where(static & ~mobile)[0]
    mob = np.where(mobile)[0]
    waypoint = [int(free[0])]
    paths = [[int(v) for v in rng.choice(free[1:], 12, replace=False)] + [int(st[0]), -1, int(mob[0])],
             [int(v) for v in rng.choice(free[1:], 30, replace=False)] + [int(st[1]), int(st[0])],
             [int(v) for v in rng.choice(free[1:], 7, replace=False)] * 2,
             [int(v) for v in rng.choice(free[1:], 70, replace=False)] + waypoint]
    got = ag.path_variance_reduction(paths, waypoint)
    want = _agent_brute_force(ag, paths, waypoint)
    for g, w in zip(got, want):
        print('agent path: got %.10e want %.10e rel %.2e' % (g, w, abs(g - w) / w))
    # the agent's context is fp32 or fp64 by its arguments: the bar of its width
    tol = TOL[np.float64] if ag.gp.ctx.dtype == np.float64 else TOL[np.float32]
    assert np.all(np.abs(got - want) < tol * np.abs(want))
    long_path = [int(v) for v in np.r_[free, st][:257]]              # 257 sites the path would change
    assert len(long_path) == 257
    with pytest.raises(ValueError, match='256'):
        ag.path_variance_reduction([long_path], waypoint)


def test_run_ipp_routes_by_variance_reduction():
    from test_agent_loops import _connected, _make
    env, agent = _make(seed=1)
    out = agent.run_ipp(num_runs=2, criterion='entropy', strategy='MaxVarRed', disp=False)
    assert len(out['error']) == 2 and np.all(np.isfinite(out['error'])) and len(out['mean']) == len(env.test_X)
    assert _connected(agent.path) and len(agent.static_locations) == 6
    static, mobile = agent._masks()
    missed = [tuple(p) for p in agent.static_locations if not static[env.map_pose_to_gp_index_matrix[tuple(p)]]]
    assert len(missed) <= 2 and all(any(np.array_equal(m, q) for q in agent.path) for m in missed), missed
    passed = {env.map_pose_to_gp_index_matrix[tuple(p)] for p in agent.path[1:]} - {None}
    assert passed <= set(np.where(static | mobile)[0].tolist())
    assert len(agent.collected['ind']) == len(agent.path) - 1
    assert sum(1 for g in agent.collected['ind'] if g != -1) == \
        sum(1 for p in agent.path[1:] if env.map_pose_to_gp_index_matrix[tuple(p)] is not None)
    env2, agent2 = _make(seed=1)
    out2 = agent2.run_ipp(num_runs=1, criterion='variance_reduction', strategy='MaxVarRed', disp=False)
    assert len(out2['error']) == 1 and np.isfinite(out2['error'][0]) and _connected(agent2.path)
