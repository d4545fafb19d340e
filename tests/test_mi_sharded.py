"""The MI criterion with its pool-wide inverses dealt over ranks (algp_comm_set_mi_groups + algp_greedy_sharded): every rank
holds a share of the rows of X = L^-T of one of the two matrices, and the picks and utilities equal algp_greedy's on one GPU.
Several ranks share the one card: each rank is a thread with a context of its own, all in this one process, joined by a host
all-gather (algp_comm_init_host) -- contexts in separate processes are covered by tests/test_mi_sharded_agent.py; the world
of one (which keeps the one-GPU state) also goes through the RCCL code path."""
import os
import subprocess
import sys
import threading
import traceback

import numpy as np
import pytest

from algp_amd import _hip
from algp_amd.sharded import ShardLink
from oracle import gp_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI = _hip.CRIT_MUTUAL_INFORMATION
SS, SM = 0.1, 1.0


def test_shardlink_splits_the_ranks_between_the_two_matrices():
    """ShardLink's MI split: half and half by default, both matrices on the one rank of a world of one; a split that leaves
    a matrix without ranks is refused."""
    g = lambda b: b
    assert ShardLink(0, 8, all_gather=g).mi_complement_ranks == 4
    assert ShardLink(0, 2, all_gather=g).mi_complement_ranks == 1
    assert ShardLink(0, 1, all_gather=g).mi_complement_ranks == 1
    assert ShardLink(3, 8, all_gather=g, mi_complement_ranks=7).mi_complement_ranks == 7
    for bad in (0, 8):
        with pytest.raises(ValueError):
            ShardLink(0, 8, all_gather=g, mi_complement_ranks=bad)


class _Gather(object):
    """the all-gather of `world` rank threads of this process (a barrier with a time limit: a broken protocol fails)"""

    def __init__(self, world):
        self.world = world
        self.bar = threading.Barrier(world, timeout=300)
        self.slots = [None] * world

    def fn(self, rank):
        def gather(send):
            self.slots[rank] = bytes(send)
            self.bar.wait()
            out = b''.join(self.slots)
            self.bar.wait()
            return out
        return gather


def run_world(world, body):
    """body(rank, gather) on `world` threads; their results in rank order"""
    g = _Gather(world)
    res, errs = [None] * world, []

    def tgt(r):
        try:
            res[r] = body(r, g.fn(r))
        except BaseException:
            errs.append('rank %d:\n%s' % (r, traceback.format_exc()))
            g.bar.abort()
    ths = [threading.Thread(target=tgt, args=(r,)) for r in range(world)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, '\n'.join(errs)
    return res


def _state(c, static, mobile, cand=None):
    A = np.where(static | mobile)[0]
    vf = 1.0 / (1.0 / SS ** 2 + 1.0 / SM ** 2)
    var = np.where(static[A] & mobile[A], vf, np.where(static[A], SS ** 2, SM ** 2))
    c.set_train(A, np.zeros(len(A)), var)
    c.factorize()
    c.set_candidates(np.where(~static)[0] if cand is None else cand, prior_includes_noise=True)
    c.solve_candidates()


def _one_rank(prep, dtype, k):
    c = _hip.Context(dtype)
    try:
        static, mobile = prep(c)
        _state(c, static, mobile)
        picks, ut = c.greedy(MI, SS, SM, k, want_utilities=True)
        return [int(p) for p in picks], [float(np.max(u[np.isfinite(u)])) for u in ut]
    finally:
        c.close()


def _sharded(prep, dtype, k, world, ncomp):
    def body(r, gather):
        c = _hip.Context(dtype)
        try:
            static, mobile = prep(c)
            _state(c, static, mobile, cand=np.where(~static)[0][r::world])
            c.comm_init_host(world, r, gather)
            c.comm_set_mi_groups(ncomp)
            picks, ut = c.greedy_sharded(MI, SS, SM, k, want_utilities=True)
            return [int(p) for p in picks], [float(u) for u in ut], c.device_bytes()
        finally:
            c.close()
    return run_world(world, body)


def _golden_prep(golden, n, kind):
    g = golden('g3_greedy')
    pre = 'g3_n%d_' % n

    def prep(c):
        c.set_hypers(g[pre + 'log_ls'], float(g[pre + 'log_os']), float(g[pre + 'log_noise']))
        c.set_pool_cov(g[pre + 'cov'].astype(np.float64))
        return g[pre + kind + '_static'].astype(bool), g[pre + kind + '_mobile'].astype(bool)
    ut0 = g[pre + kind + '_mutual_information_ut'][0]
    return prep, float(np.max(ut0[np.isfinite(ut0)]))


def _lattice_prep(R, Cc, nstatic, nmobile, seed):
    rng = np.random.RandomState(seed)
    grid, _ = O.generate_gaussian_data(R, Cc, k=5, rng=rng)
    X = grid.astype(np.float64)
    n = len(X)
    perm = rng.permutation(n)
    static = np.zeros(n, bool)
    mobile = np.zeros(n, bool)
    static[perm[:nstatic]] = True
    mobile[perm[nstatic - nstatic // 5:nstatic - nstatic // 5 + nmobile]] = True    # a fifth of the static sites carry both

    def prep(c):
        c.set_hypers(np.log([1.5, 1.5]), 0.0, np.log(1e-2))
        c.set_pool(X)
        return static, mobile
    return prep, static, mobile


@pytest.mark.gpu
@pytest.mark.parametrize('dtname', ['f64', 'f32'])
@pytest.mark.parametrize('kind', ['empty', 'static', 'mobile', 'both'])
@pytest.mark.parametrize('n', [64, 360])
def test_world_of_two_equals_one_rank_on_the_goldens(golden, n, kind, dtname):
    """World 2 on one card, host transport: complement inverse on rank 0, the whole pool's on rank 1.  Picks equal the one-rank
    algp_greedy's, utilities agree with its to 1e-10 relative in fp64 and 1e-4 in fp32, and the first pick's utility is the
    reference's best (its golden utilities; later picks of a free run may differ from the reference's at its near-ties)."""
    dtype = np.float64 if dtname == 'f64' else np.float32
    prep, best0 = _golden_prep(golden, n, kind)
    want, wut = _one_rank(prep, dtype, 4)
    got = _sharded(prep, dtype, 4, 2, 1)
    tol = 1e-10 if dtname == 'f64' else 1e-4
    for r, (picks, ut, _) in enumerate(got):
        assert picks == want, (r, picks, want)
        assert np.max(np.abs(np.array(ut) - wut)) <= tol * max(1.0, np.max(np.abs(wut))), (r, ut, wut)
    assert abs(got[0][1][0] - best0) <= 1e-4 * max(1.0, abs(best0)), (got[0][1][0], best0)   # the reference's fp32 slogdets


@pytest.mark.gpu
@pytest.mark.parametrize('shape,ncomp', [((50, 100, 500, 3000), 1), ((50, 100, 500, 3000), 4), ((50, 100, 500, 3000), 7),
                                         ((15, 20, 30, 150), 4)],
                         ids=['n5000_split1', 'n5000_split4', 'n5000_split7', 'n300_ranks_without_rows'])
def test_world_of_eight_equals_one_rank(shape, ncomp):
    """World 8 on one card: n = 5 000 (ragged last block) under three splits, and n = 300 (three row blocks of the pool's
    matrix for four or fewer ranks: some own no rows).  Six picks, one of them at least a mobile-sampled site."""
    R, Cc, ns, nm = shape
    prep, static, mobile = _lattice_prep(R, Cc, ns, nm, 9)
    want, wut = _one_rank(prep, np.float64, 6)
    assert any(mobile[p] for p in want), 'the case must commit an in-train pick'
    for r, (picks, ut, _) in enumerate(_sharded(prep, np.float64, 6, 8, ncomp)):
        assert picks == want, (r, picks, want)
        assert np.max(np.abs(np.array(ut) - wut)) <= 1e-10 * max(1.0, np.max(np.abs(wut))), (r, ut, wut)


@pytest.mark.gpu
def test_memory_per_rank_after_the_build():
    """n = 20 000, world 8 split 4 + 4: after the build each rank holds at most 0.45 of the one-rank MI build's device bytes."""
    prep, static, mobile = _lattice_prep(100, 200, 1500, 500, 3)
    c = _hip.Context(np.float64)
    try:
        static, mobile = prep(c)
        _state(c, static, mobile)
        c.scores(MI, SS, SM)
        one = c.device_bytes()
    finally:
        c.close()
    got = _sharded(prep, np.float64, 1, 8, 4)
    for r, (picks, _, b) in enumerate(got):
        assert picks == got[0][0]
        assert b <= 0.45 * one, (r, b, one)


@pytest.mark.gpu
def test_a_failure_on_one_rank_is_returned_by_every_rank():
    """algp_debug_fail_at(4): one rank fails in the build, later another in the fold of a pick; every rank raises the same
    error from the same call, the next call succeeds, and the picks end equal to the one-rank run's."""
    prep, static, mobile = _lattice_prep(15, 20, 60, 40, 4)
    want, _ = _one_rank(prep, np.float64, 3)

    def body(r, gather):
        c = _hip.Context(np.float64)
        try:
            static, mobile = prep(c)
            _state(c, static, mobile, cand=np.where(~static)[0][r::2])
            c.comm_init_host(2, r, gather)
            c.comm_set_mi_groups(1)
            if r == 1:
                c.debug_fail_at(4, _hip.ERR_NOT_PD)
            with pytest.raises(np.linalg.LinAlgError):
                c.greedy_sharded(MI, SS, SM, 2)                  # in the build
            picks = [int(p) for p in c.greedy_sharded(MI, SS, SM, 1)]
            if r == 0:
                c.debug_fail_at(4, _hip.ERR_NOT_PD)
            with pytest.raises(np.linalg.LinAlgError):
                c.greedy_sharded(MI, SS, SM, 2)                  # in the fold of the pick committed above
            picks += [int(p) for p in c.greedy_sharded(MI, SS, SM, 2)]
            return picks
        finally:
            c.close()
    for picks in run_world(2, body):
        assert picks == want, (picks, want)


@pytest.mark.gpu
def test_ranks_with_different_layouts_all_refuse_then_agree():
    """World 4: one rank attached n_complement_ranks = 2, the others 1 -- every rank returns ALGP_ERR_BAD_ARG from the same
    call (the layouts travel in the agreement word, before any payload of a layout's size); attached alike, the picks are
    the one-rank run's."""
    prep, static, mobile = _lattice_prep(15, 20, 30, 150, 5)
    want, _ = _one_rank(prep, np.float64, 3)

    def body(r, gather):
        c = _hip.Context(np.float64)
        try:
            static, mobile = prep(c)
            _state(c, static, mobile, cand=np.where(~static)[0][r::4])
            c.comm_init_host(4, r, gather)
            c.comm_set_mi_groups(2 if r == 3 else 1)
            with pytest.raises(ValueError, match='different MI layouts'):
                c.greedy_sharded(MI, SS, SM, 3)
            c.comm_set_mi_groups(2)
            return [int(p) for p in c.greedy_sharded(MI, SS, SM, 3)]
        finally:
            c.close()
    for picks in run_world(4, body):
        assert picks == want, (picks, want)


@pytest.mark.gpu
def test_shardlink_loop_equals_one_rank():
    """Three planning steps at world 2 through ShardLink (owner map + MI split attached by attach()): every step factors the
    grown train set (the sharded factor update), solves the rank's shard and takes four MI picks; the picks equal the
    one-rank loop's at every step, so the sharded MI state is rebuilt after every solve."""
    prep, static0, mobile0 = _lattice_prep(20, 30, 80, 40, 6)
    n = len(static0)

    def loop(c, cand_of, pick):
        static, mobile = static0.copy(), mobile0.copy()
        out = []
        r2 = np.random.RandomState(2)
        for step in range(3):
            A = np.where(static | mobile)[0]
            vf = 1.0 / (1.0 / SS ** 2 + 1.0 / SM ** 2)
            var = np.where(static[A] & mobile[A], vf, np.where(static[A], SS ** 2, SM ** 2))
            c.set_train(A, np.zeros(len(A)), var)
            c.factorize(incremental=True)
            c.set_candidates(cand_of(static), prior_includes_noise=True)
            c.solve_candidates()
            picks = [int(p) for p in pick(c)]
            out.append(picks)
            static[picks] = True
            mobile[r2.permutation(n)[:10]] = True
        return out

    ref = _hip.Context(np.float64)
    try:
        prep(ref)
        want = loop(ref, lambda st: np.where(~st)[0], lambda c: c.greedy(MI, SS, SM, 4))
    finally:
        ref.close()

    def body(r, gather):
        c = _hip.Context(np.float64)
        try:
            prep(c)
            link = ShardLink(r, 2, all_gather=gather)
            link.attach(c, n)
            mine = link.mine(n)
            return loop(c, lambda st: mine[~st[mine]], lambda c: c.greedy_sharded(MI, SS, SM, 4))
        finally:
            c.close()
    for got in run_world(2, body):
        assert got == want, (got, want)


_RCCL_ONE = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from algp_amd import _hip
from oracle import gp_oracle as O
rng = np.random.RandomState(5)
grid, _ = O.generate_gaussian_data(20, 30, k=5, rng=rng)
n = len(grid)
c = _hip.Context(np.float64)
c.set_hypers(np.log([2.0, 2.0]), 0.0, np.log(1e-2))
c.set_pool(grid.astype(np.float64))
perm = rng.permutation(n)
static = np.zeros(n, bool); static[perm[:60]] = True
mobile = np.zeros(n, bool); mobile[perm[40:120]] = True
A = np.where(static | mobile)[0]
vf = 1.0 / (1.0 / 0.01 + 1.0)
var = np.where(static[A] & mobile[A], vf, np.where(static[A], 0.01, 1.0))
c.set_train(A, np.zeros(len(A)), var)
c.factorize()
cand = np.where(~static)[0]
c.set_candidates(cand, prior_includes_noise=True)
c.solve_candidates()
want, ut = c.greedy(_hip.CRIT_MUTUAL_INFORMATION, 0.1, 1.0, 5, want_utilities=True)
c.comm_init(1, 0, _hip.Context.comm_unique_id())
c.comm_set_mi_groups(1)
for rep in range(2):
    c.factorize()
    c.solve_candidates()
    got, gut = c.greedy_sharded(_hip.CRIT_MUTUAL_INFORMATION, 0.1, 1.0, 5, want_utilities=True)
    assert [int(p) for p in got] == [int(p) for p in want], (got, want)
    for p in range(5):
        best = np.max(ut[p][np.isfinite(ut[p])])
        assert abs(gut[p] - best) <= 1e-10 * max(1.0, abs(best)), (p, gut[p], best)
c.comm_destroy()
c.close()
print('MI-SHARDED-ONE-OK')
"""


@pytest.mark.gpu
def test_rccl_world_of_one_equals_greedy():
    """algp_comm_init(1, 0) + the MI layout: greedy_sharded(MI) equals greedy(MI), twice across a fresh factor and solve (the
    sharded state is rebuilt).  In a process of its own: RCCL must be the only copy in its process."""
    r = subprocess.run([sys.executable, '-c', _RCCL_ONE % REPO], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'MI-SHARDED-ONE-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
