"""A transport that fails: the caller's host all-gather (algp_comm_init_host) returns a non-zero code from one collective of a
call, on every rank at the same call number.  No status word can carry such a failure -- there is no exchange left to report it
through -- so every rank returns ALGP_ERR_HIP from that call at once, with the message of the collective that failed, and keeps
its state: the next call over a working transport ends with the picks of a fresh pair of contexts.

A world of two on one card, the ranks threads of this process (as tests/test_vr_sharded.py), the raw form of the callback
(send address, receive address, bytes per rank).  The callback counts its calls per rank; the armed call returns 7 BEFORE it
touches the barrier, on both ranks, so neither is left waiting.  One case per collective:
  (a) the pick exchange of greedy_sharded (fp64 and fp32);
  (b) the agreement word of an incremental factorize with an owner map attached, (c) the row gather behind it;
  (d) the agreement word of the first scoring under the MI and the variance-reduction criterion;
  (e) the first exchange of a pick's fold under either.
The problem is (300, 130, 2) of tests/test_variance_reduction.py: 300 pool sites, 130 train rows (Npad = 256), 150 candidates
per rank (site q on rank q mod 2).  Every case also runs the same calls on a fresh pair over a transport that never fails and
checks there, by its size, that the call number it arms is the collective it names.

The expected messages are what the library produced before its three all-gathers were given one body (the agreement word and
the exchanges of a criterion's state say `factorize_update:` because they go through the factor update's gathers)."""
import ctypes
import os
import sys
import threading
import traceback

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import test_variance_reduction as V                  # noqa: E402
from algp_amd import _hip                            # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

pytestmark = pytest.mark.gpu

SS, SM = V.SS, V.SM
ENT, MI, VR = _hip.CRIT_ENTROPY, _hip.CRIT_MUTUAL_INFORMATION, V.CRIT
F64, F32 = np.float64, np.float32
WORLD, CODE = 2, 7
GREEDY = "algp_hip error 2: greedy_sharded: the caller's all-gather returned 7"
UPDATE = "algp_hip error 2: factorize_update: the caller's all-gather returned 7"


class _Transport(object):
    """the raw all-gather of two rank threads; rank r's call number `fail_at[r]` (counted from arm) returns CODE instead"""

    def __init__(self):
        self.bar = threading.Barrier(WORLD, timeout=60)
        self.slots = [None] * WORLD
        self.calls = [0] * WORLD
        self.fail_at = [None] * WORLD
        self.sizes = [[] for _ in range(WORLD)]

    def arm(self, rank, call):
        self.calls[rank], self.fail_at[rank], self.sizes[rank] = 0, call, []

    def fn(self, rank):
        def gather(send, recv, nbytes):
            k = self.calls[rank]
            self.calls[rank] += 1
            self.sizes[rank].append(nbytes)
            if k == self.fail_at[rank]:
                return CODE
            self.slots[rank] = ctypes.string_at(send, nbytes)
            self.bar.wait()
            out = b''.join(self.slots)
            self.bar.wait()
            ctypes.memmove(recv, out, len(out))
            return 0
        return gather


def run_world(body):
    """body(rank, transport) on two threads; their results in rank order"""
    t = _Transport()
    res, errs = [None] * WORLD, []

    def tgt(r):
        try:
            res[r] = body(r, t)
        except BaseException:
            errs.append('rank %d:\n%s' % (r, traceback.format_exc()))
            t.bar.abort()
    ths = [threading.Thread(target=tgt, args=(r,)) for r in range(WORLD)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, '\n'.join(errs)
    return res


def problem():
    p = V.problem(V.SHAPES[1], O.KERNEL_RBF)
    assert (p.n, p.N) == (300, 130)
    return p


def pick_bytes(p, dtype):
    """a rank's share of a pick's all-gather: 32 bytes + its row of V^T, Npad + 128 elements"""
    npad = (p.N + 127) // 128 * 128
    return 32 + ((npad + 128) * np.dtype(dtype).itemsize + 15) // 16 * 16


def rank_context(p, dtype, r, t):
    mine = np.arange(p.n)[r::WORLD]
    c = V.context(p, dtype, 'coords', cand=mine, alive=p.alive[mine])
    c.comm_init_host(WORLD, r, t.fn(r), raw=True)
    return c, mine


def both_ways(p, dtype, prepare, failing, after, fail_at):
    """prepare(c, r, mine), then on one pair of contexts `failing(c)` with call `fail_at` armed and `after(c)` over the working
    transport, on a fresh pair `failing(c)` unarmed and `after(c)`.  -> per rank ((code, message), picks after the failure),
    per rank (picks of the failing call, picks after it, the sizes of its all-gathers)"""
    def failed(r, t):
        c, mine = rank_context(p, dtype, r, t)
        try:
            prepare(c, r, mine)
            t.arm(r, fail_at)
            with pytest.raises(_hip.AlgpError) as e:
                failing(c)
            assert t.calls[r] == fail_at + 1, 'the call went on after its transport failed'
            t.arm(r, None)
            return (e.value.code, str(e.value)), after(c, r, mine)
        finally:
            c.close()

    def fresh(r, t):
        c, mine = rank_context(p, dtype, r, t)
        try:
            prepare(c, r, mine)
            t.arm(r, None)
            first = failing(c)
            sizes = list(t.sizes[r])
            return first, after(c, r, mine), sizes
        finally:
            c.close()
    return run_world(failed), run_world(fresh)


def ints(v):
    return [int(x) for x in v]


# ---------------------------------------------------------------------------------------------- (a) the pick exchange
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_the_pick_exchange_fails(dtype):
    p = problem()
    bad, good = both_ways(p, dtype, lambda c, r, mine: None, lambda c: ints(c.greedy_sharded(ENT, SS, SM, 3)),
                          lambda c, r, mine: ints(c.greedy_sharded(ENT, SS, SM, 3)), 0)
    for r in range(WORLD):
        assert good[r][2][0] == pick_bytes(p, dtype)
        assert bad[r][0] == (_hip.ERR_HIP, GREEDY), bad[r][0]
        assert good[r][0] == good[0][0] and len(set(good[r][0])) == 3
        assert bad[r][1] == good[r][0], 'no pick was committed by the failed call: the next call starts where a fresh one does'


# ---------------------------------------------------------------------------------------------- (b), (c) the factor update
@pytest.mark.parametrize('what,fail_at', [('agreement', 0), ('rows', 1)])
def test_the_factor_update_fails(what, fail_at):
    """Four sites join the 130 train rows, two owned by each rank: rows [128, 256) of the factor are the update, its agreement
    word is the call's first all-gather and the rows' gather (two rows of 128 doubles per rank) its second."""
    p = problem()
    new = np.r_[p.free[p.free % 2 == 0][:2], p.free[p.free % 2 == 1][:2]]
    A2, noise2 = np.r_[p.A, new], np.r_[p.noise, np.full(len(new), SS ** 2)]
    alive2 = p.alive.copy()
    alive2[new] = False

    def prepare(c, r, mine):
        c.comm_set_owners(np.arange(p.n) % WORLD)
        c.set_train(A2, np.zeros(len(A2)), noise2)

    def after(c, r, mine):
        c.factorize(incremental=True)
        c.set_candidates(mine, prior_includes_noise=True)
        c.solve_candidates(alive=alive2[mine])
        return ints(c.greedy_sharded(ENT, SS, SM, 3))
    bad, good = both_ways(p, F64, prepare, lambda c: c.factorize(incremental=True), after, fail_at)
    for r in range(WORLD):
        assert good[r][2] == [32, 2 * 128 * 8], 'the update exchanged its rows: an agreement word, then two rows per rank'
        assert bad[r][0] == (_hip.ERR_HIP, UPDATE), bad[r][0]
        assert good[r][1] == good[0][1] and len(set(good[r][1])) == 3
        assert bad[r][1] == good[r][1]


# ---------------------------------------------------------------------------------------------- (d), (e) a criterion's state
def _attach(crit):
    def prepare(c, r, mine):
        if crit == MI:
            c.comm_set_mi_groups(1)
        else:
            c.comm_set_vr_exchange(128)
    return prepare


@pytest.mark.parametrize('crit,word', [(MI, 32), (VR, 80)], ids=['mi', 'vr'])
def test_the_agreement_word_of_the_first_scoring_fails(crit, word):
    p = problem()
    bad, good = both_ways(p, F64, _attach(crit), lambda c: ints(c.greedy_sharded(crit, SS, SM, 2)),
                          lambda c, r, mine: ints(c.greedy_sharded(crit, SS, SM, 2)), 0)
    for r in range(WORLD):
        assert good[r][2][0] == word
        assert bad[r][0] == (_hip.ERR_HIP, UPDATE), bad[r][0]
        assert good[r][0] == good[0][0] and len(set(good[r][0])) == 2
        assert bad[r][1] == good[r][0], 'nothing was committed by the failed call'


@pytest.mark.parametrize('crit,fail_at', [(MI, 3), (VR, 6)], ids=['mi', 'vr'])
def test_the_exchange_of_a_fold_fails(crit, fail_at):
    """The second pick of a call folds the first: its first exchange is the all-gather behind the first pick's (MI: agreement,
    build, pick; the variance-reduction criterion: agreement, allocations, two rounds of 128 rows, the build's outcome, pick).
    The first pick stays committed on both ranks, so the next call's two picks are a fresh pair's second and third."""
    p = problem()
    bad, good = both_ways(p, F64, _attach(crit), lambda c: ints(c.greedy_sharded(crit, SS, SM, 2)),
                          lambda c, r, mine: ints(c.greedy_sharded(crit, SS, SM, 2)), fail_at)
    pb = pick_bytes(p, F64)
    for r in range(WORLD):
        sizes = good[r][2]
        assert sizes[fail_at - 1] == pb and sizes[fail_at] != pb and sizes[-1] == pb and sizes.count(pb) == 2, sizes
        assert bad[r][0] == (_hip.ERR_HIP, UPDATE), bad[r][0]
        four = good[r][0] + good[r][1]
        assert four == good[0][0] + good[0][1] and len(set(four)) == 4
        assert bad[r][1] == four[1:3]
