"""EMULATION of one rank of the sharded MI criterion (algp_comm_set_mi_groups + algp_greedy_sharded) at world 8 on one GPU.

The rank runs its real share -- its pool shard's candidate solve, the build and factorisation of its group's pool-wide
matrix, its row blocks of X = L^-T, the per-pick folds -- but its seven peers are fabricated: the host all-gather hands back
this rank's own bytes for every rank.  So the numbers are one rank's compute and its own collectives' staging, not xGMI
traffic or the wait for the slowest peer, and the utilities are not meaningful (the other group's rows are this rank's
zeros; the greedy then takes in-train sites).  Default: config 4's pool, 110 000 sites, 10 000 of them mobile-sampled,
rank 4 of 8 with the split 4 + 4 -- a rank of the group that holds (C + D_all)^-1, the larger matrix.

    python tools/mi_shard_time.py [--n 110000] [--train 10000] [--rank 4] [--ncomp 4] [--picks 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from algp_amd import _hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=110000)
    ap.add_argument('--train', type=int, default=10000)
    ap.add_argument('--world', type=int, default=8)
    ap.add_argument('--rank', type=int, default=4)
    ap.add_argument('--ncomp', type=int, default=4)
    ap.add_argument('--picks', type=int, default=8)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    side = int(np.ceil(np.sqrt(a.n)))
    X = np.stack(np.unravel_index(np.arange(a.n), (side, side)), 1).astype(np.float64)
    c = _hip.Context(np.float64)
    c.set_hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))
    c.set_pool(X)
    A = np.sort(rng.permutation(a.n)[:a.train])
    c.set_train(A, np.zeros(len(A)), np.full(len(A), 1.0))           # mobile-sampled: the candidates include them
    c.factorize()
    mine = np.arange(a.rank, a.n, a.world, dtype=np.int64)
    c.set_candidates(mine, prior_includes_noise=True)
    c.solve_candidates()
    c.comm_init_host(a.world, a.rank, lambda b: bytes(b) * a.world)
    c.comm_set_mi_groups(a.ncomp)
    before = c.device_bytes()
    t0 = time.perf_counter()
    c.greedy_sharded(_hip.CRIT_MUTUAL_INFORMATION, 0.1, 1.0, 1)
    t1 = time.perf_counter()
    after = c.device_bytes()
    c.greedy_sharded(_hip.CRIT_MUTUAL_INFORMATION, 0.1, 1.0, a.picks)
    t2 = time.perf_counter()
    npad = -(-a.n // 128) * 128
    g = a.ncomp if a.rank < a.ncomp else a.world - a.ncomp
    nt = npad // 128
    member = a.rank if a.rank < a.ncomp else a.rank - a.ncomp
    nloc = (nt - member + g - 1) // g
    print(json.dumps({
        'label': 'EMULATION: one rank of world %d, peers fabricated (its own bytes for every rank)' % a.world,
        'n_pool': a.n, 'train': a.train, 'rank': a.rank, 'n_complement_ranks': a.ncomp,
        'first_pick_s': round(t1 - t0, 3),
        'later_pick_ms': round(1e3 * (t2 - t1) / a.picks, 2),
        'device_bytes_before_build': before, 'device_bytes_after_build': after,
        'peak_factor_plus_rows_bytes': 8 * (npad * npad + nloc * 128 * npad),
    }))
    c.close()


if __name__ == '__main__':
    main()
