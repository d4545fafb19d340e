"""The task lists that fit_and_solve's split launches (api_candidates.hip: plan_route, split_tiles), replayed on the host, no GPU
needed: the last p tile rows of a large candidate set ride the factorisation's launch as a dense panel (mode 1, with the
factorisation's own tasks), every panel tile row but the last -- the one whose padding row carries y - ybar, which changes the
tile's content and not the list -- without its last column tile where the train set ends in a narrow tile.  Replayed by
tools/dag_sched_probe.hip exactly as tests/test_dag_schedule.py replays the other lists (strictly in ticket order by one bulk
worker beside the chain team, at 512 and at 11 workgroups): a list that passes cannot deadlock at any residency.  The shapes:
config 4's factor (79 tiles) with the sweep's 14 leftover row panels on 256 CUs and the other panel heights that were timed
(profiles/split_solve_parts.txt), and the shapes of tests/test_split_solve.py (9 and 17 tiles, 1 and 14 panel rows, with and
without a narrow last tile)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nt, mt, mode, solve_only, pshort)
SHAPES = [(79, 14, 1, 0, 13), (79, 14, 1, 0, 0), (79, 1, 1, 0, 0), (79, 8, 1, 0, 7), (79, 16, 1, 0, 15), (79, 24, 1, 0, 23),
          (79, 32, 1, 0, 31), (79, 7, 1, 0, 6), (9, 7, 1, 0, 0), (9, 1, 1, 0, 0), (9, 14, 1, 0, 0), (17, 1, 1, 0, 0), (17, 14, 1, 0, 13), (17, 14, 1, 0, 0)]


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('probe') / 'dag_sched_probe')
    src = os.path.join(REPO, 'tools', 'dag_sched_probe.hip')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O2', '-std=c++17', '-w', src, '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize('shape', SHAPES, ids=['nt%d_mt%d_short%d' % (s[0], s[1], s[4]) for s in SHAPES])
def test_the_split_routes_task_lists_replay_in_ticket_order(probe, shape):
    r = subprocess.run([probe, '--check-shape'] + [str(v) for v in shape], capture_output=True, text=True, timeout=300)
    want = 'CHECK OK: shape nt %d mt %d mode %d solve_only %d pshort %d' % shape
    assert r.returncode == 0 and want in r.stdout, (shape, r.stdout[-2000:], r.stderr[-1000:])
