"""The variance-reduction criterion at the host level: the command line, the binding's constant, and an Agent planning with
criterion='variance_reduction' on the 20 x 20 synthetic field (greedy on its three data routes: factor kept across steps,
from scratch, and an assigned covariance matrix), against the brute force of tests/test_variance_reduction.py computed
from agent.cov_matrix."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))


def test_command_line_accepts_the_criterion():
    from algp_amd.arguments import get_args
    assert get_args(['--criterion', 'variance_reduction']).criterion == 'variance_reduction'


def test_binding_constant_matches_the_header():
    from algp_amd import _hip
    assert _hip.CRIT_VARIANCE_REDUCTION == 2
    text = open(os.path.join(REPO, 'include', 'algp_hip.h')).read()
    m = re.search(r'ALGP_CRIT_VARIANCE_REDUCTION\s*=\s*(\d+)', text)
    assert m and int(m.group(1)) == _hip.CRIT_VARIANCE_REDUCTION
    from algp_amd.agent import _CRIT
    assert _CRIT['variance_reduction'] == _hip.CRIT_VARIANCE_REDUCTION


def _field_agent(incremental):
    from algp_amd.agent import Agent
    from algp_amd.arguments import get_args
    from test_agent_loops import ManhattanField       # SyntheticField + a stand-in for the planner the loops call
    np.random.seed(7)
    env = ManhattanField(20, 20, num_test=40)
    args = get_args(['--eval_only', '--kernel', 'rbf', '--max_iterations', '10', '--fraction_pretrain', '0.25',
                     '--criterion', 'variance_reduction'])
    args.incremental = incremental
    return Agent(env, args)


def _brute_force_picks(ag, k):
    from test_variance_reduction import vr_reference
    static, mobile = ag._masks()
    n = ag.env.num_samples
    A = np.where(static | mobile)[0]
    noise = ag._fused_var(static[A], mobile[A])
    picks, U = vr_reference(np.asarray(ag.cov_matrix, np.float64), A, noise, np.arange(n), ~static, ag.static_std ** 2,
                            ag.mobile_std ** 2, k)
    for u in U:                                      # the comparison below means something only without near-ties
        top = np.sort(u[np.isfinite(u)])[-2:]
        assert (top[1] - top[0]) / top[1] > 1e-7
    return picks


@pytest.mark.gpu
def test_agent_plans_with_variance_reduction(capsys):
    ag = _field_agent(True)
    out = ag.run_greedy_ipp(num_runs=2, criterion='variance_reduction', disp=False)
    assert len(out['error']) == 1 and np.isfinite(out['error'][0]) and len(ag.static_locations) == 8
    static, mobile = ag._masks()
    assert mobile.any() and static.any() and (mobile & ~static).any()
    want = _brute_force_picks(ag, 3)
    assert ag.greedy(3) == want                      # the factor kept across steps, every site a candidate
    ag.incremental = False
    assert ag.greedy(3) == want                      # from scratch, the static sites left out of the candidates
    ag.cov_matrix = np.array(ag.cov_matrix)
    assert ag.greedy(3) == want                      # an assigned covariance matrix
    with pytest.raises(NotImplementedError):
        ag.best_path([[1, 2, 3], [4, 5, 6]], [7])
    with pytest.raises(NotImplementedError):
        ag.run_ipp(num_runs=1, criterion='variance_reduction')
