"""The Agent's mission loop under the MUTUAL-INFORMATION criterion with its candidates and its pool-wide inverses sharded
over two ranks (`Agent(env, args, comm=ShardLink(...))`, algp_comm_set_mi_groups attached by ShardLink.attach): the same
paths, picks, errors and posterior as the one-GPU agent.  Two real ranks share the one card over a caller-supplied gloo
all-gather (algp_comm_init_host).  The loop covers what a direct greedy_sharded call does not: the incremental candidate
solve with its alive mask, the hyper-parameter refit after every step (update=True: the pool is reloaded and the layout
re-attached), best_path's per-path factor updates on the sharded context between two greedy calls, and the sharded MI
state rebuilt after each of them."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, os.path.join(%(repo)r, 'tests'))
import torch
import torch.distributed as dist
from algp_amd.sharded import ShardLink
from algp_amd.agent import Agent
from algp_amd.arguments import get_args
from test_agent_loops import ManhattanField

dist.init_process_group('gloo')
rank, world = dist.get_rank(), dist.get_world_size()

def gather(send):
    t = torch.frombuffer(bytearray(send), dtype=torch.uint8)
    out = torch.empty(world * len(send), dtype=torch.uint8)
    dist.all_gather_into_tensor(out, t)
    return out.numpy().tobytes()

def run(comm):
    np.random.seed(3)
    args = get_args([])
    args.kernel, args.max_iterations, args.num_samples_per_batch, args.fraction_pretrain = 'rbf', 20, 3, 0.5
    env = ManhattanField(30, 24, num_test=40)
    agent = Agent(env, args, static_std=args.static_std, mobile_std=10 * args.static_std, comm=comm)
    out = agent.run_ipp(num_runs=4, criterion='mutual_information', update=True, strategy='MaxEnt', disp=False)
    return agent, out

one, out1 = run(None)
two, out2 = run(ShardLink(rank, world, all_gather=gather))
assert np.array_equal(one.static_locations, two.static_locations), (one.static_locations, two.static_locations)
assert np.array_equal(one.path, two.path), (one.path, two.path)
assert np.allclose(out1['error'], out2['error'], rtol=0, atol=1e-9), (out1['error'], out2['error'])
assert np.max(np.abs(out1['mean'] - out2['mean'])) < 1e-8
dist.barrier()
if rank == 0:
    print('SHARDED_MI_AGENT_OK')
dist.destroy_process_group()
'''


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def test_agent_mission_loop_under_mi_sharded_over_two_ranks(tmp_path):
    """run_ipp(criterion='mutual_information', update=True) at world 2 equals the one-GPU agent."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'repo': REPO})
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                          '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), str(script)],
                         capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-6000:]
    assert 'SHARDED_MI_AGENT_OK' in out.stdout
