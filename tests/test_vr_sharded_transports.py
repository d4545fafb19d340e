"""The variance-reduction criterion over ranks (algp_comm_set_vr_exchange, tests/test_vr_sharded.py) through the two other
transports: two PROCESSES over the RCCL code path -- device-pointer all-gathers, no host staging -- against the test double
tests/fake_rccl.cpp (as tests/test_rccl_transport.py: real RCCL refuses two ranks on one device), and the Agent's greedy loop
over two gloo ranks (as tests/test_mi_sharded_agent.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RCCL_WORKER = r'''
import os, sys, time
import numpy as np
sys.path.insert(0, %(repo)r)
sys.path.insert(0, os.path.join(%(repo)r, 'tests'))
import test_vr_sharded as t
from algp_amd import _hip
assert 'torch' not in sys.modules
rank, world, tmp = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
V = t.V

def exchange(tag, payload=None):
    """rank 0 publishes bytes under `tag`, the others read them"""
    path = os.path.join(tmp, tag)
    if rank == 0:
        with open(path + '.tmp', 'wb') as f:
            f.write(payload)
        os.rename(path + '.tmp', path)
        return payload
    t0 = time.time()
    while not os.path.exists(path):
        assert time.time() - t0 < 120, 'rank 0 never published ' + tag
        time.sleep(0.01)
    return open(path, 'rb').read()

p = V.problem(V.SHAPES[1], t.RBF)
picks, U = V.reference(p, 'own')
mine = t.shards(p.n, world, 'strided')[rank]
c = V.context(p, np.float64, 'coords', cand=mine, alive=p.alive[mine])
uid = exchange('uid', _hip.Context.comm_unique_id() if rank == 0 else None)
c.comm_init(world, rank, uid)
maps = open('/proc/self/maps').read()
assert os.path.basename(os.environ['ALGP_RCCL_PATH']) in maps and 'librccl' not in maps      # the double, and only it
c.comm_set_vr_exchange(128)
u0 = c.scores(t.CRIT, t.SS, t.SM)                        # the build: two rounds of device-resident rows
V.compare(u0, U[0][mine], 1e-9, 'rank %%d scores' %% rank)
pk, ut = c.greedy_sharded(t.CRIT, t.SS, t.SM, 3, want_utilities=True)
t._check_free_picks([int(v) for v in pk], [float(v) for v in ut], picks, U, 1e-9, 'rank %%d' %% rank)
c.comm_destroy()
c.close()
print('VR_RCCL_OK rank %%d picks %%s' %% (rank, [int(v) for v in pk]))
'''


@pytest.fixture(scope='module')
def fake_rccl(tmp_path_factory):
    out = tmp_path_factory.mktemp('fake_rccl_vr') / 'libalgp_test_gather.so'
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-shared', '-fPIC', '-O2', os.path.join(REPO, 'tests', 'fake_rccl.cpp'), '-o', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_two_processes_over_the_rccl_transport(tmp_path, fake_rccl):
    """(300, 130, 2), fp64, k = 3: the collective scores and the picks and utilities of greedy_sharded against the brute force."""
    script = tmp_path / 'worker.py'
    script.write_text(RCCL_WORKER % {'repo': REPO})
    env = dict(os.environ, ALGP_RCCL_PATH=fake_rccl)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), '2', str(tmp_path)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, env=env) for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600))
    finally:
        for p in procs:                                        # exactly the processes started here
            if p.poll() is None:
                p.kill()
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, 'rank %d:\n%s\n%s' % (r, so[-2000:], se[-4000:])
        assert 'VR_RCCL_OK rank %d' % r in so
    assert outs[0][0].splitlines()[-1].split('picks')[1] == outs[1][0].splitlines()[-1].split('picks')[1]


AGENT_WORKER = r'''
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
    np.random.seed(7)                                # the field and agent of tests/test_variance_reduction_host.py
    env = ManhattanField(20, 20, num_test=40)
    args = get_args(['--eval_only', '--kernel', 'rbf', '--max_iterations', '10', '--fraction_pretrain', '0.25',
                     '--criterion', 'variance_reduction'])
    args.incremental = True
    agent = Agent(env, args, comm=comm)
    out = agent.run_greedy_ipp(num_runs=2, criterion='variance_reduction', strategy='Shortest', disp=False)
    return agent, out

one, out1 = run(None)
two, out2 = run(ShardLink(rank, world, all_gather=gather, vr_rows_per_round=128))
assert np.array_equal(one.static_locations, two.static_locations), (one.static_locations, two.static_locations)
assert np.array_equal(one.path, two.path), (one.path, two.path)
assert np.allclose(out1['error'], out2['error'], rtol=0, atol=1e-9), (out1['error'], out2['error'])
assert np.max(np.abs(out1['mean'] - out2['mean'])) < 1e-8
for refused in (lambda: two.set_target_weights(np.ones(two.env.num_samples)), two.target_variance):
    try:
        refused()
        raise SystemExit('a sharded agent answered what it must refuse')
    except NotImplementedError as e:
        assert 'not sharded' in str(e)
dist.barrier()
if rank == 0:
    print('SHARDED_VR_AGENT_OK')
dist.destroy_process_group()
'''


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def test_agent_greedy_loop_under_variance_reduction_over_two_ranks(tmp_path):
    """run_greedy_ipp(criterion='variance_reduction', strategy='Shortest') at world 2 equals the one-GPU agent: the same static
    locations, path and errors."""
    script = tmp_path / 'worker.py'
    script.write_text(AGENT_WORKER % {'repo': REPO})
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                          '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), str(script)],
                         capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-6000:]
    assert 'SHARDED_VR_AGENT_OK' in out.stdout
