"""bench.py's plain run and --dump-outputs: the plain line carries the headline and nothing that needs a leg of its own,
--steps sets the number of timed steps, and the last timed step's outputs land in DIR/<name>.npy -- the same numbers
from run to run, the picks the line reports, the log-determinant of the train covariance the oracle computes."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN, CAND = 2500, 20000


def _plain(out_dir):
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    env.pop('RANK', None)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--train', str(TRAIN), '--cand', str(CAND), '--dump-outputs', str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path, monkeypatch):
    from oracle import gp_oracle as O
    monkeypatch.setattr(os, 'environ', dict(os.environ))      # bench.py sets HIP defaults when imported: not for the suite
    import bench
    a = _plain(tmp_path / 'a')
    b = _plain(tmp_path / 'b')
    assert a['steps'] == 3 and a['warmup'] == 1 and a['ms_per_step'] > 0
    assert a['value'] == pytest.approx(CAND / (a['ms_per_step'] * 1e-3), rel=1e-9)
    # only the headline's legs ran
    assert a['ms_per_step_unprofiled'] is None and a['ms_per_step_host_inclusive'] is None
    assert a['extra'] == {} and a['cpu_baseline'] is None and 'strong_emulation' not in a
    assert 'serial_kernel_frac' not in a['roofline']
    names = ('picks', 'posterior_mean', 'posterior_var', 'alpha', 'logdet')
    da = {n: np.load(tmp_path / 'a' / (n + '.npy')) for n in names}
    db = {n: np.load(tmp_path / 'b' / (n + '.npy')) for n in names}
    for n in names:
        assert da[n].dtype == np.float64, n
        np.testing.assert_allclose(da[n], db[n], rtol=1e-12, atol=0, err_msg=n)
    assert [int(p) for p in da['picks']] == a['picks_last_step'] == b['picks_last_step']
    assert da['posterior_mean'].shape == da['posterior_var'].shape == (CAND,)
    assert da['alpha'].shape == (TRAIN,) and np.all(np.isfinite(da['alpha']))
    w = bench.build_workload(SimpleNamespace(train=TRAIN, cand=CAND, scaling='strong'), 1)
    N = w['N']
    hyp = O.Hypers(np.log([3.0, 3.0]), 0.0, np.log(1e-2))
    S = O.kernel_matrix(hyp, w['pool'][:N]) + np.diag(w['var']) + hyp.noise * np.eye(N)
    want = np.linalg.slogdet(S)[1]
    assert abs(da['logdet'][0] - want) < 1e-9 * abs(want), (da['logdet'][0], want)
