"""The triangular form's deal of a scheduled GEMM launch (algp_amd/csrc/gemm_sched.h, kcut = 1: whole tiles of 1 .. tiles_n k blocks,
longest first, even rounds dealt up the workgroups and odd rounds down) on the CPU: tests/sched_deal_main.cpp walks the
triangular shapes of tests/test_sched_units.py -- tiles_m in {1, 3, 127, 128, 129, 401, 512, 782} x tiles_n in {1, 2, 4} x grids of
{8, 512} slots -- plus 401, 475 and 782 tile rows x 4 on 512 slots, and checks against the plain round-robin deal of the same
sequence (computed there from d = wg + i * G) that the longest workgroup is no longer, that every tile is dealt exactly once,
that the longest workgroup holds exactly the mean rounded up at 782 x 4 (16 blocks) and 401 x 4 (8), and that the totals lie
within 2 blocks at 475 x 4.  Compiled with the host compiler; a second build runs under the address and undefined-behaviour
sanitizers as its own executable.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'tests', 'sched_deal_main.cpp')


def _build_and_run(tmp_path, name, flags):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', *flags, SRC, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert 'checked 51 shapes' in r.stdout and 'FAIL' not in r.stdout, r.stdout[-3000:]


def test_the_deal_is_no_longer_than_round_robin_and_even_at_the_named_shapes(tmp_path):
    _build_and_run(tmp_path, 'sched_deal', [])


def test_the_same_walk_under_the_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'sched_deal_san', ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
