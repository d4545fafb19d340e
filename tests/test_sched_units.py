"""The work list of a scheduled GEMM launch (algp_amd/csrc/gemm_sched.h: one closed-form function for the launcher, the kernel and
this test) on the CPU: tests/sched_units_main.cpp walks tiles_m in {1, 3, 127, 128, 129, 401, 512, 782} x tiles_n in {1, 2, 4}
x k blocks in {1, 4, 5, 76} x grids of {8, 512} slots, update and triangular form, and checks that every (tile, k block) is
covered exactly once, a workgroup holds at most one slice, no slice is empty, a tile's slices are contiguous and ascending
in k, the leftover tiles are the last of the row-major list, the XCD groups hold contiguous shares, and the per-workgroup
totals are balanced: within one slice plus one 128-block (update form), within one longest tile (triangular form -- the
round-robin deal of a never-increasing sequence; a tighter bound is not attainable with whole tiles, e.g. one row panel on
four workgroups is 4, 3, 2, 1 blocks).  Compiled with the host compiler; a second build runs under the address and
undefined-behaviour sanitizers as its own executable.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'tests', 'sched_units_main.cpp')


def _build_and_run(tmp_path, name, flags):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', *flags, SRC, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert 'checked 240 shapes' in r.stdout and 'FAIL' not in r.stdout, r.stdout[-3000:]


def test_every_unit_of_every_shape_is_covered_once_and_balanced(tmp_path):
    _build_and_run(tmp_path, 'sched_units', [])


def test_the_same_walk_under_the_sanitizers(tmp_path):
    _build_and_run(tmp_path, 'sched_units_san', ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
