"""The streaming backward's ring protocol, every interleaving: tools/stream_ring_model.cpp models the computing wave and the two fetching
waves over the counters of monoforce_amd/csrc/rollout_bwd_cp_kernel.h with the index arithmetic of csrc/stream_ring.h (the header the
kernel includes) and fails on a deadlock, a slot overwritten before its answer was consumed, an answer consumed twice or never, or
out-of-order publication -- for 1 .. 30 steps and every ring / batch size the kernels are built with."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_model_explores_every_interleaving_without_a_finding(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = str(tmp_path / 'stream_ring_model')
    r = subprocess.run([cxx, '-std=c++17', '-O2', '-Wall', '-I', os.path.join(REPO, 'monoforce_amd', 'csrc'),
                        os.path.join(REPO, 'tools', 'stream_ring_model.cpp'), '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r'explored (\d+) states', r.stdout)
    assert m, r.stdout[-2000:]
    # five rings x 30 horizons; the twelve-slot hand-off ring at 30 steps alone has thousands of reachable states
    assert int(m.group(1)) > 100000, r.stdout
    assert 'FINDING' not in r.stdout
