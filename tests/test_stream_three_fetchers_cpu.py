"""The ring protocol with THREE fetching waves (the twelve-slot hand-off kernels launched with 256 threads): tools/stream_ring_model.cpp
walks every interleaving of the computing wave and three fetching waves for 1 .. 30 steps -- a slot changes hands there, and the answer in
it is read by whichever wave writes the slot next -- and must find nothing; with the protocol mutated (a fetching wave granted room one
slot early) it must report findings: the model can see a broken protocol."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('ring_model') / 'stream_ring_model')
    r = subprocess.run([cxx, '-std=c++17', '-O2', '-Wall', '-I', os.path.join(REPO, 'monoforce_amd', 'csrc'),
                        os.path.join(REPO, 'tools', 'stream_ring_model.cpp'), '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_three_fetching_waves_every_interleaving_without_a_finding(model):
    r = subprocess.run([model], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'FINDING' not in r.stdout
    m = re.search(r'hand-off, three fetching waves, n_steps 1 \.\. 30: explored (\d+) states \(four programs\)', r.stdout)
    assert m, r.stdout[-2000:]
    two = re.search(r'12 slots, batches of 3, hand-off, n_steps 1 \.\. 30: explored (\d+) states', r.stdout)
    assert two and int(m.group(1)) > int(two.group(1)) > 100000, r.stdout      # a fourth program: more interleavings than with three


def test_room_released_one_slot_early_is_found(model):
    r = subprocess.run([model, 'early-room'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.stdout[-2000:], r.stderr[-2000:])
    assert re.search(r'FINDING n_steps \d+ slots 12 batch 3 fetchers 3 hand-off', r.stdout), r.stdout[-2000:]
    assert re.search(r'FINDING n_steps \d+ slots 12 batch 3 fetchers 2 hand-off', r.stdout), r.stdout[-2000:]
