"""The answer ring of the streaming backward (csrc/stream_ring.h; the kernel side was measured slower and is kept as
tools/experiments/stream_answer_ring.patch), without a GPU: the protocol model (tools/stream_ring_model.cpp) walks
every interleaving of the three waves over the twelve-slot read-counted ring with a 24-entry answer ring for 1 .. 60 steps and must
report no finding; and the code-object metadata says that the two instantiations the ring is meant for fit the CU (no scratch, at most
160 KB of LDS) while every other streaming instantiation has the LDS size it had before the answer ring was tried."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests.conftest import REPO

sys.path.insert(0, os.path.join(REPO, 'tools'))

STREAM = 'rollout_bwd_cp_kernel<{S}, {integ}, {xs}, {gc}, 3, {slots}, {batch}, false, false, false>'
# the two kernels the answer ring is meant for: float32, default integrator, positions-only upstream, twelve slots, batches of three
CHANGED = [STREAM.format(S='float', integ=1, xs='true', gc=gc, slots=12, batch=3) for gc in ('true', 'false')]
# every other streaming instantiation and the LDS it used before the answer ring existed (bytes)
UNCHANGED_LDS = {
    ('rollout_bwd_cp_stream_fast.o', STREAM.format(S='float', integ=1, xs='false', gc='true', slots=12, batch=3)): 148688,
    ('rollout_bwd_cp_stream_fast.o', STREAM.format(S='float', integ=1, xs='false', gc='false', slots=12, batch=3)): 148688,
    ('rollout_bwd_cp_stream_fast.o', STREAM.format(S='float', integ=1, xs='true', gc='true', slots=6, batch=2)): 62672,
    ('rollout_bwd_cp_stream_fast.o', STREAM.format(S='float', integ=1, xs='true', gc='false', slots=6, batch=2)): 62672,
    ('rollout_bwd_cp_stream_fast.o', STREAM.format(S='float', integ=1, xs='false', gc='true', slots=6, batch=3)): 74960,
    ('rollout_bwd_cp_stream_fast.o', STREAM.format(S='float', integ=1, xs='false', gc='false', slots=6, batch=3)): 74960,
    ('rollout_bwd_dyn_cp_stream_fast.o', STREAM.format(S='float', integ=0, xs='true', gc='true', slots=6, batch=3)): 99536,
    ('rollout_bwd_dyn_cp_stream_fast.o', STREAM.format(S='float', integ=0, xs='true', gc='false', slots=6, batch=3)): 99536,
    ('rollout_bwd_dyn_cp_stream_fast.o', STREAM.format(S='float', integ=0, xs='false', gc='true', slots=6, batch=3)): 111824,
    ('rollout_bwd_dyn_cp_stream_fast.o', STREAM.format(S='float', integ=0, xs='false', gc='false', slots=6, batch=3)): 111824,
    ('rollout_bwd_cp_f64.o', STREAM.format(S='double', integ=1, xs='true', gc='true', slots=6, batch=2)): 125344,
    ('rollout_bwd_cp_f64.o', STREAM.format(S='double', integ=1, xs='true', gc='false', slots=6, batch=2)): 125344,
    ('rollout_bwd_cp_f64.o', STREAM.format(S='double', integ=1, xs='false', gc='true', slots=6, batch=3)): 149920,
    ('rollout_bwd_cp_f64.o', STREAM.format(S='double', integ=1, xs='false', gc='false', slots=6, batch=3)): 149920,
}


@pytest.fixture(scope='module')
def model_output(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('model') / 'stream_ring_model')
    r = subprocess.run([cxx, '-std=c++17', '-O2', '-Wall', '-I', os.path.join(REPO, 'monoforce_amd', 'csrc'),
                        os.path.join(REPO, 'tools', 'stream_ring_model.cpp'), '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def test_model_reports_no_finding(model_output):
    assert 'FINDING' not in model_output and 'findings' not in model_output, model_output[-2000:]


def test_answer_ring_configuration_is_explored_to_sixty_steps(model_output):
    """The new configuration's own line: horizons 1 .. 60 (beyond two answer rings).  The twelve-slot read-counted ring alone reaches
    over 300 000 states in 30 horizons; with the answers' states on top and twice the horizons, anything below a million would mean
    the answer ring's operations are not in the programs."""
    m = re.search(r'answer ring of 24, n_steps 1 \.\. 60: explored (\d+) states', model_output)
    assert m, model_output[-2000:]
    assert int(m.group(1)) > 1000000, model_output
    lines = re.findall(r'^(.+): explored \d+ states$', model_output, re.M)
    assert len(lines) == 6, model_output      # the five rings there were, and this one


@pytest.fixture(scope='module')
def metadata():
    import __graft_entry__ as g
    g.build()
    import kernel_metadata
    return kernel_metadata.kernels()


def test_answer_ring_kernels_fit_the_cu(metadata):
    rows = {n.replace('mf::', ''): m for o, n, m in metadata if o == 'rollout_bwd_cp_stream_fast.o'}
    for name in CHANGED:
        assert name in rows, (name, sorted(rows))
        m = rows[name]
        assert m['scratch'] == 0, (name, m)
        # at least twelve slots x ten planes of one KiB; with 24 answer entries + the loss shares, the snap cell and the flags: 148.7 KB
        assert 120 * 1024 < m['lds'] <= 160 * 1024, (name, m)


def test_other_streaming_kernels_keep_their_lds(metadata):
    rows = {(o, n.replace('mf::', '')): m for o, n, m in metadata}
    for key, lds in UNCHANGED_LDS.items():
        assert key in rows, (key, sorted(k for k in rows if 'stream' in k[0]))
        assert rows[key]['lds'] == lds, (key, rows[key])
    # ... and no float32 streaming kernel uses scratch
    n_stream = 0
    for (o, n), m in rows.items():
        if o in ('rollout_bwd_cp_stream_fast.o', 'rollout_bwd_dyn_cp_stream_fast.o') and 'rollout_bwd_cp_kernel<float' in n:
            n_stream += 1
            assert m['scratch'] == 0, (o, n, m)
    assert n_stream == 12
