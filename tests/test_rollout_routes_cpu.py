"""The rollout's route policy as the public queries answer it (no GPU: the queries assume an MI355X when no device answers), pinned over a
grid of descriptors that straddles every threshold of the dispatch by one rollout -- and again under each A/B switch the tests and tools
set, in child processes (the library reads a switch once per process).  The fixture, tests/golden/rollout_routes_cpu.npz, holds the
descriptors and the answers; regenerate it only for an intended change of the policy:  python -m tests.test_rollout_routes_cpu --record"""
import ctypes as C
import io
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, 'tests', 'golden', 'rollout_routes_cpu.npz')

QUERIES = ('mf_rollout_record_bytes', 'mf_rollout_record_bytes_f64', 'mf_rollout_loss_fusable', 'mf_rollout_bwd_window',
           'mf_rollout_fwd_stages_zmu', 'mf_rollout_force_stride', 'mf_rollout_bwd_wants_gcontrols')
FIELDS = ('B', 'T', 'N', 'H', 'W', 'integrator', 'math_mode', 'points_per_lane', 'map_shared', 'has_joints', 'layout', 'force_stride')
SWITCHES = ('MF_CP_BWD_MODE=2', 'MF_CP_RECORD_MAX_WAVES=0', 'MF_CP_RECORD_DYNAMICS=1', 'MF_MW_BWD=0', 'MF_BWD_XS=0', 'MF_BWD_XS_LOSS=0',
            'MF_CP_LOSS_ONE_WAVE=0', 'MF_BWD_WIN=0', 'MF_CP_MAX_WAVES=512', 'MF_CP_BWD_MAX_WAVES=0', 'MF_CP_STREAM_MAX_GRID=128')
BODIES = (1, 4, 5, 8, 9, 32, 33, 64, 65, 128, 129, 175, 223, 256, 257, 512, 513)
SIMDS, CUS = 1024, 256      # the MI355X the queries assume without a device


def _lanes(N):
    """Lanes per rollout the lane maps can give a body of N points: one or four points per lane, the multi-wave and the 2/4/8-per-lane maps."""
    g1 = 4
    while g1 < N:
        g1 <<= 1
    return sorted({g1, max(g1 // 4, 1), 64, 128, 256, 512} if N > 64 else {g1, max(g1 // 4, 1)})


def _batches(N):
    """Batch sizes at +-1 of every wave-count bound at the lanes N implies, plus the component-parallel ones (4 rollouts a wave)."""
    out = set()
    for G in _lanes(N):
        for waves in (SIMDS // 2, 3 * CUS // 4, SIMDS, 2 * SIMDS):      # half a wave per SIMD, 3/4 of the CUs' slots, one and two per SIMD
            b = waves * 64 // G
            out |= {b - 1, b, b + 1}
    if N <= 5:
        out |= {1, 2, 3, 256, 257, 1 << 20, (1 << 22) + 3}
        for b in (1024, 2048, 4096, 8192, 16384):
            out |= {b - 1, b, b + 1}
    return sorted(b for b in out if b > 0)


def grid():
    """Rows of FIELDS: every body size x its batch sizes x the descriptor fields, then the 32-bit offset limits."""
    rows = []
    combos = list(itertools.product((0, 1), (0, 1), (0, 1, 4, 16), (0, 1), (0, 1), (0, 1), (64, 100)))
    for N in BODIES:
        for B in _batches(N):
            for integ, math, ppl, shared, joints, layout, side in combos:
                rows.append((B, 500, N, side, side, integ, math, ppl, shared, joints, layout, 0))
    for B, N in ((64, 4), (1024, 4), (4096, 4), (16384, 4), (1024, 32), (20000, 4)):
        for integ, shared, ppl in itertools.product((0, 1), (0, 1), (0, 16)):
            for H in (16383, 16384, 16385):      # H * W * 8 >= 2^31 from H = W = 16384
                rows.append((B, 500, N, H, H, integ, 1, ppl, shared, 0, 1, 0))
            for T in ((1 << 32) // (B * 12 * 4), (1 << 32) // (B * 12 * 4) + 1, (1 << 32) // (B * 12 * 8) + 1, 1 << 18):
                rows.append((B, T, N, 64, 64, integ, 1, ppl, shared, 0, 1, 0))
                rows.append((B, T, N, 64, 64, integ, 1, ppl, shared, 0, 1, 8))      # a wider force row
    return np.array(rows, dtype=np.int64)


def answers(rows):
    from monoforce_amd import _lib
    L = _lib.lib()
    for q in ('mf_rollout_record_bytes', 'mf_rollout_record_bytes_f64'):
        getattr(L, q).restype = C.c_longlong
    fns = [getattr(L, q) for q in QUERIES]
    out = np.zeros((len(rows), len(QUERIES)), dtype=np.int64)
    for i, r in enumerate(rows.tolist()):
        d = _lib.MfRolloutDesc(**dict(zip(FIELDS, r)))
        d.n_tracks = 4 if d.has_joints else 2
        p = C.byref(d)
        out[i] = [f(p) for f in fns]
    return out


def _child(switch):
    """The answers under one switch setting, from a fresh process."""
    k, v = switch.split('=')
    env = dict(os.environ, **{k: v})
    code = ('import io, sys, numpy as np; from tests.test_rollout_routes_cpu import grid, answers; b = io.BytesIO(); '
            'np.save(b, answers(grid())); sys.stdout.buffer.write(b.getvalue())')
    r = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, stdout=subprocess.PIPE, check=True)
    return np.load(io.BytesIO(r.stdout))


def _record():
    rows = grid()
    base = answers(rows)
    blob = {'fields': rows, 'default': base}
    for s in SWITCHES:      # a switch's table as the rows where it differs from the default one
        got = _child(s)
        idx = np.nonzero((got != base).any(axis=1))[0]
        blob['idx:' + s], blob['ans:' + s] = idx.astype(np.int32), got[idx]
    np.savez_compressed(FIXTURE, **{k: np.ascontiguousarray(v.T) for k, v in blob.items()})      # column-major: compresses ~20x better
    print(FIXTURE, os.path.getsize(FIXTURE), 'bytes,', len(rows), 'descriptors')


@pytest.fixture(scope='module')
def recorded():
    import __graft_entry__ as g
    g.build()
    return {k: v.T for k, v in np.load(FIXTURE).items()}


def test_grid_is_the_recorded_one(recorded):
    assert np.array_equal(grid(), recorded['fields'])


def test_routes_match_the_recorded_policy(recorded):
    got = answers(recorded['fields'])
    for j, q in enumerate(QUERIES):
        bad = np.nonzero(got[:, j] != recorded['default'][:, j])[0]
        assert bad.size == 0, (q, dict(zip(FIELDS, recorded['fields'][bad[0]].tolist())), got[bad[0], j], recorded['default'][bad[0], j])


@pytest.mark.parametrize('switch', SWITCHES)
def test_routes_match_the_recorded_policy_under_switch(recorded, switch):
    want = recorded['default'].copy()
    want[recorded['idx:' + switch]] = recorded['ans:' + switch]
    assert recorded['idx:' + switch].size > 0, 'the grid does not reach what this switch steers'
    got = _child(switch)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (switch, dict(zip(FIELDS, recorded['fields'][bad[0]].tolist())), got[bad[0]].tolist(), want[bad[0]].tolist())


if __name__ == '__main__' and sys.argv[1:] == ['--record']:
    _record()
