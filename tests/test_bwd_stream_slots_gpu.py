"""The computing wave of the streaming backward takes its cross-lane operands inside the arithmetic instructions (rollout_cp_common.h:
cp_rot_back, cp_colT, cp_cross_pair, cp_cell_terms) and walks the ring by a running byte offset (rollout_bwd_cp_kernel.h: grab).  A wrong
quad_perm selector or a wrong sign shows only where every component of every cross product is non-zero, and a wrong ring offset only where
the horizon reaches the wrap: a rolling and pitching start pose on a bump terrain with a friction map, controls that vary from step to step,
horizons with no step (T = 1), less than a batch (2, 3), and the twelve-slot ring's wrap on either parity of the step count (12, 13, 25),
one rollout and five (a trailing workgroup of one), bodies of one, three and four points, both upstreams, with and without control gradients.

Every gradient the launch produces -- terrain, friction, controls, and the four of the start state, which are the whole adjoint at step 0 --
is held to
  * the one-point-per-lane float32 kernels (sums in another order) at 2e-5 of the tensor's absolute maximum, the bar of
    tests/test_stream_scatter_gpu.py;
  * the float64 oracle at max(2e-4, 3 x the float32 oracle's own distance from it), the bar of tests/state_grad_cases.py;
and a gradient that is exactly zero in the reference is exactly zero here.  One case runs the six-slot ring (a child process: the library
reads MF_CP_STREAM_BIG_RING_MAX_GRID once)."""
import contextlib
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from oracle import dphysics_oracle as orc
from tests import helpers as hp
from tests import state_grad_cases as sg
from tests.golden_state import given_state
from tests.test_rollout_gpu import make_dphysics

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, D_MAX, NMAX = 0.1, 1.6, 5
BATCHES, HORIZONS = (1, 5), (1, 2, 3, 12, 13, 25)
NAMES = ('gz', 'gmu', 'gc', 'gx0', 'gxd0', 'gR0', 'gw0')


@functools.lru_cache(maxsize=None)
def _problem(T):
    """NMAX distinct rollouts in float64 on one shared map pair (rollout b of a smaller batch is rollout b of this one)."""
    from monoforce_amd import synthetic as syn
    z = syn.bump_terrain(syn.bump_params(20), D_MAX, RES, torch.float64) * 0.3
    mu = syn.wave_friction(D_MAX, RES, 0.5, 1.0, 1.1, 0.8, torch.float64)
    ctrl = syn.varying_controls(NMAX, max(T, 2), seed=4, dtype=torch.float64)[:, :T].contiguous()
    return dict(z=z, mu=mu, ctrl=ctrl, state=tuple(given_state(NMAX)))


def _body(N):
    from monoforce_amd import synthetic as syn
    pts4, masks4 = syn.robot_points_4()
    return pts4, masks4, pts4[:N], [m[:N] for m in masks4]


@functools.lru_cache(maxsize=None)
def _module(N, ppl):
    """(N < 4: the first N points of the four-point body WITH that body's inertia, as tests/test_stream_scatter_gpu.py builds them)"""
    pts4, masks4, pts, masks = _body(N)
    dp = make_dphysics(pts4, masks4, 1, RES, D_MAX, points_per_lane=ppl)
    if N < 4:
        iinv = dp._iinv(torch.float32)
        dp.dphys_cfg.robot_points = torch.as_tensor(pts)
        dp.dphys_cfg.driving_parts = [torch.as_tensor(m) for m in masks]
        dp.x_points = dp.dphys_cfg.robot_points.unsqueeze(0).to(dp.device)
        dp._cache = {('iinv', torch.float32): iinv}
    return dp


def _loss(outs, up, B, T, N, dtype):
    return sg.upstream_loss(outs, up, torch.arange(B), NMAX, T, N, dtype)


def _hip(N, ppl, B, T, up, gc, route=None):
    """One forward + backward; the seven gradients on the host (gc: None without control gradients).  route: a piece the backward's kernel
    name must contain."""
    from monoforce_amd import _timing
    p, dp = _problem(T), _module(N, ppl)
    z, mu = (p[k].float().to(DEV).requires_grad_(True) for k in ('z', 'mu'))
    ctrl = p['ctrl'][:B].float().to(DEV).requires_grad_(gc)
    lv = [t[:B].float().to(DEV).contiguous().requires_grad_(True) for t in p['state']]
    st = [lv[0] * 1.0] + lv[1:]      # x0 as a non-leaf: the forward writes the snapped height into it
    _timing.start(capacity=16)
    states, forces = dp(z.unsqueeze(0), ctrl, state=tuple(st), friction=mu.unsqueeze(0))
    _loss(list(states) + list(forces), up, B, T, N, torch.float32).backward()
    name = _timing.launches()['rollout_bwd_kernel']
    _timing.stop()
    if route:
        assert route in name, name
    return [z.grad.cpu(), mu.grad.cpu(), ctrl.grad.cpu() if gc else None] + [t.grad.cpu() for t in lv]


@contextlib.contextmanager
def _inertia_of_the_four_point_body():
    """The oracle computes the inertia from the points it is given; the small bodies keep the four-point body's (see _module)."""
    keep, P4 = orc.point_inertia, torch.as_tensor(_body(4)[0], dtype=torch.float64).unsqueeze(0)
    mass = hp.spec_from(*_body(4)[:2], 1, RES, D_MAX).mass
    orc.point_inertia = lambda m, pts: keep(mass, P4.to(pts.dtype))
    try:
        yield
    finally:
        orc.point_inertia = keep


@functools.lru_cache(maxsize=None)
def _oracle(N, T, up, f32):
    """The seven gradients of the oracle's autograd over NMAX rollouts; terrain and friction per rollout ([NMAX, H, W]: a smaller batch sums
    its first B)."""
    dtype = torch.float32 if f32 else torch.float64
    p = _problem(T)
    pts4, masks4, pts, masks = _body(N)
    spec = hp.spec_from(pts4, masks4, 1, RES, D_MAX)      # (the track width is the four-point body's)
    spec.points, spec.driving_parts = torch.as_tensor(pts, dtype=torch.float32), [torch.as_tensor(m) for m in masks]
    z = p['z'].to(dtype).expand(NMAX, -1, -1).clone().requires_grad_(True)
    mu = p['mu'].to(dtype).expand(NMAX, -1, -1).clone().requires_grad_(True)
    ctrl = p['ctrl'].to(dtype).clone().requires_grad_(True)
    lv = [t.clone().to(dtype).requires_grad_(True) for t in p['state']]
    with _inertia_of_the_four_point_body():
        so, fo = orc.rollout(spec, z, ctrl, state=tuple([lv[0] * 1.0] + lv[1:]), friction=mu)
    _loss(list(so) + list(fo), up, NMAX, T, N, dtype).backward()
    return [(torch.zeros_like(t) if t.grad is None else t.grad).double() for t in [z, mu, ctrl] + lv]


def _oracle_for(N, B, T, up, f32):
    g = _oracle(N, T, up, f32)
    return [g[0][:B].sum(0), g[1][:B].sum(0)] + [t[:B] for t in g[2:]]


def _held(tag, got, one_lane, r64, r32):
    for name, a, b, c64, c32 in zip(NAMES, got, one_lane, r64, r32):
        if a is None:
            assert b is None, (tag, name)
            continue
        assert torch.isfinite(a).all(), (tag, name)
        for what, ref, bar in (('one point per lane', b, 2e-5), ('float64 oracle', c64, max(2e-4, 3.0 * hp.rel_err(c32, c64)))):
            if float(ref.abs().max()) == 0.0:
                assert float(a.abs().max()) == 0.0, (tag, name, what, 'exact zero expected', float(a.abs().max()))
            else:
                err = hp.rel_err(a, ref)
                print(tag, name, what, '%.2e' % err, 'bar %.2e' % bar)
                assert err <= bar, (tag, name, what, err, bar)


def _route(up, gc, slots):
    xs = up == 'xs'
    batch = 2 if (slots == 6 and xs) else 3      # <float, 1, XS_ONLY, GCTRL, kCpStream, SLOTS, BATCH, ...>
    return '%s, %s, 3, %d, %d,' % ('true' if xs else 'false', 'true' if gc else 'false', slots, batch)


@pytest.mark.parametrize('gc', [True, False], ids=['gctrl', 'no_gctrl'])
@pytest.mark.parametrize('up', ['all', 'xs'])
@pytest.mark.parametrize('N', [1, 3, 4])
def test_streaming_backward_equals_one_point_per_lane_and_the_oracle(N, up, gc):
    """The twelve-slot kernels, every horizon and batch of the module's docstring."""
    for T in HORIZONS:
        for B in BATCHES:
            got = _hip(N, 16, B, T, up, gc, route=_route(up, gc, 12))
            ref = _hip(N, 1, B, T, up, gc)
            _held((N, up, gc, B, T), got, ref, _oracle_for(N, B, T, up, False), _oracle_for(N, B, T, up, True))


def _six_slot_runs():
    return [(N, up, gc, B, T) for N, up, gc in ((4, 'xs', False), (3, 'all', True)) for B in BATCHES for T in HORIZONS]


def _child(path):
    """(in a process started with MF_CP_STREAM_BIG_RING_MAX_GRID=0: no launch is small enough for the twelve-slot ring)"""
    torch.save({run: _hip(run[0], 16, run[3], run[4], run[1], run[2], route=_route(run[1], run[2], 6)) for run in _six_slot_runs()}, path)


_CHILD = r'''
import sys
sys.path.insert(0, %r)
from tests.test_bwd_stream_slots_gpu import _child
_child(%r)
'''


def test_six_slot_ring():
    """The same comparison through the six-slot kernels (positions only: batches of two; all outputs with control gradients: of three),
    whose computing wave keeps the cell accumulators itself."""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, 'six.pt')
        r = subprocess.run([sys.executable, '-c', _CHILD % (REPO, path)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, MF_CP_STREAM_BIG_RING_MAX_GRID='0'))
        assert r.returncode == 0, r.stderr[-2000:]
        six = torch.load(path)
    for run in _six_slot_runs():
        N, up, gc, B, T = run
        _held(run, six[run], _hip(N, 1, B, T, up, gc), _oracle_for(N, B, T, up, False), _oracle_for(N, B, T, up, True))
