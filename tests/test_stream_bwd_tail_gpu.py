"""The streaming backward's first and last steps: short horizons (fewer steps than one batch / than the ring), batches with a trailing
partial workgroup, the terrain snap of the initial pose on and off, and the fused loss value formed by the backward launch or not.
The streaming form prepares the snap's footprint cell and finishes the loss value on its fetching waves; the references are the
record read by the computing wave itself (MF_CP_BWD_MODE=2, a fresh child process: the library reads its switches once) and the
two-kernel loss route."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from tests import helpers as hp
from tests.test_rollout_gpu import make_dphysics

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(integ, B, T, snap):
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    z = syn.bump_terrain(syn.bump_params(61), 3.2, 0.05) * 0.8
    mu = syn.wave_friction(3.2, 0.05, 0.5, 1.0, 1.3, 0.9)
    ctrl = syn.varying_controls(B, T, seed=9)
    dp = make_dphysics(pts, masks, integ, 0.05, 3.2, snap_to_terrain=snap)
    zd, md, cd = z.to(DEV).requires_grad_(True), mu.to(DEV).requires_grad_(True), ctrl.to(DEV).requires_grad_(True)
    st, fo = dp(zd.unsqueeze(0), cd, friction=md.unsqueeze(0))
    hp.probe_loss(list(st) + list(fo), torch.float32).backward()
    return dict(gz=zd.grad.cpu(), gmu=md.grad.cpu(), gc=cd.grad.cpu())


_CHILD = r'''
import sys, torch
sys.path.insert(0, %r)
from tests.test_stream_bwd_tail_gpu import _case
torch.save(_case(%d, %d, %d, %r), %r)
'''


@pytest.mark.parametrize('snap', [True, False])
@pytest.mark.parametrize('integ,B,T', [(1, 5, 1), (1, 5, 2), (1, 37, 3), (1, 37, 4), (1, 1, 7), (1, 37, 14), (1, 1500, 5), (0, 5, 2), (0, 37, 4)])
def test_stream_backward_short_horizons_equal_the_one_wave_backward(integ, B, T, snap):
    """Gradients to the terrain, the friction and the controls of the streaming backward == those of the record read by one wave
    (float32 sums in another order).  T = 1 .. 4: no step, or fewer steps than one batch; T = 14: more than the twelve-slot ring;
    B = 5, 37: a trailing workgroup with 4 / 16 live lanes; 1500 rollouts: two workgroups per CU (six-slot ring)."""
    stream = _case(integ, B, T, snap)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, 'one_wave.pt')
        r = subprocess.run([sys.executable, '-c', _CHILD % (REPO, integ, B, T, snap, path)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, MF_CP_BWD_MODE='2', MF_CP_RECORD_DYNAMICS='1'))
        assert r.returncode == 0, r.stderr[-2000:]
        one_wave = torch.load(path)
    for k in ('gz', 'gmu', 'gc'):
        assert torch.isfinite(stream[k]).all(), k
        assert hp.rel_err(stream[k], one_wave[k]) <= 2e-5, (k, hp.rel_err(stream[k], one_wave[k]))


def _fit(B, T, in_kernel, value_in_backward, snap, gt_every):
    from monoforce_amd import synthetic as syn
    from monoforce_amd.train import TerrainFitProblem
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 3.2, snap_to_terrain=snap)
    z_true = (syn.bump_terrain(syn.bump_params(3), 3.2, 0.1) * 0.3).to(DEV)
    mu = syn.wave_friction(3.2, 0.1).to(DEV)
    ctrl = syn.const_controls(B, T, seed=2).to(DEV)
    prob = TerrainFitProblem(dp, z_true, mu, ctrl, gt_every=gt_every, loss_in_kernel=in_kernel)
    prob.loss_value_in_backward = value_in_backward
    z = (z_true * 0.5).clone().requires_grad_(True)
    m = mu.clone().requires_grad_(True)
    vals = [float(prob.step(z, m)) for _ in range(3)]      # launch after launch: the ticket comes back to zero
    return vals, z.grad.cpu(), m.grad.cpu(), prob


@pytest.mark.parametrize('snap', [True, False])
@pytest.mark.parametrize('value_in_backward', [True, False])
@pytest.mark.parametrize('B,T,gt_every', [(5, 2, 1), (37, 3, 1), (1, 4, 2), (37, 16, 5), (1500, 9, 3)])
def test_fused_loss_tail_equals_the_two_kernel_route(B, T, gt_every, value_in_backward, snap):
    """The loss formed inside the rollout launches -- its value finished by the backward's fetching waves (value_in_backward) or not --
    equals the two-kernel route, launch after launch, with the snap on and off, at horizons shorter than a batch and the ring."""
    vals_k, gz_k, gm_k, prob = _fit(B, T, True, value_in_backward, snap, gt_every)
    vals_r, gz_r, gm_r, _ = _fit(B, T, False, value_in_backward, snap, gt_every)
    assert prob.loss_in_kernel and prob.spec.fusable
    assert len(set(vals_k)) == 1, vals_k
    assert abs(vals_k[0] - vals_r[0]) <= 2e-6 * abs(vals_r[0]), (vals_k[0], vals_r[0])
    assert hp.rel_err(gz_k, gz_r) <= 2e-5 and hp.rel_err(gm_k, gm_r) <= 2e-5
