"""The twelve-slot streaming backward hands each step's two cell-gradient products back to the fetching waves through the ring slot the
step was read from; the fetching waves keep the per-lane cell accumulators and issue the atomics (rollout_bwd_cp_kernel.h, HANDOFF).
What can go wrong there: the first ring's worth of steps (no predecessor in the slot), the answers still in the ring after the last
write (the final drain, per wave, in ordinal order), runs on one cell that never end or end every step, absent contact points, and
state left behind from launch to launch.  References: the one-point-per-lane kernels (float32 sums in another order), the float64
oracle, and the unfused loss route."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from oracle import dphysics_oracle as orc
from tests import helpers as hp
from tests.test_rollout_gpu import make_dphysics

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# T = 1 .. 7: no step, fewer than a batch, one and two batches; 11 .. 14 and 23 .. 26: around one and two rings of twelve slots, with
# every remainder of the batches of three; 37: three rings and a trailing step
HORIZONS = list(range(1, 8)) + [11, 12, 13, 14, 23, 24, 25, 26, 37]


def _run(dp, z, mu, ctrl, shared, loss_on, want_route=None):
    """One forward + backward; returns (gz, gmu, gc) on the host.  want_route: a piece the backward's kernel name must contain."""
    from monoforce_amd import synthetic as syn, _timing
    zd = z.to(DEV).requires_grad_(True)
    md = None if mu is None else mu.to(DEV).requires_grad_(True)
    cd = ctrl.to(DEV).requires_grad_(True)
    if want_route:
        _timing.start(capacity=16)
    st, fo = dp(zd.unsqueeze(0) if shared else zd, cd, friction=None if md is None else (md.unsqueeze(0) if shared else md))
    if loss_on == 'all':
        hp.probe_loss(list(st) + list(fo), torch.float32).backward()
    else:
        (st[0] * syn.probe_weights(st[0].shape, phase=0.4).to(DEV)).sum().backward()
    if want_route:
        name = _timing.launches()['rollout_bwd_kernel']
        _timing.stop()
        assert want_route in name, name
    return zd.grad.cpu(), None if md is None else md.grad.cpu(), cd.grad.cpu()


def _same(got, ref, tag):
    for name, a_, b_ in zip(('gz', 'gmu', 'gc'), got, ref):
        if b_ is None:
            assert a_ is None
            continue
        assert torch.isfinite(a_).all(), (tag, name)
        if float(b_.abs().max()) == 0.0:
            assert float(a_.abs().max()) == 0.0, (tag, name)
        else:
            assert hp.rel_err(a_, b_) <= 2e-5, (tag, name, hp.rel_err(a_, b_))


@pytest.mark.parametrize('shared', [True, False])
@pytest.mark.parametrize('loss_on', ['all', 'xs'])
@pytest.mark.parametrize('B', [1, 4, 5])
def test_handoff_every_horizon_and_ragged_batch(B, loss_on, shared):
    """Horizons around the ring size and every batch remainder (the steps without a predecessor in their slot, the final drain), a partial
    wave / a full one / a trailing workgroup of one rollout, both upstreams, shared maps (gradient copies) and a map pair per rollout:
    the twelve-slot streaming route == the one-point-per-lane kernels at 2e-5; a gradient that is exactly zero there is exactly zero here."""
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    if shared:
        z = syn.bump_terrain(syn.bump_params(20), 1.6, 0.1) * 0.3
        mu = syn.wave_friction(1.6, 0.1, 0.5, 1.0, 1.1, 0.8)
    else:
        z = torch.stack([syn.bump_terrain(syn.bump_params(20 + k), 1.6, 0.1) * 0.3 for k in range(B)])
        mu = torch.stack([syn.wave_friction(1.6, 0.1, 0.5, 1.0, 1.1 + 0.2 * k, 0.8) for k in range(B)])
    dps = {ppl: make_dphysics(pts, masks, 1, 0.1, 1.6, points_per_lane=ppl) for ppl in (16, 1)}
    route = ('true' if loss_on == 'xs' else 'false') + ', true, 3, 12, 3,'      # <float, 1, XS_ONLY, GCTRL, kCpStream, 12, 3, ...>
    for T in HORIZONS:
        ctrl = syn.varying_controls(B, max(T, 2), seed=3)[:, :T]
        got = _run(dps[16], z, mu, ctrl, shared, loss_on, want_route=route)
        ref = _run(dps[1], z, mu, ctrl, shared, loss_on)
        _same(got, ref, T)


@pytest.mark.parametrize('snap', [True, False])
@pytest.mark.parametrize('friction', [True, False])
@pytest.mark.parametrize('N', [1, 3, 4])
@pytest.mark.parametrize('kind', ['one_cell', 'cell_per_step'])
def test_handoff_cell_run_extremes(kind, N, friction, snap):
    """T = 40, B = 5.  one_cell: zero controls on a flat map -- no point ever changes cell, so every cell gradient leaves in the final flush
    of the two fetching waves.  cell_per_step: a 0.02 m grid under ~1 m/s -- a point changes cell every step or two, so nearly every step
    flushes.  N < 4: the lanes of absent points never flush.  With and without a friction map, terrain snap on and off."""
    from monoforce_amd import synthetic as syn
    pts4, masks4 = syn.robot_points_4()
    pts, masks = pts4[:N], [m[:N] for m in masks4]
    B, T = 5, 40

    def body(ppl):
        # (N < 4: the first N points of the four-point body WITH that body's inertia -- one or three points alone have a singular or
        #  lopsided inertia tensor, and two float32 evaluation orders of such a tumbling body part ways at 1e-3 .. 1e-1 in either library;
        #  tests/test_random_shapes_gpu.py builds its small bodies the same way)
        dp = make_dphysics(pts4, masks4, 1, res, d_max, points_per_lane=ppl, snap_to_terrain=snap)
        if N < 4:
            iinv = dp._iinv(torch.float32)
            dp.dphys_cfg.robot_points = torch.as_tensor(pts)
            dp.dphys_cfg.driving_parts = [torch.as_tensor(m) for m in masks]
            dp.x_points = dp.dphys_cfg.robot_points.unsqueeze(0).to(dp.device)
            dp._cache = {('iinv', torch.float32): iinv}
        return dp
    if kind == 'one_cell':
        res, d_max = 0.1, 1.6
        z = torch.zeros(32, 32)
        ctrl = torch.zeros(B, T, 2)
    else:
        res, d_max = 0.02, 1.6
        z = syn.bump_terrain(syn.bump_params(20), d_max, res) * 0.3
        ctrl = syn.const_controls(B, T, seed=5, v_range=(0.9, 1.0))
    mu = syn.wave_friction(d_max, res, 0.5, 1.0, 1.1, 0.8) if friction else None
    got = _run(body(16), z, mu, ctrl, True, 'all', want_route=', 3, 12, 3,')
    ref = _run(body(1), z, mu, ctrl, True, 'all')
    assert float(ref[0].abs().max()) > 0.0
    _same(got, ref, kind)


def test_handoff_vs_float64_oracle():
    """B = 37, T = 90, bumpy terrain and a friction map, all six outputs in the loss: gz, gmu, gc within 2e-4 of the float64 oracle (the bar
    of the record tests)."""
    from monoforce_amd import synthetic as syn, _timing
    from tests.test_parity_net_gpu import _record_case
    B, T = 37, 90
    _timing.start(capacity=16)
    got = _record_case(1, B)
    name = _timing.launches()['rollout_bwd_kernel']
    _timing.stop()
    assert ', 3, 12, 3,' in name, name
    pts, masks = syn.robot_points_4()
    z = (syn.bump_terrain(syn.bump_params(61), 6.4, 0.05) * 0.8).double().requires_grad_(True)
    mu = syn.wave_friction(6.4, 0.05, 0.5, 1.0, 1.3, 0.9).double().requires_grad_(True)
    ctrl = syn.varying_controls(B, T, seed=9).double().requires_grad_(True)
    spec = hp.spec_from(pts, masks, 1, 0.05, 6.4)
    rs, rf = orc.rollout(spec, z.unsqueeze(0).expand(B, -1, -1), ctrl, friction=mu.unsqueeze(0).expand(B, -1, -1))
    hp.probe_loss(list(rs) + list(rf), torch.float64).backward()
    for k, ref in (('gz', z.grad), ('gmu', mu.grad), ('gc', ctrl.grad)):
        assert hp.rel_err(got[k], ref) <= 2e-4, (k, hp.rel_err(got[k], ref))


def _fit_step(B, T, in_kernel, graph):
    from monoforce_amd import synthetic as syn
    from monoforce_amd.train import TerrainFitProblem
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 3.2)
    z_true = (syn.bump_terrain(syn.bump_params(3), 3.2, 0.1) * 0.3).to(DEV)
    mu = syn.wave_friction(3.2, 0.1).to(DEV)
    ctrl = syn.const_controls(B, T, seed=2).to(DEV)
    prob = TerrainFitProblem(dp, z_true, mu, ctrl, gt_every=5, graph=graph, loss_in_kernel=in_kernel)
    z = (z_true * 0.5).clone().requires_grad_(True)
    m = mu.clone().requires_grad_(True)
    vals = [float(prob.step(z, m)) for _ in range(3)]
    assert prob.graph == graph
    if in_kernel:      # the kernel under test: one more step launch by launch, its backward named by the library
        from monoforce_amd import _timing
        _timing.start(capacity=16)
        vals.append(float(prob.step(z, m, eager=True)))
        name = _timing.launches()['rollout_bwd_kernel']
        _timing.stop()
        assert 'true, false, 3, 12, 3,' in name, name      # <float, 1, XS_ONLY, no control gradients, kCpStream, 12 slots, batches of 3>
    return dict(vals=vals, gz=z.grad.detach().cpu().clone(), gmu=m.grad.detach().cpu().clone())


_CHILD = r'''
import sys, torch
sys.path.insert(0, %r)
from tests.test_stream_scatter_gpu import _fit_step
torch.save(_fit_step(%d, %d, False, False), %r)
'''


def test_handoff_fused_fit_step_equals_the_unfused_route():
    """TerrainFitProblem.step with the loss inside the rollout launches, launch by launch and as a replayed graph, against the unfused route
    (forward, the loss's own kernels, the backward on dense rows) run by a child process: the loss equal, the gradients within 2e-5."""
    B, T = 37, 50
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, 'unfused.pt')
        r = subprocess.run([sys.executable, '-c', _CHILD % (REPO, B, T, path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        ref = torch.load(path)
    for graph in (False, True):
        got = _fit_step(B, T, True, graph)
        assert len(set(got['vals'])) == 1, got['vals']
        assert abs(got['vals'][0] - ref['vals'][0]) <= 2e-6 * abs(ref['vals'][0]), (graph, got['vals'][0], ref['vals'][0])
        for k in ('gz', 'gmu'):
            assert hp.rel_err(got[k], ref[k]) <= 2e-5, (graph, k, hp.rel_err(got[k], ref[k]))


def test_handoff_full_occupancy_contended_map_vs_oracle_and_repeated():
    """1024 rollouts (256 workgroups: every CU runs one) x 48 steps on shared maps, all from one start pose -- every rollout's first cells are
    the same few, the contended case for the atomics.  The loss touches 32 rollouts spread over the batch and the float64 oracle
    differentiates those (as test_large_batch_shared_map_backward_vs_oracle).  Then the same step twice more on the same gradient pool:
    nothing stale in accumulators, counters or pool -- the three results agree within 2e-5."""
    from monoforce_amd import synthetic as syn, _timing
    B, T, sub = 1024, 48, 32
    pts, masks = syn.robot_points_4()
    z = syn.bump_terrain(syn.bump_params(5), 6.4, 0.05)
    mu = syn.wave_friction(6.4, 0.05)
    ctrl = syn.const_controls(B, T, seed=2)
    sel = torch.arange(0, B, B // sub)[:sub]
    spec = hp.spec_from(pts, masks, 1, 0.05, 6.4)
    wts = syn.probe_weights((sub, T, 3), phase=0.3)
    dp = make_dphysics(pts, masks, 1, 0.05, 6.4)
    dp.dphys_cfg.traj_sim_time = 5.0

    def step():
        zd, md, cd = z.to(DEV).requires_grad_(True), mu.to(DEV).requires_grad_(True), ctrl.to(DEV).requires_grad_(True)
        (Xs, Xds, Rs, Om), _ = dp(zd.unsqueeze(0), cd, friction=md.unsqueeze(0))
        ((Xs[sel.to(DEV)] * wts.to(DEV)).sum() + (Om[sel.to(DEV)] * wts.to(DEV)).sum() * 0.1).backward()
        return zd.grad.cpu(), md.grad.cpu(), cd.grad.cpu()

    _timing.start(capacity=16)
    first = step()
    name = _timing.launches()['rollout_bwd_kernel']
    _timing.stop()
    assert ', 3, 12, 3,' in name and 'grid=256 ' in name + ' ', name

    def oracle_grads(dtype):
        zc, mc = z.clone().to(dtype).requires_grad_(True), mu.clone().to(dtype).requires_grad_(True)      # (clones: the float32 pass must not mark z, mu themselves)
        cc = ctrl[sel].clone().to(dtype).requires_grad_(True)
        (rX, _, _, rO), _ = orc.rollout(spec, zc.unsqueeze(0).expand(sub, -1, -1), cc, friction=mc.unsqueeze(0).expand(sub, -1, -1))
        ((rX * wts.to(dtype)).sum() + (rO * wts.to(dtype)).sum() * 0.1).backward()
        return zc.grad, mc.grad, cc.grad
    ref, env = oracle_grads(torch.float64), oracle_grads(torch.float32)
    for nm, got, r64, r32 in zip(('z', 'mu', 'controls'), (first[0], first[1], first[2][sel]), ref, env):
        bar = max(2e-4, 3.0 * hp.rel_err(r32, r64))      # (the oracle's own float32 distance where that is larger: the existing test's bar)
        assert hp.rel_err(got, r64) <= bar, (nm, hp.rel_err(got, r64), 'bar', bar)
    for again in (step(), step()):
        for nm, a_, b_ in zip(('z', 'mu', 'controls'), again, first):
            assert hp.rel_err(a_, b_) <= 2e-5, (nm, hp.rel_err(a_, b_))
