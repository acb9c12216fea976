"""The positions-only twelve-slot streaming backward (rollout_bwd_cp_kernel.h, HANDOFF with XS_ONLY: the fit step's kernel and its
control-gradient twin) over the horizons that matter to a hand-off through a 24-entry answer ring beside the twelve coefficient slots
(tools/experiments/stream_answer_ring.patch: built, measured slower, not merged -- DESIGN.md section 8) as well as to today's hand-off
through the slots: the first ring's worth of steps (no predecessor), the final drain (per wave, in ordinal order), horizons around one to
eight coefficient rings with every batch remainder, runs on one cell that never end or end every step, absent contact points, and state
left behind from launch to launch.  References: the one-point-per-lane kernels, the unfused loss route, the float64 oracle.
And the reduction over the gradient copies, which clears only the cells that were written."""
import ctypes as C

import pytest
import torch

from oracle import dphysics_oracle as orc
from tests import helpers as hp
from tests.test_rollout_gpu import make_dphysics

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# T = 1 .. 7: no step, fewer than a batch, one and two batches; 12, 13: one coefficient ring; 23 .. 27: two coefficient rings = one answer
# ring; 35 .. 38, 47 .. 51: around three coefficient rings, two answer rings; 61, 73, 97: past three and four answer rings -- with every
# remainder of the batches of three
HORIZONS = list(range(1, 8)) + [12, 13] + list(range(23, 28)) + list(range(35, 39)) + list(range(47, 52)) + [61, 73, 97]
ROUTE_GCTRL = 'true, true, 3, 12, 3,'       # <float, 1, XS_ONLY, GCTRL, kCpStream, 12 slots, batches of 3, ...>
ROUTE_FIT = 'true, false, 3, 12, 3,'        # ... without control gradients: the fused-loss fit step


def _run_xs(dp, z, mu, ctrl, want_route=None):
    """One forward + backward on shared maps with a positions-only upstream; returns (gz, gmu, gc) on the host."""
    from monoforce_amd import synthetic as syn, _timing
    zd = z.to(DEV).requires_grad_(True)
    md = None if mu is None else mu.to(DEV).requires_grad_(True)
    cd = ctrl.to(DEV).requires_grad_(True)
    if want_route:
        _timing.start(capacity=16)
    st, _ = dp(zd.unsqueeze(0), cd, friction=None if md is None else md.unsqueeze(0))
    (st[0] * syn.probe_weights(st[0].shape, phase=0.4).to(DEV)).sum().backward()
    if want_route:
        name = _timing.launches()['rollout_bwd_kernel']
        _timing.stop()
        assert want_route in name, name
    return zd.grad.cpu(), None if md is None else md.grad.cpu(), cd.grad.cpu()


def _same(got, ref, tag, names=('gz', 'gmu', 'gc')):
    for name, a_, b_ in zip(names, got, ref):
        if b_ is None:
            assert a_ is None
            continue
        assert torch.isfinite(a_).all(), (tag, name)
        if float(b_.abs().max()) == 0.0:
            assert float(a_.abs().max()) == 0.0, (tag, name)
        else:
            assert hp.rel_err(a_, b_) <= 2e-5, (tag, name, hp.rel_err(a_, b_))


def _maps(cells):
    from monoforce_amd import synthetic as syn
    d_max = cells * 0.1 / 2
    return syn.bump_terrain(syn.bump_params(20), d_max, 0.1) * 0.3, syn.wave_friction(d_max, 0.1, 0.5, 1.0, 1.1, 0.8), d_max


@pytest.mark.parametrize('cells', [16, 32])
@pytest.mark.parametrize('B', [1, 4, 5])
def test_answer_ring_every_horizon_with_control_gradients(B, cells):
    """Positions-only upstream with control gradients: the twelve-slot streaming kernel == the one-point-per-lane kernels at 2e-5 over every horizon;
    a gradient that is exactly zero there is exactly zero here.  A partial wave, a full one, a trailing workgroup of one rollout."""
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    z, mu, d_max = _maps(cells)
    dps = {ppl: make_dphysics(pts, masks, 1, 0.1, d_max, points_per_lane=ppl) for ppl in (16, 1)}
    for T in HORIZONS:
        ctrl = syn.varying_controls(B, max(T, 2), seed=3)[:, :T]
        got = _run_xs(dps[16], z, mu, ctrl, want_route=ROUTE_GCTRL)
        ref = _run_xs(dps[1], z, mu, ctrl)
        _same(got, ref, T)


def _fit_problem(dp, cells, B, T, in_kernel):
    from monoforce_amd import synthetic as syn
    from monoforce_amd.train import TerrainFitProblem
    d_max = cells * 0.1 / 2
    z_true = (syn.bump_terrain(syn.bump_params(3), d_max, 0.1) * 0.3).to(DEV)
    mu = syn.wave_friction(d_max, 0.1).to(DEV)
    ctrl = syn.const_controls(B, T, seed=2).to(DEV)
    prob = TerrainFitProblem(dp, z_true, mu, ctrl, gt_every=5 if T >= 5 else 1, graph=False, loss_in_kernel=in_kernel)
    return prob, z_true, mu


def _fit_step(prob, z_true, mu, want_route=None):
    from monoforce_amd import _timing
    z = (z_true * 0.5).clone().requires_grad_(True)
    m = mu.clone().requires_grad_(True)
    if want_route:
        _timing.start(capacity=16)
    val = float(prob.step(z, m))
    if want_route:
        name = _timing.launches()['rollout_bwd_kernel']
        _timing.stop()
        assert want_route in name, name
    return val, z.grad.detach().cpu().clone(), m.grad.detach().cpu().clone()


@pytest.mark.parametrize('cells', [16, 32])
@pytest.mark.parametrize('B', [1, 4, 5])
def test_answer_ring_every_horizon_fused_fit_step(B, cells):
    """The fit step with the loss inside the rollout launches (no control gradients) against the unfused loss route -- forward, the loss's
    own kernels, the backward on dense gradient rows -- over every horizon: gradients within 2e-5, exact zeros stay exact zeros, and the
    loss value (two float32 sums of the same terms in different orders) within the same bar."""
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, cells * 0.1 / 2)
    for T in HORIZONS:
        fused, z_true, mu = _fit_problem(dp, cells, B, T, True)
        unfused, _, _ = _fit_problem(dp, cells, B, T, False)
        got = _fit_step(fused, z_true, mu, want_route=ROUTE_FIT)
        ref = _fit_step(unfused, z_true, mu)
        assert abs(got[0] - ref[0]) <= 2e-5 * abs(ref[0]), (T, got[0], ref[0])
        _same(got[1:], ref[1:], T, names=('gz', 'gmu'))


@pytest.mark.parametrize('N', [1, 3, 4])
@pytest.mark.parametrize('kind', ['one_cell', 'cell_per_step'])
def test_answer_ring_cell_run_extremes(kind, N):
    """T = 40, B = 5, positions-only upstream.  one_cell: zero controls on a flat map -- no point ever changes cell, so every cell gradient
    leaves in the final drain of the two fetching waves.  cell_per_step: a 0.02 m grid under ~1 m/s -- a flush nearly
    every step.  N < 4: the lanes of absent points never flush."""
    from monoforce_amd import synthetic as syn
    pts4, masks4 = syn.robot_points_4()
    pts, masks = pts4[:N], [m[:N] for m in masks4]
    B, T = 5, 40

    def body(ppl):
        # (N < 4: the first N points of the four-point body WITH that body's inertia, as tests/test_stream_scatter_gpu.py builds them)
        dp = make_dphysics(pts4, masks4, 1, res, d_max, points_per_lane=ppl)
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
    mu = syn.wave_friction(d_max, res, 0.5, 1.0, 1.1, 0.8)
    got = _run_xs(body(16), z, mu, ctrl, want_route=ROUTE_GCTRL)
    ref = _run_xs(body(1), z, mu, ctrl)
    assert float(ref[0].abs().max()) > 0.0
    _same(got, ref, kind)


def test_answer_ring_nothing_survives_a_launch():
    """The same fit step three times in one process, then another horizon, then the first again: the loss bit for bit, the gradients within
    2e-7 of the largest gradient (the atomics' order is free) -- nothing of the ring, the answers or the flags survives a launch."""
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 1.6)
    first, z_true, mu = _fit_problem(dp, 32, 37, 50, True)
    other, _, _ = _fit_problem(dp, 32, 37, 29, True)
    runs = [_fit_step(first, z_true, mu, want_route=ROUTE_FIT) for _ in range(3)]
    _fit_step(other, z_true, mu, want_route=ROUTE_FIT)
    runs.append(_fit_step(first, z_true, mu, want_route=ROUTE_FIT))
    assert float(runs[0][1].abs().max()) > 0.0
    for k, again in enumerate(runs[1:]):
        assert again[0] == runs[0][0], (k, again[0], runs[0][0])
        for nm, a_, b_ in zip(('gz', 'gmu'), again[1:], runs[0][1:]):
            assert hp.rel_err(a_, b_) <= 2e-7, (k, nm, hp.rel_err(a_, b_))


def test_answer_ring_vs_float64_oracle():
    """B = 37, T = 90, bumpy terrain and a friction map, the positions in the loss: gz, gmu, gc within 2e-4 of the float64 oracle (the bar
    of test_handoff_vs_float64_oracle)."""
    from monoforce_amd import synthetic as syn
    B, T = 37, 90
    pts, masks = syn.robot_points_4()
    z = syn.bump_terrain(syn.bump_params(61), 6.4, 0.05) * 0.8
    mu = syn.wave_friction(6.4, 0.05, 0.5, 1.0, 1.3, 0.9)
    ctrl = syn.varying_controls(B, T, seed=9)
    got = _run_xs(make_dphysics(pts, masks, 1, 0.05, 6.4), z, mu, ctrl, want_route=ROUTE_GCTRL)
    zr, mr, cr = z.double().requires_grad_(True), mu.double().requires_grad_(True), ctrl.double().requires_grad_(True)
    spec = hp.spec_from(pts, masks, 1, 0.05, 6.4)
    (rX, _, _, _), _ = orc.rollout(spec, zr.unsqueeze(0).expand(B, -1, -1), cr, friction=mr.unsqueeze(0).expand(B, -1, -1))
    (rX * syn.probe_weights(rX.shape, phase=0.4, dtype=torch.float64)).sum().backward()
    for nm, a_, ref in zip(('gz', 'gmu', 'gc'), got, (zr.grad, mr.grad, cr.grad)):
        assert hp.rel_err(a_, ref) <= 2e-4, (nm, hp.rel_err(a_, ref))


def _sum_in_copy_order(saved, n_maps, copies, n):
    """out[m][i] = ((0 + pool[m][0][i]) + pool[m][1][i]) + ... in float32: the order the reduction adds in."""
    p = saved[:n_maps * copies * n].view(n_maps, copies, n)
    acc = torch.zeros(n_maps, n, dtype=saved.dtype, device=saved.device)
    for c in range(copies):
        acc = acc + p[:, c]
    return acc


def test_reduction_after_a_fit_step_sums_the_pool_and_leaves_it_zero(monkeypatch):
    """B = 5, T = 40: most cells of most copies are untouched.  .grad equals a plain torch reduction of the pool as the backward left it,
    and the pool is all zeros afterwards."""
    from monoforce_amd import rollout_launch, synthetic as syn
    saved = {}
    reduce = rollout_launch.GradPool.reduce

    def spy(self, map_shape):
        saved['before'], saved['pool'] = self.buf.clone(), self
        return reduce(self, map_shape)
    monkeypatch.setattr(rollout_launch.GradPool, 'reduce', spy)
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 1.6)
    prob, z_true, mu = _fit_problem(dp, 32, 5, 40, True)
    _, gz, gmu = _fit_step(prob, z_true, mu, want_route=ROUTE_FIT)
    pool = saved['pool']
    assert pool.n_maps == 2 and pool.n == 32 * 32
    before = saved['before']
    assert 0 < int((before != 0).sum()) < before.numel() // 2      # a sparse pool: the case the conditional clear is for
    want = _sum_in_copy_order(before, pool.n_maps, pool.copies, pool.n).cpu()
    assert torch.equal(gz.reshape(-1), want[0]) and torch.equal(gmu.reshape(-1), want[1])
    torch.cuda.synchronize()
    assert int((pool.buf != 0).sum()) == 0


def test_reduction_of_a_pool_without_a_single_zero():
    """Every cell of every copy non-zero (no store is skipped), an element count that is no multiple of the block: the sums in copy order, the
    pool all zeros, the spare elements behind it untouched."""
    from monoforce_amd import _lib
    n_maps, copies, n = 2, 7, 33 * 31
    g = torch.Generator().manual_seed(11)
    vals = torch.rand(n_maps * copies * n, generator=g) + 0.5
    vals = vals * torch.where(torch.rand(vals.shape, generator=g) < 0.5, -1.0, 1.0)
    buf = torch.cat([vals, torch.full((16,), 7.0)]).to(DEV)
    before = buf.clone()
    out = torch.full((n_maps * n + 1,), -3.0, device=DEV)
    _lib.check(_lib.lib().mf_reduce_grad_copies_f32(_lib.ptr(buf), n_maps, copies, C.c_longlong(n), _lib.ptr(out),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mf_reduce_grad_copies')
    torch.cuda.synchronize()
    assert torch.equal(out[:-1].view(n_maps, n), _sum_in_copy_order(before, n_maps, copies, n))
    assert float(out[-1]) == -3.0
    assert int((buf[:-16] != 0).sum()) == 0 and torch.equal(buf[-16:], before[-16:])
