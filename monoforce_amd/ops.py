"""`torch.ops.monoforce.*`: the hot-path kernels registered with `torch.library` ("C-ABI the replacement exports").

Schemas (tensors on the GPU, float32 or float64; `Bz` in {1, B}: a [1,H,W] map is ONE map shared by all rollouts):

    monoforce::dphys_rollout_fwd(Tensor z, Tensor? mu, Tensor controls, Tensor x0, Tensor xd0, Tensor R0, Tensor w0,
                                 Tensor pts, Tensor part_id, Tensor Iinv, float[] consts, int integrator, bool save_for_bwd)
                                 -> (Tensor Xs, Tensor Xds, Tensor Rs, Tensor Om, Tensor Fs, Tensor Ff, Tensor Xraw, Tensor x0_snapped,
                                     Tensor rec)
    monoforce::dphys_rollout_bwd(Tensor z, Tensor? mu, Tensor controls, Tensor x_init, Tensor xd0, Tensor R0, Tensor w0,
                                 Tensor pts, Tensor part_id, Tensor Iinv, float[] consts, int integrator,
                                 Tensor Xraw, Tensor Xds, Tensor Rs, Tensor Om, Tensor rec,
                                 Tensor? gXs, Tensor? gXds, Tensor? gRs, Tensor? gOm, Tensor? gFs, Tensor? gFf)
                                 -> (Tensor gz, Tensor gmu, Tensor gcontrols, Tensor gx0, Tensor gxd0, Tensor gR0, Tensor gw0)
    monoforce::bev_splat_plan(Tensor geom, float[] dx, float[] bx, int[] nx) -> Tensor plan
    monoforce::bev_splat_fwd(Tensor x, Tensor plan, int B, int n_per_sample, float[] dx, float[] bx, int[] nx) -> Tensor
    monoforce::bev_splat_bwd(Tensor grad, Tensor plan, int B, int n_per_sample, int C, float[] dx, float[] bx, int[] nx) -> Tensor
    monoforce::mppi_perturb(Tensor nominal, Tensor noise, float[] sigma, float[] lo, float[] hi, bool keep_nominal) -> Tensor controls
    monoforce::path_costs(Tensor cost_rows, Tensor? force_cost, Tensor x_last, Tensor goal, float[] weights) -> (Tensor costs, Tensor terms)
    monoforce::mppi_update(Tensor costs, Tensor controls, Tensor nominal, float lam)
                                 -> (Tensor nominal, Tensor weights, Tensor best, Tensor n_valid)
    monoforce::pose_costs(Tensor Xs, Tensor Rs, Tensor points, Tensor? cost_map, Tensor? path, Tensor? base_costs, float grid_res,
                          float d_max, float lethal, float off_map, float[] weights) -> (Tensor costs, Tensor terms)
    monoforce::traj_objective(Tensor Xs, Tensor Rs, Tensor goal, Tensor points, Tensor? cost_map, Tensor? path, float[] weights, int pose_stride,
                              float grid_res, float d_max, float lethal, float off_map) -> (Tensor costs, Tensor terms, Tensor gXs, Tensor gRs)
    monoforce::hm_loss(Tensor height_pred, Tensor height_gt, Tensor? weights, float? h_max) -> (Tensor loss, Tensor n_valid)
    monoforce::total_variation(Tensor heightmap) -> Tensor loss
    monoforce::traversability(Tensor z, Tensor? valid, Tensor? base, float grid_res, int radius_cells, float[] lo, float[] hi, float unknown,
                              int min_valid, bool return_terms) -> (Tensor cost, Tensor terms)
    monoforce::cost_to_go(Tensor cost_map, Tensor goal, float grid_res, float d_max, float lethal, float alpha, int n_rounds)
                              -> (Tensor field, Tensor status, Tensor rounds_used)
    monoforce::extract_route(Tensor field, Tensor cost_map, Tensor start, Tensor goal, float grid_res, float d_max, float lethal, float alpha,
                              int n_vertices, int max_nodes) -> (Tensor path, Tensor nodes, Tensor n_nodes, Tensor route_cost, Tensor status)

`consts` = [mass, gravity, stiffness, damping, grid_res, d_max, dt, omega_max, robot_size_y(, traj_sim_time)]; `part_id[N]` int32
(index of the last driving mask holding the point, -1 = not driving); `Iinv` [3,3] on the HOST (nine scalars of the launch
descriptor); `integrator` 0 = dynamics(), 1 = odeint-euler (MF_INTEG_*).  The ops are functional: the start position with
its z component moved onto the terrain (dphysics.py:567-571, an in-place write in the reference) comes back as `x0_snapped`,
and `rollout()` below copies it into the caller's tensor.  Outputs are `[B,T,...]` views of time-major buffers, like
`DPhysics.forward`.  Every op is one or two launches of the C ABI (include/monoforce_hip.h) on
the current stream; no synchronisation, no host round trip, so they can be captured into a hipGraph.  Autograd formulas are
registered (`rollout_fwd` -> `rollout_bwd`, `bev_splat_fwd` -> `bev_splat_bwd`), as are shape functions for tracing.  `rec` is
the per-step record small launches keep for the backward (MfRolloutFwdBufs.rec; empty otherwise).

The three MPPI ops (float32, no autograd; monoforce_amd/mppi.py is their consumer): `nominal` [T,2], `noise` / `controls` [B,T,2], `cost_rows`
[B,T,4] in any strides whose last axis is dense (the [B,T,4] view `DPhysics.rollout_costs` returns is read in place), `x_last` [B,>=2], `goal`
[2] on the device, `weights` = (inclination, force, goal) with `force_cost` given exactly when the force weight is non-zero; `best` / `n_valid`
are int32 [1] on the device.

`pose_costs` (float32, no autograd; monoforce_amd/csrc/pose_costs.hip, formulas in include/monoforce_hip.h at MfPoseCostDesc): `Xs` [B,Tp,3] and
`Rs` [B,Tp,3,3] are the kept poses of `DPhysics.rollout_costs`, read in place through their strides (the time-major views need no copy);
`points` [N,3] the footprint in the body frame; `cost_map` [H,W] on the nodes of z_grid; `path` [P,2]; `weights` = (map, path), each 0 when
its input is None; `costs` [B] = base_costs + w_map map + w_path xtrack, `terms` [B,2] = (map, xtrack).  One launch.

`traj_objective` (float32, autograd to `Xs` and `Rs`; monoforce_amd/csrc/traj_objective.hip, formulas in include/monoforce_hip.h at
MfTrajObjDesc): the planner's cost of B rollouts from the FULL outputs of the rollout op, `Xs` [B,T,3] and `Rs` [B,T,3,3] read in place through
their strides, at the steps `rollout_costs` keeps for `pose_stride`; `weights` = (map, path, goal, inclination); `costs` [B], `terms` [B,4];
`gXs` / `gRs` are dcosts.sum()/dXs and /dRs in the strides of the inputs (the backward scales them by the upstream gradient).  One launch;
it delegates to monoforce_amd/refine.py, which marshals the entry point (its `trajectory_objective` is the drop-in form, with the ATen route).

`hm_loss` / `total_variation` (float32 or float64, autograd to `height_pred` / `heightmap`; monoforce_amd/csrc/map_losses.hip, formulas in
include/monoforce_hip.h at MfMapLossDesc): map tensors [...,H,W], channel views and row-strided crops read in place; `loss` a scalar, `n_valid`
int32 [1] = the cells that entered the mean.  One launch forward, one backward; both delegate to monoforce_amd/losses.py, which marshals
the entry points (its `hm_loss` / `total_variation` are the drop-in forms, with the ATen route for CPU tensors).

`traversability` (float32 or float64, no autograd; monoforce_amd/csrc/traversability.hip, definition in include/monoforce_hip.h at
MfTraversabilityDesc): `z` [H,W] or [S,H,W] with unit stride along W, read in place (as `valid` and `base` of the same shape); `lo` / `hi` the
ramps of (slope, roughness, step); `cost` has z's shape, `terms` is [..,3,H,W] (empty without `return_terms`).  One launch; it delegates to
monoforce_amd/costmap.py, which marshals the entry point (`traversability_into` below writes caller-owned buffers; `traversability_map` is
the form with the radius in metres and the ATen route for CPU tensors).

`cost_to_go` / `extract_route` (float32 or float64, no autograd; monoforce_amd/csrc/cost_to_go.hip, definition in include/monoforce_hip.h at
MfCostToGoDesc): `cost_map` [H,W] or [S,H,W] with unit stride along W, read in place; `goal` / `start` [2] or [S,2]; `n_rounds` / `max_nodes`
<= 0 ask for the defaults.  `field` has cost_map's shape, `status` / `rounds_used` / `n_nodes` are int32 [S], `path` float32 [S,P,2], `nodes`
int32 [S,max_nodes].  Both delegate to monoforce_amd/route.py, which marshals the entry points (`RoutePlanner` there owns static buffers).

The rollout ops and `DPhysics`'s own autograd function (monoforce_amd/dphysics.py: more options -- articulated bodies, path costs,
strided controls) launch through the same marshalling (monoforce_amd/rollout_launch.py), the splat ops and `voxel_pooling` likewise
(monoforce_amd/splat.py); only the MPPI and pose-cost entry points, which have no other caller, are marshalled here (`_lib.launch`).
`rollout()` / `splat()` below are the functional entries.
"""
import ctypes as C

import torch

from . import _lib, costmap as _costmap, losses as _losses, refine as _refine, rollout_launch as rl, route as _route, splat as _splat


class _PoolOwner:       # the registered ops have no module to hang the persistent gradient-copy pools on
    pass


_POOL_OWNER = _PoolOwner()

__all__ = ['rollout', 'splat', 'CONST_NAMES']

CONST_NAMES = ('mass', 'gravity', 'stiffness', 'damping', 'grid_res', 'd_max', 'dt', 'omega_max', 'robot_size_y')      # + optional traj_sim_time

_L = torch.library.Library('monoforce', 'DEF')
_L.define('dphys_rollout_fwd(Tensor z, Tensor? mu, Tensor controls, Tensor x0, Tensor xd0, Tensor R0, Tensor w0, Tensor pts, '
          'Tensor part_id, Tensor Iinv, float[] consts, int integrator, bool save_for_bwd) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)')
_L.define('dphys_rollout_bwd(Tensor z, Tensor? mu, Tensor controls, Tensor x_init, Tensor xd0, Tensor R0, Tensor w0, Tensor pts, '
          'Tensor part_id, Tensor Iinv, float[] consts, int integrator, Tensor Xraw, Tensor Xds, Tensor Rs, Tensor Om, Tensor rec, '
          'Tensor? gXs, Tensor? gXds, Tensor? gRs, Tensor? gOm, Tensor? gFs, Tensor? gFf) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)')
_L.define('bev_splat_plan(Tensor geom, float[] dx, float[] bx, int[] nx) -> Tensor')
_L.define('bev_splat_fwd(Tensor x, Tensor plan, int B, int n_per_sample, float[] dx, float[] bx, int[] nx) -> Tensor')
_L.define('bev_splat_bwd(Tensor grad, Tensor plan, int B, int n_per_sample, int C, float[] dx, float[] bx, int[] nx) -> Tensor')
_L.define('mppi_perturb(Tensor nominal, Tensor noise, float[] sigma, float[] lo, float[] hi, bool keep_nominal) -> Tensor')
_L.define('path_costs(Tensor cost_rows, Tensor? force_cost, Tensor x_last, Tensor goal, float[] weights) -> (Tensor, Tensor)')
_L.define('mppi_update(Tensor costs, Tensor controls, Tensor nominal, float lam) -> (Tensor, Tensor, Tensor, Tensor)')
_L.define('pose_costs(Tensor Xs, Tensor Rs, Tensor points, Tensor? cost_map, Tensor? path, Tensor? base_costs, float grid_res, float d_max, '
          'float lethal, float off_map, float[] weights) -> (Tensor, Tensor)')
_L.define('traj_objective(Tensor Xs, Tensor Rs, Tensor goal, Tensor points, Tensor? cost_map, Tensor? path, float[] weights, int pose_stride, '
          'float grid_res, float d_max, float lethal, float off_map) -> (Tensor, Tensor, Tensor, Tensor)')
_L.define('hm_loss(Tensor height_pred, Tensor height_gt, Tensor? weights, float? h_max) -> (Tensor, Tensor)')
_L.define('total_variation(Tensor heightmap) -> Tensor')
_L.define('traversability(Tensor z, Tensor? valid, Tensor? base, float grid_res, int radius_cells, float[] lo, float[] hi, float unknown, '
          'int min_valid, bool return_terms) -> (Tensor, Tensor)')
_L.define('cost_to_go(Tensor cost_map, Tensor goal, float grid_res, float d_max, float lethal, float alpha, int n_rounds) -> (Tensor, Tensor, Tensor)')
_L.define('extract_route(Tensor field, Tensor cost_map, Tensor start, Tensor goal, float grid_res, float d_max, float lethal, float alpha, '
          'int n_vertices, int max_nodes) -> (Tensor, Tensor, Tensor, Tensor, Tensor)')


def _time_grid(consts, T, dt, dev):
    """The reference's grid: linspace(0, T_sim, int(T_sim / dt))[:T] (dphysics.py:166-167, 581); T_sim defaults to T * dt."""
    step = float(consts[6])
    t_sim = float(consts[9]) if len(consts) > 9 else T * step
    return rl.time_grid(t_sim, max(int(t_sim / step), T), T, dt, dev)


def _prep(z, mu, controls, pts, part_id, Iinv, consts, integrator, states):
    """(descriptor, z, mu, controls, pts, part_id, state, ts) in the kernels' dtype and layout.  The maps go through the same checks and
    canonical form as on the module path (`rollout_launch.canonical_maps`), except that here only a [1,H,W] map counts as shared -- an
    expanded one (stride 0) is read per rollout; every start-state tensor has the B rows of `controls`."""
    dt = z.dtype
    assert len(consts) in (len(CONST_NAMES), len(CONST_NAMES) + 1), f'consts = {CONST_NAMES} (+ traj_sim_time)'
    assert controls.dim() == 3 and controls.shape[2] == 2, f'controls must be [B,T,2], got {tuple(controls.shape)}'
    B, T = controls.shape[:2]
    for name, t in zip(('x0', 'xd0', 'R0', 'w0'), states):
        assert t.shape[0] == B, f'{name} has {t.shape[0]} rows, controls {B} rollouts'
    assert pts.dim() == 2 and pts.shape[1] == 3 and part_id.shape[0] == pts.shape[0], 'pts must be [N,3] with one part id per point'
    unshare = lambda m: m if m is None or m.shape[0] == 1 else m.to(dt).contiguous()  # noqa: E731
    zc, muc, shared = rl.canonical_maps(unshare(z), unshare(None if mu is None else mu.to(dt)), B)
    # (n_tracks = 2: the ops' schema carries no track count.  Iinv: 9 host scalars -- a device read: build the op's inputs once)
    d = rl.rollout_desc(B, T, pts.shape[0], z.shape[1], z.shape[2], int(integrator), consts=dict(zip(CONST_NAMES, (float(v) for v in consts))),
                        Iinv=Iinv.detach().double().flatten().tolist(), n_tracks=2, layout=_lib.MF_LAYOUT_TIME_MAJOR, map_shared=int(shared),
                        math_mode=_lib.MF_MATH_EXACT if dt == torch.float64 else _lib.MF_MATH_FAST)
    return (d, zc, muc, controls.to(dt).contiguous(), pts.to(dt).contiguous(), part_id.to(torch.int32).contiguous(),
            tuple(t.to(dt).contiguous() for t in states), _time_grid(consts, T, dt, z.device))


@torch.library.impl(_L, 'dphys_rollout_fwd', 'CUDA')
def _rollout_fwd(z, mu, controls, x0, xd0, R0, w0, pts, part_id, Iinv, consts, integrator, save_for_bwd):
    dt = z.dtype
    d, zc, muc, cc, pc, part, (x0, xd0, R0, w0), ts = _prep(z, mu, controls, pts, part_id, Iinv, consts, integrator, (x0, xd0, R0, w0))
    x0 = x0.clone()          # the kernel moves its z component onto the terrain: returned, not written in place
    with torch.cuda.device(z.device):      # (the policy queries read the CU count of the CURRENT device)
        # the component-parallel kernels' per-step record for the backward (MfRolloutFwdBufs.rec), where the library keeps one: float32
        f = rl.launch_forward(d, zc, muc, cc, ts, pc, part, (x0, xd0, R0, w0), want_xraw=save_for_bwd,
                              want_rec=save_for_bwd and dt == torch.float32)
    tr = lambda t: t.transpose(0, 1)  # noqa: E731
    empty = lambda: torch.empty(0, dtype=dt, device=z.device)  # noqa: E731
    return (tr(f.Xs), tr(f.Xds), tr(f.Rs), tr(f.Om), tr(f.Fs[:, :, :d.N]), tr(f.Ff[:, :, :d.N]), (tr(f.Xraw) if save_for_bwd else empty()), x0,
            empty() if f.rec is None else f.rec)


@torch.library.impl(_L, 'dphys_rollout_bwd', 'CUDA')
def _rollout_bwd(z, mu, controls, x_init, xd0, R0, w0, pts, part_id, Iinv, consts, integrator, Xraw, Xds, Rs, Om, rec, gXs, gXds, gRs, gOm, gFs, gFf):
    dt = z.dtype
    d, zc, muc, cc, pc, part, state, ts = _prep(z, mu, controls, pts, part_id, Iinv, consts, integrator, (x_init, xd0, R0, w0))
    saved = [t.to(dt).transpose(0, 1).contiguous() for t in (Xraw, Xds, Rs, Om)]      # ([B,T,..] -> time-major rows)
    if d.map_shared:
        d.grad_copies = rl.grad_copies_for(d.B, d.N)
    with torch.cuda.device(z.device):
        g = rl.launch_backward(d, zc, muc, cc, ts, pc, part, state, saved, (gXs, gXds, gRs, gOm, gFs, gFf), pool_owner=_POOL_OWNER,
                               rec=rec if rec.numel() else None)
    # [1,H,W] for ONE shared map; a map that came in as one shared map next to a per-rollout one was expanded: its gradient is the sum over the rollouts
    to_input = lambda g_, m: g_.unsqueeze(0) if g_.dim() == 2 else (g_.sum(0, keepdim=True) if g_.shape[0] != m.shape[0] else g_)  # noqa: E731
    gmu = to_input(g.gmu, mu) if g.gmu is not None else torch.zeros(0, dtype=dt, device=z.device)
    return to_input(g.gz, z), gmu, g.gcontrols, g.gx0, g.gxd0, g.gR0, g.gw0


def _rollout_setup(ctx, inputs, output):
    z, mu, controls, x0, xd0, R0, w0, pts, part_id, Iinv, consts, integrator, save_for_bwd = inputs
    ctx.consts, ctx.integrator, ctx.has_mu = list(consts), integrator, mu is not None
    if not save_for_bwd:
        ctx.ok = False
        return
    ctx.ok = True
    Xs, Xds, Rs, Om, Fs, Ff, Xraw, x0s, rec = output
    ctx.save_for_backward(z, mu, controls, x0s, xd0, R0, w0, pts, part_id, Iinv, Xraw, Xds, Rs, Om, rec)
    ctx.set_materialize_grads(False)


def _rollout_backward(ctx, gXs, gXds, gRs, gOm, gFs, gFf, _gXraw, _gx0s, _grec):
    if not ctx.ok:
        raise RuntimeError('monoforce::dphys_rollout_fwd was called with save_for_bwd=False: no gradient available')
    z, mu, controls, x_init, xd0, R0, w0, pts, part_id, Iinv, Xraw, Xds, Rs, Om, rec = ctx.saved_tensors
    gz, gmu, gc, gx0, gxd0, gR0, gw0 = torch.ops.monoforce.dphys_rollout_bwd(
        z, mu, controls, x_init, xd0, R0, w0, pts, part_id, Iinv, ctx.consts, ctx.integrator, Xraw, Xds, Rs, Om, rec, gXs, gXds, gRs, gOm, gFs, gFf)
    return gz, (gmu if ctx.has_mu else None), gc, gx0, gxd0, gR0, gw0, None, None, None, None, None, None


torch.library.register_autograd('monoforce::dphys_rollout_fwd', _rollout_backward, setup_context=_rollout_setup, lib=_L)


@torch.library.register_fake('monoforce::dphys_rollout_fwd', lib=_L)
def _rollout_fwd_fake(z, mu, controls, x0, xd0, R0, w0, pts, part_id, Iinv, consts, integrator, save_for_bwd):
    B, T = controls.shape[:2]
    N = pts.shape[0]
    e = lambda *s: z.new_empty(s)  # noqa: E731
    return e(B, T, 3), e(B, T, 3), e(B, T, 3, 3), e(B, T, 3), e(B, T, N, 3), e(B, T, N, 3), (e(B, T, 3) if save_for_bwd else e(0)), e(B, 3), e(0)


@torch.library.register_fake('monoforce::dphys_rollout_bwd', lib=_L)
def _rollout_bwd_fake(z, mu, controls, x_init, xd0, R0, w0, pts, part_id, Iinv, consts, integrator, Xraw, Xds, Rs, Om, rec, gXs, gXds, gRs, gOm, gFs, gFf):
    B = controls.shape[0]
    return (torch.empty_like(z), torch.empty_like(mu) if mu is not None else z.new_empty(0), torch.empty_like(controls), z.new_empty(B, 3),
            z.new_empty(B, 3), z.new_empty(B, 3, 3), z.new_empty(B, 3))


# ---- BEV voxel pooling -------------------------------------------------------------------------------------------------
@torch.library.impl(_L, 'bev_splat_plan', 'CUDA')
def _splat_plan(geom, dx, bx, nx):
    return _splat.SplatPlan(geom, dx, bx, nx).workspace


@torch.library.impl(_L, 'bev_splat_fwd', 'CUDA')
def _splat_fwd(x, plan, B, n_per_sample, dx, bx, nx):
    return _splat.pool_forward(x, _splat.SplatPlan.wrap(plan, B, n_per_sample, _splat.grid_host(dx, bx, nx)))


@torch.library.impl(_L, 'bev_splat_bwd', 'CUDA')
def _splat_bwd(grad, plan, B, n_per_sample, Cc, dx, bx, nx):
    return _splat.pool_backward(grad, _splat.SplatPlan.wrap(plan, B, n_per_sample, _splat.grid_host(dx, bx, nx)), Cc)


def _splat_setup(ctx, inputs, output):
    x, plan, B, n_per_sample, dx, bx, nx = inputs
    ctx.save_for_backward(plan)
    ctx.args = (B, n_per_sample, x.shape[-1], list(dx), list(bx), list(nx))
    ctx.x_shape = x.shape


def _splat_backward(ctx, grad):
    plan, = ctx.saved_tensors
    B, n, Cc, dx, bx, nx = ctx.args
    return torch.ops.monoforce.bev_splat_bwd(grad, plan, B, n, Cc, dx, bx, nx).view(ctx.x_shape), None, None, None, None, None, None


torch.library.register_autograd('monoforce::bev_splat_fwd', _splat_backward, setup_context=_splat_setup, lib=_L)


@torch.library.register_fake('monoforce::bev_splat_fwd', lib=_L)
def _splat_fwd_fake(x, plan, B, n_per_sample, dx, bx, nx):
    return x.new_empty(B, int(nx[2]) * x.shape[-1], int(nx[0]), int(nx[1]))


@torch.library.register_fake('monoforce::bev_splat_bwd', lib=_L)
def _splat_bwd_fake(grad, plan, B, n_per_sample, Cc, dx, bx, nx):
    return grad.new_empty(B * n_per_sample, Cc)


# ---- MPPI iteration ------------------------------------------------------------------------------------------------------------
def _mppi_desc(B, T, sigma=(0., 0.), lo=(0., 0.), hi=(0., 0.), weights=(0., 0., 0.), lam=1.0, keep_nominal=False):
    f2 = lambda v: (C.c_float * 2)(float(v[0]), float(v[1]))  # noqa: E731
    return _lib.MfMppiDesc(B=int(B), T=int(T), keep_nominal=int(bool(keep_nominal)), sigma=f2(sigma), lo=f2(lo), hi=f2(hi),
                           w_incl=float(weights[0]), w_force=float(weights[1]), w_goal=float(weights[2]), lam=float(lam))


def _f32(t, name):
    _lib.require_hip_tensor(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f'monoforce MPPI ops compute in float32, {name} is {t.dtype}')
    return t


@torch.library.impl(_L, 'mppi_perturb', 'CUDA')
def _mppi_perturb(nominal, noise, sigma, lo, hi, keep_nominal):
    nom, nz = _f32(nominal, 'nominal').contiguous(), _f32(noise, 'noise').contiguous()
    assert nz.dim() == 3 and nz.shape[2] == 2 and tuple(nom.shape) == (nz.shape[1], 2), \
        f'noise must be [B,T,2] and nominal [T,2], got {tuple(nz.shape)} and {tuple(nom.shape)}'
    d = _mppi_desc(nz.shape[0], nz.shape[1], sigma=sigma, lo=lo, hi=hi, keep_nominal=keep_nominal)
    controls = torch.empty_like(nz)
    _lib.launch('mf_mppi_perturb', nz.device, d, nom, nz, controls, dtype=torch.float32, timer='mppi_perturb_kernel')
    return controls


@torch.library.impl(_L, 'path_costs', 'CUDA')
def _path_costs(cost_rows, force_cost, x_last, goal, weights):
    rows = _f32(cost_rows, 'cost_rows')
    assert rows.dim() == 3 and rows.shape[2] == 4, f'cost_rows must be [B,T,4], got {tuple(rows.shape)}'
    B, T = rows.shape[:2]
    if rows.stride(2) != 1:
        rows = rows.contiguous()
    xl = _f32(x_last, 'x_last')
    assert xl.dim() == 2 and xl.shape[0] == B and xl.shape[1] >= 2, f'x_last must be [B,>=2], got {tuple(xl.shape)}'
    if xl.stride(1) != 1:
        xl = xl.contiguous()
    g = _f32(goal, 'goal').contiguous()
    assert g.numel() == 2, 'goal must hold (x, y)'
    assert len(weights) == 3, 'weights = (inclination, force, goal)'
    fc = None if force_cost is None else _f32(force_cost, 'force_cost').contiguous()
    assert fc is None or fc.numel() == B, 'force_cost must be [B]'
    d = _mppi_desc(B, T, weights=weights)
    d.row_stride_b, d.row_stride_t, d.x_stride_b = rows.stride(0), rows.stride(1), xl.stride(0)
    costs, terms = torch.empty(B, dtype=torch.float32, device=rows.device), torch.empty(B, 3, dtype=torch.float32, device=rows.device)
    _lib.launch('mf_path_costs', rows.device, d, rows, fc, xl, g, costs, terms, dtype=torch.float32, timer='path_costs_kernel')
    return costs, terms


def mppi_update_into(costs, controls, nominal, lam, out):
    """`torch.ops.monoforce.mppi_update` writing the new nominal into `out` [T,2] (which may be `nominal` itself: the planner's resident buffer);
    returns (out, weights, best, n_valid)."""
    c, u, nom = _f32(costs, 'costs').contiguous(), _f32(controls, 'controls').contiguous(), _f32(nominal, 'nominal')
    assert u.dim() == 3 and u.shape[2] == 2 and c.shape == (u.shape[0],) and tuple(nom.shape) == (u.shape[1], 2), \
        f'costs [B], controls [B,T,2], nominal [T,2] expected, got {tuple(c.shape)}, {tuple(u.shape)}, {tuple(nom.shape)}'
    assert nom.is_contiguous() and out.is_contiguous() and out.shape == nom.shape and out.dtype == torch.float32 and out.device == u.device
    B, T = u.shape[:2]
    dev = u.device
    d = _mppi_desc(B, T, lam=lam)
    nbytes = _lib.size_query('mf_mppi_scratch_bytes', d)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    weights = torch.empty(B, dtype=torch.float32, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    best, n_valid = flags[:1], flags[1:]
    _lib.launch('mf_mppi_update', dev, d, c, u, nom, weights, out, best, n_valid, scratch, C.c_longlong(nbytes), dtype=torch.float32,
                timer='mppi_update_kernel')
    return out, weights, best, n_valid


@torch.library.impl(_L, 'mppi_update', 'CUDA')
def _mppi_update(costs, controls, nominal, lam):
    nom = _f32(nominal, 'nominal').contiguous()
    return mppi_update_into(costs, controls, nom, lam, torch.empty_like(nom))


@torch.library.register_fake('monoforce::mppi_perturb', lib=_L)
def _mppi_perturb_fake(nominal, noise, sigma, lo, hi, keep_nominal):
    return noise.new_empty(noise.shape)


@torch.library.register_fake('monoforce::path_costs', lib=_L)
def _path_costs_fake(cost_rows, force_cost, x_last, goal, weights):
    B = cost_rows.shape[0]
    return cost_rows.new_empty(B), cost_rows.new_empty(B, 3)


@torch.library.register_fake('monoforce::mppi_update', lib=_L)
def _mppi_update_fake(costs, controls, nominal, lam):
    B = controls.shape[0]
    return (nominal.new_empty(nominal.shape), costs.new_empty(B), costs.new_empty(1, dtype=torch.int32), costs.new_empty(1, dtype=torch.int32))


# ---- planner costs from the kept poses -------------------------------------------------------------------------------------------
def footprint_points(dphysics):
    """The default footprint of the cost-map term: the DPhysics robot points [N,3], float32 on its device (cached on the module)."""
    key = ('footprint_f32', str(dphysics.device))
    if key not in dphysics._cache:
        dphysics._cache[key] = dphysics.dphys_cfg.robot_points.detach().to(device=dphysics.device, dtype=torch.float32).reshape(-1, 3).contiguous()
    return dphysics._cache[key]


def pose_costs_into(Xs, Rs, points, cost_map, path, base_costs, grid_res, d_max, lethal, off_map, weights, out):
    """`torch.ops.monoforce.pose_costs` writing the costs into `out` [B] (which may be `base_costs` itself); returns (out, terms)."""
    x, r = _f32(Xs, 'Xs'), _f32(Rs, 'Rs')
    assert x.dim() == 3 and x.shape[2] == 3 and tuple(r.shape) == (x.shape[0], x.shape[1], 3, 3), \
        f'Xs must be [B,Tp,3] and Rs [B,Tp,3,3], got {tuple(x.shape)} and {tuple(r.shape)}'
    B, Tp = x.shape[:2]
    if x.stride(2) != 1:
        x = x.contiguous()
    if r.stride(3) != 1 or r.stride(2) != 3:
        r = r.contiguous()
    pts = _f32(points, 'points').contiguous()
    assert pts.dim() == 2 and pts.shape[1] == 3, f'points must be [N,3], got {tuple(pts.shape)}'
    assert len(weights) == 2, 'weights = (map, path)'
    cm = None if cost_map is None else _f32(cost_map, 'cost_map').contiguous()
    assert cm is None or cm.dim() == 2, 'cost_map must be [H,W]'
    pa = None if path is None else _f32(path, 'path').contiguous()
    assert pa is None or (pa.dim() == 2 and pa.shape[1] == 2), 'path must be [P,2]'
    base = None if base_costs is None else _f32(base_costs, 'base_costs')
    assert base is None or (tuple(base.shape) == (B,) and base.is_contiguous()), 'base_costs must be a dense [B]'
    assert tuple(out.shape) == (B,) and out.is_contiguous() and out.dtype == torch.float32 and out.device == x.device
    H, W = (2, 2) if cm is None else cm.shape
    d = _lib.MfPoseCostDesc(B=B, Tp=Tp, N=pts.shape[0], P=0 if pa is None else pa.shape[0], H=H, W=W,
                            x_stride_b=x.stride(0), x_stride_t=x.stride(1), r_stride_b=r.stride(0), r_stride_t=r.stride(1),
                            grid_res=float(grid_res), d_max=float(d_max), lethal=float(lethal), off_map=float(off_map),
                            w_map=float(weights[0]), w_path=float(weights[1]))
    terms = torch.empty(B, 2, dtype=torch.float32, device=x.device)
    _lib.launch('mf_pose_costs', x.device, d, x, r, pts, cm, pa, base, out, terms, dtype=torch.float32, timer='pose_costs_kernel')
    return out, terms


@torch.library.impl(_L, 'pose_costs', 'CUDA')
def _pose_costs(Xs, Rs, points, cost_map, path, base_costs, grid_res, d_max, lethal, off_map, weights):
    return pose_costs_into(Xs, Rs, points, cost_map, path, base_costs, grid_res, d_max, lethal, off_map, weights,
                           torch.empty(Xs.shape[0], dtype=torch.float32, device=Xs.device))


@torch.library.register_fake('monoforce::pose_costs', lib=_L)
def _pose_costs_fake(Xs, Rs, points, cost_map, path, base_costs, grid_res, d_max, lethal, off_map, weights):
    B = Xs.shape[0]
    return Xs.new_empty(B), Xs.new_empty(B, 2)


# ---- the planner's cost with its gradient (monoforce_amd/refine.py) ----------------------------------------------------------------------
@torch.library.impl(_L, 'traj_objective', 'CUDA')
def _traj_objective(Xs, Rs, goal, points, cost_map, path, weights, pose_stride, grid_res, d_max, lethal, off_map):
    return _refine.objective_launch(Xs, Rs, goal, points, cost_map, path, weights, pose_stride, grid_res, d_max, lethal, off_map)


def _traj_objective_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2], output[3])
    ctx.set_materialize_grads(False)


def _traj_objective_backward(ctx, gcosts, _gterms, _ggXs, _ggRs):
    none = (None,) * 12
    if gcosts is None:
        return none
    gXs, gRs = ctx.saved_tensors
    return (_refine._scaled(gXs, gcosts), _refine._scaled(gRs, gcosts)) + none[2:]


torch.library.register_autograd('monoforce::traj_objective', _traj_objective_backward, setup_context=_traj_objective_setup, lib=_L)


@torch.library.register_fake('monoforce::traj_objective', lib=_L)
def _traj_objective_fake(Xs, Rs, goal, points, cost_map, path, weights, pose_stride, grid_res, d_max, lethal, off_map):
    B = Xs.shape[0]
    return Xs.new_empty(B), Xs.new_empty(B, 4), torch.empty_like(Xs), torch.empty_like(Rs)


# ---- height-map losses ---------------------------------------------------------------------------------------------------------------
def _map_loss_input(ok, what):
    if not ok:
        raise TypeError(f'monoforce::{what}: float32 / float64 map tensors [...,H,W] of one dtype on one GPU, below 2^31 cells, are expected '
                        '(monoforce_amd.losses has the ATen forms for everything else)')


@torch.library.impl(_L, 'hm_loss', 'CUDA')
def _hm_loss(height_pred, height_gt, weights, h_max):
    _map_loss_input(height_pred.shape == height_gt.shape and (weights is None or weights.shape == height_gt.shape)
                    and _losses._hm_loss_takes_the_hip_route(height_pred, height_gt.detach(), None if weights is None else weights.detach(), h_max),
                    'hm_loss')
    loss, n_valid, _ = _losses.hm_loss_forward(height_pred, height_gt, weights, h_max)
    return loss, n_valid


def _hm_loss_setup(ctx, inputs, output):
    height_pred, height_gt, weights, h_max = inputs
    ctx.h_max, ctx.has_w = h_max, weights is not None
    ctx.save_for_backward(height_pred, height_gt, output[1], *(() if weights is None else (weights,)))
    ctx.set_materialize_grads(False)


def _hm_loss_backward(ctx, gloss, _g_n_valid):
    if gloss is None or not ctx.needs_input_grad[0]:
        return None, None, None, None
    pred, gt, n_valid = ctx.saved_tensors[:3]
    state = _losses.hm_loss_state(pred.detach(), gt.detach(), ctx.saved_tensors[3].detach() if ctx.has_w else None, ctx.h_max)
    return _losses.hm_loss_grad(state, n_valid, gloss, pred.shape), None, None, None


torch.library.register_autograd('monoforce::hm_loss', _hm_loss_backward, setup_context=_hm_loss_setup, lib=_L)


@torch.library.register_fake('monoforce::hm_loss', lib=_L)
def _hm_loss_fake(height_pred, height_gt, weights, h_max):
    return height_pred.new_empty(()), height_pred.new_empty(1, dtype=torch.int32)


@torch.library.impl(_L, 'total_variation', 'CUDA')
def _total_variation(heightmap):
    _map_loss_input(_losses._map_dtype_ok(heightmap), 'total_variation')
    return _losses.total_variation_forward(heightmap)[0]


def _total_variation_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])
    ctx.set_materialize_grads(False)


def _total_variation_backward(ctx, gloss):
    if gloss is None:
        return None
    z, = ctx.saved_tensors
    return _losses.total_variation_grad(_losses.total_variation_state(z.detach()), gloss, z.shape)


torch.library.register_autograd('monoforce::total_variation', _total_variation_backward, setup_context=_total_variation_setup, lib=_L)


@torch.library.register_fake('monoforce::total_variation', lib=_L)
def _total_variation_fake(heightmap):
    return heightmap.new_empty(())


# ---- planner cost maps from terrain (monoforce_amd/costmap.py) ------------------------------------------------------------------------------
traversability_into = _costmap.traversability_into      # the op writing caller-owned `cost` / `terms` buffers


def _terms_shape(z):
    return tuple(z.shape[:-2]) + (3,) + tuple(z.shape[-2:])


@torch.library.impl(_L, 'traversability', 'CUDA')
def _traversability(z, valid, base, grid_res, radius_cells, lo, hi, unknown, min_valid, return_terms):
    cost = torch.empty(z.shape, dtype=z.dtype, device=z.device)
    terms = torch.empty(_terms_shape(z), dtype=z.dtype, device=z.device) if return_terms else None
    _costmap.traversability_into(z.detach(), valid, base, grid_res, radius_cells, list(lo), list(hi), unknown, min_valid, cost, terms)
    return cost, (terms if return_terms else torch.empty(0, dtype=z.dtype, device=z.device))


@torch.library.register_fake('monoforce::traversability', lib=_L)
def _traversability_fake(z, valid, base, grid_res, radius_cells, lo, hi, unknown, min_valid, return_terms):
    return z.new_empty(z.shape), z.new_empty(_terms_shape(z) if return_terms else (0,))


# ---- global routes on a cost map (monoforce_amd/route.py) ------------------------------------------------------------------------------------
@torch.library.impl(_L, 'cost_to_go', 'CUDA')
def _cost_to_go(cost_map, goal, grid_res, d_max, lethal, alpha, n_rounds):
    return _route.cost_to_go(cost_map, goal, grid_res, d_max, lethal, alpha, n_rounds if n_rounds > 0 else None, return_status=True)


@torch.library.register_fake('monoforce::cost_to_go', lib=_L)
def _cost_to_go_fake(cost_map, goal, grid_res, d_max, lethal, alpha, n_rounds):
    S = cost_map.shape[0] if cost_map.dim() == 3 else 1
    return cost_map.new_empty(cost_map.shape), cost_map.new_empty((S,), dtype=torch.int32), cost_map.new_empty((S,), dtype=torch.int32)


@torch.library.impl(_L, 'extract_route', 'CUDA')
def _extract_route(field, cost_map, start, goal, grid_res, d_max, lethal, alpha, n_vertices, max_nodes):
    out = _route.extract_route(field, cost_map, start, goal, grid_res, d_max, lethal, alpha, n_vertices, max_nodes if max_nodes > 0 else None)
    path = out['path'] if cost_map.dim() == 3 else out['path'][None]
    return path, out['nodes'], out['n_nodes'], out['route_cost'], out['status']


@torch.library.register_fake('monoforce::extract_route', lib=_L)
def _extract_route_fake(field, cost_map, start, goal, grid_res, d_max, lethal, alpha, n_vertices, max_nodes):
    S = cost_map.shape[0] if cost_map.dim() == 3 else 1
    n = max_nodes if max_nodes > 0 else cost_map.shape[-2] * cost_map.shape[-1]
    i32 = dict(dtype=torch.int32)
    return (cost_map.new_empty((S, n_vertices, 2), dtype=torch.float32), cost_map.new_empty((S, n), **i32), cost_map.new_empty((S,), **i32),
            cost_map.new_empty((S,)), cost_map.new_empty((S,), **i32))


# ---- functional entries ------------------------------------------------------------------------------------------------------
def rollout(dphysics, z_grid, controls, state, friction=None):
    """`DPhysics.forward` through `torch.ops.monoforce.dphys_rollout_fwd` for a rigid body and a given start state:
    returns ((Xs, Xds, Rs, Omegas), (F_springs, F_frictions)); differentiable w.r.t. the maps, controls and start state."""
    cfg = dphysics.dphys_cfg
    dev, dt = z_grid.device, z_grid.dtype
    x0, xd0, R0, w0 = state
    consts = [float(cfg.robot_mass), float(cfg.gravity), float(dphysics.stiffness), float(dphysics.damping), float(cfg.grid_res),
              float(cfg.d_max), float(cfg.dt), float(cfg.omega_max), float(cfg.robot_size[1]), float(dphysics._ts_T)]
    pts = dphysics._points_dev(dev, dt)
    Iinv = torch.tensor(dphysics._iinv(dt), dtype=torch.float64).view(3, 3)
    need = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (z_grid, friction, controls, x0, xd0, R0, w0))
    outs = torch.ops.monoforce.dphys_rollout_fwd(z_grid, friction, controls, x0, xd0, R0, w0, pts, dphysics._part_dev(dev), Iinv, consts,
                                                 1 if cfg.use_odeint else 0, need)
    with torch.no_grad():
        x0.data[..., 2] = outs[7][..., 2].to(x0.dtype)       # the reference's in-place terrain snap of the caller's start position
    return tuple(outs[:4]), tuple(outs[4:6])


def splat(geom, x, dx, bx, nx):
    """`LiftSplatShoot.voxel_pooling(geom, x)` through `torch.ops.monoforce.bev_splat_*` (plan built per call)."""
    B = geom.shape[0]
    dxl, bxl, nxl = [float(v) for v in dx], [float(v) for v in bx], [int(v) for v in nx]
    plan = torch.ops.monoforce.bev_splat_plan(geom, dxl, bxl, nxl)
    n = geom.numel() // 3 // B
    return torch.ops.monoforce.bev_splat_fwd(x, plan, B, n, dxl, bxl, nxl)
