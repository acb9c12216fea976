"""Gradient descent on control sequences through the differentiable rollout, with nothing left on the host: `ControlRefiner`.

The two planners sample (`TrajectoryShooter` scores constant (v, w) samples, `MPPIPlanner` perturbs and averages); neither uses
dL/dcontrols, which the rollout's backward delivers for a fraction of a millisecond.  This module is the descent: the planner's cost as one
differentiable objective over the outputs of `DPhysics.forward` (`trajectory_objective`: cost map under the footprint, distance to a path,
distance to the goal, inclination -- value AND gradient in one launch, csrc/traj_objective.hip), and Adam on the K sequences with
per-sequence best-so-far bookkeeping in one more launch (csrc/control_refine.hip); in graph mode the rollout's launches and these two
replay as ONE hipGraph per iteration and the host never waits for the device.

`mf_traj_objective_f32` and `mf_control_refine_update_f32` are marshalled here and nowhere else (`objective_launch`, `update`).
"""
import math
import warnings

import torch

from . import _lib
from .capture import capture

__all__ = ['ControlRefiner', 'trajectory_objective', 'trajectory_objective_aten', 'objective_launch', 'update', 'new_state', 'refine_desc', 'kept_steps', 'same_layout']

INF = float('inf')
TERM_NAMES = ('map', 'path', 'goal', 'inclination')        # the order of `terms` [B,4] and of the four weights of the C ABI


def kept_steps(T, pose_stride):
    """The steps the objective scores, by the rule of `DPhysics.rollout_costs`: t_p = min(p * pose_stride, T - 1), p < 1 + ceil((T-1) / pose_stride)."""
    ps = int(pose_stride)
    if ps < 1:
        raise ValueError(f'pose_stride must be at least 1, got {pose_stride}')
    Tp = 1 + (int(T) - 1 + ps - 1) // ps
    return [min(p * ps, int(T) - 1) for p in range(Tp)]


def _weights4(weights):
    """dict(map, path, goal, inclination) (missing: 0) or a sequence in that order -> a tuple of four floats."""
    if isinstance(weights, dict):
        unknown = set(weights) - set(TERM_NAMES)
        if unknown:
            raise ValueError(f'unknown cost weights {sorted(unknown)}: {", ".join(TERM_NAMES)}')
        return tuple(float(weights.get(k, 0.0)) for k in TERM_NAMES)
    w = tuple(float(v) for v in weights)
    if len(w) != 4:
        raise ValueError(f'weights = ({", ".join(TERM_NAMES)})')
    return w


def _check_shapes(Xs, Rs, points, cost_map, path, w):
    if Xs.dim() != 3 or Xs.shape[2] != 3 or tuple(Rs.shape) != (Xs.shape[0], Xs.shape[1], 3, 3):
        raise ValueError(f'Xs must be [B,T,3] and Rs [B,T,3,3], got {tuple(Xs.shape)} and {tuple(Rs.shape)}')
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f'points must be [N,3], got {tuple(points.shape)}')
    if cost_map is not None and cost_map.dim() != 2:
        raise ValueError('cost_map must be [H,W]')
    if path is not None and (path.dim() != 2 or path.shape[1] != 2 or path.shape[0] < 1):
        raise ValueError('path must be [P,2] with P >= 1')
    if cost_map is None and w[0] != 0:
        raise ValueError('the map weight needs a cost_map')
    if path is None and w[1] != 0:
        raise ValueError('the path weight needs a path')


# ---- the ATen form: the fallback (CPU tensors, float64), the benchmark's other leg, the tests' float32 comparator ------------------------------
def _safe_norm(v):
    """|v| over the last axis with derivative 0 at 0 (torch.sqrt's is inf there)."""
    n2 = (v * v).sum(-1)
    pos = n2 > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, n2, torch.ones_like(n2))), n2)       # (n2 itself: 0, or the NaN of a NaN input)


def trajectory_objective_aten(Xs, Rs, goal, *, points, cost_map=None, path=None, weights, pose_stride, grid_res, d_max, lethal=INF, off_map=INF):
    """`trajectory_objective` as a plain-torch composition of the same formulas (include/monoforce_hip.h at MfTrajObjDesc), in the dtype of
    `Xs`, differentiable by autograd with the documented rules: the first maximum and the first nearest segment on a tie (`torch.max` /
    `torch.min` over an axis hand out the first index), derivative 0 at 0 for |.| and for a zero path or goal distance, zero gradient for an
    off-map sample and a clamped pitch; a lethal rollout costs +inf and keeps the gradient of its finite map term.  Returns (costs [B],
    terms [B,4]); `terms` carries no gradient."""
    w = _weights4(weights)
    _check_shapes(Xs, Rs, points, cost_map, path, w)
    dt, dev = Xs.dtype, Xs.device
    B, T = Xs.shape[:2]
    steps = torch.tensor(kept_steps(T, pose_stride), device=dev)
    Tp = steps.numel()
    X, R = Xs.index_select(1, steps), Rs.index_select(1, steps)
    xy = X[..., :2]
    zero = torch.zeros(B, dtype=dt, device=dev)
    mp, mp_g, xt, lethal_b = zero, zero, zero, torch.zeros(B, dtype=torch.bool, device=dev)
    if cost_map is not None:
        H, W = cost_map.shape
        m = cost_map.to(dt)
        q = xy[..., None, :] + torch.einsum('bpij,nj->bpni', R[..., :2, :], points.to(dt))
        u, v = (q[..., 0] + d_max) / grid_res, (q[..., 1] + d_max) / grid_res
        on = (u >= 0) & (u <= H - 1) & (v >= 0) & (v <= W - 1)
        u, v = torch.where(on, u, torch.zeros_like(u)), torch.where(on, v, torch.zeros_like(v))
        ix, iy = torch.clamp(torch.floor(u.detach()).long(), max=H - 2), torch.clamp(torch.floor(v.detach()).long(), max=W - 2)
        fx, fy = u - ix.to(dt), v - iy.to(dt)
        s = (1 - fx) * (1 - fy) * m[ix, iy] + fx * (1 - fy) * m[ix + 1, iy] + (1 - fx) * fy * m[ix, iy + 1] + fx * fy * m[ix + 1, iy + 1]
        s = torch.where(on, s, torch.full_like(s, off_map))
        lethal_b = (~(s.detach() < lethal)).flatten(1).any(dim=1)
        f = s.max(dim=-1).values                                                          # [B,Tp]
        mp = torch.where(lethal_b, torch.full_like(zero, INF), f.detach().sum(-1) / Tp)
        mp_g = torch.where(torch.isfinite(f.detach()), f, torch.zeros_like(f)).sum(-1) / Tp     # what carries the map term's gradient: always finite
    if path is not None:
        pa = path.to(dt)
        a, b = (pa[:-1], pa[1:]) if pa.shape[0] > 1 else (pa, pa)
        ab, ap = b - a, xy[..., None, :] - a
        len2 = (ab * ab).sum(-1)
        pos = len2 > 0
        t = torch.where(pos, torch.clamp((ap * ab).sum(-1) / torch.where(pos, len2, torch.ones_like(len2)), 0.0, 1.0), torch.zeros_like(len2))
        off = ap - t[..., None] * ab                                                      # [B,Tp,S,2]
        d2 = (off * off).sum(-1)
        k = d2.detach().min(dim=-1).indices
        nearest = torch.gather(off, 2, k[..., None, None].expand(-1, -1, 1, 2)).squeeze(2)
        dist = _safe_norm(nearest)
        dist = torch.where(torch.isnan(d2.detach()).any(-1), torch.full_like(dist, math.nan), dist)      # a NaN position gives a NaN term
        xt = dist.sum(-1) / Tp
    gl = _safe_norm(Xs[:, T - 1, :2] - goal.to(dt).reshape(2))
    r = R[..., 2, :]
    h = r / torch.sqrt((r * r).sum(-1, keepdim=True))
    roll = torch.atan2(h[..., 1], h[..., 2])
    sp = -h[..., 0]
    open_ = (sp > -1) & (sp < 1)
    pitch = torch.asin(torch.where(open_, sp, torch.clamp(sp.detach(), -1.0, 1.0)))
    incl = (roll.abs() + pitch.abs()).sum(-1) / Tp
    rest = w[2] * gl + w[3] * incl
    if path is not None:
        rest = w[1] * xt + rest
    value = rest.detach()
    carrier = rest
    if cost_map is not None:
        value = torch.where(lethal_b, torch.full_like(zero, INF), w[0] * mp) + value
        carrier = w[0] * mp_g + carrier
    costs = value + (carrier - carrier.detach())           # the value as documented, the gradient of the finite expression
    return costs, torch.stack([mp, xt.detach(), gl.detach(), incl.detach()], dim=-1)


# ---- the HIP route ------------------------------------------------------------------------------------------------------------------------
def _f32_dev(t, name):
    _lib.require_hip_tensor(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f'the trajectory objective kernel computes in float32, {name} is {t.dtype}')
    return t


def same_layout(a, b):
    """Equal shapes, and equal strides on every axis longer than one (the stride of an axis of length 1 addresses nothing)."""
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


def _dense_like(t):
    """An uninitialised tensor of t's shape AND strides, or None where t is not dense (a slice, an expand)."""
    e = torch.empty_like(t)
    return e if same_layout(e, t) else None


def _scaled(g, gc):
    """g * gc (gc [B], one factor per rollout) in g's own strides."""
    return torch.mul(g, gc.to(g.dtype).view((-1,) + (1,) * (g.dim() - 1)), out=torch.empty_like(g))


def objective_launch(Xs, Rs, goal, points, cost_map, path, weights, pose_stride, grid_res, d_max, lethal=INF, off_map=INF, gcosts=None,
                     want_grad=True):
    """One `mf_traj_objective_f32` launch on Xs's device and current stream (include/monoforce_hip.h): float32 device tensors, `Xs` [B,T,3]
    and `Rs` [B,T,3,3] read in place through their strides (unit inner strides), `weights` = (map, path, goal, inclination).  Returns
    (costs [B], terms [B,4], gXs, gRs): the gradients -- scaled by `gcosts` [B] where given -- in the strides of `Xs` / `Rs`, rows of steps
    that are not kept zeroed (None, None with `want_grad=False`)."""
    w = _weights4(weights)
    x, r = _f32_dev(Xs, 'Xs'), _f32_dev(Rs, 'Rs')
    _check_shapes(x, r, points, cost_map, path, w)
    B, T = x.shape[:2]
    gx = gr = None
    if want_grad:
        gx, gr = _dense_like(x), _dense_like(r)
    if x.stride(2) != 1 or (want_grad and gx is None):
        x = x.contiguous()
        gx = torch.empty_like(x) if want_grad else None
    if r.stride(3) != 1 or r.stride(2) != 3 or (want_grad and gr is None):
        r = r.contiguous()
        gr = torch.empty_like(r) if want_grad else None
    pts = _f32_dev(points, 'points').contiguous()
    g = _f32_dev(goal, 'goal').contiguous()
    if g.numel() != 2:
        raise ValueError('goal must hold (x, y)')
    cm = None if cost_map is None else _f32_dev(cost_map, 'cost_map').contiguous()
    pa = None if path is None else _f32_dev(path, 'path').contiguous()
    gc = None if gcosts is None else _f32_dev(gcosts, 'gcosts').contiguous()
    if gc is not None and tuple(gc.shape) != (B,):
        raise ValueError(f'gcosts must be [{B}], got {tuple(gc.shape)}')
    H, W = (2, 2) if cm is None else cm.shape
    d = _lib.MfTrajObjDesc(B=B, T=T, N=pts.shape[0], P=0 if pa is None else pa.shape[0], H=H, W=W, pose_stride=int(pose_stride),
                           x_stride_b=x.stride(0), x_stride_t=x.stride(1), r_stride_b=r.stride(0), r_stride_t=r.stride(1),
                           grid_res=float(grid_res), d_max=float(d_max), lethal=float(lethal), off_map=float(off_map),
                           w_map=w[0], w_path=w[1], w_goal=w[2], w_incl=w[3])
    costs = torch.empty(B, dtype=torch.float32, device=x.device)
    terms = torch.empty(B, 4, dtype=torch.float32, device=x.device)
    _lib.launch('mf_traj_objective', x.device, d, x, r, pts, cm, pa, g, gc, costs, terms, gx, gr, dtype=torch.float32, timer='traj_objective_kernel')
    return costs, terms, gx, gr


class _TrajObjective(torch.autograd.Function):
    """`mf_traj_objective_f32`: the value launch also forms dJ/dXs and dJ/dRs and stashes them (`grad_fn.grads`), in the strides of the inputs --
    for the rollout's time-major outputs: what `mf_rollout_bwd_*` takes without a copy; backward multiplies them by the upstream gradient."""

    @staticmethod
    def forward(ctx, Xs, Rs, goal, points, cost_map, path, w, pose_stride, grid_res, d_max, lethal, off_map):
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        costs, terms, gXs, gRs = objective_launch(Xs.detach(), Rs.detach(), goal.detach(), points, cost_map, path, w, pose_stride, grid_res, d_max,
                                                  lethal, off_map, want_grad=need)
        ctx.grads = (gXs, gRs)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return costs, terms

    @staticmethod
    def backward(ctx, gcosts, _gterms):
        none = (None,) * 12
        if gcosts is None:
            return none
        gXs, gRs = ctx.grads
        return (_scaled(gXs, gcosts) if ctx.needs_input_grad[0] else None, _scaled(gRs, gcosts) if ctx.needs_input_grad[1] else None) + none[2:]


def _takes_the_hip_route(Xs, Rs, goal, points, cost_map, path):
    ts = [t for t in (Xs, Rs, goal, points, cost_map, path) if t is not None]
    return (all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.device == Xs.device for t in ts)
            and Xs.dim() == 3 and Xs.stride(2) == 1 and Rs.dim() == 4 and Rs.stride(3) == 1 and Rs.stride(2) == 3)


def trajectory_objective(Xs, Rs, goal, *, points, cost_map=None, path=None, weights, pose_stride, grid_res, d_max, lethal=INF, off_map=INF):
    """The planner's cost of B rollouts from the outputs of `DPhysics.forward`, differentiable in `Xs` [B,T,3] and `Rs` [B,T,3,3]:

        J[b] = w_map mean_p max_n s(b,p,n) + w_path mean_p d(b,p) + w_goal |Xs[b,T-1,0:2] - goal| + w_inclination mean_p (|roll| + |pitch|)

    over the kept steps `kept_steps(T, pose_stride)` -- `s` the bilinear sample of `cost_map` [H,W] under footprint point n of `points`
    [N,3], `d` the distance to the polyline `path` [P,2] (both exactly `torch.ops.monoforce.pose_costs`' terms), roll and pitch from the
    normalised third row of R; any sample not below `lethal` makes J[b] = +inf.  `weights`: dict(map, path, goal, inclination).  Returns
    (costs [B], terms [B,4] = (map, path, goal, inclination), no gradient).  Formulas and gradient rules: include/monoforce_hip.h at
    MfTrajObjDesc.  float32 device tensors with unit inner strides take ONE HIP launch for value and gradient (the rollout's time-major
    views are read in place, the gradients come back in their strides); everything else -- CPU tensors, float64 -- goes to
    `trajectory_objective_aten`."""
    w = _weights4(weights)
    if not _takes_the_hip_route(Xs, Rs, goal, points, cost_map, path):
        return trajectory_objective_aten(Xs, Rs, goal, points=points, cost_map=cost_map, path=path, weights=w, pose_stride=pose_stride,
                                         grid_res=grid_res, d_max=d_max, lethal=lethal, off_map=off_map)
    return _TrajObjective.apply(Xs, Rs, goal, points, cost_map, path, w, int(pose_stride), float(grid_res), float(d_max), float(lethal), float(off_map))


# ---- the update launch ----------------------------------------------------------------------------------------------------------------------
def new_state(K, max_iters, device):
    """Fresh device state of a refinement: (state int32 [2] = step, ticket; best_cost [K] = +inf; best_iter int32 [K] = -1;
    history [max_iters,K] = NaN)."""
    return (torch.zeros(2, dtype=torch.int32, device=device), torch.full((K,), INF, dtype=torch.float32, device=device),
            torch.full((K,), -1, dtype=torch.int32, device=device), torch.full((max_iters, K), math.nan, dtype=torch.float32, device=device))


def refine_desc(K, T, max_iters, lr, betas, eps, lo, hi):
    f2, d2 = _lib.C.c_float * 2, _lib.C.c_double * 2
    return _lib.MfRefineDesc(K=int(K), T=int(T), max_iters=int(max_iters), lr=d2(float(lr[0]), float(lr[1])), beta1=float(betas[0]),
                             beta2=float(betas[1]), eps=float(eps), lo=f2(float(lo[0]), float(lo[1])), hi=f2(float(hi[0]), float(hi[1])))


def update(desc, controls, grad, costs, m, v, best_controls, best_cost, best_iter, history, state):
    """One `mf_control_refine_update_f32` launch on the controls' device and current stream (include/monoforce_hip.h): history, the
    per-sequence snapshot of the controls BEFORE the update on a strict improvement, Adam on every sequence whose cost is not NaN and whose
    gradient row is finite, the clamp.  Contiguous float32 tensors [K,T,2] / [K] / [max_iters,K]; `best_iter` int32 [K], `state` int32 [2].
    Writes through raw pointers: tensor versions are the caller's business."""
    _lib.require_hip_tensor(controls, 'controls')
    for name, t in (('controls', controls), ('grad', grad), ('m', m), ('v', v), ('best_controls', best_controls)):
        if t.dtype != torch.float32 or tuple(t.shape) != (desc.K, desc.T, 2) or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous float32 [{desc.K},{desc.T},2], got {t.dtype} {tuple(t.shape)}')
    for name, t, dt, shape in (('costs', costs, torch.float32, (desc.K,)), ('best_cost', best_cost, torch.float32, (desc.K,)),
                               ('best_iter', best_iter, torch.int32, (desc.K,)), ('state', state, torch.int32, (2,)),
                               ('history', history, torch.float32, (desc.max_iters, desc.K))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous {dt} {list(shape)}, got {t.dtype} {tuple(t.shape)}')
    _lib.launch('mf_control_refine_update', controls.device, desc, controls, grad, costs, m, v, best_controls, best_cost, best_iter,
                history if history.numel() else None, state, dtype=torch.float32, timer='control_refine_kernel')


class ControlRefiner:
    """Adam on K control sequences through the differentiable rollout, on the GPU: `step(...)` = one iteration of (rollout forward through
    the autograd route, `trajectory_objective`, `torch.autograd.grad(costs.sum(), controls)`, one update launch), `run(n, ...)` = n of
    them, neither with a host synchronisation.

        ref = ControlRefiner.from_mppi(planner, out, 8)             # the new nominal and the 7 cheapest samples of the last MPPI step
        res = ref.run(20, z_grid, goal, cost_map=cm)                # res['best_controls'][res['best']]: the sequence to drive

    The refiner owns `controls` ([K,T,2] float32, a leaf cloned from `controls0`), Adam's moments, the snapshots `best_controls` and the
    device state: `best_cost` [K] (+inf before any improvement), `best_iter` [K] (-1), `history` [max_iters,K] (NaN) and the device's own
    step count.  The cost of iteration i is the cost at the controls BEFORE update i; a sequence improves iff `cost < best_cost` (strict: a
    NaN or +inf never does) and the snapshot then taken holds the controls before the update -- the controls the cost belongs to.  A
    sequence whose cost is NaN or whose gradient has a non-finite entry is left untouched in that iteration, moments included; a lethal
    sequence (cost +inf) still descends on the gradient of its finite terms.  Adam is `torch.optim.Adam`'s default single-tensor step with
    `lr = (lr_v, lr_w)`; behind it the controls are clamped to +-cfg.vel_max / +-cfg.omega_max.

    `weights`: dict(goal, map, path, inclination) (default: the goal alone); `lethal`, `off_map`, `footprint`, `pose_stride` as
    `MPPIPlanner`.  `goal` [2], `cost_map` [H,W] and `path` [P,2] are DEVICE tensors the launches read (`goal.copy_(...)` moves a captured
    iteration's goal).  `graph=True`: the iteration is captured once, on one stream, into one hipGraph and replayed (captured again when a
    call hands in other tensors); a capture the runtime refuses falls back to launch by launch with a warning.  The update kernel writes
    `controls` through a raw pointer; its version counter is bumped after every `step()` and once after every `run()`."""

    def __init__(self, dphysics, controls0, *, weights=None, lr=(0.05, 0.1), betas=(0.9, 0.999), eps=1e-8, pose_stride=None, lethal=INF,
                 off_map=INF, footprint=None, max_iters=100, graph=True):
        if dphysics.precise or dphysics.contiguous_outputs:
            raise ValueError('ControlRefiner uses the float32 fast-math rollout with time-major outputs: construct DPhysics(precise=False, contiguous_outputs=False)')
        if controls0.dim() != 3 or controls0.shape[2] != 2:
            raise ValueError(f'controls0 must be [K,T,2], got {tuple(controls0.shape)}')
        self.dp = dphysics
        self.cfg = cfg = dphysics.dphys_cfg
        self.device = torch.device(dphysics.device)
        K, T = controls0.shape[:2]
        if T > int(cfg.traj_sim_time / cfg.dt):
            raise ValueError(f'{T} steps exceed the rollout horizon of {int(cfg.traj_sim_time / cfg.dt)}')
        w = dict(goal=1.0, map=0.0, path=0.0, inclination=0.0)
        if weights is not None:
            if 'force' in weights and float(weights['force']) != 0:
                raise ValueError('the force cost has no gradient here: ControlRefiner takes goal, map, path and inclination weights only')
            weights = {k: v for k, v in weights.items() if k != 'force'}
            _weights4(weights)
            w.update(weights)
        self.weights = _weights4(w)
        beta1, beta2 = (float(b) for b in betas)
        max_iters = int(max_iters)
        if float(lr[0]) < 0 or float(lr[1]) < 0 or not (0 <= beta1 < 1 and 0 <= beta2 < 1) or not eps > 0 or max_iters < 0:
            raise ValueError(f'need lr >= 0, betas in [0, 1), eps > 0, max_iters >= 0; got lr={lr}, betas={betas}, eps={eps}, max_iters={max_iters}')
        self.lo = (-float(cfg.vel_max), -float(cfg.omega_max))
        self.hi = (float(cfg.vel_max), float(cfg.omega_max))
        self.desc = refine_desc(K, T, max_iters, lr, (beta1, beta2), eps, self.lo, self.hi)
        self.pose_stride = pose_stride
        self.lethal, self.off_map = float(lethal), float(off_map)
        if footprint is None:
            from . import ops
            self.footprint = ops.footprint_points(dphysics)
        else:
            self.footprint = torch.as_tensor(footprint).detach().to(device=self.device, dtype=torch.float32).reshape(-1, 3).contiguous()
        self.max_iters = max_iters
        self.graph = bool(graph)
        self.iteration = 0          # iterations launched so far (host side; the device keeps its own count)
        self.controls = controls0.detach().to(device=self.device, dtype=torch.float32).clone().contiguous().requires_grad_(True)
        self.m, self.v = torch.zeros_like(self.controls.detach()), torch.zeros_like(self.controls.detach())
        self.best_controls = self.controls.detach().clone()
        self.state, self.best_cost, self.best_iter, self.history = new_state(K, max_iters, self.device)
        self.terms = None           # [K,4] of the last iteration
        self._captured = None

    @classmethod
    def from_mppi(cls, planner, out, k, **kw):
        """A refiner seeded from the result `out` of the last `planner.step(...)`: row 0 is the new nominal, rows 1 .. k-1 the k - 1 sampled
        sequences of lowest finite cost (`torch.topk` on the device, cheapest first; with fewer than k - 1 finite costs -- `out['n_valid']` --
        the remaining rows are non-finite samples), with the planner's weights, footprint, pose stride, `lethal` and `off_map`.  The force cost
        has no gradient here: a planner with a non-zero `force` weight is refused."""
        w_incl, w_force, w_goal = planner.weights
        if w_force != 0:
            raise ValueError(f'the force cost has no gradient here: the planner weighs it with {w_force}; refine with a planner whose force weight is 0')
        k = int(k)
        controls, costs = out['controls'], out['costs']
        if not 1 <= k <= controls.shape[0] + 1:
            raise ValueError(f'k must be in [1, {controls.shape[0] + 1}], got {k}')
        seeds = [out['nominal'].detach().unsqueeze(0)]
        if k > 1:
            ranked = torch.where(torch.isfinite(costs), costs, torch.full_like(costs, INF))
            seeds.append(controls.detach()[torch.topk(ranked, k - 1, largest=False, sorted=True).indices])
        w_map, w_path = planner.pose_weights
        return cls(planner.dp, torch.cat(seeds), weights=dict(goal=w_goal, map=w_map, path=w_path, inclination=w_incl), pose_stride=planner.pose_stride,
                   lethal=planner.lethal, off_map=planner.off_map, footprint=planner.footprint, **kw)

    # -- state ---------------------------------------------------------------------------------------------------------------------
    @property
    def device_step(self):
        """0-d int32 device view of the device's own iteration count."""
        return self.state[0]

    def _everything(self):
        return (self.controls.detach(), self.m, self.v, self.best_controls, self.state, self.best_cost, self.best_iter, self.history)

    def reset(self, controls0=None):
        """Back to the start: moments, step, `best_cost`, `best_iter` and the history; the controls to `controls0` where given, else kept
        (the snapshots follow the controls).  In place: a captured graph stays valid.  No host synchronisation."""
        with torch.no_grad():
            if controls0 is not None:
                self.controls.copy_(controls0)
            self.m.zero_()
            self.v.zero_()
            self.best_controls.copy_(self.controls)
            self.state.zero_()
            self.best_cost.fill_(INF)
            self.best_iter.fill_(-1)
            self.history.fill_(math.nan)
        self.iteration = 0

    # -- one iteration ---------------------------------------------------------------------------------------------------------------
    def _check(self, z_grid, goal, cost_map, path):
        if z_grid.dtype != torch.float32:
            raise TypeError('ControlRefiner.step: float32 only')
        if not (torch.is_tensor(goal) and goal.is_cuda and goal.numel() == 2):
            raise TypeError('ControlRefiner.step: goal must be a device tensor [2]')
        for name, t, wt in (('cost_map', cost_map, self.weights[0]), ('path', path, self.weights[1])):
            if t is None and wt != 0:
                raise ValueError(f'ControlRefiner.step: the {name.split("_")[-1]} weight is {wt} but no {name} was given')
            if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
                raise TypeError(f'ControlRefiner.step: {name} must be a float32 device tensor')

    def _stride(self, scored):
        if self.pose_stride is not None:
            return int(self.pose_stride)
        cfg = self.cfg
        if scored:      # one kept pose per map cell at full speed (as MPPIPlanner)
            return max(int(float(cfg.grid_res) / (float(cfg.vel_max) * float(cfg.dt)) + 1e-9), 1)
        return max(int(0.5 / cfg.dt), 1)

    def _forward_backward(self, z_grid, goal, friction, pose0, cost_map, path):
        """(costs [K], terms [K,4], dcosts.sum()/dcontrols [K,T,2]) at the live controls."""
        dev, K = self.device, self.desc.K
        z = z_grid if z_grid.dim() == 3 else z_grid.unsqueeze(0)
        mu = None if friction is None else (friction if friction.dim() == 3 else friction.unsqueeze(0))
        state = None
        if pose0 is not None:       # as MPPIPlanner.step
            x = pose0[:3, 3].to(dev).repeat(K, 1)
            state = (x, torch.zeros_like(x), pose0[:3, :3].to(dev).repeat(K, 1, 1).contiguous(), torch.zeros_like(x))
        with torch.enable_grad():
            states, _ = self.dp(z, self.controls, state=state, friction=mu, _want_forces=False)
            costs, terms = trajectory_objective(states[0], states[2], goal, points=self.footprint, cost_map=cost_map, path=path, weights=self.weights,
                                                pose_stride=self._stride(cost_map is not None or path is not None), grid_res=self.cfg.grid_res,
                                                d_max=self.cfg.d_max, lethal=self.lethal, off_map=self.off_map)
            grad, = torch.autograd.grad(costs.sum(), self.controls)
        return costs.detach(), terms, grad

    def _update(self, costs, grad):
        update(self.desc, self.controls.detach(), grad.detach().contiguous(), costs, self.m, self.v, self.best_controls, self.best_cost,
               self.best_iter, self.history, self.state)

    def _iterate_eager(self, args):
        costs, terms, grad = self._forward_backward(*args)
        self._update(costs, grad)
        self.controls.grad, self.terms = grad, terms

    def _restore(self, snap):
        with torch.no_grad():
            for t, old in zip(self._everything(), snap):
                t.copy_(old)

    def _capture(self, args):
        dev = self.device
        snap = [t.clone() for t in self._everything()]

        def iterate():
            costs, terms, grad = self._forward_backward(*args)
            self._update(costs, grad)
            return terms, grad

        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        try:
            with torch.cuda.stream(s):      # warm-up on the capture stream (per-stream workspaces exist, both code objects are loaded) ...
                for _ in range(2):
                    iterate()
                self._restore(snap)         # ... which leaves no trace: controls, moments, snapshots and state as they were
            torch.cuda.current_stream(dev).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with capture(g, stream=s, capture_error_mode='thread_local'):      # ONE stream: the graph has no parallel branches
                terms, grad = iterate()
        except RuntimeError:
            torch.cuda.synchronize(dev)
            self._restore(snap)
            raise
        return dict(graph=g, terms=terms, grad=grad, key=self._key(args), keep=args)

    @staticmethod
    def _key(args):
        return tuple(None if t is None else (t.data_ptr(), tuple(t.shape), tuple(t.stride())) for t in args)

    def _iterate(self, args):
        if self.graph:
            if self._captured is None or self._captured['key'] != self._key(args):
                try:
                    self._captured = self._capture(args)
                except RuntimeError as e:       # a capture the runtime refuses: launch by launch, from the state the capture found
                    warnings.warn(f'ControlRefiner: hipGraph capture failed ({str(e).splitlines()[0][:120]}); running launch by launch')
                    self.graph = False
                    return self._iterate_eager(args)
            self._captured['graph'].replay()
            self.controls.grad, self.terms = self._captured['grad'], self._captured['terms']
            return
        self._iterate_eager(args)

    def _room(self, n):
        if n < 0 or self.iteration + n > self.max_iters:
            raise ValueError(f'{n} more iterations after {self.iteration} do not fit the history of max_iters={self.max_iters}')

    def step(self, z_grid, goal, friction=None, pose0=None, cost_map=None, path=None):
        """One iteration.  z_grid [H,W] (or [1,H,W]) float32, shared by the K rollouts; goal: DEVICE tensor [2]; pose0: optional 4x4 start
        pose shared by all sequences; cost_map [H,W] / path [P,2]: DEVICE tensors, required by a non-zero map / path weight.  Returns this
        iteration's costs [K] (a view of the history); no host synchronisation."""
        self._check(z_grid, goal, cost_map, path)
        self._room(1)
        self._iterate((z_grid, goal, friction, pose0, cost_map, path))
        torch.autograd.graph.increment_version(self.controls)
        self.iteration += 1
        return self.history[self.iteration - 1]

    def run(self, n, z_grid, goal, friction=None, pose0=None, cost_map=None, path=None):
        """`n` iterations without a host synchronisation.  Returns device tensors only: the live `controls`, the snapshots
        `best_controls` [K,T,2] with `best_cost` [K] and `best_iter` [K], `history` (this call's rows [n,K]) and `best`, the int64 index of
        the first minimum of `best_cost`."""
        n = int(n)
        self._check(z_grid, goal, cost_map, path)
        self._room(n)
        start = self.iteration
        args = (z_grid, goal, friction, pose0, cost_map, path)
        try:
            for _ in range(n):
                self._iterate(args)
                self.iteration += 1
        finally:
            torch.autograd.graph.increment_version(self.controls)
        return dict(controls=self.controls, best_controls=self.best_controls, best_cost=self.best_cost, best_iter=self.best_iter,
                    history=self.history[start:start + n], best=torch.argmin(self.best_cost))
