"""Planner cost maps from terrain: `traversability_map` / `TraversabilityMap` turn a height map (`bev['terrain']`, a fitted `z_best`, an
`estimate_heightmap` result) into the `cost_map=` that `MPPIPlanner`, `TrajectoryShooter` and `ControlRefiner` score rollouts on.

Per cell, over the usable cells of a disc of `r` cells around it: the slope of the least-squares plane (rise over run), the RMS of the
plane's residuals (roughness, metres) and max - min height (step, metres); each goes through a linear ramp `(lo, hi) -> (0, 1)`, the cost is
the largest of the three, `unknown` where the window holds fewer than `min_valid` usable cells or only collinear ones; an optional `base`
keep-out map is merged with `max`.  The full definition is the comment of `MfTraversabilityDesc` in include/monoforce_hip.h.

GPU tensors take ONE launch of monoforce_amd/csrc/traversability.hip (`mf_traversability_*`, marshalled here and nowhere else): the map is
read in place through its strides, nothing is allocated by the launch and the host reads nothing back, so a call sits in a hipGraph next to
the planner's launches.  `traversability_map_aten` is the same definition as a float32 ATen composition (`unfold`, masked sums): it runs on
any device, serves CPU tensors, and is the yardstick of tests and tools/bench_traversability.py.

NOT DIFFERENTIABLE: there is no backward.  Cost maps feed planners; gradients with respect to the terrain stop here (the outputs never
require grad)."""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib

__all__ = ['TILE', 'MAX_RADIUS_CELLS', 'DEFAULT_SLOPE', 'DEFAULT_ROUGHNESS', 'DEFAULT_STEP', 'traversability_map', 'traversability_map_aten',
           'traversability_into', 'TraversabilityMap']

TILE = _lib.MF_TRAVERSABILITY_TILE                      # edge of the tile of output cells one workgroup owns (MF_TRAVERSABILITY_TILE)
MAX_RADIUS_CELLS = _lib.MF_TRAVERSABILITY_MAX_RADIUS    # largest window radius, in cells
DEFAULT_SLOPE = (0.2, 0.6)          # rise over run: free below ~11 degrees, lethal from ~31 degrees
DEFAULT_ROUGHNESS = (0.02, 0.10)    # metres RMS about the fitted plane
DEFAULT_STEP = (0.10, 0.30)         # metres between the highest and the lowest cell of the window


def cells_of_radius(radius, grid_res):
    """The window radius in cells of a radius in metres: max(1, round(radius / grid_res)); beyond MAX_RADIUS_CELLS a ValueError."""
    r = max(1, int(round(float(radius) / float(grid_res))))
    if r > MAX_RADIUS_CELLS:
        raise ValueError(f'traversability: radius {radius} m is {r} cells of {grid_res} m; the window radius is limited to {MAX_RADIUS_CELLS} cells')
    return r


def _checked(z, valid, base, grid_res, r, lo, hi, min_valid):
    """Argument errors, the same for the kernel and the ATen form (raised before any device is touched)."""
    if z.dim() not in (2, 3):
        raise ValueError(f'traversability: z must be [H,W] or [S,H,W], got {tuple(z.shape)}')
    if not 1 <= int(r) <= MAX_RADIUS_CELLS:
        raise ValueError(f'traversability: the window radius must be 1..{MAX_RADIUS_CELLS} cells, got {r}')
    if int(min_valid) < 3:
        raise ValueError(f'traversability: min_valid must be at least 3 (a plane has three parameters), got {min_valid}')
    if not float(grid_res) > 0:
        raise ValueError(f'traversability: grid_res must be positive, got {grid_res}')
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError('traversability: three (lo, hi) pairs are expected: slope, roughness, step')
    for name, a, b in zip(('slope', 'roughness', 'step'), lo, hi):
        if not float(b) > float(a):
            raise ValueError(f'traversability: the {name} ramp needs hi > lo, got ({a}, {b})')
    for name, t in (('valid', valid), ('base', base)):
        if t is not None and tuple(t.shape) != tuple(z.shape):
            raise ValueError(f'traversability: {name} has shape {tuple(t.shape)}, z has {tuple(z.shape)}')
    for name, t in (('z', z), ('valid', valid), ('base', base)):
        if t is not None and t.shape[-1] != 1 and t.stride(-1) != 1:
            raise ValueError(f'traversability: {name} must have unit stride along W (it is read in place), got stride {t.stride(-1)}')


def _strides(t):
    """(stride_s, stride_h) in elements of an [H,W] or [S,H,W] map."""
    return (t.stride(0) if t.dim() == 3 else 0), t.stride(-2)


def traversability_into(z, valid, base, grid_res, r, lo, hi, unknown, min_valid, cost, terms=None):
    """The launch: `z` [H,W] or [S,H,W] on the GPU (float32 or float64, read in place through its strides), `r` in cells, `lo` / `hi` the
    three ramps; writes `cost` (the shape of z, contiguous) and, when given, `terms` ([3,H,W] or [S,3,H,W], contiguous).  Returns (cost, terms).
    No allocation, no host read."""
    _checked(z, valid, base, grid_res, r, lo, hi, min_valid)
    _lib.require_hip_tensor(z, 'z')
    _lib.scalar_suffix(z.dtype)
    S = z.shape[0] if z.dim() == 3 else 1
    H, W = z.shape[-2:]
    for name, t in (('valid', valid), ('base', base), ('cost', cost), ('terms', terms)):
        if t is not None and (t.dtype != z.dtype or t.device != z.device):
            raise TypeError(f'traversability: {name} is {t.dtype} on {t.device}, z is {z.dtype} on {z.device}')
    if tuple(cost.shape) != tuple(z.shape) or not cost.is_contiguous():
        raise ValueError(f'traversability: cost must be a contiguous {tuple(z.shape)} buffer, got {tuple(cost.shape)}')
    t_shape = tuple(z.shape[:-2]) + (3, H, W)
    if terms is not None and (tuple(terms.shape) != t_shape or not terms.is_contiguous()):
        raise ValueError(f'traversability: terms must be a contiguous {t_shape} buffer, got {tuple(terms.shape)}')
    f3 = lambda v: (C.c_float * 3)(*(float(x) for x in v))  # noqa: E731
    d = _lib.MfTraversabilityDesc(S=S, H=H, W=W, r=int(r), min_valid=int(min_valid), grid_res=float(grid_res), unknown=float(unknown),
                                  lo=f3(lo), hi=f3(hi))
    d.z_stride_s, d.z_stride_h = _strides(z)
    if valid is not None:
        d.v_stride_s, d.v_stride_h = _strides(valid)
    if base is not None:
        d.b_stride_s, d.b_stride_h = _strides(base)
    _lib.launch('mf_traversability', z.device, d, z, valid, base, cost, terms, dtype=z.dtype, timer='traversability_kernel')
    return cost, terms


_DISC = {}


def _disc(r, device):
    """(row index, column index) into a (2r+1)^2 window and the offsets (di, dj) of the K cells of the disc, int64 on `device`; built on
    the host once per (r, device) and kept, so that a later call can be captured into a hipGraph."""
    key = (int(r), str(device))
    if key not in _DISC:
        d = torch.arange(-r, r + 1)
        di, dj = torch.meshgrid(d, d, indexing='ij')
        inside = di * di + dj * dj <= r * r
        di, dj = di[inside], dj[inside]
        _DISC[key] = tuple(t.to(device) for t in (di + r, dj + r, di, dj))
    return _DISC[key]


def traversability_map_aten(z, grid_res, radius=None, slope=DEFAULT_SLOPE, roughness=DEFAULT_ROUGHNESS, step=DEFAULT_STEP, valid=None, base=None,
                            unknown=0.5, min_valid=3, return_terms=False, radius_cells=None):
    """`traversability_map` as a float32 ATen composition on z's device: the windows of every cell gathered into [S,H,W,K] (K cells of the
    disc), the integer rule in int64, the centred normal equations, the residuals.  Returns float32 `cost` (and `terms`).  After one call
    per (radius, device) it reads nothing on the host and can be captured into a hipGraph."""
    r = radius_cells if radius_cells is not None else cells_of_radius(radius, grid_res)
    lo, hi = [slope[0], roughness[0], step[0]], [slope[1], roughness[1], step[1]]
    _checked(z, valid, base, grid_res, r, lo, hi, min_valid)
    r = int(r)
    dev, f32 = z.device, torch.float32
    with torch.no_grad():
        x = (z if z.dim() == 3 else z[None]).to(f32)
        nan = torch.full((), float('nan'), dtype=f32, device=dev)
        ok = torch.isfinite(x)
        if valid is not None:
            ok = ok & ((valid if valid.dim() == 3 else valid[None]) != 0)
        x = torch.where(ok, x, nan)
        wi, wj, di, dj = _disc(r, dev)
        k = 2 * r + 1
        win = F.pad(x, (r, r, r, r), value=float('nan')).unfold(1, k, 1).unfold(2, k, 1)[..., wi, wj]      # [S,H,W,K]
        m = ~torch.isnan(win)
        ml = m.long()
        n, si, sj = ml.sum(-1), (ml * di).sum(-1), (ml * dj).sum(-1)
        A = n * (ml * (di * di)).sum(-1) - si * si
        B = n * (ml * (dj * dj)).sum(-1) - sj * sj
        Cc = n * (ml * (di * dj)).sum(-1) - si * sj
        known = (n >= int(min_valid)) & (A * B - Cc * Cc > 0)
        nf = n.clamp(min=1).to(f32)[..., None]
        mf = m.to(f32)
        g = torch.full((), float(grid_res), dtype=f32, device=dev)
        u, v = di.to(f32) * g, dj.to(f32) * g
        zero = torch.zeros((), dtype=f32, device=dev)
        du = (u - (mf * u).sum(-1, keepdim=True) / nf) * mf
        dv = (v - (mf * v).sum(-1, keepdim=True) / nf) * mf
        dz = torch.where(m, win - torch.where(m, win, zero).sum(-1, keepdim=True) / nf, zero)
        Suu, Svv, Suv = (du * du).sum(-1), (dv * dv).sum(-1), (du * dv).sum(-1)
        Suz, Svz = (du * dz).sum(-1), (dv * dz).sum(-1)
        det = torch.where(known, Suu * Svv - Suv * Suv, torch.ones((), dtype=f32, device=dev))
        a, b = (Svv * Suz - Suv * Svz) / det, (Suu * Svz - Suv * Suz) / det
        res = dz - a[..., None] * du - b[..., None] * dv
        inf = torch.full((), float('inf'), dtype=f32, device=dev)
        terms = torch.stack([torch.sqrt(a * a + b * b), torch.sqrt((res * res).sum(-1) / nf[..., 0]),
                             torch.where(m, win, -inf).amax(-1) - torch.where(m, win, inf).amin(-1)], dim=1)      # [S,3,H,W]
        terms = torch.where(known[:, None], terms, nan)
        lo_t = torch.stack([torch.full((), float(t), dtype=f32, device=dev) for t in lo]).view(1, 3, 1, 1)      # (fills, not host copies:
        hi_t = torch.stack([torch.full((), float(t), dtype=f32, device=dev) for t in hi]).view(1, 3, 1, 1)      #  capturable)
        ramp = ((terms - lo_t) / (hi_t - lo_t)).clamp(0.0, 1.0)
        cost = torch.where(known, ramp.amax(1), torch.full((), float(unknown), dtype=f32, device=dev))
        if base is not None:
            b3 = (base if base.dim() == 3 else base[None]).to(f32)
            cost = torch.where(torch.isnan(b3), cost, torch.maximum(cost, b3))
        if z.dim() == 2:
            cost, terms = cost[0], terms[0]
    return (cost, terms) if return_terms else cost


def traversability_map(z, grid_res, radius=None, slope=DEFAULT_SLOPE, roughness=DEFAULT_ROUGHNESS, step=DEFAULT_STEP, valid=None, base=None,
                       unknown=0.5, min_valid=3, return_terms=False, out=None, radius_cells=None):
    """Cost map in [0,1] of the terrain `z` ([H,W] or [S,H,W]; float32 or float64, unit stride along W, read in place).

    `grid_res`: metres per cell.  `radius`: window radius in METRES, r = max(1, round(radius / grid_res)) cells, at most 16 cells (or give
    `radius_cells=` directly).  `slope=(lo, hi)` rise over run, `roughness=(lo, hi)` metres, `step=(lo, hi)` metres: each term ramps from 0 at
    lo to 1 at hi and the cost is the largest ramp.  `valid`: same shape and dtype as z, nonzero = usable (non-finite z is never usable).
    `base`: a keep-out map of z's shape merged with `max` (its NaN cells leave the cost alone).  A cell whose window holds fewer than
    `min_valid` (>= 3) usable cells, or only collinear ones, costs `unknown` and its terms are NaN.  `out`: a contiguous buffer of z's shape
    to write the cost into.  Returns `cost`, or `(cost, terms)` with `terms` [3,H,W] / [S,3,H,W] = (slope, roughness, step).

    GPU tensors: one launch of the HIP kernel, in z's dtype.  CPU tensors: `traversability_map_aten` (float32 arithmetic), cast to z's dtype.
    Not differentiable: the result never requires grad."""
    r = radius_cells if radius_cells is not None else cells_of_radius(radius, grid_res)
    lo, hi = [slope[0], roughness[0], step[0]], [slope[1], roughness[1], step[1]]
    z = z.detach()
    valid, base = (None if t is None else t.detach() for t in (valid, base))
    if not z.is_cuda:
        res = traversability_map_aten(z, grid_res, None, slope, roughness, step, valid, base, unknown, min_valid, True, radius_cells=r)
        cost, terms = (t.to(z.dtype) for t in res)
        if out is not None:
            cost = out.copy_(cost)
        return (cost, terms) if return_terms else cost
    _checked(z, valid, base, grid_res, r, lo, hi, min_valid)
    cost = torch.empty(z.shape, dtype=z.dtype, device=z.device) if out is None else out
    terms = torch.empty(tuple(z.shape[:-2]) + (3,) + tuple(z.shape[-2:]), dtype=z.dtype, device=z.device) if return_terms else None
    traversability_into(z, valid, base, grid_res, r, lo, hi, unknown, min_valid, cost, terms)
    return (cost, terms) if return_terms else cost


class TraversabilityMap:
    """The cost map of a planner loop, in static buffers: `tm = TraversabilityMap(dphysics)`, then per frame `tm(z)` writes `tm.cost` (and
    `tm.terms`) in place and returns `tm.cost`, e.g. `planner.plan(z, goal, cost_map=tm(z))`.  The buffers are allocated by the FIRST call
    (from z's shape, dtype and device); every later call is one kernel launch with no allocation and no host read, so it can be captured into
    a hipGraph ahead of `MPPIPlanner.step(..., cost_map=tm.cost)` or `ControlRefiner.step` and replayed.

    `dphysics_or_cfg`: a `DPhysics` module or a `DPhysConfig` (its `grid_res` and `robot_size` are read).  `radius` in metres; default: half
    the shorter side of `cfg.robot_size`.  Default thresholds: slope (0.2, 0.6) rise over run, roughness (0.02, 0.10) m, step (0.10, 0.30) m;
    `unknown` 0.5; `min_valid` 3.  `terms=False` skips the [.., 3, H, W] term layers.  GPU tensors only.  Not differentiable."""

    def __init__(self, dphysics_or_cfg, radius=None, slope=DEFAULT_SLOPE, roughness=DEFAULT_ROUGHNESS, step=DEFAULT_STEP, unknown=0.5, min_valid=3,
                 terms=True):
        cfg = getattr(dphysics_or_cfg, 'dphys_cfg', dphysics_or_cfg)
        self.grid_res = float(cfg.grid_res)
        self.radius = 0.5 * float(min(cfg.robot_size[0], cfg.robot_size[1])) if radius is None else float(radius)
        self.r = cells_of_radius(self.radius, self.grid_res)
        self.lo, self.hi = [slope[0], roughness[0], step[0]], [slope[1], roughness[1], step[1]]
        self.unknown, self.min_valid, self.want_terms = float(unknown), int(min_valid), bool(terms)
        self.cost = self.terms = None

    def __call__(self, z, valid=None, base=None):
        z = z.detach()
        if self.cost is None:
            _lib.require_hip_tensor(z, 'z')
            self.cost = torch.empty(z.shape, dtype=z.dtype, device=z.device)
            if self.want_terms:
                self.terms = torch.empty(tuple(z.shape[:-2]) + (3,) + tuple(z.shape[-2:]), dtype=z.dtype, device=z.device)
        traversability_into(z, None if valid is None else valid.detach(), None if base is None else base.detach(), self.grid_res, self.r,
                            self.lo, self.hi, self.unknown, self.min_valid, self.cost, self.terms)
        return self.cost
