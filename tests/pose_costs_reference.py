"""Referee of the pose-cost kernel (monoforce_amd/csrc/pose_costs.hip): the formulas of include/monoforce_hip.h (MfPoseCostDesc) restated in
plain torch, in the dtype of `Xs` (float32 or float64).  Test code: the product never imports it.

The scalars of the launch descriptor (grid_res, d_max, lethal, off_map, the two weights) are C floats: every function rounds them to float32
first (as tests/mppi_reference.py does), so a float64 evaluation differs from the kernel by its arithmetic alone."""
import torch

from tests.mppi_reference import _f32


def footprint(Xs, Rs, points):
    """Xs [B,Tp,3], Rs [B,Tp,3,3], points [N,3] -> world (x, y) of every footprint point [B,Tp,N,2]: q = Xs[0:2] + Rs[0:2,:] . points[n]."""
    dt = Xs.dtype
    return Xs[..., None, :2] + torch.einsum('btij,nj->btni', Rs[..., :2, :], points.to(dt))


def sample(cost_map, q, grid_res, d_max, off_map):
    """cost_map [H,W], q [...,2] -> (s [...], on [...]): the bilinear sample at q (off_map where q is off the map or NaN) and the on-map mask."""
    dt = q.dtype
    H, W = cost_map.shape
    m = cost_map.to(dt)
    u, v = (q[..., 0] + _f32(d_max, dt)) / _f32(grid_res, dt), (q[..., 1] + _f32(d_max, dt)) / _f32(grid_res, dt)
    on = (u >= 0) & (u <= H - 1) & (v >= 0) & (v <= W - 1)
    u, v = torch.where(on, u, torch.zeros_like(u)), torch.where(on, v, torch.zeros_like(v))
    ix, iy = torch.clamp(torch.floor(u).long(), max=H - 2), torch.clamp(torch.floor(v).long(), max=W - 2)
    fx, fy = u - ix.to(dt), v - iy.to(dt)
    s = (1 - fx) * (1 - fy) * m[ix, iy] + fx * (1 - fy) * m[ix + 1, iy] + (1 - fx) * fy * m[ix, iy + 1] + fx * fy * m[ix + 1, iy + 1]
    return torch.where(on, s, _f32(off_map, dt).expand_as(s)), on


def polyline_distance(xy, path):
    """xy [...,2], path [P,2] (P >= 1) -> distance [...] to the polyline: min over the P-1 segments, projection clamped to [0,1]; a zero-length
    segment is its point, P = 1 the distance to that point."""
    dt = xy.dtype
    path = path.to(dt)
    a, b = (path[:-1], path[1:]) if path.shape[0] > 1 else (path, path)
    ab, ap = b - a, xy[..., None, :] - a
    len2 = (ab * ab).sum(-1)
    dot = (ap * ab).sum(-1)
    t = torch.where(len2 > 0, torch.clamp(dot / torch.where(len2 > 0, len2, torch.ones_like(len2)), 0.0, 1.0), torch.zeros_like(dot))
    d = ap - t[..., None] * ab
    return torch.sqrt((d * d).sum(-1).min(dim=-1).values)


def pose_costs(Xs, Rs, points, cost_map, path, base_costs, grid_res, d_max, lethal, off_map, weights):
    """Xs [B,Tp,3], Rs [B,Tp,3,3], points [N,3], cost_map [H,W] or None, path [P,2] or None, base_costs [B] or None, weights (map, path)
    -> costs [B], terms [B,2] = (map, xtrack)."""
    dt = Xs.dtype
    B, Tp = Xs.shape[:2]
    w = _f32(list(weights), dt)
    assert cost_map is not None or float(w[0]) == 0, 'a map weight needs a cost map'
    assert path is not None or float(w[1]) == 0, 'a path weight needs a path'
    costs = torch.zeros(B, dtype=dt) if base_costs is None else base_costs.to(dt).clone()
    mp, xt = torch.zeros(B, dtype=dt), torch.zeros(B, dtype=dt)
    if cost_map is not None:
        s, _ = sample(cost_map, footprint(Xs, Rs, points), grid_res, d_max, off_map)
        is_lethal = (~(s < _f32(lethal, dt))).flatten(1).any(dim=1)
        inf = torch.full_like(mp, float('inf'))
        mp = torch.where(is_lethal, inf, s.max(dim=-1).values.sum(dim=-1) / Tp)
        costs = costs + torch.where(is_lethal, inf, w[0] * mp)
    if path is not None:
        xt = polyline_distance(Xs[..., :2], path).sum(dim=-1) / Tp
        costs = costs + w[1] * xt
    return costs, torch.stack([mp, xt], dim=-1)
