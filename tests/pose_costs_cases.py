"""Constructed inputs of the pose-cost tests (tests/test_pose_costs_gpu.py): poses, a footprint, a cost map with a lethal block, a path.

The discontinuous decisions of the formulas (on / off the map, below / not below `lethal`) must not hang on float32 rounding, so the generator
works in float64 on the float32-rounded inputs and REDRAWS (never drops) any pose with a footprint point within `MARGIN` cells of the map
border or a sample within `MARGIN` of `lethal`."""
import math

import torch

from tests import pose_costs_reference as ref

F64 = torch.float64
GRID_RES, D_MAX, LETHAL, HW = 0.1, 3.2, 2.0, 64
MARGIN = 1e-3
SHAPES = [(1, 1, 1), (3, 2, 4), (65, 5, 7), (130, 11, 65), (33, 3, 223)]      # partial wave, second group, odd body, body one past a wave, the reference's body
PATH = torch.tensor([[-2.0, -2.0], [-1.0, 0.0], [-1.0, 0.0], [1.0, 1.0], [2.5, 0.5]])      # one repeated vertex


def cost_map(seed=0):
    m = torch.rand(HW, HW, generator=torch.Generator().manual_seed(seed))
    m[34:48, 14:28] = 5.0          # x in [0.2, 1.5], y in [-1.8, -0.5]
    return m


def _draw(g, centre, n):
    """n poses around `centre` [n,2]: position jitter +-0.15 m, random yaw, tilt up to 0.2 rad, R scaled entrywise by 1 + 0.02 randn."""
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, dtype=F64, generator=g)  # noqa: E731
    X = torch.stack([centre[:, 0] + u(-0.15, 0.15), centre[:, 1] + u(-0.15, 0.15), u(-0.1, 0.3)], -1)
    yaw, pitch, roll = u(-math.pi, math.pi), u(-0.2, 0.2), u(-0.2, 0.2)
    cy, sy, cp, sp, cr, sr = torch.cos(yaw), torch.sin(yaw), torch.cos(pitch), torch.sin(pitch), torch.cos(roll), torch.sin(roll)
    R = torch.stack([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                     sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                     -sp, cp * sr, cp * cr], -1).reshape(n, 3, 3)
    return X, R * (1 + 0.02 * torch.randn(n, 3, 3, dtype=F64, generator=g))


def constructed(B, Tp, N, seed=None):
    """dict(Xs [B,Tp,3], Rs [B,Tp,3,3], points [N,3], cost_map, path, base, redraws), float32 on the CPU.  The margins hold for off_map = inf
    and any finite off_map not within MARGIN of LETHAL."""
    g = torch.Generator().manual_seed(1000 * B + 10 * Tp + N if seed is None else seed)
    m = cost_map()
    points = ((torch.rand(N, 3, dtype=F64, generator=g) - 0.5) * torch.tensor([0.8, 0.6, 0.2], dtype=F64)).float()
    centre = (torch.rand(B, 2, dtype=F64, generator=g) - 0.5) * 7.0          # the map spans [-3.2, 3.1]: some footprints leave it
    cb = centre.repeat_interleave(Tp, 0)
    X, R = _draw(g, cb, B * Tp)
    X, R = X.float(), R.float()
    redraws = 0
    while True:
        q = ref.footprint(X.double().unsqueeze(0), R.double().unsqueeze(0), points.double())[0]      # [B*Tp, N, 2]
        uv = (q + D_MAX) / torch.tensor(GRID_RES, dtype=torch.float32).double()
        near_border = ((uv.abs() < MARGIN) | ((uv - (HW - 1)).abs() < MARGIN)).any(-1)
        s, _ = ref.sample(m.double(), q, GRID_RES, D_MAX, 0.0)                     # (off-map points: 0, far from LETHAL)
        bad = (near_border | ((s - LETHAL).abs() < MARGIN)).any(-1)
        if not bool(bad.any()):
            break
        k = int(bad.sum())
        redraws += k
        Xn, Rn = _draw(g, cb[bad], k)
        X[bad], R[bad] = Xn.float(), Rn.float()
    base = torch.rand(B, generator=g)
    return dict(Xs=X.reshape(B, Tp, 3), Rs=R.reshape(B, Tp, 3, 3), points=points, cost_map=m, path=PATH.clone(), base=base, redraws=redraws)


def cells_read(case):
    """Per rollout, the set of flat map cells its on-map footprint samples read (all four corners, whatever their weights)."""
    Xs, Rs = case['Xs'].double(), case['Rs'].double()
    q = ref.footprint(Xs, Rs, case['points'].double())
    uv = (q + D_MAX) / torch.tensor(GRID_RES, dtype=torch.float32).double()
    on = ((uv >= 0) & (uv <= HW - 1)).all(-1)
    ij = torch.clamp(torch.floor(torch.where(on[..., None], uv, torch.zeros_like(uv))).long(), max=HW - 2)
    out = []
    for b in range(Xs.shape[0]):
        c = ij[b][on[b]]
        flat = c[:, 0] * HW + c[:, 1]
        out.append(set(torch.cat([flat, flat + 1, flat + HW, flat + HW + 1]).tolist()))
    return out
