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
# The launch configurations SHAPES does not reach (pose_costs.hip picks them on the host: lanes = rollouts runs S = 16 / 8 / 4 waves per group
# for B <= 8192 / <= 16384 / above; lanes = points runs 4 / 2 / 1 waves = 16 / 8 / 4 rows per rollout for B <= 1024 / <= 4096 / above; the body
# changes mapping above kLaneBodyMax = 8 points).  tests/test_side_kernel_shapes_cpu.py holds these thresholds to the source.
CONFIG_SHAPES = [(8193, 3, 4),       # lanes, S = 8, one rollout in the last group
                 (8193, 11, 5),      # lanes, S = 8, every wave holds a pose (at Tp = 3 five of the eight partial sums are zeros), a ragged second trip
                 (16385, 5, 7),      # lanes, S = 4, Tp > S: a ragged second trip
                 (70, 53, 8),        # lanes at N = kLaneBodyMax, four ragged trips of the pose loop
                 (1025, 17, 9),      # points, 2 waves (8 rows), a partial 16-lane row, three ragged trips
                 (40, 67, 16),       # points, 4 waves, exactly one full row of points, five ragged trips
                 (4097, 19, 17),     # points, 1 wave (4 rows), lane 0 takes a second point, five ragged trips
                 (4097, 5, 65),      # points, 1 wave, the body one past a wave
                 (5, 9, 1024)]       # the largest body (the LDS table full)
RECT = (48, 80)                      # a map that is not square: x spans [-3.2, 1.5], y spans [-3.2, 4.7]
RECT_SHAPES = [(65, 5, 7), (33, 3, 223)]      # one per kernel
PATH_LENGTHS = [1, 2, 17, 18, 256]            # a point, one segment, 16 / 17 / 255 segments: one trip, a second lane-0 trip, sixteen trips of the 16-lane deal


def cost_map(seed=0, map_shape=(HW, HW)):
    m = torch.rand(*map_shape, generator=torch.Generator().manual_seed(seed))
    if tuple(map_shape) == (HW, HW):
        m[34:48, 14:28] = 5.0      # x in [0.2, 1.5], y in [-1.8, -0.5]
    else:
        assert tuple(map_shape) == RECT
        m[18:32, 52:66] = 5.0      # x in [-1.4, -0.1], y in [2.0, 3.3]: second-axis indices no first axis of this map has
    return m


def walk_path(P, seed=0, map_shape=(HW, HW)):
    """[P,2] float32: a random walk of 0.25 m steps kept 0.3 m inside the map, one vertex repeated (a zero-length segment) where P >= 3."""
    g = torch.Generator().manual_seed(7000 + 10 * P + seed)
    lo = torch.tensor([-D_MAX + 0.3, -D_MAX + 0.3], dtype=F64)
    hi = torch.tensor([(map_shape[0] - 1) * GRID_RES - D_MAX - 0.3, (map_shape[1] - 1) * GRID_RES - D_MAX - 0.3], dtype=F64)
    v = [lo + (hi - lo) * torch.rand(2, dtype=F64, generator=g)]
    for _ in range(P - 1):
        v.append(torch.minimum(torch.maximum(v[-1] + 0.25 * torch.randn(2, dtype=F64, generator=g), lo), hi))
    path = torch.stack(v).float()
    if P >= 3:
        path[P // 2] = path[P // 2 - 1]
    return path


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


def constructed(B, Tp, N, seed=None, map_shape=(HW, HW)):
    """dict(Xs [B,Tp,3], Rs [B,Tp,3,3], points [N,3], cost_map, path, base, redraws), float32 on the CPU.  The margins hold for off_map = inf
    and any finite off_map not within MARGIN of LETHAL.  `map_shape`: (H, W) of the cost map (first axis x); the 64 x 64 default draws what it
    always drew."""
    g = torch.Generator().manual_seed(1000 * B + 10 * Tp + N if seed is None else seed)
    m = cost_map(map_shape=map_shape)
    last = torch.tensor([map_shape[0] - 1, map_shape[1] - 1], dtype=F64)      # the last node of each axis: H - 1 and W - 1, each on its own
    points = ((torch.rand(N, 3, dtype=F64, generator=g) - 0.5) * torch.tensor([0.8, 0.6, 0.2], dtype=F64)).float()
    # the map spans [-3.2, 3.1] (64 nodes): a 7 m square around its middle, so that some footprints leave it; as much room around another shape
    grow = (last - (HW - 1)) * GRID_RES
    centre = (torch.rand(B, 2, dtype=F64, generator=g) - 0.5) * (7.0 + grow) + 0.5 * grow
    cb = centre.repeat_interleave(Tp, 0)
    X, R = _draw(g, cb, B * Tp)
    X, R = X.float(), R.float()
    redraws = 0
    while True:
        q = ref.footprint(X.double().unsqueeze(0), R.double().unsqueeze(0), points.double())[0]      # [B*Tp, N, 2]
        uv = (q + D_MAX) / torch.tensor(GRID_RES, dtype=torch.float32).double()
        near_border = ((uv.abs() < MARGIN) | ((uv - last).abs() < MARGIN)).any(-1)
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


def cells_read(case, map_shape=(HW, HW)):
    """Per rollout, the set of flat map cells its on-map footprint samples read (all four corners, whatever their weights)."""
    H, W = map_shape
    assert tuple(case['cost_map'].shape) == (H, W)
    Xs, Rs = case['Xs'].double(), case['Rs'].double()
    q = ref.footprint(Xs, Rs, case['points'].double())
    uv = (q + D_MAX) / torch.tensor(GRID_RES, dtype=torch.float32).double()
    on = ((uv >= 0) & (uv <= torch.tensor([H - 1, W - 1]))).all(-1)
    ij = torch.minimum(torch.floor(torch.where(on[..., None], uv, torch.zeros_like(uv))).long(), torch.tensor([H - 2, W - 2]))
    out = []
    for b in range(Xs.shape[0]):
        c = ij[b][on[b]]
        flat = c[:, 0] * W + c[:, 1]
        out.append(set(torch.cat([flat, flat + 1, flat + W, flat + W + 1]).tolist()))
    return out
