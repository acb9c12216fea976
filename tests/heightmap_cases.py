"""Constructed clouds of the heightmap tests (tests/test_heightmap_gpu.py, pinned on the CPU in tests/test_heightmap_cpu.py): name ->
(points, keyword arguments of estimate_heightmap).  Every height of a cloud is distinct wherever a maximum is to tell which point won."""
import numpy as np
import torch

KW = dict(grid_res=0.1, d_max=6.4, h_max=1.0)
R_MIN = 1.25                                          # = |(0.75, 1.0)| exactly, in float32 and in float64
ODD_GRIDS = [(0.3, 6.4), (0.07, 3.0)]                 # 2 d_max / grid_res = 42.67 and 85.71: 43 and 86 edges, the last cell narrower


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ulp(v, towards):
    return torch.nextafter(v, torch.full_like(v, towards))


def _cloud(n, seed, d_max=6.4, h=0.9):
    g = _gen(seed)
    xy = (torch.rand(n, 2, generator=g) * 2 - 1) * d_max * 1.05          # a few outside the box
    return torch.cat([xy, (torch.rand(n, 1, generator=g) * 2 - 1) * h], dim=1)


def contention():
    """100 000 points inside the cell [0.3, 0.4) x [-1.2, -1.1) and 1000 spread out: every thread of 391 workgroups on one address."""
    g = _gen(1)
    one = torch.stack([0.31 + 0.08 * torch.rand(100000, generator=g), -1.19 + 0.08 * torch.rand(100000, generator=g),
                       torch.randn(100000, generator=g) * 0.4], dim=1)          # a few heights beyond +-1: filtered
    pts = torch.cat([one, _cloud(1000, 2)])
    return pts[torch.randperm(pts.shape[0], generator=g)], dict(KW)


def negative():
    """Every height below zero: a measured cell's maximum is negative (the integer key of the atomic must order negative floats), the largest
    of one cell is -0.0, of another a subnormal."""
    pts = _cloud(5000, 3)
    pts[:, 2] = -(pts[:, 2].abs() + 0.01)
    pts[:40, :2] = torch.tensor([2.05, 2.05])          # forty points in one cell ...
    pts[7, 2] = -0.0                                   # ... the highest of them -0.0
    pts[40:80, :2] = torch.tensor([-2.05, 3.05])
    pts[55, 2] = -1e-40                                # subnormal
    return pts, dict(KW)


def infinite_and_on_the_box():
    """z = +-inf and x or y exactly +-d_max: dropped (the box is open), among points that stay; one cell would otherwise hold +inf."""
    pts = _cloud(600, 4)
    inf, d = float('inf'), KW['d_max']
    pts[0:50, 2], pts[50:100, 2] = inf, -inf
    pts[100:110, 0], pts[110:120, 0], pts[120:130, 1], pts[130:140, 1] = d, -d, d, -d
    pts[140, :] = torch.tensor([0.55, 0.55, inf])
    return pts, dict(KW)


def six_columns():
    """x, y, z and three more fields; NaNs in the extra columns alone drop the row (its x, y, z are fine), as NaNs in x, y, z do."""
    g = _gen(5)
    pts = torch.cat([_cloud(800, 5), torch.rand(800, 3, generator=g)], dim=1)
    pts[0:100, 3], pts[100:200, 4], pts[200:300, 5] = float('nan'), float('nan'), float('nan')
    pts[300:330, 0], pts[330:360, 2] = float('nan'), float('nan')
    pts[:300, 2] = 0.95                                 # the rows to be dropped would be the highest of their cells
    return pts, dict(KW)


def _ring(x, y):
    """(+-x, +-y) and (+-y, +-x), heights 0.5."""
    s = [(a * x, b * y) for a in (1, -1) for b in (1, -1)] + [(a * y, b * x) for a in (1, -1) for b in (1, -1)]
    return torch.tensor([[u, v, 0.5] for u, v in s], dtype=torch.float32)


def at_r_min():
    """The eight points (+-0.75, +-1.0), (+-1.0, +-0.75): at distance 1.25 = r_min exactly, not beyond it."""
    return _ring(0.75, 1.0), dict(KW, r_min=R_MIN)


def one_ulp_beyond_r_min():
    """Their neighbours with the LARGER coordinate one ulp out: the distance rounds to the next float32 above 1.25 (the smaller coordinate one
    ulp out moves it by 0.3 ulp of 1.25 only, and the norm is still 1.25: second half of the cloud, whatever the referee says)."""
    one, q = np.float32(1.0), np.float32(0.75)
    return torch.cat([_ring(0.75, float(np.nextafter(one, np.float32(2.0)))), _ring(float(np.nextafter(q, one)), 1.0)]), dict(KW, r_min=R_MIN)


def edges_of(grid_res, d_max):
    return torch.arange(-d_max, d_max, grid_res, dtype=torch.float32)


def on_and_around_every_edge(grid_res, d_max):
    """Coordinates on every float32 edge, one ulp below and above it, and between the last edge and d_max (the narrow last cell), as x against a
    shuffled copy as y, and each against random partners.  The kernel's first guess floor((v - edges[0]) / grid_res) is off by one on and next to
    many of these edges; its two correcting loops must end on torch.bucketize's index."""
    e = edges_of(grid_res, d_max)
    top = torch.tensor(d_max, dtype=torch.float32)
    last = torch.stack([e[-1] + (top - e[-1]) * f for f in (0.25, 0.5, 0.75)] + [_ulp(top, 0.0)])
    v = torch.cat([e, _ulp(e, -float('inf')), _ulp(e, float('inf')), last])
    g = _gen(int(1000 * grid_res))
    n = v.numel()
    rnd = lambda: (torch.rand(n, generator=g) * 2 - 1) * d_max  # noqa: E731
    xy = torch.cat([torch.stack([v, v[torch.randperm(n, generator=g)]], 1), torch.stack([v, rnd()], 1), torch.stack([rnd(), v], 1)])
    z = torch.randperm(3 * n, generator=g).float() / (3 * n) - 0.5           # distinct heights
    return torch.cat([xy, z.unsqueeze(1)], dim=1), dict(grid_res=grid_res, d_max=d_max, h_max=1.0)


def few(n):
    """n points inside the box: one thread of one workgroup (n = 1), a second, partial workgroup (n = 257)."""
    return _cloud(n, 10 + n, d_max=6.0), dict(KW)


CASES = {'contention': contention, 'negative': negative, 'infinite and on the box': infinite_and_on_the_box, 'six columns': six_columns,
         'at r_min': at_r_min, 'one ulp beyond r_min': one_ulp_beyond_r_min, 'N = 1': lambda: few(1), 'N = 257': lambda: few(257)}
CASES.update({f'edges {r} / {d}': (lambda r=r, d=d: on_and_around_every_edge(r, d)) for r, d in ODD_GRIDS})
