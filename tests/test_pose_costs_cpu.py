"""Pose costs without a GPU: the referee of the kernel (tests/pose_costs_reference.py) pinned against explicit loops and hand-computed values,
the descriptor mirror, argument validation of the entry point, and the code-object metadata of pose_costs.o."""
import ctypes
import math
import os
import sys

import pytest
import torch

from tests import pose_costs_reference as ref
from tests.conftest import REPO

F64 = torch.float64
INF = float('inf')


# ---- the referee against explicit loops -----------------------------------------------------------------------------------------------
def _loop_sample(m, qx, qy, grid_res, d_max, off_map):
    H, W = m.shape
    u, v = (qx + d_max) / grid_res, (qy + d_max) / grid_res
    if not (0 <= u <= H - 1 and 0 <= v <= W - 1):       # (a NaN fails every comparison)
        return off_map
    ix, iy = min(math.floor(u), H - 2), min(math.floor(v), W - 2)
    fx, fy = u - ix, v - iy
    g = lambda i, j: float(m[i, j])  # noqa: E731
    return (1 - fx) * (1 - fy) * g(ix, iy) + fx * (1 - fy) * g(ix + 1, iy) + (1 - fx) * fy * g(ix, iy + 1) + fx * fy * g(ix + 1, iy + 1)


def _loop_segment(x, y, a, b):
    abx, aby, apx, apy = b[0] - a[0], b[1] - a[1], x - a[0], y - a[1]
    len2 = abx * abx + aby * aby
    t = min(max((apx * abx + apy * aby) / len2, 0.0), 1.0) if len2 > 0 else 0.0
    return math.hypot(apx - t * abx, apy - t * aby)


def _loop_pose_costs(Xs, Rs, points, m, path, base, grid_res, d_max, lethal, off_map, w):
    B, Tp = Xs.shape[:2]
    costs, terms = torch.zeros(B, dtype=F64), torch.zeros(B, 2, dtype=F64)
    for b in range(B):
        c = 0.0 if base is None else float(base[b])
        if m is not None:
            total, is_lethal = 0.0, False
            for p in range(Tp):
                f = -INF
                for n in range(points.shape[0]):
                    q = [float(Xs[b, p, i]) + sum(float(Rs[b, p, i, j]) * float(points[n, j]) for j in range(3)) for i in range(2)]
                    s = _loop_sample(m, q[0], q[1], grid_res, d_max, off_map)
                    is_lethal = is_lethal or not s < lethal
                    f = max(f, s)
                total += f
            terms[b, 0] = INF if is_lethal else total / Tp
            c += INF if is_lethal else w[0] * total / Tp
        if path is not None:
            P = path.shape[0]
            pv = [(float(path[k, 0]), float(path[k, 1])) for k in range(P)]
            segs = [(pv[k], pv[k + 1]) for k in range(P - 1)] or [(pv[0], pv[0])]
            xt = sum(min(_loop_segment(float(Xs[b, p, 0]), float(Xs[b, p, 1]), a, bb) for a, bb in segs) for p in range(Tp)) / Tp
            terms[b, 1] = xt
            c += w[1] * xt
        costs[b] = c
    return costs, terms


def _tiny_case(B, Tp, N, P, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(6, 7, dtype=F64, generator=g)
    m[2:4, 3:5] = 5.0
    Xs = (torch.rand(B, Tp, 3, dtype=F64, generator=g) - 0.5) * 4.0          # the 6 x 7 map spans [-1.5, 1] x [-1.5, 1.5]: some points leave it
    yaw = torch.rand(B, Tp, dtype=F64, generator=g) * 6.28
    Rs = torch.zeros(B, Tp, 3, 3, dtype=F64)
    Rs[..., 0, 0], Rs[..., 0, 1], Rs[..., 1, 0], Rs[..., 1, 1], Rs[..., 2, 2] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw), 1.0
    Rs = Rs * (1 + 0.02 * torch.randn(B, Tp, 3, 3, dtype=F64, generator=g))
    points = (torch.rand(N, 3, dtype=F64, generator=g) - 0.5) * 0.6
    path = (torch.rand(P, 2, dtype=F64, generator=g) - 0.5) * 3.0 if P else None
    if P >= 3:
        path[2] = path[1]                                                     # a zero-length segment
    base = torch.rand(B, dtype=F64, generator=g)
    return Xs, Rs, points, m, path, base


# (scalars that float32 holds exactly: the referee rounds the descriptor's scalars to float32, the loops take them as they are)
@pytest.mark.parametrize('B,Tp,N,P', [(1, 1, 1, 1), (2, 3, 4, 2), (3, 2, 5, 4)])
def test_referee_matches_explicit_loops(B, Tp, N, P):
    Xs, Rs, points, m, path, base = _tiny_case(B, Tp, N, P, 10 * B + Tp)
    seen = set()
    for lethal, off_map in ((2.0, INF), (2.0, 1.5), (INF, 0.25)):
        for mm, pp, bb, w in ((m, path, base, (0.5, 2.0)), (m, None, None, (1.0, 0.0)), (None, path, base, (0.0, 1.0)), (m, path, None, (0.0, 1.0))):
            c, t = ref.pose_costs(Xs, Rs, points, mm, pp, bb, 0.5, 1.5, lethal, off_map, w)
            lc, lt = _loop_pose_costs(Xs, Rs, points, mm, pp, bb, 0.5, 1.5, lethal, off_map, w)
            assert torch.equal(torch.isinf(c), torch.isinf(lc)) and torch.equal(torch.isinf(t), torch.isinf(lt))
            fin = torch.isfinite(lc)
            assert torch.allclose(c[fin], lc[fin], rtol=1e-13, atol=1e-15) and torch.allclose(t[torch.isfinite(lt)], lt[torch.isfinite(lt)], rtol=1e-13, atol=1e-15)
            seen |= {bool(v) for v in fin}
    if B > 1:
        assert seen == {True, False}       # both a finite and a lethal rollout occurred


def test_sample_is_the_map_at_nodes_and_the_four_term_blend_inside_cells():
    g = torch.Generator().manual_seed(1)
    H, W, res, d_max = 5, 9, 0.25, 0.5
    m = torch.randn(H, W, dtype=F64, generator=g)
    ii, jj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    nodes = torch.stack([ii * res - d_max, jj * res - d_max], -1).to(F64)      # (0.25 and 0.5 are exact: u and v are integers)
    s, on = ref.sample(m, nodes, res, d_max, INF)
    assert bool(on.all()) and torch.equal(s, m)                               # the last row / column included (ix = H-2, fx = 1)
    # interior of every cell, the formula written out
    fx, fy = 0.375, 0.8125
    q = torch.stack([(ii[:-1, :-1] + fx) * res - d_max, (jj[:-1, :-1] + fy) * res - d_max], -1).to(F64)
    s, on = ref.sample(m, q, res, d_max, INF)
    want = (1 - fx) * (1 - fy) * m[:-1, :-1] + fx * (1 - fy) * m[1:, :-1] + (1 - fx) * fy * m[:-1, 1:] + fx * fy * m[1:, 1:]
    assert bool(on.all()) and torch.allclose(s, want, rtol=1e-14, atol=1e-15)
    # continuous across a cell edge (interpolate_grid's swapped weights are not): both sides of u = 2 agree to the step taken
    eps = 1e-9
    a, _ = ref.sample(m, torch.tensor([[2 * res - d_max - eps, 0.3]], dtype=F64), res, d_max, INF)
    b, _ = ref.sample(m, torch.tensor([[2 * res - d_max + eps, 0.3]], dtype=F64), res, d_max, INF)
    assert abs(float(a - b)) < 1e-6
    # off the map, and NaN: off_map
    off = torch.tensor([[-d_max - 1e-9, 0.0], [0.0, (W - 1) * res - d_max + 1e-9], [float('nan'), 0.0], [0.0, float('nan')]], dtype=F64)
    s, on = ref.sample(m, off, res, d_max, 1.5)
    assert not bool(on.any()) and s.tolist() == [1.5] * 4


def test_referee_hand_computed_values():
    m = torch.zeros(8, 8, dtype=F64)
    m[4, 4], m[5, 4], m[4, 5], m[5, 5] = 1.0, 3.0, 5.0, 7.0
    eye = torch.eye(3, dtype=F64)
    Xs = torch.tensor([[[0.5, 0.25, 9.0]]], dtype=F64)
    origin = torch.zeros(1, 3, dtype=F64)
    # u = 4.5, v = 4.25: 0.5 * 0.75 * 1 + 0.5 * 0.75 * 3 + 0.5 * 0.25 * 5 + 0.5 * 0.25 * 7 = 0.375 + 1.125 + 0.625 + 0.875
    c, t = ref.pose_costs(Xs, eye.expand(1, 1, 3, 3), origin, m, None, None, 1.0, 4.0, INF, INF, (1.0, 0.0))
    assert t.tolist() == [[3.0, 0.0]] and c.tolist() == [3.0]
    for dt in (torch.float32, F64):
        c, t = ref.pose_costs(Xs.to(dt), eye.to(dt).expand(1, 1, 3, 3), origin.to(dt), m.to(dt), None, None, 1.0, 4.0, INF, INF, (1.0, 0.0))
        assert c.dtype == dt and c.tolist() == [3.0]
    # lethal = 3: the sample is not < 3; lethal = 3.5: it is.  w_map = 0 keeps the lethal rule and nothing else
    assert ref.pose_costs(Xs, eye.expand(1, 1, 3, 3), origin, m, None, None, 1.0, 4.0, 3.0, INF, (1.0, 0.0))[0].tolist() == [INF]
    assert ref.pose_costs(Xs, eye.expand(1, 1, 3, 3), origin, m, None, None, 1.0, 4.0, 3.0, INF, (0.0, 0.0))[0].tolist() == [INF]
    assert ref.pose_costs(Xs, eye.expand(1, 1, 3, 3), origin, m, None, None, 1.0, 4.0, 3.5, INF, (0.0, 0.0))[0].tolist() == [0.0]
    # two points: the one at body (1, 0, 0) reads node (5, 4) + (0.5, 0.25) = 0 (all zero there but m[5][4], m[5][5]):
    # 0.5 * 0.75 * 3 + 0.5 * 0.25 * 7 = 1.125 + 0.875 = 2.0 < 3.0: the maximum stays 3.0; yawed a quarter turn it reads u = 4.5, v = 5.25:
    # 0.5 * 0.75 * 5 + 0.5 * 0.75 * 7 = 1.875 + 2.625 = 4.5
    two = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=F64)
    assert ref.pose_costs(Xs, eye.expand(1, 1, 3, 3), two, m, None, None, 1.0, 4.0, INF, INF, (1.0, 0.0))[1].tolist() == [[3.0, 0.0]]
    quarter = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=F64)
    assert ref.pose_costs(Xs, quarter.expand(1, 1, 3, 3), two, m, None, None, 1.0, 4.0, INF, INF, (1.0, 0.0))[1].tolist() == [[4.5, 0.0]]
    # the path (0,0) -> (2,0) -> (2,2): (0.5, 0.25) is 0.25 above the first segment, (3, 1) is 1 to the right of the second,
    # (-1, 0) is 1 before the start (clamped), (3, 3) is sqrt(2) past the end (clamped)
    path = torch.tensor([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0]], dtype=F64)
    xy = torch.tensor([[0.5, 0.25], [3.0, 1.0], [-1.0, 0.0], [3.0, 3.0]], dtype=F64)
    assert torch.allclose(ref.polyline_distance(xy, path), torch.tensor([0.25, 1.0, 1.0, math.sqrt(2.0)], dtype=F64), rtol=1e-15, atol=0)
    X2 = torch.tensor([[[0.5, 0.25, 0.0], [3.0, 1.0, 0.0]]], dtype=F64)
    c, t = ref.pose_costs(X2, eye.expand(1, 2, 3, 3), origin, None, path, torch.tensor([10.0], dtype=F64), 1.0, 4.0, INF, INF, (0.0, 2.0))
    assert t.tolist() == [[0.0, 0.625]] and c.tolist() == [11.25]
    assert ref.polyline_distance(xy[1:2], path[:1]).tolist() == [math.sqrt(10.0)]                       # P = 1: the point itself
    assert ref.polyline_distance(xy[:1], torch.tensor([[1.0, 1.0], [1.0, 1.0]], dtype=F64)).tolist() == [math.hypot(0.5, 0.75)]      # zero-length


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def built_lib():
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import _lib
    return _lib.lib()


def test_descriptor_mirror_matches_header(built_lib):
    from monoforce_amd import _lib
    built_lib.mf_sizeof.restype = ctypes.c_int
    built_lib.mf_sizeof.argtypes = [ctypes.c_char_p]
    assert built_lib.mf_sizeof(b'MfPoseCostDesc') == ctypes.sizeof(_lib.MfPoseCostDesc) == 80
    assert built_lib.mf_sizeof(b'MfMppiDesc') == ctypes.sizeof(_lib.MfMppiDesc) == 80           # untouched
    assert 'mf_pose_costs_f32' in _lib.SYMBOLS and hasattr(built_lib, 'mf_pose_costs_f32')


def test_argument_validation_without_gpu(built_lib):
    """Every rejected argument is reported before any launch: an error code and a message, on a box without a GPU."""
    from monoforce_amd import _lib
    p = ctypes.c_void_p(1 << 20)       # never dereferenced: validation fails first
    nan = float('nan')

    def desc(**kw):
        d = dict(B=8, Tp=5, N=4, P=3, H=16, W=16, x_stride_b=3, x_stride_t=24, r_stride_b=9, r_stride_t=72, grid_res=0.1, d_max=0.8,
                 lethal=INF, off_map=INF, w_map=1.0, w_path=1.0)
        d.update(kw)
        return _lib.MfPoseCostDesc(**d)

    def call(d, Xs=p, Rs=p, points=p, cost_map=p, path=p, base=p, costs=p, terms=p):
        return built_lib.mf_pose_costs_f32(ctypes.byref(d) if d is not None else None, Xs, Rs, points, cost_map, path, base, costs, terms, None)

    INVALID, UNSUPPORTED = 1, 2
    cases = [(dict(d=None), INVALID, b'null descriptor'),
             (dict(d=desc(), Xs=None), INVALID, b'null'), (dict(d=desc(), Rs=None), INVALID, b'null'), (dict(d=desc(), points=None), INVALID, b'null'),
             (dict(d=desc(), costs=None), INVALID, b'null'),
             (dict(d=desc(B=0)), INVALID, b'positive'), (dict(d=desc(Tp=-1)), INVALID, b'positive'), (dict(d=desc(N=0)), INVALID, b'positive'),
             (dict(d=desc(N=1025)), UNSUPPORTED, b'1024'), (dict(d=desc(P=257)), UNSUPPORTED, b'256'),
             (dict(d=desc(P=-1)), INVALID, b'negative'), (dict(d=desc(H=1)), INVALID, b'H >= 2'), (dict(d=desc(W=1)), INVALID, b'W >= 2'),
             (dict(d=desc(x_stride_b=-3)), INVALID, b'stride'), (dict(d=desc(x_stride_t=-1)), INVALID, b'stride'),
             (dict(d=desc(r_stride_b=-9)), INVALID, b'stride'), (dict(d=desc(r_stride_t=-1)), INVALID, b'stride'),
             (dict(d=desc(grid_res=0.0)), INVALID, b'grid_res'), (dict(d=desc(grid_res=-0.1)), INVALID, b'grid_res'), (dict(d=desc(grid_res=nan)), INVALID, b'grid_res'),
             (dict(d=desc(lethal=nan)), INVALID, b'NaN'), (dict(d=desc(off_map=nan)), INVALID, b'NaN'),
             (dict(d=desc(), cost_map=None), INVALID, b'w_map'),                                   # a weight without its input
             (dict(d=desc(P=0), path=None), INVALID, b'w_path'),
             (dict(d=desc(P=0, w_path=0.0)), INVALID, b'path must be NULL'),                       # a path without P
             (dict(d=desc(), path=None), INVALID, b'path must be NULL'),                           # P without a path
             (dict(d=desc(H=1 << 16, W=1 << 15)), UNSUPPORTED, b'2^31'),
             (dict(d=desc(B=1 << 20, x_stride_b=1 << 12)), UNSUPPORTED, b'2^31'), (dict(d=desc(Tp=1 << 20, r_stride_t=1 << 12)), UNSUPPORTED, b'2^31'),
             (dict(d=desc(x_stride_t=1 << 31)), UNSUPPORTED, b'2^31')]
    for kw, code, word in cases:
        rc = call(**kw)
        assert rc == code and word in built_lib.mf_last_error(), (kw, rc, built_lib.mf_last_error())


def test_pose_cost_kernels_use_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_metadata
    rows = [(n, m) for o, n, m in kernel_metadata.kernels() if o == 'pose_costs.o']
    names = ' '.join(n for n, _ in rows)
    for k in ('pose_costs_lanes_kernel', 'pose_costs_points_kernel'):
        assert k in names, (k, names)
    assert all(m['scratch'] == 0 for _, m in rows), rows
