"""No-GPU checks of the route feature (monoforce_amd/route.py, mf_cost_to_go_* / mf_extract_route_*): descriptor sizes, every refusal of the
C entry points without a device, the ATen / host forms bit-equal to the referee of tests/route_reference.py, hand-made cases with their
expected values written out, and the new kernels' code-object metadata."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import route_reference as rr
from tests.conftest import REPO

INF, NAN = float('inf'), float('nan')
RES, DMAX = rr.GRID_RES, rr.D_MAX
TORCH = {'f32': torch.float32, 'f64': torch.float64}


def _aten(cost, goal, **kw):
    from monoforce_amd import route
    return route.cost_to_go_aten(torch.from_numpy(np.array(cost)), goal, RES, DMAX, return_status=True, **kw)


def _host(field, cost, start, goal, **kw):
    from monoforce_amd import route
    return route.extract_route_host(field, torch.from_numpy(np.array(cost)), start, goal, RES, DMAX, **kw)


def _same_route(got, want, s=0):
    n = int(got['n_nodes'][s])
    assert n == want['n_nodes']
    assert np.array_equal(got['nodes'][s, :n].numpy(), want['nodes'])
    path = got['path'] if got['path'].dim() == 2 else got['path'][s]
    assert np.array_equal(path.numpy(), want['path'])
    assert int(got['status'][s]) & (rr.START_UNREACHABLE | rr.TRUNCATED) == want['status']
    assert float(got['route_cost'][s]) == float(want['route_cost'])


# ---- 1. the ATen / host forms against the referee ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('shape', rr.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_aten_and_host_forms_equal_the_referee(shape, dt):
    H, W = shape
    for kind, goal_node, seed in (('random', (H // 2, W // 3), 1), ('random', (0, W - 1), 2), ('open', (H - 1, 0), 0)):
        c = rr.case(kind, H, W, dt, goal_node, seed)
        assert c['status'] == 0 and (kind != 'random' or rr.reachable_share(c['field'], c['cost']) >= 0.5)
        field, status, sweeps = _aten(c['cost'], c['goal'])
        assert field.dtype == TORCH[dt] and sweeps >= 2 and int(status[0]) == 0
        assert np.array_equal(field.numpy(), c['field'])          # bit-equal, the +inf pattern included
        finite = np.argwhere(np.isfinite(c['field']))
        for pick, P in ((0, 2), (len(finite) // 2, 64), (len(finite) - 1, 256)):
            start = rr.position_of(tuple(finite[pick]))
            want = rr.extract_route(c['field'], c['cost'], start, c['goal'], n_vertices=P)
            got = _host(field, c['cost'], start, c['goal'], n_vertices=P)
            _same_route(got, want)
            assert float(got['route_cost'][0]) == float(c['field'][tuple(finite[pick])])
            rr.check_route_is_legal(want['nodes'], c['cost'])
            assert want['nodes'][-1] == goal_node[0] * W + goal_node[1] and want['status'] == 0


def test_fixed_sweep_counts_and_the_public_forms_on_cpu_tensors():
    import monoforce_amd
    from monoforce_amd import route
    c = rr.case('serpentine', 70, 45, 'f32', (0, 0))
    cost = torch.from_numpy(np.array(c['cost']))
    few, status, sweeps = route.cost_to_go_aten(cost, c['goal'], RES, DMAX, n_sweeps=5, return_status=True)
    assert sweeps == 5 and int(status[0]) == rr.NOT_CONVERGED and bool((few.numpy() >= c['field']).all())
    field, status, rounds = monoforce_amd.cost_to_go(cost, c['goal'], RES, DMAX, return_status=True)
    assert np.array_equal(field.numpy(), c['field']) and int(status[0]) == 0 and int(rounds[0]) > 70
    # the only route runs the full width between every pair of walls
    start = rr.position_of((69, 44))
    out = monoforce_amd.extract_route(field, cost, start, c['goal'], RES, DMAX, n_vertices=16)
    want = rr.extract_route(c['field'], c['cost'], start, c['goal'], n_vertices=16)
    _same_route(out, want)
    assert out['path'].shape == (16, 2) and want['n_nodes'] > 9 * 44
    # [S,H,W] maps with a goal each
    three = torch.stack([cost, cost, cost])
    goals = torch.tensor([rr.position_of(n) for n in ((0, 0), (69, 44), (30, 20))], dtype=torch.float32)
    f3 = route.cost_to_go(three, goals, RES, DMAX)
    assert f3.shape == (3, 70, 45) and torch.equal(f3[0], field) and float(f3[1, 69, 44]) == 0.0 and float(f3[2, 30, 20]) == 0.0
    r3 = route.extract_route(f3, three, goals[[1, 2, 0]], goals, RES, DMAX, n_vertices=8)
    assert r3['path'].shape == (3, 8, 2) and r3['nodes'].shape == (3, 70 * 45) and int(r3['status'].max()) == 0
    assert route.default_rounds(70, 45) == 4 * 3 * 2 + 2 and route.default_rounds(256, 256) == 4 * 64 + 2


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_goal_on_a_tile_border_behind_a_doorway_or_in_a_dead_end(dt):
    """The maps of the GPU test of the same name: the ATen form equals the referee, and the far side of the wall is reachable."""
    from monoforce_amd import route
    for name, (cost, g) in rr.border_goal_maps(route.TILE, dtype=rr.DTYPES[dt]).items():
        ref, st = rr.cost_to_go(cost, rr.position_of(g))
        assert st == 0 and rr.reachable_share(ref, cost) >= 0.9 and ref[g] == 0, name
        assert np.array_equal(_aten(cost, rr.position_of(g))[0].numpy(), ref), name


# ---- 2. hand-made cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_corner_rule_walls_touching_diagonally_are_walked_round(dt):
    """Free 4 x 4 map, alpha = 0 (every factor 1), goal (2,2), start (1,1): one diagonal move.  With a wall at (1,2) that diagonal would
    cut the wall's corner: the way is the two axial moves through (2,1), exactly res + res.  With (2,1) a wall as well -- two lethal cells
    touching diagonally, the start and the goal in the two other corners of the square -- every diagonal next to either wall cuts a corner
    too, and the way round one of them is six axial moves, e.g. (1,1) (0,1) (0,2) (0,3) (1,3) (2,3) (2,2): more than two axial moves dearer
    than the diagonal, and never through a wall."""
    T = rr.DTYPES[dt]
    cost = np.zeros((4, 4), T)
    res = T(np.float32(RES))
    diag = res * T(1.4142135623730951)
    goal = rr.position_of((2, 2))
    assert rr.cost_to_go(cost, goal, alpha=0.0)[0][1, 1] == diag and _aten(cost, goal, alpha=0.0)[0].numpy()[1, 1] == diag
    cost[1, 2] = 5.0
    one = _aten(cost, goal, alpha=0.0)[0].numpy()
    assert one[1, 1] == res + res and np.array_equal(one, rr.cost_to_go(cost, goal, alpha=0.0)[0])
    cost[2, 1] = 5.0
    field, status, _ = _aten(cost, goal, alpha=0.0)
    six = T(0)
    for _ in range(6):
        six = six + res
    assert field.numpy()[1, 1] == six and six > diag + (res + res) and int(status[0]) == 0
    assert np.array_equal(field.numpy(), rr.cost_to_go(cost, goal, alpha=0.0)[0]) and np.isinf(field.numpy()[1, 2]) and np.isinf(field.numpy()[2, 1])
    out = _host(field, cost, rr.position_of((1, 1)), goal, alpha=0.0, n_vertices=4)
    nodes = out['nodes'][0, :int(out['n_nodes'][0])].tolist()
    rr.check_route_is_legal(nodes, cost)
    # ties between the two ways round go to the earlier move, (-1,0): round the wall at (1,2)
    assert nodes == [5, 1, 2, 3, 7, 11, 10] and float(out['route_cost'][0]) == float(six)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_tie_rule_on_a_free_map(dt):
    """All-free 6 x 6 map, alpha = 0, goal (0,0).  From (3,3), due north-east of the goal in (x, y), three moves (-1,-1) are the only
    cheapest route.  From (2,1) two candidates tie to the bit: through (1,1), fl(diag + res), and through (1,0), fl(res + diag) -- rounded
    addition commutes.  (1,1) is move (-1,0), the first of the fixed order, (1,0) is move (-1,-1), the fifth: the walk goes through (1,1)."""
    T = rr.DTYPES[dt]
    cost = np.zeros((6, 6), T)
    goal = rr.position_of((0, 0))
    field, _, _ = _aten(cost, goal, alpha=0.0)
    out = _host(field, cost, rr.position_of((3, 3)), goal, alpha=0.0, n_vertices=4)
    assert out['nodes'][0, :4].tolist() == [3 * 6 + 3, 2 * 6 + 2, 1 * 6 + 1, 0] and int(out['n_nodes'][0]) == 4
    assert np.array_equal(out['path'][:, 0].numpy(), out['path'][:, 1].numpy())
    want = rr.extract_route(field.numpy(), cost, rr.position_of((2, 1)), goal, alpha=0.0, n_vertices=3)
    got = _host(field, cost, rr.position_of((2, 1)), goal, alpha=0.0, n_vertices=3)
    _same_route(got, want)
    a = field.numpy()[1, 1] + T(np.float32(RES))
    b = field.numpy()[1, 0] + T(np.float32(RES)) * T(1.4142135623730951)
    assert a == b and field.numpy()[2, 1] == a and got['nodes'][0, :3].tolist() == [2 * 6 + 1, 1 * 6 + 1, 0]


def test_goal_cases_and_nan_walls():
    cost = np.zeros((5, 7), np.float32)
    cost[2, 3] = 1.0                                   # lethal = 1: not below it
    cost[0, 0] = NAN
    cost[4, 6] = INF
    cost[1, 1] = -INF
    for goal in (rr.position_of((2, 3)), rr.position_of((0, 0)), rr.position_of((4, 6)), rr.position_of((1, 1)), (-3.3, 0.0), (0.0, 5.0), (NAN, 0.0)):
        field, status, _ = _aten(cost, goal)
        assert bool(torch.isinf(field).all()) and int(status[0]) == rr.GOAL_BLOCKED, goal
        ref, st = rr.cost_to_go(cost, goal)
        assert st == rr.GOAL_BLOCKED and np.isinf(ref).all()
        out = _host(field, cost, rr.position_of((3, 3)), goal, n_vertices=5)
        assert int(out['status'][0]) == rr.START_UNREACHABLE and int(out['n_nodes'][0]) == 0 and math.isinf(float(out['route_cost'][0]))
        assert torch.equal(out['path'], torch.tensor(rr.position_of((3, 3)), dtype=torch.float32).expand(5, 2))
    # NaN cells are walls: a NaN column with one gap
    cost = np.zeros((5, 7), np.float64)
    cost[:, 3] = NAN
    cost[4, 3] = 0.25
    goal = rr.position_of((0, 6))
    field, status, _ = _aten(cost, goal)
    ref, _ = rr.cost_to_go(cost, goal)
    assert np.array_equal(field.numpy(), ref) and np.isinf(ref[:4, 3]).all() and np.isfinite(ref[:, :3]).all() and int(status[0]) == 0
    out = _host(field, cost, rr.position_of((0, 0)), goal, n_vertices=9)
    nodes = out['nodes'][0, :int(out['n_nodes'][0])].tolist()
    assert 4 * 7 + 3 in nodes
    rr.check_route_is_legal(nodes, cost)
    # start == goal node: L = 1, P copies; a start off the map; a route longer than max_nodes
    same = _host(field, cost, goal, goal, n_vertices=6)
    assert int(same['n_nodes'][0]) == 1 and float(same['route_cost'][0]) == 0.0
    assert torch.equal(same['path'], torch.tensor(goal, dtype=torch.float32).expand(6, 2))
    off = _host(field, cost, (9.0, 9.0), goal, n_vertices=3)
    assert int(off['status'][0]) == rr.START_UNREACHABLE and torch.equal(off['path'], torch.full((3, 2), 9.0))
    short = _host(field, cost, rr.position_of((0, 0)), goal, n_vertices=4, max_nodes=3)
    want = rr.extract_route(ref, cost, rr.position_of((0, 0)), goal, n_vertices=4, max_nodes=3)
    _same_route(short, want)
    assert want['status'] == rr.TRUNCATED and want['n_nodes'] == 3


def test_argument_errors():
    from monoforce_amd import route
    c = torch.zeros(8, 9)
    for bad, text in ((dict(grid_res=0.0), 'grid_res must be positive'), (dict(alpha=-1.0), 'alpha must be finite and not negative'),
                      (dict(alpha=INF), 'alpha must be finite and not negative')):
        kw = dict(grid_res=0.1, d_max=3.2)
        kw.update(bad)
        with pytest.raises(ValueError, match=text):
            route.cost_to_go(c, (0.0, 0.0), **kw)
    with pytest.raises(ValueError, match=r'\[H,W\] or \[S,H,W\]'):
        route.cost_to_go(torch.zeros(1, 1, 8, 9), (0.0, 0.0), 0.1, 3.2)
    with pytest.raises(ValueError, match='unit stride along W'):
        route.cost_to_go(torch.zeros(8, 18)[:, ::2], (0.0, 0.0), 0.1, 3.2)
    with pytest.raises(TypeError, match='float32 or float64'):
        route.cost_to_go(torch.zeros(8, 9, dtype=torch.float16), (0.0, 0.0), 0.1, 3.2)
    with pytest.raises(ValueError, match='1 position'):
        route.cost_to_go(c, (0.0, 0.0, 1.0), 0.1, 3.2)
    f = route.cost_to_go(c, (0.0, 0.0), 0.1, 3.2)
    for kw, text in ((dict(n_vertices=1), r'n_vertices must be in 2\.\.256'), (dict(n_vertices=257), r'n_vertices must be in 2\.\.256'),
                     (dict(max_nodes=1), 'max_nodes must be at least 2')):
        with pytest.raises(ValueError, match=text):
            route.extract_route(f, c, (0.0, 0.0), (0.0, 0.0), 0.1, 3.2, **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        route.cost_to_go_into(c, torch.zeros(1, 2), 0.1, 3.2, 1.0, 4.0, 3, torch.empty(8, 9), torch.zeros(1, dtype=torch.int32),
                              torch.zeros(1, dtype=torch.int32), torch.zeros(64, dtype=torch.int32))
    from monoforce_amd.dphys_config import DPhysConfig
    from monoforce_amd import synthetic as syn
    import monoforce_amd
    pts, masks = syn.robot_points_4()
    cfg = DPhysConfig(robot='tradr', grid_res=0.1, robot_points=pts, driving_parts=masks)
    rp = monoforce_amd.RoutePlanner(cfg, n_vertices=32)
    assert rp.grid_res == 0.1 and rp.d_max == float(cfg.d_max) and rp.path is None and rp.n_vertices == 32
    with pytest.raises(ValueError, match=r'n_vertices must be in 2\.\.256'):
        monoforce_amd.RoutePlanner(cfg, n_vertices=300)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rp(c, torch.zeros(2), torch.zeros(2))


# ---- 3. the C ABI without a GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def built_lib():
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import _lib
    return _lib.lib()


def test_c_abi_symbols_structs_and_every_refusal(built_lib):
    from monoforce_amd import _lib, route
    header = open(os.path.join(REPO, 'include', 'monoforce_hip.h')).read()
    assert int(re.search(r'#define MF_ROUTE_TILE (\d+)', header).group(1)) == route.TILE == _lib.MF_ROUTE_TILE
    assert int(re.search(r'#define MF_ROUTE_MAX_VERTICES (\d+)', header).group(1)) == route.MAX_VERTICES == 256
    for name, value in (('GOAL_BLOCKED', 1), ('NOT_CONVERGED', 2), ('START_UNREACHABLE', 4), ('TRUNCATED', 8)):
        assert int(re.search(rf'#define MF_ROUTE_{name} (\d+)', header).group(1)) == getattr(route, name) == getattr(rr, name) == value
    for name in ('mf_cost_to_go_f32', 'mf_cost_to_go_f64', 'mf_extract_route_f32', 'mf_extract_route_f64'):
        assert hasattr(built_lib, name) and name in _lib.SYMBOLS and getattr(built_lib, name).restype is ctypes.c_int
    built_lib.mf_sizeof.restype = ctypes.c_int
    built_lib.mf_sizeof.argtypes = [ctypes.c_char_p]
    assert built_lib.mf_sizeof(b'MfCostToGoDesc') == ctypes.sizeof(_lib.MfCostToGoDesc) == 48
    assert built_lib.mf_sizeof(b'MfRouteDesc') == ctypes.sizeof(_lib.MfRouteDesc) == 56
    assert route.work_ints(3, 70, 45, 10) == 3 * (2 * math.ceil(70 / route.TILE) * math.ceil(45 / route.TILE) + 10)
    p = lambda a: ctypes.c_void_p(0x1000) if a else None  # noqa: E731      (never dereferenced: validation fails before any launch)
    err = lambda: built_lib.mf_last_error().decode()  # noqa: E731

    def field_call(fn, ptrs=(1,) * 6, **kw):
        d = dict(S=1, H=8, W=9, n_rounds=4, c_stride_h=9, grid_res=0.1, d_max=3.2, lethal=1.0, alpha=4.0)
        d.update(kw)
        return fn(ctypes.byref(_lib.MfCostToGoDesc(**d)), *(p(a) for a in ptrs), None), err()

    def route_call(fn, ptrs=(1,) * 9, **kw):
        d = dict(S=1, H=8, W=9, P=16, max_nodes=72, c_stride_h=9, grid_res=0.1, d_max=3.2, lethal=1.0, alpha=4.0)
        d.update(kw)
        return fn(ctypes.byref(_lib.MfRouteDesc(**d)), *(p(a) for a in ptrs), None), err()
    common = ((dict(S=0), 'must be positive'), (dict(H=-1), 'must be positive'), (dict(W=0), 'must be positive'),
              (dict(grid_res=0.0), 'grid_res must be positive'), (dict(grid_res=NAN), 'grid_res must be positive'),
              (dict(alpha=-0.5), 'alpha must be finite and not negative'), (dict(alpha=NAN), 'alpha must be finite and not negative'),
              (dict(alpha=INF), 'alpha must be finite and not negative'),
              (dict(H=1 << 16, W=1 << 15), 'below 2^31'))
    for fn in (built_lib.mf_cost_to_go_f32, built_lib.mf_cost_to_go_f64):
        assert fn(None, *(None,) * 7) == 1 and 'null descriptor' in err()
        for kw, text in common + ((dict(n_rounds=0), 'n_rounds must be at least 1, got 0'), (dict(n_rounds=-3), 'n_rounds must be at least 1')):
            rc, msg = field_call(fn, **kw)
            assert rc == 1 and text in msg, (kw, rc, msg)
        for k in range(6):
            rc, msg = field_call(fn, ptrs=tuple(0 if i == k else 1 for i in range(6)))
            assert rc == 1 and 'null input' in msg, (k, rc, msg)
    for fn in (built_lib.mf_extract_route_f32, built_lib.mf_extract_route_f64):
        assert fn(None, *(None,) * 10) == 1 and 'null descriptor' in err()
        for kw, text in common + ((dict(P=1), 'P must be in 2..256 vertices, got 1'), (dict(P=257), 'P must be in 2..256 vertices, got 257'),
                                  (dict(max_nodes=1), 'max_nodes must be at least 2, got 1')):
            rc, msg = route_call(fn, **kw)
            assert rc == 1 and text in msg, (kw, rc, msg)
        for k in range(9):
            rc, msg = route_call(fn, ptrs=tuple(0 if i == k else 1 for i in range(9)))
            assert rc == 1 and 'null input' in msg, (k, rc, msg)
    built_lib.mf_cost_to_go_work_ints.restype = ctypes.c_longlong
    assert built_lib.mf_cost_to_go_work_ints(None) == -1
    assert built_lib.mf_cost_to_go_work_ints(ctypes.byref(_lib.MfCostToGoDesc(S=1, H=8, W=9, n_rounds=0, grid_res=0.1))) == -1


# ---- 4. kernel metadata ------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_fit_the_lds():
    """Code-object metadata only (tools/kernel_metadata.py): three kernels in both scalar types, no scratch; the round kernel holds two
    (TILE + 2)^2 images in LDS, the others none."""
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import route
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_metadata
    rows = {name: m for o, name, m in kernel_metadata.kernels() if o == 'cost_to_go.o'}
    assert set(rows) == {f'mf::{k}<{t}>' for k in ('cost_to_go_init', 'cost_to_go_round', 'extract_route_kernel') for t in ('float', 'double')}, rows
    for name, m in rows.items():
        size = 4 if 'float' in name else 8
        assert m['scratch'] == 0 and m['agpr'] == 0 and m['vgpr'] <= 128, (name, m)
        images = 2 * (route.TILE + 2) ** 2 * size if 'round' in name else 0
        assert images <= m['lds'] <= images + 64, (name, m)
