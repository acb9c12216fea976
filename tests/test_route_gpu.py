"""The route kernels on the MI355X (mf_cost_to_go_*: tiled rounds, mf_extract_route_*: one wave per map) against the referee of
tests/route_reference.py -- a heap Dijkstra and the walk in numpy scalars of the case's dtype.  The field is the unique fixed point of
the relaxation, so every comparison is EXACT: `torch.equal` on the field with its +inf pattern, on the nodes, the path, the route cost and
the status words.  Every random case is checked (on the referee alone) to have at least half of its passable nodes reachable, so the
equality is never met by inf == inf.  Largest map: 70 x 45."""
import numpy as np
import pytest
import torch

from tests import route_reference as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RES, DMAX = rr.GRID_RES, rr.D_MAX
TORCH = {'f32': torch.float32, 'f64': torch.float64}
DTS = ['f32', 'f64']


def _tile():
    from monoforce_amd import route
    return route.TILE


def _shapes():
    T = _tile()
    return [(5, 7), (T, T), (T + 1, T + 8), (70, 45)]


def _goal_nodes(H, W):
    """Each corner, on a tile border, one node inside a border -- those that exist on the map."""
    T = _tile()
    nodes = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (min(T - 1, H - 1), min(T, W - 1)), (min(T, H - 1), min(T - 1, W - 1)),
             (min(T + 1, H - 1), W // 2), (H // 2, min(T - 2, W - 1))]
    return list(dict.fromkeys(nodes))


def _field(cost, goal, dt, **kw):
    from monoforce_amd import route
    c = torch.from_numpy(np.array(cost)).to(DEV)
    return route.cost_to_go(c, goal, RES, DMAX, return_status=True, **kw)


def _check_route(got, want, s=0):
    n = int(got['n_nodes'][s])
    assert n == want['n_nodes'], (n, want['n_nodes'])
    assert np.array_equal(got['nodes'][s, :n].cpu().numpy(), want['nodes'])
    path = got['path'] if got['path'].dim() == 2 else got['path'][s]
    assert path.dtype == torch.float32 and np.array_equal(path.cpu().numpy(), want['path'], equal_nan=True)      # (a NaN start is handed through)
    assert int(got['status'][s]) & (rr.START_UNREACHABLE | rr.TRUNCATED) == want['status']
    assert float(got['route_cost'][s]) == float(want['route_cost'])


# ---- 1. the field, exact -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('shape', range(4), ids=['5x7', 'TxT', 'T+1xT+8', '70x45'])
def test_field_and_routes_equal_the_referee(shape, dt):
    """Random obstacle maps (12 % walls over costs uniform in [0,1)), one seed per goal node; plus a route from the farthest reachable
    node with P = 2, 64 and 256 vertices, and from the goal node itself (L = 1)."""
    from monoforce_amd import route
    H, W = _shapes()[shape]
    for k, g in enumerate(_goal_nodes(H, W)):
        c = rr.case('random', H, W, dt, g, 30 + k)
        assert c['status'] == 0 and rr.reachable_share(c['field'], c['cost']) >= 0.5, (g, rr.reachable_share(c['field'], c['cost']))
        field, status, rounds = _field(c['cost'], c['goal'], dt)
        assert field.dtype == TORCH[dt] and torch.equal(field.cpu(), torch.from_numpy(np.array(c['field']))), g
        assert int(status[0]) == 0 and 1 <= int(rounds[0]) < route.default_rounds(H, W)
        if k % 3:
            continue
        far = np.unravel_index(np.argmax(np.where(np.isfinite(c['field']), c['field'], -1.0)), (H, W))
        cost_t = torch.from_numpy(np.array(c['cost'])).to(DEV)
        for node, P in ((far, 2), (far, 64), (far, 256), (g, 5)):
            start = rr.position_of(node)
            want = rr.extract_route(c['field'], c['cost'], start, c['goal'], n_vertices=P)
            got = route.extract_route(field, cost_t, start, c['goal'], RES, DMAX, n_vertices=P, status=status)
            _check_route(got, want)
            assert int(got['status'][0]) == 0 and want['nodes'][-1] == g[0] * W + g[1] and (node != g or want['n_nodes'] == 1)
            rr.check_route_is_legal(got['nodes'][0, :int(got['n_nodes'][0])].cpu().numpy(), c['cost'])      # (without the referee's field)


@pytest.mark.parametrize('dt', DTS)
def test_goal_blocked_and_off_the_map(dt):
    c = rr.case('random', 70, 45, dt, (35, 20), 3)
    cost = np.array(c['cost'])
    cost[10, 10], cost[11, 11] = 2.0, np.nan
    for goal in (rr.position_of((10, 10)), rr.position_of((11, 11)), (-3.4, 0.0), (0.0, 1.4), (float('nan'), 0.0), (float('inf'), 0.0)):
        field, status, rounds = _field(cost, goal, dt)
        assert bool(torch.isinf(field).all()) and bool((field > 0).all()) and int(status[0]) == rr.GOAL_BLOCKED and int(rounds[0]) == 0, goal


@pytest.mark.parametrize('dt', DTS)
def test_goal_on_a_tile_border_behind_a_doorway_or_in_a_dead_end(dt):
    """The goal's 0 is written by the initialisation, not by a round: the tiles that have the goal only in their halo must be woken for
    round 0 all the same.  A wall along the last row (column) of a tile whose only gap is the goal, a goal walled in on three sides whose
    only exit is in the next tile, and a corner goal whose three exits are in three other tiles: the far side is finite in the referee and
    the field equals it."""
    from monoforce_amd import route
    T = route.TILE
    far = {'row': (T + 8, 5), 'col': (5, T + 8), 'dead_end': (T + 8, 10), 'corner': (T + 8, T + 8)}
    for name, (cost, g) in rr.border_goal_maps(T, dtype=rr.DTYPES[dt]).items():
        goal = rr.position_of(g)
        ref, st = rr.cost_to_go(cost, goal)
        assert st == 0 and np.isfinite(ref[far[name]]) and rr.reachable_share(ref, cost) >= 0.9, name
        field, status, rounds = _field(cost, goal, dt)
        assert torch.equal(field.cpu(), torch.from_numpy(ref)), name
        assert int(status[0]) == 0 and int(rounds[0]) >= 2, name
        start = rr.position_of(far[name])
        want = rr.extract_route(ref, cost, start, goal, n_vertices=9)
        _check_route(route.extract_route(field, torch.from_numpy(cost).to(DEV), start, goal, RES, DMAX, n_vertices=9), want)
        assert want['status'] == 0 and want['nodes'][-1] == g[0] * 45 + g[1]


@pytest.mark.parametrize('dt', DTS)
def test_serpentine_default_rounds_too_few_rounds_and_again(dt):
    """Walls every 7 rows of a 70 x 45 map with one-node gaps on alternating sides: the route re-enters the tile columns once per lane."""
    from monoforce_amd import route
    c = rr.case('serpentine', 70, 45, dt, (0, 0))
    want = torch.from_numpy(np.array(c['field']))
    assert np.isfinite(c['field'][69, 44]) and rr.reachable_share(c['field'], c['cost']) == 1.0
    cost = torch.from_numpy(np.array(c['cost'])).to(DEV)
    field, status, rounds = route.cost_to_go(cost, c['goal'], RES, DMAX, return_status=True)
    assert torch.equal(field.cpu(), want) and int(status[0]) == 0
    print(f'serpentine 70x45 {dt}: rounds_used {int(rounds[0])} of {route.default_rounds(70, 45)}')
    few, status2, rounds2 = route.cost_to_go(cost, c['goal'], RES, DMAX, n_rounds=2, return_status=True)
    assert int(status2[0]) == rr.NOT_CONVERGED and int(rounds2[0]) == 2
    assert bool((few.cpu() >= want).all()) and not torch.equal(few.cpu(), want)
    again, status3, rounds3 = route.cost_to_go(cost, c['goal'], RES, DMAX, return_status=True, out=few)
    assert again is few and torch.equal(few.cpu(), want) and int(status3[0]) == 0 and int(rounds3[0]) == int(rounds[0])
    start = rr.position_of((69, 44))
    ref = rr.extract_route(c['field'], c['cost'], start, c['goal'], n_vertices=64)
    got = route.extract_route(field, cost, start, c['goal'], RES, DMAX, n_vertices=64)
    _check_route(got, ref)
    assert ref['n_nodes'] > 9 * 44
    # max_nodes shorter than the route: TRUNCATED, resampled from the nodes walked
    ref = rr.extract_route(c['field'], c['cost'], start, c['goal'], n_vertices=16, max_nodes=50)
    got = route.extract_route(field, cost, start, c['goal'], RES, DMAX, n_vertices=16, max_nodes=50)
    _check_route(got, ref)
    assert ref['status'] == rr.TRUNCATED and int(got['n_nodes'][0]) == 50


@pytest.mark.parametrize('dt', DTS)
def test_views_three_maps_scalars_and_determinism(dt):
    from monoforce_amd import ops, route  # noqa: F401
    H, W = 70, 45
    goals = [(0, 0), (69, 44), (31, 32)]
    cases = [rr.case('random', H, W, dt, g, 20 + k) for k, g in enumerate(goals)]
    three = torch.stack([torch.from_numpy(np.array(c['cost'])) for c in cases]).to(DEV)
    want = torch.stack([torch.from_numpy(np.array(c['field'])) for c in cases])
    goal_t = torch.tensor([c['goal'] for c in cases], dtype=TORCH[dt], device=DEV)
    # S = 3 with three goals
    f3, st3, _ = route.cost_to_go(three, goal_t, RES, DMAX, return_status=True)
    assert torch.equal(f3.cpu(), want) and st3.tolist() == [0, 0, 0]
    # a [:, 0] channel view and a row-sliced view, read in place (the rest is poison)
    chan = torch.full((3, 2, H, W), float('nan'), dtype=TORCH[dt], device=DEV)
    chan[:, 0] = three
    assert not chan[:, 0].is_contiguous() and torch.equal(route.cost_to_go(chan[:, 0], goal_t, RES, DMAX).cpu(), want)
    big = torch.full((H + 6, W + 11), -1.0, dtype=TORCH[dt], device=DEV)
    big[3:3 + H, :W] = three[1]
    crop = big[3:3 + H, :W]
    assert crop.stride(0) == W + 11 and torch.equal(route.cost_to_go(crop, cases[1]['goal'], RES, DMAX).cpu(), want[1])
    # two calls bit-identical; the registered op
    again = route.cost_to_go(three, goal_t, RES, DMAX)
    assert torch.equal(again, f3)
    op_f, op_s, op_r = torch.ops.monoforce.cost_to_go(three, goal_t, RES, DMAX, 1.0, 4.0, 0)
    assert torch.equal(op_f, f3) and op_s.tolist() == [0, 0, 0]
    # routes of the three maps in one launch: to its goal from another map's goal (which may be in a walled-off pocket or a wall here)
    starts = goal_t[[1, 2, 0]].contiguous()
    got = route.extract_route(f3, three, starts, goal_t, RES, DMAX, n_vertices=33, status=st3)
    op = torch.ops.monoforce.extract_route(f3, three, starts, goal_t, RES, DMAX, 1.0, 4.0, 33, 0)
    assert got['path'].shape == (3, 33, 2) and torch.equal(op[0], got['path']) and torch.equal(op[1], got['nodes'])
    for s, c in enumerate(cases):
        ref = rr.extract_route(c['field'], c['cost'], cases[(s + 1) % 3]['goal'], c['goal'], n_vertices=33)
        _check_route(got, ref, s)
    # alpha = 0 and lethal = +inf (only non-finite costs are walls)
    c = cases[2]
    ref, _ = rr.cost_to_go(c['cost'], c['goal'], lethal=float('inf'), alpha=0.0)
    f, st, _ = _field(c['cost'], c['goal'], dt, lethal=float('inf'), alpha=0.0)
    assert torch.equal(f.cpu(), torch.from_numpy(ref)) and int(st[0]) == 0 and int(np.isinf(ref).sum()) == int(np.isnan(c['cost']).sum())


@pytest.mark.parametrize('dt', DTS)
def test_start_in_a_walled_off_pocket_and_off_the_map(dt):
    from monoforce_amd import route
    T = rr.DTYPES[dt]
    cost = np.full((33, 40), 0.125, T)
    cost[10:15, 10] = cost[10:15, 14] = cost[10, 10:15] = cost[14, 10:15] = 3.0      # a closed box around (12, 12)
    goal = rr.position_of((30, 35))
    ref, _ = rr.cost_to_go(cost, goal)
    field, status, _ = _field(cost, goal, dt)
    assert torch.equal(field.cpu(), torch.from_numpy(ref)) and np.isinf(ref[12, 12]) and np.isfinite(ref[9, 9])
    cost_t = torch.from_numpy(cost).to(DEV)
    for start in (rr.position_of((12, 12)), rr.position_of((10, 12)), (-3.3, 0.0), (0.05, 0.85), (float('nan'), 0.0)):
        want = rr.extract_route(ref, cost, start, goal, n_vertices=7)
        got = route.extract_route(field, cost_t, start, goal, RES, DMAX, n_vertices=7)
        _check_route(got, want)
        assert want['status'] == rr.START_UNREACHABLE and int(got['status'][0]) == rr.START_UNREACHABLE and int(got['n_nodes'][0]) == 0
        p = got['path'].cpu()
        assert p.shape == (7, 2) and torch.equal(p.isnan(), torch.tensor(start, dtype=torch.float32).isnan().expand(7, 2))
        assert torch.equal(p.nan_to_num(7.0), torch.tensor(start, dtype=torch.float32).expand(7, 2).nan_to_num(7.0))


# ---- 2. capture --------------------------------------------------------------------------------------------------------------------------
def _cfg():
    from monoforce_amd.dphys_config import DPhysConfig
    from monoforce_amd import synthetic as syn
    pts4, masks = syn.robot_points_4()
    cfg = DPhysConfig(robot='tradr', grid_res=0.1, robot_points=pts4, driving_parts=masks)
    cfg.d_max = 3.2
    return cfg


def test_map_then_route_replay_as_one_graph(monkeypatch):
    """`tm(z)` then `rp(tm.cost, start, goal)` captured once on one stream: the replay equals the eager calls, a replay after
    `goal.copy_()` and `z.copy_()` equals fresh eager calls on those.  "No parallel branches" is checked by PROXY: the graph itself is not
    inspected (the runtime's graph dump writes no file); instead every launch call the Python layer made during the capture is asserted to
    have been handed the one capture stream, i.e. nothing was forked to a side stream."""
    from monoforce_amd import _lib, costmap as cm, route
    from monoforce_amd.capture import capture
    from tests import traversability_reference as tr
    cfg = _cfg()
    H = W = 64
    z0, z1 = (tr.terrain(1, H, W, s)[0].float().to(DEV) for s in (11, 12))
    z1[20:24, 30] = float('nan')
    start = torch.tensor([-2.0, -2.5], device=DEV)
    goal = torch.tensor([2.0, 1.5], device=DEV)
    z = z0.clone()
    tm, rp = cm.TraversabilityMap(cfg, radius=0.3), route.RoutePlanner(cfg, n_vertices=32, lethal=0.9)

    def run():
        return rp(tm(z), start, goal)

    def fresh(zz, gg):
        tm2, rp2 = cm.TraversabilityMap(cfg, radius=0.3), route.RoutePlanner(cfg, n_vertices=32, lethal=0.9)
        rp2(tm2(zz), start, gg)
        return [t.clone() for t in (rp2.path, rp2.field, rp2.status, rp2.route_cost, rp2.n_nodes, rp2.nodes[:, :int(rp2.n_nodes[0])])]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    streams, stream_ptr = [], _lib.stream_ptr
    monkeypatch.setattr(_lib, 'stream_ptr', lambda device: streams.append(stream_ptr(device).value) or stream_ptr(device))
    with capture(graph, stream=s, capture_error_mode='thread_local'):
        static = run()
    monkeypatch.undo()
    # one launch call for the map, one for the field (1 + n_rounds kernels), one for the route -- all handed the capture stream: nothing was
    # forked to another stream, so the captured graph is a chain
    assert streams == [s.cuda_stream] * 3 and rp.n_rounds == route.default_rounds(H, W)
    assert static is rp.path and static.shape == (32, 2)
    ptrs = [t.data_ptr() for t in (rp.path, rp.field, rp.nodes)]
    for zz, gg in ((z0, goal.clone()), (z1, torch.tensor([2.5, 2.5], device=DEV))):
        z.copy_(zz)
        goal.copy_(gg)
        graph.replay()
        torch.cuda.synchronize()
        got = [rp.path, rp.field, rp.status, rp.route_cost, rp.n_nodes, rp.nodes[:, :int(rp.n_nodes[0])]]      # (nodes past n_nodes are not written)
        want = fresh(zz, gg)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert int(rp.status[0]) == 0 and int(rp.n_nodes[0]) > 40 and float((rp.path[-1] - gg).abs().max()) < 1e-5
    assert [t.data_ptr() for t in (rp.path, rp.field, rp.nodes)] == ptrs


# ---- 3. the planner ----------------------------------------------------------------------------------------------------------------------
def test_route_round_a_u_shaped_wall_feeds_the_planner():
    """A U-shaped lethal wall on a 64 x 64 map, open towards -x, the start inside it and the goal behind its bottom: the straight line is
    blocked, `rp.path` leaves through the opening and goes round an arm.  `MPPIPlanner.step(cost_map=, path=rp.path)` runs on it and its
    cross-track term is what `torch.ops.monoforce.pose_costs` gives for that polyline on the step's own poses."""
    from monoforce_amd import MPPIPlanner, RoutePlanner
    from monoforce_amd import ops  # noqa: F401
    from monoforce_amd import synthetic as syn
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 3.2)
    dp.dphys_cfg.traj_sim_time = 0.2
    dp = type(dp)(dp.dphys_cfg, device=DEV)                      # rebuild the time grid: T = 20
    B = 64
    keep_out = torch.zeros(64, 64, device=DEV)
    keep_out[40, 16:49] = 1.0                                    # the bottom of the U, x = 0.8
    keep_out[24:41, 16] = keep_out[24:41, 48] = 1.0              # its arms, y = -1.6 and y = 1.6, from x = -0.8
    start = torch.tensor([0.0, 0.0], device=DEV)                 # node (32, 32), inside
    goal = torch.tensor([2.0, 0.0], device=DEV)                  # node (52, 32), behind the bottom
    rp = RoutePlanner(dp, n_vertices=64, lethal=0.5)
    path = rp(keep_out, start, goal)
    assert path is rp.path and path.shape == (64, 2) and int(rp.status[0]) == 0
    n = int(rp.n_nodes[0])
    nodes = rp.nodes[0, :n].cpu().numpy()
    rr.check_route_is_legal(nodes, keep_out.cpu().numpy(), lethal=0.5)
    ii, jj = nodes // 64, nodes % 64
    assert (ii[0], jj[0]) == (32, 32) and (ii[-1], jj[-1]) == (52, 32)
    assert ii.min() < 24 and (jj.min() < 16 or jj.max() > 48)   # out through the opening, round an arm
    ref, _ = rr.cost_to_go(keep_out.cpu().numpy(), (2.0, 0.0), lethal=0.5)
    assert float(rp.route_cost[0]) == float(ref[32, 32]) and torch.equal(rp.field.cpu(), torch.from_numpy(ref))
    assert float((path[0] - start).abs().max()) < 1e-5 and float((path[-1] - goal).abs().max()) < 1e-5 and float(path[:, 0].min()) < -0.5
    mp = MPPIPlanner(dp, n_trajs=B, weights=dict(inclination=1.0, force=0.02, goal=1.0, map=1.0, path=0.5), lethal=0.5)
    z = torch.zeros(64, 64, device=DEV)
    g = torch.Generator().manual_seed(5)
    noise = (torch.randn(B, 20, 2, generator=g) + 2.0 * torch.randn(B, 1, 2, generator=g)).to(DEV)
    out = mp.step(z, goal, noise=noise, cost_map=keep_out, path=rp.path)
    assert out['pose_terms'].shape == (B, 2)
    _, terms = torch.ops.monoforce.pose_costs(out['Xs'], out['Rs'], mp.footprint, keep_out, rp.path, None, 0.1, 3.2, mp.lethal, mp.off_map,
                                              list(mp.pose_weights))
    assert torch.equal(out['pose_terms'][:, 1], terms[:, 1]) and float(terms[:, 1].max()) > 0 and bool(torch.isfinite(terms[:, 1]).all())
