"""Pose costs on the GPU (monoforce_amd/csrc/pose_costs.hip, torch.ops.monoforce.pose_costs, MPPIPlanner / TrajectoryShooter with a cost map and a
path): the kernel against the referee of tests/pose_costs_reference.py (pinned on the CPU in tests/test_pose_costs_cpu.py), layouts and
determinism, isolation of a lethal rollout, the term switches, a real rollout, the planner stage by stage, its behaviour, capture, the shooter.

Error bars as in tests/test_mppi_gpu.py: "rel-to-absmax" against the referee's float64 evaluation of the same float32 inputs, bar
max(1e-5, 3 d32) with d32 the referee's own float32-to-float64 distance (1e-7 .. 3e-7 at the shapes of pc.SHAPES: the floor governs; up to 4.3e-6 on the map term of pc.CONFIG_SHAPES, where the maximum
over thousands of rollouts meets the worst rounding of the blend).  The sets of +inf
costs must be EQUAL; the constructed inputs keep every discontinuous decision 1e-3 away from its threshold (tests/pose_costs_cases.py)."""
import pytest
import torch

from monoforce_amd import ops as mf_ops      # (registers torch.ops.monoforce.*)
from tests import helpers as hp
from tests import mppi_reference as mref
from tests import pose_costs_cases as pc
from tests import pose_costs_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
INF = float('inf')


def _bar(r32, r64):
    return max(1e-5, 3 * hp.rel_err(r32, r64))


def _close(got, r32, r64, what):
    err, bar = hp.rel_err(got, r64), _bar(r32, r64)
    print(f'{what}: err {err:.3g} bar {bar:.3g}')
    return err <= bar


def _op(Xs, Rs, points, cost_map, path, base, grid_res, d_max, lethal, off_map, weights):
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    c, t = torch.ops.monoforce.pose_costs(d(Xs), d(Rs), d(points), d(cost_map), d(path), d(base), grid_res, d_max, lethal, off_map, list(weights))
    return c.cpu(), t.cpu()


def _check(costs, terms, args, scalars, weights, what):
    """costs / terms of the op (CPU tensors) against the referee on `args` = (Xs, Rs, points, cost_map, path, base), CPU float32."""
    c32, t32 = ref.pose_costs(*args, *scalars, weights)
    c64, t64 = ref.pose_costs(*[None if a is None else a.double() for a in args], *scalars, weights)
    lethal = torch.isinf(c64) & (c64 > 0)
    assert torch.equal(torch.isinf(c32) & (c32 > 0), lethal), f'{what}: the referee itself is not decided in float32'
    assert torch.equal(torch.isinf(costs) & (costs > 0), lethal), f'{what}: the +inf sets differ'
    assert torch.equal(torch.isinf(terms[:, 0]), torch.isinf(t64[:, 0]))
    fin = ~lethal
    if bool(fin.any()):
        assert _close(costs[fin], c32[fin], c64[fin], what + ' costs')
        if args[3] is not None:
            assert _close(terms[fin, 0], t32[fin, 0], t64[fin, 0], what + ' map term')
    if args[4] is not None:
        assert _close(terms[:, 1], t32[:, 1], t64[:, 1], what + ' path term')
    else:
        assert not bool(terms[:, 1].any())
    if args[3] is None:
        assert not bool(terms[:, 0].any())
    return lethal


@pytest.fixture(scope='module')
def cases():
    """The constructed inputs, made once per shape and left unchanged."""
    return {s: pc.constructed(*s) for s in pc.SHAPES}


def _args(c, cost_map=True, path=True, base=True):
    return (c['Xs'], c['Rs'], c['points'], c['cost_map'] if cost_map else None, c['path'] if path else None, c['base'] if base else None)


# ---- 1. constructed poses ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', pc.SHAPES)
def test_constructed_poses_match_the_referee(cases, shape):
    c = cases[shape]
    print(f'{shape}: {c["redraws"]} poses redrawn')
    for off_map in (INF, 1.5):
        scalars = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, off_map)
        costs, terms = _op(*_args(c), *scalars, (0.7, 1.3))
        lethal = _check(costs, terms, _args(c), scalars, (0.7, 1.3), f'{shape} off_map={off_map}')
        if shape[0] >= 65:
            assert bool(lethal.any()) and not bool(lethal.all())      # both kinds occur, or the test shows nothing


# ---- 1b. every launch configuration ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', pc.CONFIG_SHAPES)
def test_every_launch_configuration_matches_the_referee(shape):
    """The workgroup shapes the host picks from B and N, and the trips of the pose loop beyond the first (pc.CONFIG_SHAPES says which shape
    reaches what).  On the CPU the referee's float32 and float64 +inf sets are equal at every shape, both kinds of cost occur at every one
    (1 .. 8091 lethal rollouts), and its own float32-to-float64 distance is at most 4.3e-6 (the map term at (8193, 3, 4)): the bar of the
    file header, unchanged."""
    c = pc.constructed(*shape)
    print(f'{shape}: {c["redraws"]} poses redrawn')
    for off_map in (INF, 1.5):
        scalars = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, off_map)
        costs, terms = _op(*_args(c), *scalars, (0.7, 1.3))
        lethal = _check(costs, terms, _args(c), scalars, (0.7, 1.3), f'{shape} off_map={off_map}')
        assert bool(lethal.any()) and not bool(lethal.all())      # both kinds occur, or the test shows nothing


def test_a_body_or_a_path_beyond_the_tables_is_refused():
    """N = 1025 and P = 257 do not fit the LDS tables: an error from the entry point's checks (which run before the launch, see
    tests/test_pose_costs_cpu.py), the one next to it still answers."""
    c = pc.constructed(5, 9, 1024)
    scalars = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, INF)
    a = dict(zip(('Xs', 'Rs', 'points', 'cost_map', 'path', 'base'), _args(c)))
    with pytest.raises(RuntimeError, match='1024 footprint points'):
        _op(*{**a, 'points': torch.cat([c['points'], c['points'][:1]])}.values(), *scalars, (0.7, 1.3))
    with pytest.raises(RuntimeError, match='256 path vertices'):
        _op(*{**a, 'path': pc.walk_path(257)}.values(), *scalars, (0.7, 1.3))
    _check(*_op(*a.values(), *scalars, (0.7, 1.3)), tuple(a.values()), scalars, (0.7, 1.3), 'after the refusals')


@pytest.mark.parametrize('P', pc.PATH_LENGTHS)
@pytest.mark.parametrize('shape', pc.RECT_SHAPES)
def test_paths_of_every_length(cases, shape, P):
    """A path of one vertex, of one segment, and of 16, 17 and 255 segments (the 16-lane deal of the points kernel: one full trip, a second
    trip of lane 0 alone, sixteen trips with the last one short), in both kernels: a random walk inside the map with one zero-length segment."""
    c = cases[shape]
    path = pc.walk_path(P)
    assert tuple(path.shape) == (P, 2) and (P < 3 or int((path[1:] == path[:-1]).all(-1).sum()) == 1)
    scalars = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, 1.5)
    for what, a, w in (('with the map', (c['Xs'], c['Rs'], c['points'], c['cost_map'], path, c['base']), (0.7, 1.3)),
                       ('path only', (c['Xs'], c['Rs'], c['points'], None, path, None), (0.0, 1.0))):
        costs, terms = _op(*a, *scalars, w)
        _check(costs, terms, a, scalars, w, f'{shape} P={P} {what}')
        assert float(terms[:, 1].min()) > 0


@pytest.fixture(scope='module')
def rect_cases():
    return {s: pc.constructed(*s, map_shape=pc.RECT) for s in pc.RECT_SHAPES}


@pytest.mark.parametrize('shape', pc.RECT_SHAPES)
def test_a_map_that_is_not_square(rect_cases, shape):
    """48 x 80 nodes, the lethal block at second-axis indices 52 .. 65: `sample_map` takes one bound and one clamp from H, the other bound, the
    other clamp and the row stride from W, and on a square map any of them could be swapped unnoticed.  The referee with the swap applied,
    float64 on the CPU, against the referee as it is -- (65, 5, 7) / (33, 3, 223), off_map = inf and 1.5:
      bounds swapped   the +inf set differs in 12, 8 / 4, 5 rollouts; the map term of the rollouts finite in both moves by 0.53 / 0.43 (off_map = 1.5)
      clamps swapped   8, 14 / 5, 14 rollouts; 6.2e-3 .. 4.8e-2
      stride swapped   23, 32 / 11, 16 rollouts; 0.12 .. 0.22
    where the test asks for EQUAL +inf sets and a map term within 1e-5."""
    c = rect_cases[shape]
    assert tuple(c['cost_map'].shape) == pc.RECT and float(c['cost_map'][:, 48:].max()) == 5.0 and float(c['cost_map'][:, :48].max()) < 1.0
    for off_map in (INF, 1.5):
        scalars = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, off_map)
        costs, terms = _op(*_args(c), *scalars, (0.7, 1.3))
        lethal = _check(costs, terms, _args(c), scalars, (0.7, 1.3), f'{shape} on 48x80 off_map={off_map}')
        assert bool(lethal.any()) and not bool(lethal.all())
    # the cells a rollout reads, counted with the row stride W: raising one that only rollout b0 reads makes b0 lethal and no other
    read = pc.cells_read(c, pc.RECT)
    scalars = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, INF)
    costs, _ = _op(*_args(c), *scalars, (0.7, 1.3))
    B = shape[0]
    b0, cell = next((b, k) for b in range(B) if bool(torch.isfinite(costs[b]))
                    for k in sorted(read[b]) if not any(k in read[o] for o in range(B) if o != b))
    m = c['cost_map'].clone()
    m.view(-1)[cell] = 100.0
    got, _ = _op(c['Xs'], c['Rs'], c['points'], m, c['path'], c['base'], *scalars, (0.7, 1.3))
    keep = torch.arange(B) != b0
    assert float(got[b0]) == INF and torch.equal(got[keep], costs[keep])


# ---- 2. layouts and determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(65, 5, 7), (130, 11, 65)])
def test_layouts_and_determinism(cases, shape):
    c = cases[shape]
    B = shape[0]
    Xs, Rs, pts, cm, path, base = (t.to(DEV) for t in _args(c))
    tail = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, INF, [0.7, 1.3])
    costs, terms = torch.ops.monoforce.pose_costs(Xs, Rs, pts, cm, path, base, *tail)
    # the rollout's layout: time-major buffers viewed [B,Tp,...]
    Xt, Rt = Xs.transpose(0, 1).contiguous().transpose(0, 1), Rs.transpose(0, 1).contiguous().transpose(0, 1)
    assert Xt.stride() == (3, 3 * B, 1) and Rt.stride() == (9, 9 * B, 3, 1)
    c_tm, t_tm = torch.ops.monoforce.pose_costs(Xt, Rt, pts, cm, path, base, *tail)
    c_2, t_2 = torch.ops.monoforce.pose_costs(Xs, Rs, pts, cm, path, base, *tail)
    assert torch.equal(c_tm, costs) and torch.equal(t_tm, terms) and torch.equal(c_2, costs) and torch.equal(t_2, terms)
    # costs written in place over base_costs
    buf = base.clone()
    c_in, t_in = mf_ops.pose_costs_into(Xt, Rt, pts, cm, path, buf, *tail, buf)
    assert c_in is buf and torch.equal(buf, costs) and torch.equal(t_in, terms)
    assert bool(torch.isinf(costs).any()) and bool(torch.isfinite(costs).any())


# ---- 3. isolation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(65, 5, 7), (33, 3, 223)])
def test_one_lethal_rollout_leaves_the_others_bit_identical(cases, shape):
    c = cases[shape]
    B = shape[0]
    scalars = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, INF)
    costs, _ = _op(*_args(c), *scalars, (0.7, 1.3))
    read = pc.cells_read(c)
    b0, cell = next((b, k) for b in range(B) if bool(torch.isfinite(costs[b]))
                    for k in sorted(read[b]) if not any(k in read[o] for o in range(B) if o != b))       # a cell only rollout b0 reads
    keep = torch.arange(B) != b0

    def changed(**kw):
        a = dict(zip(('Xs', 'Rs', 'points', 'cost_map', 'path', 'base'), _args(c)))
        a.update(kw)
        return _op(*a.values(), *scalars, (0.7, 1.3))[0]

    for what, value in (('cell raised', 100.0), ('NaN cell', float('nan'))):
        m = c['cost_map'].clone()
        m.view(-1)[cell] = value
        got = changed(cost_map=m)
        assert float(got[b0]) == INF and torch.equal(got[keep], costs[keep]), what
    Rs = c['Rs'].clone()
    Rs[b0, shape[1] - 1, 0, 1] = float('nan')      # an entry of R the footprint reads: the points leave the map (off_map = inf)
    got = changed(Rs=Rs)
    assert float(got[b0]) == INF and torch.equal(got[keep], costs[keep])


# ---- 4. term switches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(65, 5, 7), (130, 11, 65)])
def test_term_switches(cases, shape):
    c = cases[shape]
    scalars = (pc.GRID_RES, pc.D_MAX, pc.LETHAL, 1.5)
    for what, a, w in (('map only', _args(c, path=False), (1.0, 0.0)), ('path only', _args(c, cost_map=False), (0.0, 1.0)),
                       ('both', _args(c), (0.7, 1.3)), ('no base', _args(c, base=False), (0.7, 1.3))):
        _check(*_op(*a, *scalars, w), a, scalars, w, f'{shape} {what}')
    # w_map = 0 with a map given: the path-only cost bit for bit, +inf where the map is lethal
    path_only, _ = _op(*_args(c, cost_map=False), *scalars, (0.0, 1.3))
    gated, terms = _op(*_args(c), *scalars, (0.0, 1.3))
    lethal = _check(gated, terms, _args(c), scalars, (0.0, 1.3), f'{shape} w_map = 0')
    assert bool(lethal.any()) and not bool(lethal.all())
    assert torch.equal(gated[~lethal], path_only[~lethal]) and bool(torch.isfinite(path_only).all())


# ---- 5. a real rollout -----------------------------------------------------------------------------------------------------------------
def test_pose_costs_of_a_real_rollout():
    """The bump_rollout recipe of tests/test_mppi_gpu.py, its strided views fed straight into the op."""
    from monoforce_amd import synthetic as syn
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    B, T = 37, 120
    dp = make_dphysics(pts, masks, 1, 0.1, 3.2, points_per_lane=1)
    z = torch.stack([syn.bump_terrain(syn.bump_params(3 + k % 3), 3.2, 0.1) * 0.5 for k in range(B)]).to(DEV)
    out = dp.rollout_costs(z, syn.varying_controls(B, T, seed=5).to(DEV), pose_stride=7)
    Tp = out['Xs'].shape[1]
    assert out['Xs'].shape == (B, Tp, 3) and out['Xs'].stride() == (3, 3 * B, 1) and out['Rs'].stride() == (9, 9 * B, 3, 1)
    g = torch.Generator().manual_seed(2)
    cm = torch.rand(64, 64, generator=g)
    points = torch.as_tensor(pts, dtype=torch.float32)
    path = torch.tensor([[0.0, 0.2], [0.5, 0.3], [1.0, 0.8]])
    base = torch.rand(B, generator=g)
    scalars = (0.1, 3.2, INF, INF)
    costs, terms = torch.ops.monoforce.pose_costs(out['Xs'], out['Rs'], points.to(DEV), cm.to(DEV), path.to(DEV), base.to(DEV), *scalars, [1.0, 2.0])
    args = (out['Xs'].cpu(), out['Rs'].cpu(), points, cm, path, base)
    lethal = _check(costs.cpu(), terms.cpu(), args, scalars, (1.0, 2.0), 'rollout')
    assert not bool(lethal.any()) and float(terms[:, 0].min()) > 0 and float(terms[:, 1].max()) > 0.05


# ---- 6. the planner, stage by stage ----------------------------------------------------------------------------------------------------
def _planner_inputs():
    g = torch.Generator().manual_seed(6)
    cm = torch.rand(128, 128, generator=g)
    cm[70:74, 60:67] = 5.0                      # x in [0.6, 0.9], y in [-0.4, 0.2]: ahead of the start, reached by the faster rollouts
    path = torch.tensor([[0.0, 0.3], [0.4, 0.35], [0.7, 0.55], [0.9, 0.9]])
    return cm, path


def _spread_noise(B, T, g):
    """Per-step noise plus a per-rollout constant: independent steps alone average out over the horizon (every rollout would end within
    centimetres of the others, all of them in the block or none)."""
    return torch.randn(B, T, 2, generator=g) + 2.0 * torch.randn(B, 1, 2, generator=g)


def test_planner_step_stage_by_stage():
    from tests.test_mppi_gpu import _planner
    B, T = 256, 100
    mp, dp, z = _planner(B, 'bump', weights=dict(inclination=1.0, force=0.02, goal=1.0, map=0.5, path=0.75), lethal=2.0)
    cm, path = _planner_inputs()
    g = torch.Generator().manual_seed(4)
    nominal0 = torch.stack([torch.full((T,), 0.6), 0.3 * torch.sin(torch.arange(T) / 20.0)], -1)
    mp.reset(nominal0.to(DEV))
    noise, goal = _spread_noise(B, T, g), torch.tensor([1.0, 0.5])
    out = mp.step(z, goal.to(DEV), noise=noise.to(DEV), cost_map=cm.to(DEV), path=path.to(DEV))
    assert set(out) == {'controls', 'cost_rows', 'Xs', 'Rs', 'pose_steps', 'force_cost', 'terms', 'costs', 'weights', 'best', 'n_valid', 'nominal', 'pose_terms'}
    # default pose stride with a map in play: one kept pose per cell at full speed (0.1 m / (1 m/s * 0.01 s) = 10 steps)
    assert out['Xs'].shape == (B, 11, 3) and out['pose_terms'].shape == (B, 2) and out['terms'].shape == (B, 3)
    assert out['pose_steps'].tolist() == [0, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99]
    # pose costs: the referee on the step's own poses and on path_costs' result (recomputed from the step's rows: bit-identical from call to call)
    base, terms = torch.ops.monoforce.path_costs(out['cost_rows'], out['force_cost'], out['Xs'][:, -1], goal.to(DEV), list(mp.weights))
    assert torch.equal(terms, out['terms'])
    args = (out['Xs'].cpu(), out['Rs'].cpu(), mp.footprint.cpu(), cm, path, base.cpu())
    lethal = _check(out['costs'].cpu(), out['pose_terms'].cpu(), args, (0.1, 6.4, 2.0, INF), mp.pose_weights, 'step')
    assert bool(lethal.any()) and not bool(lethal.all()) and int(out['n_valid']) == B - int(lethal.sum())
    # the update: mppi_reference on the step's own costs
    cpu = {k: v.cpu() for k, v in out.items()}
    assert torch.equal(cpu['controls'], mref.perturb(nominal0, noise, mp.sigma, mp.lo, mp.hi, mp.keep_nominal))
    n32, w32, b32, v32 = mref.update(cpu['costs'], cpu['controls'], nominal0, mp.lam)
    n64, w64, b64, v64 = mref.update(cpu['costs'].double(), cpu['controls'].double(), nominal0.double(), mp.lam)
    assert (int(cpu['best']), int(cpu['n_valid'])) == (b64, v64)
    for k, r32, r64 in (('weights', w32, w64), ('nominal', n32, n64)):
        err, bar = hp.rel_err(cpu[k], r64), max(2e-6, 3 * hp.rel_err(r32, r64))
        print(f'step {k}: err {err:.3g} bar {bar:.3g}')
        assert err <= bar
    # without map and path: today's dict; a weight without its input is an error
    mp0, _, _ = _planner(B, 'bump')
    out0 = mp0.step(z, goal.to(DEV), noise=noise.to(DEV))
    assert set(out0) == {'controls', 'cost_rows', 'Xs', 'Rs', 'pose_steps', 'force_cost', 'terms', 'costs', 'weights', 'best', 'n_valid', 'nominal'}
    assert out0['Xs'].shape == (B, 3, 3)             # the 0.5 s default stride
    with pytest.raises(ValueError, match='no cost_map'):
        mp.step(z, goal.to(DEV), noise=noise.to(DEV), path=path.to(DEV))


# ---- 7. planner behaviour, directional only ----------------------------------------------------------------------------------------------
def _nominal_rollout(dp, z, mp):
    return dp.rollout_costs(z.unsqueeze(0), mp.nominal.unsqueeze(0).clone(), project=False, pose_stride=10)['Xs'][0].cpu()


def test_plan_follows_the_map_and_the_path_on_flat_ground():
    """Flat ground, B = 512, 8 iterations, sigma = (0.6, 1.5), the same fixed noise for every plan (white noise moves a pose by centimetres only:
    the weights are chosen so that centimetres show in the softmin at lam = 0.05).
    Observed on an MI355X: the plan without the map ends at y = +0.0043 m, the plan with it (weight 5) at y = -0.0606 m: a margin of 0.065 m,
    asserted as 0.02; mean cross-track distance 0.3536 m for the zero nominal, 0.1290 m for the planned one (path weight 5): a margin of 0.225 m,
    asserted as 0.05.  The noise is an argument and every kernel on the way has a fixed summation order, so the spread from call to call is
    that of the rollout kernel alone."""
    from tests.test_mppi_gpu import _planner
    B, T, iters = 512, 100, 8
    noise = torch.randn(iters, B, T, 2, generator=torch.Generator().manual_seed(7)).to(DEV)
    kw = dict(n_iters=iters, sigma=(0.6, 1.5))
    # a map that grows linearly with y (0 at y = -6.4, 1 per metre), the goal straight ahead, the plans start from "drive straight on"
    ys = torch.arange(128, dtype=torch.float32) * 0.1
    cm = ys.expand(128, 128).contiguous().to(DEV)
    goal = torch.tensor([1.0, 0.0], device=DEV)
    straight = torch.tensor([0.6, 0.0], device=DEV).expand(T, 2)
    ends = {}
    for name, w_map in (('plain', 0.0), ('map', 5.0)):
        mp, dp, z = _planner(B, 'flat', weights=dict(inclination=0.0, force=0.0, goal=1.0, map=w_map), **kw)
        mp.reset(straight)
        mp.plan(z, goal, noise=noise, cost_map=cm if w_map else None)
        ends[name] = _nominal_rollout(dp, z, mp)[-1]
    print(f'end of the planned path: without the map y = {float(ends["plain"][1]):+.4f} m, with it y = {float(ends["map"][1]):+.4f} m')
    assert float(ends['map'][1]) < float(ends['plain'][1]) - 0.02
    # a left-curving path that crosses ahead of the start, no goal term, the plan starts from the zero nominal
    path = torch.tensor([[0.2, -0.3], [0.6, 0.1], [0.8, 0.6]])
    mp, dp, z = _planner(B, 'flat', weights=dict(inclination=0.0, force=0.0, goal=0.0, path=5.0), **kw)
    d_zero = float(ref.polyline_distance(_nominal_rollout(dp, z, mp)[:, :2], path).mean())
    mp.plan(z, goal, noise=noise, path=path.to(DEV))
    d_plan = float(ref.polyline_distance(_nominal_rollout(dp, z, mp)[:, :2], path).mean())
    print(f'mean cross-track distance: zero nominal {d_zero:.4f} m, planned nominal {d_plan:.4f} m')
    assert d_plan < d_zero - 0.05


# ---- 8. capture -----------------------------------------------------------------------------------------------------------------------
def test_step_with_map_and_path_can_be_captured_and_follows_the_map():
    from monoforce_amd.capture import capture
    from tests.test_mppi_gpu import _planner
    B, T = 256, 100
    noise = _spread_noise(B, T, torch.Generator().manual_seed(9)).to(DEV)
    nominal0 = torch.stack([torch.full((T,), 0.5), torch.full((T,), 0.2)], -1).to(DEV)
    goal = torch.tensor([1.0, 0.5], device=DEV)
    cm0, path0 = _planner_inputs()
    weights = dict(map=0.5, path=0.75)
    eager, _, z = _planner(B, 'bump', weights=weights, lethal=2.0)
    eager.reset(nominal0)
    want = {k: v.clone() for k, v in eager.step(z, goal, noise=noise, cost_map=cm0.to(DEV), path=path0.to(DEV)).items()}
    mp, _, _ = _planner(B, 'bump', weights=weights, lethal=2.0)
    cm, path = cm0.to(DEV), path0.to(DEV)
    mp.step(z, goal, noise=noise, cost_map=cm, path=path)            # warm-up: every cached constant exists before the capture
    mp.reset(nominal0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture(graph):
        out = mp.step(z, goal, noise=noise, cost_map=cm, path=path)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out['controls'], want['controls']) and torch.equal(torch.isinf(out['costs']), torch.isinf(want['costs']))
    fin = torch.isfinite(want['costs'])
    assert bool(fin.any()) and not bool(fin.all())
    for k, floor in (('costs', 1e-5), ('pose_terms', 1e-5), ('weights', 2e-6), ('nominal', 2e-6)):
        a, b = (out[k][fin], want[k][fin]) if k in ('costs', 'pose_terms') else (out[k], want[k])
        assert hp.rel_err(a, b) <= floor, (k, hp.rel_err(a, b))
    # the map and the path are read on the device: the same controls score differently after copy_
    costs_before, terms_before = out['costs'].clone(), out['pose_terms'].clone()
    mp.reset(nominal0)
    cm.copy_(torch.full_like(cm, 0.25))
    path.copy_(path0.to(DEV) + torch.tensor([0.0, 1.0], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out['controls'], want['controls'])
    assert bool(torch.isfinite(out['costs']).all()) and torch.equal(out['pose_terms'][:, 0], torch.full((B,), 0.25, device=DEV))
    assert float((out['pose_terms'][:, 1] - terms_before[:, 1]).abs().min()) > 0.1 and not torch.equal(out['costs'], costs_before)


# ---- 9. the shooter ---------------------------------------------------------------------------------------------------------------------
def test_shooter_takes_the_argmin_of_the_summed_cost():
    from monoforce_amd import TrajectoryShooter
    from monoforce_amd import synthetic as syn
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 6.4)
    z = (syn.bump_terrain(syn.bump_params(2), 6.4, 0.1) * 0.8).to(DEV)
    cm, path = _planner_inputs()
    B = 96
    plain = TrajectoryShooter(dp, n_trajs=B, pose_stride=10).shoot(z, generator=torch.Generator(device=DEV).manual_seed(3))
    sh = TrajectoryShooter(dp, n_trajs=B, pose_stride=10, map_weight=0.5, path_weight=0.75, lethal=2.0)
    out = sh.shoot(z, controls=plain['controls'], cost_map=cm.to(DEV), path=path.to(DEV))
    assert torch.equal(out['Xs'], plain['Xs'])            # the same rollouts: the shooter's own cost is `plain['costs']`
    args = (out['Xs'].cpu(), out['Rs'].cpu(), torch.as_tensor(pts, dtype=torch.float32), cm, path, plain['costs'].cpu())
    lethal = _check(out['costs'].cpu(), out['pose_terms'].cpu(), args, (0.1, 6.4, 2.0, INF), sh.pose_weights, 'shooter')
    assert bool(lethal.any()) and not bool(lethal.all())
    assert out['best'] == int(torch.argmin(out['costs'])) and not bool(lethal[out['best']])
    assert not torch.equal(out['costs'], plain['costs'])
    with pytest.raises(ValueError, match='fused'):
        TrajectoryShooter(dp, n_trajs=B, fused=False, map_weight=0.5).shoot(z, controls=plain['controls'], cost_map=cm.to(DEV))
    with pytest.raises(ValueError, match='no cost_map'):
        sh.shoot(z, controls=plain['controls'], path=path.to(DEV))
