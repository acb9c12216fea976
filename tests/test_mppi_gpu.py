"""MPPI on the GPU (monoforce_amd/csrc/mppi.hip, monoforce_amd/mppi.py): the three kernels against the referee of tests/mppi_reference.py
(pinned on the CPU in tests/test_mppi_cpu.py), the planner step stage by stage, its behaviour on flat ground, and its capture into a graph.

Error bars ("rel-to-absmax", helpers.rel_err) are taken against the referee's float64 evaluation of the same float32 inputs:
  path costs   max(1e-5, 3 d32)    1e-5: what test_planner_gpu.py holds the shooter's costs to
  update       max(2e-6, 3 d32)    2e-6: the project's bar for in-launch reductions (test_physics_loss_gpu.py)
with d32 the distance between the referee's own float32 and float64 evaluations (the softmin amplifies a rounding of the costs by 1 / lambda
whatever computes it)."""
import numpy as np
import pytest
import torch

from monoforce_amd import ops as mf_ops  # noqa: F401      (registers torch.ops.monoforce.*)
from tests import helpers as hp
from tests import mppi_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(1, 1), (2, 3), (65, 41), (257, 120), (1030, 7)]      # partial wave, second workgroup, several 64-rollout chunks
# The launch configurations beyond: path_costs_kernel runs S = 16 / 8 / 4 waves per 64-rollout group for B <= 8192 / <= 16384 / above (the
# first three shapes: S = 8 with one rollout in the last group, S = 4 with T < S and with T < S on three of the four waves' second trip);
# mppi_finish_kernel deals the ceil(B / 64) chunks to 16 waves, `per` chunks each: 129 chunks -> per = 9 (wave 14 takes 3 of 9, wave 15 none),
# 257 -> per = 17 (wave 15 takes 2 of 17), 65 -> per = 5 (waves 13 .. 15 take none); T = 70: a second, partial 64-step tile.
# tests/test_side_kernel_shapes_cpu.py holds these thresholds to the source.
SHAPES += [(8193, 3), (16385, 2), (16385, 3), (4097, 70)]
SHAPES += [(8193, 9), (16385, 5)]      # ... and S = 8, S = 4 with a step in every wave (above, most of the S partial sums are zeros) and a ragged second trip
SIGMA, LO, HI = (0.3, 0.6), (-1.0, -2.0), (1.0, 2.0)


def _bar(floor, r32, r64):
    return max(floor, 3 * hp.rel_err(r32, r64))


def _close(got, r32, r64, floor, what=''):
    err, bar = hp.rel_err(got, r64), _bar(floor, r32, r64)
    print(f'{what}: err {err:.3g} bar {bar:.3g}')
    return err <= bar


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- 1. perturb -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', SHAPES)
def test_perturb_is_bit_equal_to_the_torch_expression(B, T):
    g = _gen(B + T)
    nominal = (torch.rand(T, 2, generator=g) * 2 - 1) * torch.tensor([1.2, 2.4])      # partly outside the limits
    noise = torch.randn(B, T, 2, generator=g)
    for keep in (False, True):
        got = torch.ops.monoforce.mppi_perturb(nominal.to(DEV), noise.to(DEV), SIGMA, LO, HI, keep).cpu()
        assert torch.equal(got, ref.perturb(nominal, noise, SIGMA, LO, HI, keep))      # float32, op by op
        if keep:
            assert torch.equal(got[0], torch.minimum(torch.maximum(nominal, torch.tensor(LO)), torch.tensor(HI)))
    # sigma = 10: (nearly) every sample is beyond a limit, and is exactly the limit
    got = torch.ops.monoforce.mppi_perturb(nominal.to(DEV), noise.to(DEV), (10.0, 10.0), LO, HI, False).cpu()
    assert torch.equal(got, ref.perturb(nominal, noise, (10.0, 10.0), LO, HI, False))
    lim = torch.tensor([LO, HI])
    assert bool(((got >= lim[0]) & (got <= lim[1])).all())
    raw = nominal + torch.tensor([10.0, 10.0]) * noise
    assert torch.equal(got[raw > lim[1]], lim[1].expand_as(got)[raw > lim[1]]) and torch.equal(got[raw < lim[0]], lim[0].expand_as(got)[raw < lim[0]])
    if B * T >= 100:
        assert bool((raw > lim[1]).any()) and bool((raw < lim[0]).any())


# ---- 2. path costs --------------------------------------------------------------------------------------------------------------------
def _check_costs(rows_dev, force_dev, x_last_dev, goal, weights, what):
    costs, terms = torch.ops.monoforce.path_costs(rows_dev, force_dev, x_last_dev, goal.to(DEV), list(weights))
    rows, force, x_last = rows_dev.cpu(), None if force_dev is None else force_dev.cpu(), x_last_dev.cpu()
    c32, t32 = ref.path_costs(rows, force, x_last, goal, weights)
    c64, t64 = ref.path_costs(rows.double(), None if force is None else force.double(), x_last.double(), goal.double(), weights)
    assert _close(costs, c32, c64, 1e-5, what + ' costs')
    for k, name in enumerate(('incl', 'force', 'goal')):
        assert _close(terms[:, k], t32[:, k], t64[:, k], 1e-5, f'{what} {name}')
    return costs, terms


@pytest.fixture(scope='module')
def bump_rollout():
    """B = 37 rollouts of T = 120 steps on bump terrains (the case of test_planner_gpu.test_cost_rows_match_full_outputs): computed once."""
    from monoforce_amd import synthetic as syn
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    B, T = 37, 120
    dp = make_dphysics(pts, masks, 1, 0.1, 3.2, points_per_lane=1)
    z = torch.stack([syn.bump_terrain(syn.bump_params(3 + k % 3), 3.2, 0.1) * 0.5 for k in range(B)]).to(DEV)
    out = dp.rollout_costs(z, syn.varying_controls(B, T, seed=5).to(DEV), pose_stride=7)
    assert out['cost_rows'].shape == (B, T, 4) and out['cost_rows'].stride() == (4, 4 * B, 1)      # the time-major buffer, viewed [B,T,4]
    return out


def test_path_costs_of_a_real_rollout(bump_rollout):
    out = bump_rollout
    goal = torch.tensor([1.0, 0.5])
    costs, terms = _check_costs(out['cost_rows'], out['force_cost'], out['Xs'][:, -1], goal, (1.0, 0.5, 2.0), 'rollout')
    assert torch.isfinite(costs).all() and float(terms[:, 0].max()) > 0.01 and float(terms[:, 1].max()) > 0
    assert torch.equal(terms[:, 1], out['force_cost'])
    _check_costs(out['cost_rows'], None, out['Xs'][:, -1], goal, (1.0, 0.0, 1.0), 'rollout, no force term')
    # a NaN in one row: that rollout's cost is not finite, its neighbours' are what they were -- in both layouts
    for rows in (out['cost_rows'].transpose(0, 1).contiguous().transpose(0, 1), out['cost_rows'].contiguous()):
        rows[5, 17, 1] = float('nan')
        bad, _ = torch.ops.monoforce.path_costs(rows, out['force_cost'], out['Xs'][:, -1], goal.to(DEV), [1.0, 0.5, 2.0])
        keep = torch.arange(37, device=DEV) != 5
        assert not bool(torch.isfinite(bad[5])) and torch.equal(bad[keep], costs[keep])


@pytest.mark.parametrize('B,T', SHAPES)
def test_path_costs_of_constructed_rows(B, T):
    g = _gen(7 * B + T)
    rows = torch.randn(B, T, 4, generator=g)
    rows[..., :3] /= rows[..., :3].norm(dim=-1, keepdim=True)
    one = np.float32(1.0)
    rows[0, 0, 0] = float(np.nextafter(one, np.float32(2.0)))             # r0 just outside +-1: the clamp keeps asin defined
    rows[-1, -1, 0] = -float(np.nextafter(one, np.float32(2.0)))
    rows[B // 2, T // 2, :3] = 0.0                                        # (0, 0, 0): atan2(0, 0) = asin(0) = 0
    if T > 2:
        rows[0, 1, 0], rows[0, 2, 0] = 1.5, -1.0
    x_last, goal, force = torch.randn(B, 3, generator=g), torch.tensor([0.3, -0.2]), torch.rand(B, generator=g)
    costs, _ = _check_costs(rows.to(DEV), force.to(DEV), x_last.to(DEV), goal, (1.0, 0.5, 2.0), f'contiguous {B}x{T}')
    assert torch.isfinite(costs).all()
    # the same rows where they are not 16-byte aligned (the scalar-load kernel) and time-major (the rollout's layout)
    wide = torch.zeros(B, T, 5, device=DEV)
    wide[..., :4] = rows.to(DEV)
    odd, _ = torch.ops.monoforce.path_costs(wide[..., :4], force.to(DEV), x_last.to(DEV), goal.to(DEV), [1.0, 0.5, 2.0])
    tm, _ = torch.ops.monoforce.path_costs(rows.to(DEV).transpose(0, 1).contiguous().transpose(0, 1), force.to(DEV), x_last.to(DEV), goal.to(DEV), [1.0, 0.5, 2.0])
    assert torch.equal(odd, costs) and torch.equal(tm, costs)            # same sums in the same order, whatever the strides


# ---- 3. update ------------------------------------------------------------------------------------------------------------------------
def _update(costs, controls, nominal, lam):
    n, w, best, nv = torch.ops.monoforce.mppi_update(costs.to(DEV), controls.to(DEV), nominal.to(DEV), lam)
    assert best.dtype == torch.int32 and best.shape == (1,) and nv.dtype == torch.int32 and nv.shape == (1,) and best.is_cuda
    return n.cpu(), w.cpu(), int(best), int(nv)


def _check_update(costs, controls, nominal, lam, what):
    n, w, best, nv = _update(costs, controls, nominal, lam)
    n32, w32, b32, v32 = ref.update(costs, controls, nominal, lam)
    n64, w64, b64, v64 = ref.update(costs.double(), controls.double(), nominal.double(), lam)
    assert (best, nv) == (b64, v64)
    assert _close(w, w32, w64, 2e-6, what + ' weights') and _close(n, n32, n64, 2e-6, what + ' nominal')
    if nv:
        assert abs(float(w.double().sum()) - 1.0) <= _bar(2e-6, w32, w64)
    return n, w, best, nv


@pytest.mark.parametrize('B,T', SHAPES)
def test_update_matches_the_referee(B, T):
    g = _gen(11 * B + T)
    costs = torch.rand(B, generator=g) * 2 + 0.5
    controls, nominal = torch.randn(B, T, 2, generator=g), torch.randn(T, 2, generator=g)
    n, w, best, nv = _check_update(costs, controls, nominal, 0.05, f'{B}x{T}')
    assert nv == B and best == int(torch.argmin(costs))
    n2, w2, best2, nv2 = _update(costs, controls, nominal, 0.05)           # fixed summation order: bit-identical from call to call
    assert torch.equal(n, n2) and torch.equal(w, w2) and (best, nv) == (best2, nv2)
    # lambda = 1e6: the mean of the sequences
    n, w, _, _ = _check_update(costs, controls, nominal, 1e6, f'{B}x{T} lambda=1e6')
    # (every weight is within spread / lambda of 1 / B; 2e-6: the float32 sums)
    spread, mean = float(costs.max() - costs.min()) / 1e6, controls.double().mean(0)
    assert float((w.double() * B - 1).abs().max()) <= spread + 2e-6
    assert float((n.double() - mean).abs().max()) <= spread * float(controls.abs().mean(0).max()) + 2e-6 * float(controls.abs().max())
    # lambda = 1e-6 on well-separated costs: one-hot weights, the best sequence itself, nothing non-finite
    sep = torch.randperm(B, generator=g).float() * 0.01 + 0.25
    n, w, best, nv = _check_update(sep, controls, nominal, 1e-6, f'{B}x{T} lambda=1e-6')
    onehot = torch.zeros(B)
    onehot[best] = 1.0
    assert best == int(torch.argmin(sep)) and torch.equal(w, onehot) and torch.isfinite(n).all()
    assert bool(((n - controls[best]).abs() <= torch.abs(torch.nextafter(controls[best], torch.full_like(n, float('inf'))) - controls[best])).all())
    # NaN / +-inf costs: weight exactly 0; a tie for the minimum: the first index
    if B >= 65:
        c = costs.clone()
        c[1] = c[B - 2] = 0.25                                               # the minimum of the finite ones, twice
        c[0], c[B // 2], c[-1] = float('nan'), float('inf'), float('-inf')
        n, w, best, nv = _check_update(c, controls, nominal, 0.05, f'{B}x{T} non-finite costs')
        assert nv == B - 3 and best == 1 and w[1] == w[B - 2] and torch.isfinite(n).all()
        assert w[0] == 0 and w[B // 2] == 0 and w[-1] == 0
    # no finite cost at all: the nominal comes back
    n, w, best, nv = _update(torch.full((B,), float('nan')), controls, nominal, 0.05)
    assert torch.equal(n, nominal) and not bool(w.any()) and (best, nv) == (-1, 0)


def test_update_small_cases():
    g = _gen(5)
    controls, nominal = torch.randn(2, 9, 2, generator=g), torch.randn(9, 2, generator=g)
    n, w, best, nv = _update(torch.tensor([3.25]), controls[:1], nominal, 0.05)              # B = 1: the sequence itself
    assert torch.equal(n, controls[0]) and w.tolist() == [1.0] and (best, nv) == (0, 1)
    n, w, best, nv = _update(torch.tensor([0.75, 0.75]), controls, nominal, 0.05)            # equal costs: the mean, first index
    assert w.tolist() == [0.5, 0.5] and torch.equal(n, 0.5 * controls[0] + 0.5 * controls[1]) and (best, nv) == (0, 2)
    n, w, best, nv = _update(torch.tensor([0.75, float('nan')]), controls, nominal, 0.05)
    assert w.tolist() == [1.0, 0.0] and torch.equal(n, controls[0]) and (best, nv) == (0, 1)


# ---- 4. - 6. the planner --------------------------------------------------------------------------------------------------------------
def _planner(B, terrain, weights=None, **kw):
    from monoforce_amd import MPPIPlanner
    from monoforce_amd import synthetic as syn
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 6.4)
    dp.dphys_cfg.traj_sim_time = 1.0
    dp = type(dp)(dp.dphys_cfg, device=DEV)                      # rebuild the time grid for the 1 s horizon: T = 100
    z = (syn.bump_terrain(syn.bump_params(2), 6.4, 0.1) * 0.8).to(DEV) if terrain == 'bump' else torch.zeros(128, 128, device=DEV)
    return MPPIPlanner(dp, n_trajs=B, weights=weights, **kw), dp, z


def _check_stages(out, nominal_before, noise, goal, mp, what):
    """Every stage of a step's dict against the referee applied to the PREVIOUS stage's returned tensor."""
    cpu = {k: v.cpu() for k, v in out.items()}
    assert torch.equal(cpu['controls'], ref.perturb(nominal_before, noise, mp.sigma, mp.lo, mp.hi, mp.keep_nominal))
    force = cpu['force_cost'] if mp.weights[1] != 0 else None
    x_last = cpu['Xs'][:, -1]
    c32, t32 = ref.path_costs(cpu['cost_rows'], force, x_last, goal, mp.weights)
    c64, t64 = ref.path_costs(cpu['cost_rows'].double(), None if force is None else force.double(), x_last.double(), goal.double(), mp.weights)
    assert _close(cpu['costs'], c32, c64, 1e-5, what + ' costs')
    for k, name in enumerate(('incl', 'force', 'goal')):
        assert _close(cpu['terms'][:, k], t32[:, k], t64[:, k], 1e-5, f'{what} {name}')
    n32, w32, b32, v32 = ref.update(cpu['costs'], cpu['controls'], nominal_before, mp.lam)
    n64, w64, b64, v64 = ref.update(cpu['costs'].double(), cpu['controls'].double(), nominal_before.double(), mp.lam)
    assert (int(cpu['best']), int(cpu['n_valid'])) == (b64, v64)
    assert _close(cpu['weights'], w32, w64, 2e-6, what + ' weights') and _close(cpu['nominal'], n32, n64, 2e-6, what + ' nominal')


def test_planner_step_stage_by_stage():
    B, T = 256, 100
    mp, dp, z = _planner(B, 'bump', weights=dict(inclination=1.0, force=0.02, goal=1.0))
    assert mp.T == T and mp.lo == (-1.0, -2.0) and mp.hi == (1.0, 2.0)
    g = _gen(4)
    nominal0 = torch.stack([torch.full((T,), 0.6), 0.3 * torch.sin(torch.arange(T) / 20.0)], -1)
    assert torch.equal(mp.reset(nominal0.to(DEV)).cpu(), nominal0)
    noise, goal = torch.randn(B, T, 2, generator=g), torch.tensor([1.0, 0.5])
    out = mp.step(z, goal.to(DEV), noise=noise.to(DEV))
    assert set(out) == {'controls', 'cost_rows', 'Xs', 'Rs', 'pose_steps', 'force_cost', 'terms', 'costs', 'weights', 'best', 'n_valid', 'nominal'}
    assert all(v.is_cuda for v in out.values()) and out['cost_rows'].shape == (B, T, 4) and out['terms'].shape == (B, 3)
    assert out['nominal'] is mp.nominal and int(out['n_valid']) == B
    _check_stages(out, nominal0, noise, goal, mp, 'step')
    # shift(k): drop the first k controls, repeat the last
    before = mp.nominal.cpu().clone()
    assert torch.equal(mp.shift(1).cpu(), torch.cat([before[1:], before[-1:]]))
    assert torch.equal(mp.shift(3).cpu(), torch.cat([before[4:], before[-1:].expand(4, 2)]))
    assert torch.equal(mp.reset().cpu(), torch.zeros(T, 2))


def test_planner_rejects_what_rollout_costs_rejects():
    mp, dp, z = _planner(64, 'flat')
    goal = torch.tensor([1.0, 0.5], device=DEV)
    with pytest.raises(TypeError, match='float32 only'):
        mp.step(z.double(), goal)
    from monoforce_amd import MPPIPlanner
    with pytest.raises(ValueError, match='precise=False'):
        MPPIPlanner(type(dp)(dp.dphys_cfg, device=DEV, precise=True))


def test_plan_moves_towards_the_goal_on_flat_ground():
    B, T = 512, 100
    mp, dp, z = _planner(B, 'flat', weights=dict(inclination=0.0, force=0.0, goal=1.0), n_iters=8)
    goal = torch.tensor([1.0, 0.5], device=DEV)
    out = mp.plan(z, goal, generator=torch.Generator(device=DEV).manual_seed(0))
    assert all(bool(torch.isfinite(v).all()) for k, v in out.items() if v.dtype.is_floating_point)
    assert int(out['n_valid']) == B and 0 <= int(out['best']) < B
    alone = dp.rollout_costs(z.unsqueeze(0), mp.nominal.unsqueeze(0).clone(), project=False)
    start, end = torch.zeros(2, device=DEV), alone['Xs'][0, -1, :2]
    d_start, d_end = float((start - goal).norm()), float((end - goal).norm())
    print(f'distance to the goal: start {d_start:.3f} m, end of the planned path {d_end:.3f} m')
    assert d_end < d_start


def test_step_can_be_captured_and_follows_the_goal():
    from monoforce_amd.capture import capture
    B, T = 256, 100
    g = _gen(9)
    noise = torch.randn(B, T, 2, generator=g).to(DEV)
    nominal0 = torch.stack([torch.full((T,), 0.5), torch.full((T,), 0.2)], -1).to(DEV)
    goal0 = torch.tensor([1.0, 0.5])
    eager, _, z = _planner(B, 'bump')
    eager.reset(nominal0)
    want = []
    for _ in range(2):            # two eager steps with the same noise: the second starts from the first one's nominal
        want.append({k: v.clone() for k, v in eager.step(z, goal0.to(DEV), noise=noise).items()})
    mp, _, _ = _planner(B, 'bump')
    goal = goal0.to(DEV)
    mp.step(z, goal, noise=noise)            # warm-up: every cached constant exists before the capture
    mp.reset(nominal0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture(graph):
        out = mp.step(z, goal, noise=noise)
    for i in range(2):            # a replay is a step: the nominal buffer carries over
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out['controls'], want[i]['controls'])
        for k, floor in (('costs', 1e-5), ('terms', 1e-5), ('weights', 2e-6), ('nominal', 2e-6)):
            assert hp.rel_err(out[k], want[i][k]) <= floor, (i, k, hp.rel_err(out[k], want[i][k]))
        assert int(out['best']) == int(want[i]['best']) and int(out['n_valid']) == B
    # the goal is read on the device: the second step again, after goal.copy_, scores the same controls against the new goal
    costs_before = out['costs'].clone()
    mp.reset(want[0]['nominal'])
    goal.copy_(torch.tensor([-1.0, 2.0]))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out['controls'], want[1]['controls'])
    assert not torch.equal(out['costs'], costs_before) and float((out['costs'] - costs_before).abs().max()) > 0.1
