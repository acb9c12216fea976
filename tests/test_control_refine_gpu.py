"""Gradient descent on control sequences on the GPU (monoforce_amd/refine.py, csrc/control_refine.hip).

Kernel level: `refine.update` alone, fed hand-made costs and gradients, against `torch.optim.Adam` itself on the CPU in float64 with the same
clamp, the same skip rule and the same best rule.  Exact: the step count, `best_iter`, `best_cost`, the history, the snapshots (the controls
BEFORE the update of the best iteration, to the bit) and a skipped sequence (controls and moments keep their bits).  The controls: the rule of
tests/test_terrain_fit_gpu.py, max(1e-6, 2 x the error of torch.optim.Adam in float32 on the CPU against the same referee).
Loop level: `ControlRefiner` on flat ground with the goal off to one side.

Every measured figure is printed on a line starting with `control-refine-error` (`pytest -s`); profiles/control_refine_errors.txt keeps them.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN, INF = math.nan, math.inf
ITERS = 6
LR, BETAS, EPS = (0.05, 0.1), (0.9, 0.999), 1e-8
LO, HI = (-1.0, -1.5), (1.0, 1.5)
# per sequence: an improving cost, an equal one (no snapshot), a NaN, a +inf, and a late improvement
COSTS = [[5.0, 4.0, 4.0, NAN, INF, 3.0], [2.0, 3.0, NAN, 1.0, 1.0, INF], [INF, NAN, 7.0, 7.0, 6.5, 6.5]]


def make_inputs(K, T, seed):
    """Controls near the box (some will be clamped), ITERS gradients per sequence; two non-finite entries: +inf in the LAST element of the last
    sequence at iteration 2 (the ragged last trip), a NaN in the first element of sequence 0 at iteration 4."""
    g = torch.Generator().manual_seed(seed)
    c0 = ((torch.rand(K, T, 2, generator=g) * 2 - 1) * torch.tensor([1.0, 1.5])).float()
    grads = torch.randn(ITERS, K, T, 2, generator=g).float()
    zero = torch.rand(ITERS, K, T, 2, generator=g) < 0.1
    zero[:, :, 0] = False                      # (every sequence has a non-zero gradient in every iteration: a sequence that is not skipped moves)
    grads[zero] = 0.0
    grads[2, K - 1, T - 1, 1] = INF
    grads[4, 0, 0, 0] = NAN
    costs = torch.tensor(COSTS[:K], dtype=torch.float32).t().contiguous()          # [ITERS,K]
    return c0, grads, costs


def referee(c0, grads, costs, dtype):
    """torch.optim.Adam on the CPU in `dtype`, one optimiser per sequence with the two channels as two parameter groups (lr_v, lr_w); the
    step count advances for every sequence in every iteration (the kernel's bias correction reads ONE device step), a skipped sequence keeps
    controls and moments; the clamp behind the step, outside Adam; the snapshot BEFORE the step."""
    K, T = c0.shape[:2]
    params = [[c0[k, :, ch].to(dtype).clone().requires_grad_(True) for ch in (0, 1)] for k in range(K)]
    opts = [torch.optim.Adam([{'params': [p[0]], 'lr': LR[0]}, {'params': [p[1]], 'lr': LR[1]}], betas=BETAS, eps=EPS) for p in params]
    cur = lambda k: torch.stack([p.detach() for p in params[k]], -1).clone()  # noqa: E731
    best_cost, best_iter, best = [INF] * K, [-1] * K, [cur(k) for k in range(K)]
    skipped = []
    for i in range(ITERS):
        for k in range(K):
            cost, g = float(costs[i, k]), grads[i, k].to(dtype)
            if cost < best_cost[k]:
                best_cost[k], best_iter[k], best[k] = cost, i, cur(k)
            skip = math.isnan(cost) or not bool(torch.isfinite(g).all())
            keep = None
            if skip:
                skipped.append((i, k))
                keep = [(p.detach().clone(), {n: v.clone() for n, v in opts[k].state[p].items() if n != 'step'}) for p in params[k]]
            for ch, p in enumerate(params[k]):
                p.grad = torch.zeros_like(p) if skip else g[:, ch].clone()
            opts[k].step()
            with torch.no_grad():
                for ch, p in enumerate(params[k]):
                    if skip:
                        p.copy_(keep[ch][0])
                        for n in ('exp_avg', 'exp_avg_sq'):
                            opts[k].state[p][n].copy_(keep[ch][1][n]) if n in keep[ch][1] else opts[k].state[p][n].zero_()
                    else:
                        p.clamp_(LO[ch], HI[ch])
    mom = lambda n: torch.stack([torch.stack([opts[k].state[p][n] for p in params[k]], -1) for k in range(K)])  # noqa: E731
    return dict(controls=torch.stack([cur(k) for k in range(K)]), best=torch.stack(best), best_cost=best_cost, best_iter=best_iter,
                m=mom('exp_avg'), v=mom('exp_avg_sq'), skipped=skipped)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('T', [1, 128, 129, 300])
@pytest.mark.parametrize('K', [1, 3])
def test_update_kernel_against_torch_adam(K, T):
    """2 T = 2, 256, 258, 600 elements per sequence: below, equal to and above one 256-thread trip, with a ragged last trip."""
    from monoforce_amd import refine
    c0, grads, costs = make_inputs(K, T, seed=100 * K + T)
    ref, ref32 = referee(c0, grads, costs, torch.float64), referee(c0, grads, costs, torch.float32)
    assert {(2, K - 1), (4, 0)} <= set(ref['skipped']) and any(math.isnan(float(costs[i, k])) for i, k in ref['skipped'])
    desc = refine.refine_desc(K, T, ITERS, LR, BETAS, EPS, LO, HI)
    ctrl, m, v = c0.to(DEV), torch.zeros(K, T, 2, device=DEV), torch.zeros(K, T, 2, device=DEV)
    best = ctrl.clone()
    state, best_cost, best_iter, history = refine.new_state(K, ITERS, DEV)
    g_dev, c_dev = grads.to(DEV), costs.to(DEV)
    before = []
    for i in range(ITERS):
        before.append((ctrl.clone(), m.clone(), v.clone()))
        refine.update(desc, ctrl, g_dev[i], c_dev[i], m, v, best, best_cost, best_iter, history, state)
    torch.cuda.synchronize()
    tag = f'kernel K={K} T={T}'
    # exact: the step count with its ticket back at zero, the best iterations and costs, the history
    assert state.tolist() == [ITERS, 0], (tag, state.tolist())
    assert best_iter.tolist() == ref['best_iter'] and best_cost.tolist() == ref['best_cost'], (tag, best_iter.tolist(), best_cost.tolist())
    assert same_bits(history, c_dev), tag
    # the snapshots: the controls BEFORE the update of the best iteration, to the bit
    for k in range(K):
        assert same_bits(best[k], before[ref['best_iter'][k]][0][k]), (tag, k)
    # a skipped sequence keeps its bits in that iteration, moments included -- and the others moved
    after = before[1:] + [(ctrl, m, v)]
    for i in range(ITERS):
        for k in range(K):
            still = all(same_bits(a[k], b[k]) for a, b in zip(before[i], after[i]))
            assert still == ((i, k) in ref['skipped']), (tag, i, k)
    assert float(ctrl[:, :, 0].abs().max()) <= HI[0] and float(ctrl[:, :, 1].abs().max()) <= HI[1]
    for name, got in (('controls', ctrl), ('best', best), ('m', m), ('v', v)):
        e_hip = float((got.double().cpu() - ref[name]).abs().max())
        e_aten = float((ref32[name].double() - ref[name]).abs().max())
        bar = max(1e-6, 2.0 * e_aten)
        print(f'control-refine-error {tag} {name}: hip {e_hip:.3g} aten_f32 {e_aten:.3g} bar {bar:.3g}')
        assert e_hip <= bar, (tag, name, e_hip, bar)


def test_update_kernel_history_stops_at_max_iters():
    """ITERS launches into a history of ITERS - 2 rows: nothing is written behind the buffer, the step keeps counting."""
    from monoforce_amd import refine
    K, T = 3, 129
    c0, grads, costs = make_inputs(K, T, seed=9)
    desc = refine.refine_desc(K, T, ITERS - 2, LR, BETAS, EPS, LO, HI)
    ctrl, m, v = c0.to(DEV), torch.zeros(K, T, 2, device=DEV), torch.zeros(K, T, 2, device=DEV)
    best = ctrl.clone()
    state, best_cost, best_iter, _ = refine.new_state(K, ITERS - 2, DEV)
    guarded = torch.full((ITERS - 1, K), -777.0, device=DEV)
    history = guarded[:ITERS - 2]
    for i in range(ITERS):
        refine.update(desc, ctrl, grads[i].to(DEV), costs[i].to(DEV), m, v, best, best_cost, best_iter, history, state)
    assert state.tolist() == [ITERS, 0] and same_bits(history, costs[:ITERS - 2].to(DEV)) and guarded[ITERS - 2].tolist() == [-777.0] * K
    assert best_iter.tolist() == [5, 3, 4]


# ---- loop level ------------------------------------------------------------------------------------------------------------------------
K_LOOP, T_LOOP, N_LOOP = 4, 50, 10
GOAL = (0.4, 0.3)
D_MAX, GRID_RES = 3.2, 0.1


def _setup():
    from monoforce_amd import synthetic as syn
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, GRID_RES, D_MAX)
    z = torch.zeros(64, 64, device=DEV)
    v = torch.tensor([0.3, 0.5, 0.7, 0.9])
    ctrl0 = torch.stack([v[:, None].expand(K_LOOP, T_LOOP), torch.zeros(K_LOOP, T_LOOP)], -1).contiguous()
    return pts, masks, dp, z, ctrl0


def cpu_loop(pts, masks, ctrl0, n):
    """The same loop on the CPU in float64: the oracle's rollout, `trajectory_objective_aten`, torch.optim.Adam, the clamp.  Returns the
    history [n,K]."""
    from monoforce_amd import refine
    from oracle import dphysics_oracle as orc
    from tests import helpers as hp
    spec = hp.spec_from(pts, masks, 1, GRID_RES, D_MAX)
    ctrl = ctrl0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ctrl], lr=1.0, betas=BETAS, eps=EPS)
    lr = torch.tensor(LR, dtype=torch.float64)
    z = torch.zeros(K_LOOP, 64, 64, dtype=torch.float64)
    hist = []
    for _ in range(n):
        (Xs, _, Rs, _), _ = orc.rollout(spec, z, ctrl)
        costs, _ = refine.trajectory_objective_aten(Xs, Rs, torch.tensor(GOAL, dtype=torch.float64), points=torch.as_tensor(pts, dtype=torch.float64),
                                                    weights=dict(goal=1.0), pose_stride=50, grid_res=GRID_RES, d_max=D_MAX)
        hist.append(costs.detach().clone())
        g, = torch.autograd.grad(costs.sum(), ctrl)
        before = ctrl.detach().clone()
        ctrl.grad = g
        opt.step()
        with torch.no_grad():       # (lr = 1: the step is Adam's direction; the rate per channel is applied here)
            ctrl.copy_(before + lr * (ctrl - before))
            ctrl.clamp_(torch.tensor([-1.0, -2.0], dtype=torch.float64), torch.tensor([1.0, 2.0], dtype=torch.float64))
    return torch.stack(hist)


def test_refiner_graph_and_eager_descend_alike():
    from monoforce_amd import ControlRefiner
    pts, masks, dp, z, ctrl0 = _setup()
    assert (float(dp.dphys_cfg.vel_max), float(dp.dphys_cfg.omega_max)) == (1.0, 2.0)      # the clamp of cpu_loop
    goal = torch.tensor(GOAL, device=DEV)
    out = {}
    for graph in (True, False):
        r = ControlRefiner(dp, ctrl0, weights=dict(goal=1.0), lr=LR, betas=BETAS, eps=EPS, pose_stride=50, max_iters=N_LOOP, graph=graph)
        v0 = r.controls._version
        res = r.run(N_LOOP, z, goal)
        assert r.graph == graph and (r._captured is not None) == graph and r.iteration == N_LOOP and int(r.device_step) == N_LOOP
        assert r.controls._version > v0 and res['best'].dtype == torch.int64
        out[graph] = {k: t.detach().clone() for k, t in res.items()}
        with pytest.raises(ValueError, match='max_iters'):
            r.step(z, goal)
    # the control gradient is written, not accumulated: replayed and launch by launch, the same bits
    for k in ('controls', 'history', 'best_controls', 'best_cost', 'best_iter', 'best'):
        assert same_bits(out[True][k], out[False][k]) if out[True][k].dtype != torch.int64 else torch.equal(out[True][k], out[False][k]), k
    res = out[True]
    h = res['history']
    assert h.shape == (N_LOOP, K_LOOP) and bool(torch.isfinite(h).all())
    assert torch.equal(res['best_cost'], h.min(0).values) and torch.equal(res['best_iter'].long(), h.argmin(0))
    assert int(res['best']) == int(res['best_cost'].argmin())
    # it descends, at least half as far as the same loop on the CPU in float64
    ref = cpu_loop(pts, masks, ctrl0, N_LOOP)
    drop_gpu = float(h[0].min() - res['best_cost'].min())
    drop_cpu = float(ref[0].min() - ref.min())
    print(f'control-refine-error loop K={K_LOOP} T={T_LOOP} n={N_LOOP}: decrease gpu {drop_gpu:.4g} cpu_f64 {drop_cpu:.4g}; first costs gpu '
          f'{[round(float(x), 5) for x in h[0]]} cpu {[round(float(x), 5) for x in ref[0]]}')
    assert drop_cpu > 0.01 and drop_gpu >= 0.5 * drop_cpu


def test_refiner_step_and_reset():
    from monoforce_amd import ControlRefiner
    pts, masks, dp, z, ctrl0 = _setup()
    goal = torch.tensor(GOAL, device=DEV)
    r = ControlRefiner(dp, ctrl0, weights=dict(goal=1.0), pose_stride=50, max_iters=4, graph=True)
    c_first = r.step(z, goal).clone()
    assert r.controls.grad is not None and r.controls.grad.shape == (K_LOOP, T_LOOP, 2) and r.terms.shape == (K_LOOP, 4)
    assert torch.equal(r.terms[:, 2], c_first) and same_bits(r.best_controls, ctrl0.to(DEV)) and r.best_iter.tolist() == [0] * K_LOOP
    moved = r.controls.detach().clone()
    assert not torch.equal(moved, ctrl0.to(DEV))
    goal.copy_(torch.tensor([0.4, -0.3], device=DEV))       # read on the device: the replay follows the new goal
    c_second = r.step(z, goal)
    states, _ = dp(z.unsqueeze(0), moved, _want_forces=False)
    want = (states[0][:, -1, :2] - goal).norm(dim=-1)
    assert float((c_second - want).abs().max()) <= 1e-5
    r.reset(ctrl0)
    assert r.state.tolist() == [0, 0] and bool(r.history.isnan().all()) and bool(torch.isinf(r.best_cost).all()) and r.best_iter.tolist() == [-1] * K_LOOP
    assert same_bits(r.controls.detach(), ctrl0.to(DEV)) and float(r.m.abs().max()) == 0.0
    goal.copy_(torch.tensor(GOAL, device=DEV))
    assert same_bits(r.step(z, goal), c_first)


def test_refiner_never_synchronises():
    from monoforce_amd import ControlRefiner
    pts, masks, dp, z, ctrl0 = _setup()
    goal = torch.tensor(GOAL, device=DEV)
    r = ControlRefiner(dp, ctrl0, weights=dict(goal=1.0), pose_stride=50, max_iters=N_LOOP, graph=True)
    r.run(1, z, goal)                                # (the capture)
    torch.cuda.set_sync_debug_mode('error')
    try:
        res = r.run(N_LOOP - 1, z, goal)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert res['history'].shape == (N_LOOP - 1, K_LOOP) and bool(torch.isfinite(res['history']).all())


def test_from_mppi_takes_the_nominal_and_the_cheapest_samples():
    from monoforce_amd import ControlRefiner
    from tests.test_mppi_gpu import _planner
    B = 64
    weights = dict(inclination=0.5, force=0.0, goal=1.0)
    mp, dp, z = _planner(B, 'bump', weights=weights)
    goal = torch.tensor([1.0, 0.5], device=DEV)
    noise = torch.randn(B, mp.T, 2, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = mp.step(z, goal, noise=noise)
    costs = out['costs'].clone()
    costs[[3, 17]] = torch.tensor([NAN, INF], device=DEV)        # two samples that must not be taken, however they would rank
    out = dict(out, costs=costs)
    r = ControlRefiner.from_mppi(mp, out, 4, max_iters=3)
    order = sorted((b for b in range(B) if math.isfinite(float(costs[b]))), key=lambda b: (float(costs[b]), b))[:3]
    assert r.controls.shape == (4, mp.T, 2) and same_bits(r.controls.detach()[0], out['nominal'])
    assert same_bits(r.controls.detach()[1:], out['controls'][order])
    assert r.weights == (0.0, 0.0, 1.0, 0.5) and r.lethal == mp.lethal and r.off_map == mp.off_map and r.footprint.data_ptr() == mp.footprint.data_ptr()
    res = r.run(3, z, goal)
    assert bool(torch.isfinite(res['history']).all()) and int(r.device_step) == 3
    mp_force, _, _ = _planner(B, 'bump', weights=dict(force=0.02))
    with pytest.raises(ValueError, match='force cost has no gradient'):
        ControlRefiner.from_mppi(mp_force, out, 4)
