"""The trajectory objective on the GPU (monoforce_amd/csrc/traj_objective.hip, monoforce_amd/refine.py, torch.ops.monoforce.traj_objective)
against the float64 referee of tests/traj_objective_reference.py.

Values: costs and the four terms by the bar of tests/test_pose_costs_gpu.py, rel-to-absmax <= max(1e-5, 3 d32) with d32 the referee's own
float32-to-float64 distance; map and path term against tests/pose_costs_reference.py on the kept poses; EQUAL +inf sets (the inputs of
tests/pose_costs_cases.py keep every discontinuous decision 1e-3 away from its threshold).
Gradients: max |g - g_ref| over the compared rows <= max(2 x the same error of `trajectory_objective_aten` in float32 on the CPU, 1e-6 max(1,
max |g_ref|)) -- the project's float32 protocol (tests/test_map_losses_gpu.py); the referee alone decides which rows lie too close to a kink
to be compared (at most 5 % of a case), the rows of steps that are not kept must be exactly 0.
Every measured error is printed on a line starting with `traj-objective-error` (`pytest -s`); profiles/traj_objective_errors.txt keeps them.
"""
import math

import pytest
import torch

from monoforce_amd import ops as mf_ops  # noqa: F401  (registers torch.ops.monoforce.*)
from monoforce_amd import refine
from tests import helpers as hp
from tests import pose_costs_cases as pc
from tests import pose_costs_reference as ref
from tests import traj_objective_reference as tr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
INF = float('inf')
W4 = tr.WEIGHTS


def _dev(t):
    return None if t is None else t.to(DEV)


def _launch(case, weights=W4, layout='contiguous', gcosts=None, want_grad=True, **scalars):
    """`refine.objective_launch` on one case; returns CPU tensors (costs, terms, gXs, gRs) and the strides the gradients came back in."""
    sc = dict(grid_res=pc.GRID_RES, d_max=pc.D_MAX, lethal=INF, off_map=INF)
    sc.update(scalars)
    Xs, Rs = _dev(case['Xs']), _dev(case['Rs'])
    if layout == 'time-major':
        Xs, Rs = tr.time_major(Xs), tr.time_major(Rs)
        B = Xs.shape[0]
        assert min(Xs.shape[:2]) == 1 or (Xs.stride() == (3, 3 * B, 1) and Rs.stride() == (9, 9 * B, 3, 1))      # (an axis of length 1 has no stride to speak of)
    costs, terms, gX, gR = refine.objective_launch(Xs, Rs, _dev(case['goal']), _dev(case['points']), _dev(case['cost_map']), _dev(case['path']),
                                                   tr.case_weights(case, weights), case['pose_stride'], gcosts=_dev(gcosts), want_grad=want_grad, **sc)
    if want_grad:
        assert refine.same_layout(gX, Xs) and refine.same_layout(gR, Rs)          # dense in the inputs' own strides
        return costs.cpu(), terms.cpu(), gX.cpu(), gR.cpu()
    assert gX is None and gR is None
    return costs.cpu(), terms.cpu(), None, None


def _bar(r32, r64):
    return max(1e-5, 3 * hp.rel_err(r32, r64))


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------
VALUE_CASES = [(1, 1, 1, 1), (3, 50, 7, 4), (65, 50, 7, 7), (65, 50, 50, 17), (33, 50, 3, 65)]       # (B, T, pose_stride, N)


def _value_case(B, T, stride, N, map_shape=(pc.HW, pc.HW)):
    c = pc.constructed(B, T, N, map_shape=map_shape)
    g = torch.Generator().manual_seed(B + T)
    return dict(Xs=c['Xs'], Rs=c['Rs'], points=c['points'], cost_map=c['cost_map'], path=c['path'], goal=torch.rand(2, generator=g) * 4 - 2,
                pose_stride=stride)


@pytest.mark.parametrize('shape', VALUE_CASES)
def test_values_match_the_referee(shape):
    """The rough map with its lethal block of tests/pose_costs_cases.py (every decision 1e-3 from its threshold), off_map infinite and finite, and
    w_map = 0 with the map given: the lethal rule holds whatever the weight."""
    case = _value_case(*shape)
    steps = tr.kept_steps(shape[1], shape[2])
    for off_map, weights in ((INF, W4), (1.5, W4), (INF, (0.0,) + W4[1:])):
        sc = dict(lethal=pc.LETHAL, off_map=off_map)
        costs, terms, _, _ = _launch(case, weights, want_grad=False, **sc)
        o32 = tr.evaluate(case['Xs'], case['Rs'], case['goal'], case['points'], case['cost_map'], case['path'], weights, shape[2], **sc)
        d = lambda t: t.double()  # noqa: E731
        o64 = tr.evaluate(d(case['Xs']), d(case['Rs']), d(case['goal']), d(case['points']), d(case['cost_map']), d(case['path']), weights, shape[2], **sc)
        lethal = torch.isinf(o64['costs'])
        assert torch.equal(torch.isinf(o32['costs']), lethal), 'the referee itself is not decided in float32'
        assert torch.equal(torch.isinf(costs) & (costs > 0), lethal) and torch.equal(torch.isinf(terms[:, 0]), lethal)
        if shape[0] >= 33:
            assert bool(lethal.any()) and not bool(lethal.all())
        fin = ~lethal
        what = f'values {shape} off_map={off_map} w_map={weights[0]}'
        for name, got, r32, r64 in (('costs', costs[fin], o32['costs'][fin], o64['costs'][fin]), ('map', terms[fin, 0], o32['terms'][fin, 0], o64['terms'][fin, 0]),
                                    ('path', terms[:, 1], o32['terms'][:, 1], o64['terms'][:, 1]), ('goal', terms[:, 2], o32['terms'][:, 2], o64['terms'][:, 2]),
                                    ('incl', terms[:, 3], o32['terms'][:, 3], o64['terms'][:, 3])):
            if got.numel() == 0:
                continue
            err, bar = hp.rel_err(got, r64), _bar(r32, r64)
            print(f'traj-objective-error {what} {name}: err {err:.3g} bar {bar:.3g}')
            assert err <= bar, (what, name, err, bar)
        # map and path term are pose_costs' own, on the kept poses: the older referee agrees with the new one
        _, t_pose = ref.pose_costs(d(case['Xs'])[:, steps], d(case['Rs'])[:, steps], d(case['points']), d(case['cost_map']), d(case['path']), None,
                                   pc.GRID_RES, pc.D_MAX, pc.LETHAL, off_map, (weights[0], weights[1]))
        assert torch.equal(torch.isinf(t_pose[:, 0]), lethal) and hp.rel_err(terms[fin, :2], t_pose[fin]) <= 1e-5


def test_nan_poses_propagate_and_stay_isolated():
    """A NaN position at a kept step: a NaN path term and cost; a zero third row: a NaN inclination and cost; a NaN at a step that is NOT kept:
    nothing.  The other rollouts keep their bits."""
    case = _value_case(65, 50, 7, 7)
    costs, terms, _, _ = _launch(case, want_grad=False, off_map=1.5)
    keep = torch.ones(65, dtype=torch.bool)
    keep[[5, 40]] = False
    changed = dict(case, Xs=case['Xs'].clone(), Rs=case['Rs'].clone())
    changed['Xs'][5, 14, 0] = math.nan          # step 14 = 2 x 7 is kept
    changed['Rs'][40, 49, 2] = 0.0              # the clamp step T - 1
    changed['Xs'][7, 13, :] = math.nan          # not kept
    changed['Rs'][7, 15] = math.nan             # not kept
    c2, t2, _, _ = _launch(changed, want_grad=False, off_map=1.5)
    assert math.isnan(float(c2[5])) and math.isnan(float(t2[5, 1])) and not math.isnan(float(t2[5, 3]))
    assert math.isnan(float(c2[40])) and math.isnan(float(t2[40, 3])) and not math.isnan(float(t2[40, 1]))
    assert torch.equal(c2[keep], costs[keep]) and torch.equal(t2[keep], terms[keep])


# ---- 2. gradients ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def grad_cases():
    """Per case of tr.CASES, made once and left unchanged: the inputs, the excluded rows, the float64 referee and the float32 ATen comparator."""
    out = {}
    for shape in tr.CASES:
        case = tr.make_case(*shape)
        bad = tr.excluded_rows(case)
        assert float(bad.float().mean()) <= 0.05, (shape, float(bad.float().mean()))
        out[shape] = dict(case=case, mask=tr.row_mask(case, bad), excluded=int(bad.sum()), rows=bad.numel(), ref=tr.gradients(case),
                          aten=tr.gradients(case, dtype=torch.float32, fn=refine.trajectory_objective_aten))
    return out


def _grad_check(what, got, want, aten, mask):
    for name, g, g64, g32 in (('gXs', got[0], want[0], aten[0]), ('gRs', got[1], want[1], aten[1])):
        e_hip = float((g.double() - g64)[mask].abs().max())
        e_aten = float((g32.double() - g64)[mask].abs().max())
        bar = max(2.0 * e_aten, 1e-6 * max(1.0, float(g64.abs().max())))
        print(f'traj-objective-error {what} {name}: hip {e_hip:.3g} aten_f32 {e_aten:.3g} bar {bar:.3g} max|g| {float(g64.abs().max()):.3g}')
        assert e_hip <= bar, (what, name, e_hip, bar)


@pytest.mark.parametrize('shape', tr.CASES)
def test_gradients_match_float64_autograd_of_the_referee(grad_cases, shape):
    c = grad_cases[shape]
    case, mask = c['case'], c['mask']
    B, T = shape[:2]
    what = f'gradients {shape} excluded {c["excluded"]}/{c["rows"]}'
    costs, terms, gX, gR = _launch(case)
    _grad_check(what, (gX, gR), c['ref'][2:], c['aten'][2:], mask)
    fin = torch.isfinite(c['ref'][0])
    assert torch.equal(torch.isfinite(costs), fin) and (not bool(fin.any()) or hp.rel_err(costs[fin], c['ref'][0][fin]) <= 1e-5)
    # the rows of steps that are not kept are exactly zero
    kept = torch.zeros(T, dtype=torch.bool)
    kept[tr.kept_steps(T, shape[2])] = True
    assert not bool(gX[:, ~kept].any()) and not bool(gR[:, ~kept].any()) and not bool(gX[..., 2].any())
    assert bool(gX[:, kept].any()) and bool(gR[:, kept].any())
    # the views the rollout hands out, and a second call: the same bits
    for layout in ('time-major', 'contiguous'):
        c2, t2, gX2, gR2 = _launch(case, layout=layout)
        assert torch.equal(c2, costs) and torch.equal(t2, terms), layout
        assert torch.equal(gX2.contiguous().view(torch.int32), gX.view(torch.int32)) and torch.equal(gR2.contiguous().view(torch.int32), gR.view(torch.int32)), layout
    # value only: the same value
    c3, t3, _, _ = _launch(case, want_grad=False)
    assert torch.equal(c3, costs) and torch.equal(t3, terms)


@pytest.mark.parametrize('shape', [(65, 50, 7, 17, 18), (3, 50, 2, 65, 18)])
def test_gcosts_scale_the_gradient_rows(grad_cases, shape):
    c = grad_cases[shape]
    case = c['case']
    gc = torch.rand(shape[0], generator=torch.Generator().manual_seed(3)) * 4 - 2
    gc[0] = 0.0
    _, _, gX, gR = _launch(case, gcosts=gc)
    want = tr.gradients(case, gcosts=gc)
    aten = tr.gradients(case, gcosts=gc, dtype=torch.float32, fn=refine.trajectory_objective_aten)
    _grad_check(f'gradients-gcosts {shape}', (gX, gR), want[2:], aten[2:], c['mask'])
    assert not bool(gX[0].any()) and not bool(gR[0].any())
    # through autograd: the stashed gradients times the upstream gradient, row by row
    Xs, Rs = tr.time_major(_dev(case['Xs'])).requires_grad_(True), tr.time_major(_dev(case['Rs'])).requires_grad_(True)
    costs, terms = refine.trajectory_objective(Xs, Rs, _dev(case['goal']), points=_dev(case['points']), cost_map=_dev(case['cost_map']),
                                               path=_dev(case['path']), weights=dict(zip(refine.TERM_NAMES, W4)), pose_stride=case['pose_stride'],
                                               grid_res=pc.GRID_RES, d_max=pc.D_MAX)
    assert not terms.requires_grad
    sX, sR = costs.grad_fn.grads
    gX_a, gR_a = torch.autograd.grad(costs, [Xs, Rs], grad_outputs=_dev(gc))
    assert torch.equal(gX_a, sX * _dev(gc).view(-1, 1, 1)) and torch.equal(gR_a, sR * _dev(gc).view(-1, 1, 1, 1))
    assert gX_a.stride() == Xs.stride() and gR_a.stride() == Rs.stride()
    # the registered op: the same numbers
    o = torch.ops.monoforce.traj_objective(Xs, Rs, _dev(case['goal']), _dev(case['points']), _dev(case['cost_map']), _dev(case['path']), list(W4),
                                           case['pose_stride'], pc.GRID_RES, pc.D_MAX, INF, INF)
    assert torch.equal(o[0], costs) and torch.equal(o[1], terms) and torch.equal(o[2], sX) and torch.equal(o[3], sR)
    gX_o, gR_o = torch.autograd.grad(o[0], [Xs, Rs], grad_outputs=_dev(gc))
    assert torch.equal(gX_o, gX_a) and torch.equal(gR_o, gR_a)


def test_a_lethal_rollout_keeps_the_gradient_of_its_finite_terms(grad_cases):
    """`lethal` changes the VALUE alone: with a threshold that makes some rollouts lethal the gradients keep their bits -- the finite map term
    still pushes -- and exactly the referee's rollouts cost +inf (those with a sample within 1e-4 of the threshold are not asked)."""
    shape = (65, 50, 7, 17, 18)
    case = grad_cases[shape]['case']
    off = 0.25                                   # far below the threshold chosen here: an off-map point is never the lethal one
    costs, terms, gX, gR = _launch(case, off_map=off)
    d = lambda t: t.detach().double()  # noqa: E731
    with torch.no_grad():
        o = tr.evaluate(d(case['Xs']), d(case['Rs']), d(case['goal']), d(case['points']), d(case['cost_map']), d(case['path']), W4, shape[2], off_map=off)
    tops = o['s'].amax((1, 2)).sort().values
    level = float(torch.tensor(float(tops[32] + tops[33]) / 2, dtype=torch.float32))       # between the 33rd and the 34th of the 65 rollouts' largest samples
    near = ((o['s'] - level).abs() < 1e-4).flatten(1).any(1)
    want = (~(o['s'] < level)).flatten(1).any(1)
    c2, t2, gX2, gR2 = _launch(case, off_map=off, lethal=level)
    assert bool(want.any()) and not bool(want.all()) and int(near.sum()) < 5
    assert torch.equal(torch.isinf(c2)[~near], want[~near]) and torch.equal(torch.isinf(t2[:, 0]), torch.isinf(c2))
    assert torch.equal(gX2.view(torch.int32), gX.view(torch.int32)) and torch.equal(gR2.view(torch.int32), gR.view(torch.int32))
    assert bool(gR2[want & ~near][:, :, :2].any())          # the map term's gradient of the lethal rollouts is there
    assert torch.equal(t2[:, 1:], terms[:, 1:]) and torch.equal(c2[~torch.isinf(c2)], costs[~torch.isinf(c2)])


def test_gradient_rules_at_the_kinks():
    """tests/traj_objective_reference.py `kink_case`: exact ties and exact zeros (dyadic numbers: float32 and float64 evaluate them alike) --
    the first maximum takes the gradient, an off-map maximum has none, a zero path / goal distance and a zero roll / pitch have derivative 0."""
    case, sc = tr.kink_case()
    want = tr.gradients(case, **sc)
    costs, terms, gX, gR = _launch(case, **sc)
    assert hp.rel_err(costs, want[0]) <= 1e-6 and hp.rel_err(terms, want[1]) <= 1e-6
    for name, g, g64 in (('gXs', gX, want[2]), ('gRs', gR, want[3])):
        err = float((g.double() - g64).abs().max())
        print(f'traj-objective-error kinks {name}: hip {err:.3g} bar 1e-06')
        assert err <= 1e-6 and bool(torch.isfinite(g).all())
    c_map = W4[0] / 3 / 0.25
    assert abs(float(gR[0, 0, 0, 1]) - c_map * -0.125) <= 1e-6          # point 0 (y = -0.125), not its twin (y = +0.25)
    assert not bool(gR[0, 1, :2].any())                                 # pose 1: the maximum is off the map


# ---- 3. through the rollout -------------------------------------------------------------------------------------------------------------
def test_gradient_reaches_the_controls_without_a_copy():
    """B = 3, T = 40, a bump on flat ground, the 4-point body: `costs.sum().backward()` leaves in `controls.grad` exactly what the rollout's
    backward makes of the objective's own stashed gradients -- nothing copied, transposed or dropped in between."""
    from monoforce_amd import synthetic as syn
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    B, T = 3, 40
    dp = make_dphysics(pts, masks, 1, 0.1, 3.2)
    z = (syn.bump_terrain(syn.bump_params(3), 3.2, 0.1) * 0.3).unsqueeze(0).to(DEV)
    ctrl0 = syn.varying_controls(B, T, seed=5).to(DEV)
    points = torch.as_tensor(pts, dtype=torch.float32).to(DEV)
    cm = tr.smooth_map((64, 64)).to(DEV)
    path = torch.tensor([[0.0, 0.2], [0.5, 0.3], [1.0, 0.8]], device=DEV)
    goal = torch.tensor([0.8, 0.4], device=DEV)
    kw = dict(points=points, cost_map=cm, path=path, weights=dict(zip(refine.TERM_NAMES, W4)), pose_stride=7, grid_res=0.1, d_max=3.2)

    def forward():
        ctrl = ctrl0.clone().requires_grad_(True)
        states, _ = dp(z, ctrl, _want_forces=False)
        Xs, Rs = states[0], states[2]
        assert Xs.stride() == (3, 3 * B, 1) and Rs.stride() == (9, 9 * B, 3, 1)
        return ctrl, Xs, Rs, refine.trajectory_objective(Xs, Rs, goal, **kw)

    ctrl, Xs, Rs, (costs, terms) = forward()
    sX, sR = costs.grad_fn.grads
    assert sX.stride() == Xs.stride() and sR.stride() == Rs.stride()
    costs.sum().backward()
    ctrl2, Xs2, Rs2, (costs2, _) = forward()
    sX2, sR2 = costs2.grad_fn.grads
    assert torch.equal(sX2, sX) and torch.equal(sR2, sR) and torch.equal(costs2, costs)
    g2, = torch.autograd.grad([Xs2, Rs2], ctrl2, grad_outputs=[sX2, sR2])
    assert bool(torch.isfinite(ctrl.grad).all()) and float(ctrl.grad.abs().max()) > 0
    assert torch.equal(ctrl.grad.view(torch.int32), g2.view(torch.int32))
    # and the stashed gradients are the referee's, on this real rollout
    case = dict(Xs=Xs.detach().cpu(), Rs=Rs.detach().cpu(), points=points.cpu(), cost_map=cm.cpu(), path=path.cpu(), goal=goal.cpu(), pose_stride=7)
    bad = tr.excluded_rows(case)
    want = tr.gradients(case, grid_res=0.1, d_max=3.2)
    aten = tr.gradients(case, dtype=torch.float32, fn=refine.trajectory_objective_aten, grid_res=0.1, d_max=3.2)
    _grad_check(f'gradients rollout excluded {int(bad.sum())}/{bad.numel()}', (sX.cpu(), sR.cpu()), want[2:], aten[2:], tr.row_mask(case, bad))
