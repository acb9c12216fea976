"""Fused pose loss (mf_pose_loss_*: physics_loss(rotation_loss=True) as one value launch and one backward launch) against the reference's
golden vector (tests/golden/pose_loss.npz), the ATen restatement in float64, through the rollout, under capture, and `evaluate`."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as hp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# (value, gradient): float32 from a CPU probe of the kernel's formula in float32 against float64 (1e-7 / 2e-7 at angles in [0.3, 2.5]) with
# 20-50x of room for another acos; float64 a few hundred ulps
BARS = {torch.float32: (2e-6, 1e-5), torch.float64: (1e-12, 1e-11)}


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


def _rotation(axis, angle):
    """Rodrigues' formula on [...,3] axes and [...] angles, float64."""
    a = axis / axis.norm(dim=-1, keepdim=True)
    K = torch.zeros(*a.shape[:-1], 3, 3, dtype=torch.float64)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -a[..., 2], a[..., 1], a[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -a[..., 0], -a[..., 1], a[..., 0]
    s, c = torch.sin(angle)[..., None, None], torch.cos(angle)[..., None, None]
    return torch.eye(3, dtype=torch.float64) + s * K + (1 - c) * (K @ K)


def _problem(B, T1, T2, seed, lo=0.3, hi=2.5, noise=0.02, crowded=False):
    """float64 CPU inputs: positions, rotations `noise` off SO(3), ground truth = the nearest predicted rotation turned by an angle in
    U(lo, hi) about a random axis.  `crowded`: stamps within the first five predicted steps (many stamps of a rollout share a step)."""
    from monoforce_amd.losses import nearest_steps
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    uni = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    pred_ts = (torch.arange(T1, dtype=torch.float64) * 0.01).unsqueeze(0).expand(B, -1)
    gt_ts = uni(B, T2) * 0.05 if crowded else torch.sort(uni(B, T2) * (T1 - 1) * 0.01, dim=1).values
    near = nearest_steps(pred_ts, gt_ts)
    X = rnd(B, T1, 3)
    Xgt = X[torch.arange(B).unsqueeze(1), near] + 0.3 * rnd(B, T2, 3)
    R = _rotation(rnd(B, T1, 3), uni(B, T1) * math.pi) + noise * rnd(B, T1, 3, 3)
    Rgt = R[torch.arange(B).unsqueeze(1), near] @ _rotation(rnd(B, T2, 3), lo + (hi - lo) * uni(B, T2))
    return dict(X=X, R=R, Xgt=Xgt, Rgt=Rgt, pred_ts=pred_ts, gt_ts=gt_ts, near=near)


def _aten64(p, gamma, wx=1.0, wr=1.0):
    """physics_loss_aten in float64 on the CPU: (loss, loss_rot, dX, dR) of wx loss + wr loss_rot."""
    from monoforce_amd.losses import physics_loss_aten
    X, R = p['X'].double().cpu().clone().requires_grad_(True), p['R'].double().cpu().clone().requires_grad_(True)
    loss, rot = physics_loss_aten([X, None, R], [p['Xgt'].double().cpu(), None, p['Rgt'].double().cpu()], None, p['gt_ts'].double().cpu(),
                                  gamma=gamma, rotation_loss=True, nearest=p['near'].cpu().long())
    (wx * loss + wr * rot).backward()
    return float(loss.detach()), float(rot.detach()), X.grad, R.grad


def _check(got, want, dtype, what=''):
    (l, r, gX, gR), (l0, r0, gX0, gR0) = got, want
    figs = (_rel(l, l0), _rel(r, r0), hp.rel_err(gX, gX0), hp.rel_err(gR, gR0))
    bv, bg = BARS[dtype]
    print(what, str(dtype), 'value err %.3g %.3g bar %.3g, gradient err %.3g %.3g bar %.3g' % (*figs[:2], bv, *figs[2:], bg))
    assert figs[0] <= bv and figs[1] <= bv and figs[2] <= bg and figs[3] <= bg, (what, figs)


# ---- 1: the reference's own numbers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dtype', [('f32', torch.float32), ('f64', torch.float64)])
def test_fused_pose_loss_matches_reference_golden(tag, dtype):
    from monoforce_amd.losses import physics_loss_fused
    g = hp.load('pose_loss')
    t = lambda k: torch.as_tensor(g[f'{tag}/{k}']).to(DEV)  # noqa: E731
    X, R = t('X').requires_grad_(True), t('R').requires_grad_(True)
    loss, rot = physics_loss_fused([X, None, R], [t('Xgt'), None, t('Rgt')], t('pred_ts'), t('gt_ts'), gamma=0.9, rotation_loss=True)
    assert type(loss.grad_fn).__name__.startswith('_FusedPoseLoss') and loss.dtype == dtype and loss.shape == rot.shape == ()
    (loss + rot).backward()
    _check((loss.detach(), rot.detach(), X.grad, R.grad), (g[f'{tag}/loss'], g[f'{tag}/loss_rot'], g[f'{tag}/g_X'], g[f'{tag}/g_R']), dtype, 'golden')


# ---- 2: the rollout's layout, stamps sharing steps, unequal upstream gradients ------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_fused_pose_loss_on_time_major_views_with_duplicate_stamps(dtype):
    from monoforce_amd.losses import physics_loss_fused
    B, T1, T2 = 37, 120, 11
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in _problem(B, T1, T2, 0, crowded=True).items()}
    assert int((p['near'].sort(dim=1).values.diff(dim=1) == 0).sum()) > B                 # many stamps share their step
    want = _aten64(p, 0.9, 3.0, 0.5)
    bX = p['X'].transpose(0, 1).contiguous().to(DEV).requires_grad_(True)                 # [T1,B,3] / [T1,B,3,3]: the rollout's buffers
    bR = p['R'].transpose(0, 1).contiguous().to(DEV).requires_grad_(True)
    X, R = bX.transpose(0, 1), bR.transpose(0, 1)
    assert not X.is_contiguous() and not R.is_contiguous()
    loss, rot = physics_loss_fused([X, None, R], [p['Xgt'].to(DEV), None, p['Rgt'].to(DEV)], None, p['gt_ts'].to(DEV), gamma=0.9,
                                   nearest=p['near'].to(DEV), rotation_loss=True)
    gX, gR = torch.autograd.grad(3.0 * loss + 0.5 * rot, (X, R))
    assert gX.stride() == X.stride() and gR.stride() == R.stride()                        # what mf_rollout_bwd_* takes without a copy
    _check((loss.detach(), rot.detach(), gX, gR), want, dtype, 'time-major')
    # a None upstream is a zero for that half; rows no stamp is nearest to stay zero
    (gR1,) = torch.autograd.grad(physics_loss_fused([X, None, R], [p['Xgt'].to(DEV), None, p['Rgt'].to(DEV)], None, p['gt_ts'].to(DEV), gamma=0.9,
                                                    nearest=p['near'].to(DEV), rotation_loss=True)[1], (R,))
    assert hp.rel_err(gR1 * 0.5, gR) <= BARS[dtype][1] and float(gR1[:, 6:].abs().max()) == 0.0


# ---- 3: the mean finished inside the launch, the ticket shared with the position-only loss ------------------------------------------------
# (1311, 50): 257 blocks, the first grid at which the finishing loop makes a second trip (thread 0 alone); (9000, 23): 809 blocks, four trips
@pytest.mark.parametrize('B,T2', [(1, 1), (5, 50), (1024, 50), (3000, 7), (1311, 50), (9000, 23)])
def test_pose_loss_value_is_finished_inside_the_launch_and_reusable(B, T2):
    """Bar 2e-6 against the float64 ATen form, or three times the distance d32 of the float32 ATen form on the CPU from the same where that is
    more (it is not at these shapes: d32 is printed next to the error)."""
    from monoforce_amd.losses import physics_loss_aten, physics_loss_fused
    T1 = 2 * T2 + 3
    p = {k: (v.float().to(DEV) if v.is_floating_point() else v.to(DEV)) for k, v in _problem(B, T1, T2, B).items()}
    args = ([p['X'], None, p['R']], [p['Xgt'], None, p['Rgt']], None, p['gt_ts'])
    pairs, singles = [], []
    for _ in range(4):                                   # launch after launch on one stream: the ticket comes back to zero every time
        loss, rot = physics_loss_fused(*args, gamma=0.9, nearest=p['near'], rotation_loss=True)
        singles.append(float(physics_loss_fused(*args, gamma=0.9, nearest=p['near'])))
        pairs.append((float(loss), float(rot)))
    assert len(set(pairs)) == 1 and len(set(singles)) == 1, (pairs, singles)
    l0, r0, _, _ = _aten64(p, 0.9)
    c = {k: v.cpu() for k, v in p.items()}               # the float32 inputs, on the CPU
    l32, r32 = physics_loss_aten([c['X'], None, c['R']], [c['Xgt'], None, c['Rgt']], None, c['gt_ts'], gamma=0.9, rotation_loss=True, nearest=c['near'])
    bl, br = max(2e-6, 3 * _rel(l32, l0)), max(2e-6, 3 * _rel(r32, r0))
    print(f'pose loss value {B}x{T2}: xyz err {_rel(pairs[0][0], l0):.3g} bar {bl:.3g} (d32 {_rel(l32, l0):.3g}); rot err {_rel(pairs[0][1], r0):.3g} bar {br:.3g} '
          f'(d32 {_rel(r32, r0):.3g}); position-only err {_rel(singles[0], l0):.3g} bar {bl:.3g}')
    assert _rel(pairs[0][0], l0) <= bl and _rel(pairs[0][1], r0) <= br and _rel(singles[0], l0) <= bl


def test_pose_loss_gradients_on_time_major_views_of_a_batch_that_is_no_multiple_of_a_wave():
    """B = 1311 = 20 x 64 + 31 rollouts x 50 stamps on the rollout's time-major buffers: the backward kernel maps thread t to rollout t % B, so a
    wave straddles two stamps almost everywhere.  d/dXs and d/dRs of 3 loss + 0.5 loss_rot against the float64 ATen form, BARS as everywhere."""
    from monoforce_amd.losses import physics_loss_fused
    B, T2 = 1311, 50
    p = {k: (v.float() if v.is_floating_point() else v) for k, v in _problem(B, 2 * T2 + 3, T2, 1311).items()}
    want = _aten64(p, 0.9, 3.0, 0.5)
    bX = p['X'].transpose(0, 1).contiguous().to(DEV).requires_grad_(True)
    bR = p['R'].transpose(0, 1).contiguous().to(DEV).requires_grad_(True)
    X, R = bX.transpose(0, 1), bR.transpose(0, 1)
    assert X.stride() == (3, 3 * B, 1) and R.stride() == (9, 9 * B, 3, 1)
    loss, rot = physics_loss_fused([X, None, R], [p['Xgt'].to(DEV), None, p['Rgt'].to(DEV)], None, p['gt_ts'].to(DEV), gamma=0.9,
                                   nearest=p['near'].to(DEV), rotation_loss=True)
    gX, gR = torch.autograd.grad(3.0 * loss + 0.5 * rot, (X, R))
    _check((loss.detach(), rot.detach(), gX, gR), want, torch.float32, 'pose loss gradient 1311x50 time-major')
    # ... and the position-only kernels on the same views
    (gX1,) = torch.autograd.grad(physics_loss_fused([X], [p['Xgt'].to(DEV)], None, p['gt_ts'].to(DEV), gamma=0.9, nearest=p['near'].to(DEV)) * 3.0, (X,))
    err = hp.rel_err(gX1, want[2])
    print(f'position-only gradient 1311x50 time-major: err {err:.3g} bar {BARS[torch.float32][1]:.3g}')
    assert err <= BARS[torch.float32][1]


# ---- 4: which calls take the HIP route ----------------------------------------------------------------------------------------------------
def test_public_physics_loss_routes_rotation_calls(monkeypatch):
    from monoforce.losses import physics_loss
    from monoforce_amd import losses as L
    p = {k: (v.float().to(DEV) if v.is_floating_point() else v.to(DEV)) for k, v in _problem(6, 30, 5, 4).items()}
    sg = [p['Xgt'], None, p['Rgt']]
    aten = L.physics_loss_aten

    def run(fn, X, R, Rgt=p['Rgt']):
        X, R = X.detach().requires_grad_(True), R.detach().requires_grad_(True)
        loss, rot = fn([X, None, R], [p['Xgt'], None, Rgt], p['pred_ts'], p['gt_ts'], gamma=0.9, rotation_loss=True)
        gX, gR = torch.autograd.grad(loss + rot, (X, R))
        return loss, rot, gX, gR
    want = run(aten, p['X'], p['R'])
    with monkeypatch.context() as m:
        m.setattr(L, 'physics_loss_aten', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the ATen form was called')))
        got = run(physics_loss, p['X'], p['R'])
        assert type(got[0].grad_fn).__name__.startswith('_FusedPoseLoss')
        with torch.no_grad():                            # and without a graph
            loss, rot = physics_loss([p['X'], None, p['R']], sg, p['pred_ts'], p['gt_ts'], gamma=0.9, rotation_loss=True)
        assert float(loss) == float(got[0]) and float(rot) == float(got[1])
    _check([t.detach() for t in got], [t.detach().cpu() for t in want], torch.float32, 'route')
    # left to the ATen form, with its result: aliased rows of R_pred, a 3x3 that is not contiguous, a ground truth that wants a gradient
    calls = []
    monkeypatch.setattr(L, 'physics_loss_aten', lambda *a, **k: (calls.append(1), aten(*a, **k))[1])
    cases = {'aliased': (p['R'][:, :1].expand(-1, 30, -1, -1), p['Rgt']),
             'inner': (p['R'].transpose(2, 3).contiguous().transpose(2, 3), p['Rgt']),
             'gt grad': (p['R'], p['Rgt'].clone().requires_grad_(True))}
    for name, (R, Rgt) in cases.items():
        n = len(calls)
        X = p['X'].clone().requires_grad_(True)
        loss, rot = physics_loss([X, None, R], [p['Xgt'], None, Rgt], p['pred_ts'], p['gt_ts'], gamma=0.9, rotation_loss=True)
        assert len(calls) == n + 1 and not type(loss.grad_fn).__name__.startswith('_FusedPoseLoss'), name
        ref = aten([X, None, R], [p['Xgt'], None, Rgt], p['pred_ts'], p['gt_ts'], gamma=0.9, rotation_loss=True)
        assert float(loss) == float(ref[0]) and float(rot) == float(ref[1]), name
    # the position-only call keeps its own kernels
    assert type(physics_loss([p['X'].clone().requires_grad_(True)], sg, p['pred_ts'], p['gt_ts']).grad_fn).__name__.startswith('_FusedPhysicsLoss')


# ---- 5: |cos| == 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_rotation_gradient_is_zero_where_the_cosine_is_one(dtype):
    """The one documented difference from autograd (identical rotations: torch's arccos backward gives NaN; exactly pi: inf), and clip's mask."""
    from monoforce_amd.losses import physics_loss_aten, physics_loss_fused
    B, T1, T2 = 4, 6, 3
    p = {k: (v.to(dtype).to(DEV) if v.is_floating_point() else v.to(DEV)) for k, v in _problem(B, T1, T2, 1).items()}
    eye = torch.eye(3, dtype=dtype, device=DEV)
    w = 1.0 / (1.0 + 0.9 * p['gt_ts'].double())

    def run(R, Rgt, fn=physics_loss_fused):
        X, R = p['X'].clone().requires_grad_(True), R.clone().requires_grad_(True)
        loss, rot = fn([X, None, R], [p['Xgt'], None, Rgt], None, p['gt_ts'], gamma=0.9, nearest=p['near'], rotation_loss=True)
        gX, gR = torch.autograd.grad(loss + rot, (X, R))
        return loss, rot, gX, gR
    # identity against identity
    loss, rot, gX, gR = run(eye.repeat(B, T1, 1, 1), eye.repeat(B, T2, 1, 1))
    assert float(rot) == 0.0 and torch.isfinite(gX).all() and torch.isfinite(gR).all() and float(gR.abs().max()) == 0.0
    X = p['X'].clone().requires_grad_(True)
    Rl = eye.repeat(B, T1, 1, 1).requires_grad_(True)
    rot_only = physics_loss_fused([X, None, Rl], [p['Xgt'], None, eye.repeat(B, T2, 1, 1)], None, p['gt_ts'], gamma=0.9, nearest=p['near'], rotation_loss=True)[1]
    gX1, gR1 = torch.autograd.grad(rot_only, (X, Rl), allow_unused=True)
    assert (gX1 is None or float(gX1.abs().max()) == 0.0) and float(gR1.abs().max()) == 0.0
    assert not torch.isfinite(run(eye.repeat(B, T1, 1, 1), eye.repeat(B, T2, 1, 1), physics_loss_aten)[3]).all()      # the ATen form: NaN
    # 1.01 R against R: tr = 3.03, outside the clip range -> zero, like ATen
    Q = torch.linalg.qr(_problem(B, T1, T2, 1)['R']).Q.to(dtype).to(DEV)      # exact rotations (to rounding): tr(1.01 Q Q^T) = 3.03
    Rp, Rgt = 1.01 * Q, Q[torch.arange(B, device=DEV).unsqueeze(1), p['near']].contiguous()
    got, ref = run(Rp, Rgt), run(Rp, Rgt, physics_loss_aten)
    assert float(got[1]) == 0.0 == float(ref[1]) and float(got[3].abs().max()) == 0.0 == float(ref[3].abs().max())
    # diag(1, -1, -1) against I: tr = -1 exactly, theta = pi
    half_turn = torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=dtype, device=DEV))
    loss, rot, gX, gR = run(half_turn.repeat(B, T1, 1, 1), eye.repeat(B, T2, 1, 1))
    assert _rel(rot, math.pi ** 2 * float(w.mean())) <= (1e-6 if dtype == torch.float32 else 1e-14)
    assert torch.isfinite(gX).all() and float(gR.abs().max()) == 0.0


# ---- 6: small angles -----------------------------------------------------------------------------------------------------------------------
def test_small_angles_are_no_worse_than_the_aten_form_in_float32():
    """Angles in [1e-3, 0.05] between exact rotations: cos = 1 - theta^2 / 2 sits 5e-7 .. 1.25e-3 below 1, where float32 has a spacing of
    6e-8, so ANY float32 formula built on the trace carries an absolute error of ~2e-7 per theta^2 (of 1e-6 .. 2.5e-3).  The HIP value
    and gradient are held to max(1e-5, 3 x the error of the float32 ATen form on the same inputs), both against float64.
    8192 terms: the mean's error is then ~2e-7 / sqrt(8192) = 2e-9 on a mean theta^2 of ~8e-4, i.e. ~3e-6 -- below the 1e-5 floor, so
    the comparison does not hang on which of two equally good roundings happens to come out smaller."""
    from monoforce_amd.losses import physics_loss_aten, physics_loss_fused
    B, T1, T2 = 256, 64, 32
    p64 = _problem(B, T1, T2, 6, lo=1e-3, hi=0.05, noise=0.0)
    p = {k: (v.float().to(DEV) if v.is_floating_point() else v.to(DEV)) for k, v in p64.items()}
    want = _aten64(p, 0.9)                               # float64 on the float32 inputs
    res = {}
    for name, fn in (('hip', physics_loss_fused), ('aten', physics_loss_aten)):
        X, R = p['X'].clone().requires_grad_(True), p['R'].clone().requires_grad_(True)
        loss, rot = fn([X, None, R], [p['Xgt'], None, p['Rgt']], None, p['gt_ts'], gamma=0.9, nearest=p['near'].long(), rotation_loss=True)
        gX, gR = torch.autograd.grad(loss + rot, (X, R))
        res[name] = (_rel(rot, want[1]), hp.rel_err(gR, want[3]), _rel(loss, want[0]), hp.rel_err(gX, want[2]))
    print('small angles: (rot value, rot gradient, xyz value, xyz gradient) hip %s aten %s' % (res['hip'], res['aten']))
    assert all(np.isfinite(res['aten'])), res
    for k in range(4):
        assert res['hip'][k] <= max(1e-5, 3 * res['aten'][k]), (k, res)


# ---- 7: through the rollout ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def through_rollout():
    """loss + loss_rot of a 48 x 100 rollout against poses from another terrain, backward to z, friction and controls: (values, gradients)
    per (dtype, loss route)."""
    from monoforce_amd import losses as L
    from monoforce_amd import synthetic as syn
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    B, T = 48, 100
    z = syn.bump_terrain(syn.bump_params(3), 3.2, 0.1, torch.float64) * 0.3
    xs = torch.arange(z.shape[0], dtype=torch.float64) * 0.1 - 3.2
    z_gt = syn.bump_terrain(syn.bump_params(8), 3.2, 0.1, torch.float64) * 0.4 + 0.3 * xs[:, None] + 0.15 * xs[None, :]
    mu = syn.wave_friction(3.2, 0.1, dtype=torch.float64)
    ctrl = syn.const_controls(B, T, seed=2, dtype=torch.float64)
    sel = torch.arange(9, T, 10)
    out = {}
    for dtype in (torch.float64, torch.float32):
        dp = make_dphysics(pts, masks, 1, 0.1, 3.2)
        ts = torch.linspace(0, dp.dphys_cfg.traj_sim_time, int(dp.dphys_cfg.traj_sim_time / dp.dphys_cfg.dt))[:T].to(DEV, dtype)
        pred_ts, gt_ts = ts.unsqueeze(0).expand(B, -1), ts[sel].unsqueeze(0).expand(B, -1).contiguous()
        with torch.no_grad():
            (Xg, _, Rg, _), _ = dp(z_gt.to(DEV, dtype).unsqueeze(0), ctrl.to(DEV, dtype), friction=mu.to(DEV, dtype).unsqueeze(0))
            gt = [Xg[:, sel].contiguous(), None, Rg[:, sel].contiguous()]
        for route in ('hip', 'aten'):
            zl, ml, cl = (t.to(DEV, dtype).requires_grad_(True) for t in (z, mu, ctrl))
            states, _ = dp(zl.unsqueeze(0), cl, friction=ml.unsqueeze(0))
            fn = L.physics_loss if route == 'hip' else L.physics_loss_aten
            loss, rot = fn(states, gt, pred_ts, gt_ts, gamma=0.9, rotation_loss=True)
            assert type(loss.grad_fn).__name__.startswith('_FusedPoseLoss') == (route == 'hip')
            (loss + rot).backward()
            out[dtype, route] = ((float(loss), float(rot)), (zl.grad.cpu(), ml.grad.cpu(), cl.grad.cpu()))
    return out


def _route_error(got, want):
    return max([_rel(a, b) for a, b in zip(got[0], want[0])] + [hp.rel_err(a, b) for a, b in zip(got[1], want[1])])


def test_pose_loss_through_the_rollout_float64(through_rollout):
    r = through_rollout
    assert all(abs(v) > 0 for v in r[torch.float64, 'aten'][0]) and all(float(g.abs().max()) > 0 for g in r[torch.float64, 'aten'][1])
    err = _route_error(r[torch.float64, 'hip'], r[torch.float64, 'aten'])
    print('through the rollout, float64: %.3g' % err)
    assert err <= 1e-9


def test_pose_loss_through_the_rollout_float32(through_rollout):
    r = through_rollout
    want = r[torch.float64, 'aten']
    hip, aten = _route_error(r[torch.float32, 'hip'], want), _route_error(r[torch.float32, 'aten'], want)
    print('through the rollout, float32 against float64: hip %.3g aten %.3g' % (hip, aten))
    assert hip <= max(1e-3, 3 * aten)


# ---- 8: capture -------------------------------------------------------------------------------------------------------------------------------
def test_pose_loss_value_and_backward_replay_as_one_graph():
    from monoforce_amd.capture import capture
    from monoforce_amd.losses import physics_loss_fused
    B, T1, T2 = 37, 40, 11
    p = {k: (v.float().to(DEV) if v.is_floating_point() else v.to(DEV)) for k, v in _problem(B, T1, T2, 8).items()}
    others = [_problem(B, T1, T2, 80 + k)['Rgt'].float().to(DEV) for k in range(3)]
    bX = p['X'].transpose(0, 1).contiguous().requires_grad_(True)
    bR = p['R'].transpose(0, 1).contiguous().requires_grad_(True)
    Rgt = p['Rgt'].clone()

    def fwd_bwd():
        loss, rot = physics_loss_fused([bX.transpose(0, 1), None, bR.transpose(0, 1)], [p['Xgt'], None, Rgt], None, p['gt_ts'], gamma=0.9,
                                       nearest=p['near'], rotation_loss=True)
        gX, gR = torch.autograd.grad(3.0 * loss + 0.5 * rot, (bX, bR))
        return loss.detach(), rot.detach(), gX, gR
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # warm-up on the capture stream: its ticket exists
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with capture(g, stream=s, capture_error_mode='thread_local'):
        static = fwd_bwd()
    seen = set()
    for new in others:
        Rgt.copy_(new)
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        want = fwd_bwd()                                 # launch by launch, the same R_gt
        seen.add(float(got[1]))
        assert float(got[0]) == float(want[0]) and float(got[1]) == float(want[1])
        assert hp.rel_err(got[2], want[2]) <= 1e-6 and hp.rel_err(got[3], want[3]) <= 1e-6      # (stamps sharing a step: float atomics)
    assert len(seen) == 3                                # every replay read the R_gt copied in before it


# ---- 9: the evaluation step ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_returns_the_four_losses_of_the_references_eval_script():
    from monoforce_amd.losses import hm_loss, physics_loss_aten
    from tests.test_encoder_gpu import _stamp_rig
    enc, dp, step, b16 = _stamp_rig()
    (imgs, rots, trans, intrins, post_rots, post_trans, hm_geom, hm_terrain, control_ts, controls, pose0, traj_ts, Xs, Xds, Rs, Om) = b16
    Xs_before = Xs.clone()
    for prm in enc.parameters():
        prm.grad = None
    out = step.evaluate(tuple(b16))
    assert out.shape == (4,) and out.dtype == torch.float32 and out.is_cuda and not out.requires_grad
    assert torch.equal(Xs, Xs_before)
    assert all(prm.grad is None for prm in enc.parameters())
    with torch.no_grad():
        terrain = enc(imgs, rots, trans, intrins, post_rots, post_trans)
        k = max(int(round(dp.dphys_cfg.grid_res / float(enc.dx[0]))), 1)
        pool = torch.nn.AvgPool2d(k, k) if k > 1 else torch.nn.Identity()
        state0 = (Xs[:, 0].clone(), Xds[:, 0].clone(), Rs[:, 0].clone(), Om[:, 0].clone())
        states, _ = dp(z_grid=pool(terrain['terrain']).squeeze(1), controls=controls, state=state0, friction=pool(terrain['friction']).squeeze(1))
        xyz, rot = physics_loss_aten(states, [Xs, Xds, Rs, Om], control_ts, traj_ts, gamma=1.0, rotation_loss=True)
        want = [hm_loss(terrain['geom'][:, 0], hm_geom[:, 0], hm_geom[:, 1]), hm_loss(terrain['terrain'][:, 0], hm_terrain[:, 0], hm_terrain[:, 1]), xyz, rot]
    figs = [_rel(a, b) for a, b in zip(out.tolist(), [float(v) for v in want])]
    print('evaluate:', out.tolist(), 'relative differences', figs)
    assert all(np.isfinite(out.tolist())) and all(f <= 1e-5 for f in figs), figs
