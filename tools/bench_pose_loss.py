"""`physics_loss(..., rotation_loss=True)` (scripts/eval.py:151-153): the HIP route (`mf_nearest_steps_*` + `mf_pose_loss_value_*` /
`mf_pose_loss_bwd_*`) against the ATen form (`physics_loss_aten`, the route of this call before the kernels existed).

    python tools/bench_pose_loss.py [--sizes 1024,16384] [--iters 60] [--warmup 10] [--out profiles/pose_loss.txt]

Inputs: the states of a real rollout (`DPhysics.forward`, the 4-point body on the shared 256 x 256 bump terrain, T = 500: Xs / Rs are [B,T,...]
views of the kernel's time-major buffers, read and differentiated in place), 50 ground-truth stamps (every 10th step), ground-truth poses = the
rollout's own at the stamps, moved by N(0, 0.1) and turned by an angle in U(0.05, 0.5) about a random axis.
    value          both scalars, no autograd graph              (hip: one launch after the index table's; aten: ~40)
    value_bwd      both scalars and d(loss + loss_rot) / d(Xs, Rs), the gradients in the layout of the rollout's buffers
    *_near         the same with the nearest-step table given (callers with fixed stamps cache it): the loss launches alone
Method: HIP events around every call, the forms alternating in one process after a warm-up of all of them; median, minimum and p90 over the calls."""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_problem  # noqa: E402
from monoforce_amd import losses as L  # noqa: E402

DEV = 'cuda'
T, EVERY, GAMMA = 500, 10, 1.0


def small_rotations(n, gen):
    """[n,3,3] rotations by an angle in U(0.05, 0.5) about random axes (Rodrigues)."""
    a = torch.randn(n, 3, generator=gen)
    a = a / a.norm(dim=1, keepdim=True)
    ang = 0.05 + 0.45 * torch.rand(n, generator=gen)
    K = torch.zeros(n, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    return torch.eye(3) + torch.sin(ang)[:, None, None] * K + (1 - torch.cos(ang))[:, None, None] * (K @ K)


def alternate(forms, iters, warmup):
    """forms: dict name -> callable.  HIP events around every call, the forms alternating; returns dict name -> ms array."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in forms}
    for i in range(iters):
        for k, fn in forms.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4), p90_ms=round(float(np.percentile(ms, 90)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1024,16384')
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pose_loss.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pose_loss needs the MI355X'
    lines = ['# tools/bench_pose_loss.py: physics_loss(rotation_loss=True, gamma=1.0) on the time-major outputs of a T = 500 rollout, 50 stamps:',
             '# the HIP route (mf_nearest_steps + mf_pose_loss_value / _bwd) vs physics_loss_aten; *_near: the nearest-step table given',
             f'# HIP events per call, forms alternating in one process, {args.warmup} warm-up + {args.iters} timed calls each; ms',
             f'# device: {torch.cuda.get_device_name(0)}']
    gen = torch.Generator().manual_seed(0)
    verdicts = []
    for B in [int(v) for v in args.sizes.split(',')]:
        cfg, dp, pts, masks, z, mu, ctrl = build_problem(B, T, 4, DEV, 1)
        with torch.no_grad():
            (Xs, _, Rs, _), _ = dp(z.to(DEV).unsqueeze(0), ctrl.to(DEV), friction=mu.to(DEV).unsqueeze(0))
        assert Xs.stride(0) < Xs.stride(1) and Rs.stride(0) < Rs.stride(1), 'expected the time-major buffers'
        sel = torch.arange(EVERY - 1, T, EVERY, device=DEV)
        T2 = sel.numel()
        ts = torch.linspace(0, cfg.traj_sim_time, int(cfg.traj_sim_time / cfg.dt), device=DEV)[:T]
        pred_ts, gt_ts = ts.unsqueeze(0).expand(B, -1), ts[sel].unsqueeze(0).expand(B, -1).contiguous()
        Xgt = (Xs[:, sel] + 0.1 * torch.randn(B, T2, 3, generator=gen).to(DEV)).contiguous()
        Rgt = (Rs[:, sel] @ small_rotations(B * T2, gen).view(B, T2, 3, 3).to(DEV)).contiguous()
        X, R = Xs.detach().requires_grad_(True), Rs.detach().requires_grad_(True)       # same memory, same strides
        sp, sg = [X, None, R], [Xgt, None, Rgt]
        near_hip, near_aten = L.nearest_steps_hip(pred_ts, gt_ts), L.nearest_steps(pred_ts, gt_ts)
        assert torch.equal(near_hip.long(), near_aten)

        def value(fn, **kw):
            with torch.no_grad():
                return fn(sp, sg, pred_ts, gt_ts, gamma=GAMMA, rotation_loss=True, **kw)

        def value_bwd(fn, **kw):
            loss, rot = fn(sp, sg, pred_ts, gt_ts, gamma=GAMMA, rotation_loss=True, **kw)
            return (loss, rot) + torch.autograd.grad(loss + rot, (X, R))
        forms = dict(hip_value=lambda: value(L.physics_loss), aten_value=lambda: value(L.physics_loss_aten),
                     hip_value_bwd=lambda: value_bwd(L.physics_loss), aten_value_bwd=lambda: value_bwd(L.physics_loss_aten),
                     hip_value_near=lambda: value(L.physics_loss, nearest=near_hip), aten_value_near=lambda: value(L.physics_loss_aten, nearest=near_aten),
                     hip_value_bwd_near=lambda: value_bwd(L.physics_loss, nearest=near_hip),
                     aten_value_bwd_near=lambda: value_bwd(L.physics_loss_aten, nearest=near_aten))
        h, a = forms['hip_value_bwd'](), forms['aten_value_bwd']()
        assert type(h[0].grad_fn).__name__.startswith('_FusedPoseLoss') and h[2].stride() == X.stride() and h[3].stride() == R.stride()
        dev = dict(loss=abs(float(h[0]) - float(a[0])) / abs(float(a[0])), loss_rot=abs(float(h[1]) - float(a[1])) / abs(float(a[1])),
                   gXs=float((h[2] - a[2]).abs().max() / a[2].abs().max()), gRs=float((h[3] - a[3]).abs().max() / a[3].abs().max()))
        assert all(math.isfinite(v) for v in dev.values()), dev
        ms = alternate(forms, args.iters, args.warmup)
        for k in forms:
            row = dict(what='pose_loss', B=B, T1=T, T2=T2, form=k, **stats(ms[k]))
            if k == 'hip_value_bwd':
                row.update(rel_dev_from_aten={n: float('%.3g' % v) for n, v in dev.items()})
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        for k in ('value', 'value_bwd', 'value_near', 'value_bwd_near'):
            ratio = float(np.median(ms['aten_' + k]) / np.median(ms['hip_' + k]))
            verdicts.append(ratio >= 1)
            lines.append(f'# B = {B}, {k}: aten / hip = {ratio:.2f} (median); the hip route is {"below" if ratio >= 1 else "NOT BELOW"} the ATen form')
            print(lines[-1], flush=True)
    lines.append('# the hip route is below the ATen form at every size and form measured' if all(verdicts) else
                 '# the hip route is NOT below the ATen form everywhere: see the lines marked NOT BELOW')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
