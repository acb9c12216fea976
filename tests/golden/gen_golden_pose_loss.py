#!/usr/bin/env python
"""Generate tests/golden/pose_loss.npz by running the REAL reference losses (monoforce/src/monoforce/losses.py) on the CPU.

Runs only where the reference tree is present (`MONOFORCE_REFERENCE`, default /root/reference); the module is loaded by file path,
unmodified.  Stored (numeric arrays only, float32 and float64, a few KB):
  `<dt>/X, R, Xgt, Rgt, pred_ts, gt_ts`   B = 3 rollouts, T1 = 48 predicted steps, T2 = 7 stamps.  R = random rotations + 0.02 N(0,1) per entry
                                           (off SO(3), as the default integrator's are); Rgt = R[nearest] . Rot(random axis, angle in U(0.3, 2.5));
                                           stamps crowded enough that one rollout has two stamps on one predicted step
  `<dt>/loss, loss_rot`                    physics_loss(rotation_loss=True, gamma=0.9)
  `<dt>/g_X, g_R`                          autograd gradients of loss + loss_rot
  `<dt>/rd_mean, rd_sum, rd_none`          rotation_difference(R[:, :T2], Rgt) for the three reductions; `td_*`: translation_difference(X[:, :T2], Xgt)
  `<dt>/q1_near, q2_near, q1_far, q2_far, t, slerp_near, slerp_far`   slerp on a pair with dot > 0.9995 and one below
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.path.realpath(os.environ.get('MONOFORCE_REFERENCE', '/root/reference'))
REF_LOSSES = os.path.realpath(os.path.join(REF_ROOT, 'monoforce', 'src', 'monoforce', 'losses.py'))
assert REF_LOSSES.startswith(REF_ROOT + os.sep) and os.path.isfile(REF_LOSSES), REF_LOSSES
_spec = importlib.util.spec_from_file_location('reference_losses', REF_LOSSES)
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
assert os.path.realpath(ref.__file__).startswith(REF_ROOT + os.sep), ref.__file__

B, T1, T2, GAMMA = 3, 48, 7, 0.9


def rotation(axis, angle):
    """Rodrigues' formula, float64."""
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def inputs():
    rng = np.random.default_rng(20)
    pred_ts = np.tile(np.arange(T1) * 0.1, (B, 1))
    gt_ts = np.sort(rng.random((B, T2)) * 1.5, axis=1)                      # 7 stamps on ~15 steps: crowded
    nearest = np.abs(pred_ts[:, None, :] - gt_ts[:, :, None]).argmin(axis=2)
    assert any(len(set(row)) < T2 for row in nearest.tolist()), 'no rollout has two stamps on one step: pick another seed'
    X = rng.standard_normal((B, T1, 3))
    Xgt = X[np.arange(B)[:, None], nearest] + 0.3 * rng.standard_normal((B, T2, 3))
    R = np.stack([np.stack([rotation(rng.standard_normal(3), rng.uniform(0, np.pi)) for _ in range(T1)]) for _ in range(B)])
    R = R + 0.02 * rng.standard_normal(R.shape)
    Rgt = np.stack([np.stack([R[b, nearest[b, j]] @ rotation(rng.standard_normal(3), rng.uniform(0.3, 2.5)) for j in range(T2)]) for b in range(B)])
    q1 = rng.standard_normal(4); q1 /= np.linalg.norm(q1)
    q2n = q1 + 0.01 * rng.standard_normal(4); q2n /= np.linalg.norm(q2n)
    q2f = rng.standard_normal(4); q2f /= np.linalg.norm(q2f)
    assert q1 @ q2n > 0.9995 > q1 @ q2f
    return dict(X=X, R=R, Xgt=Xgt, Rgt=Rgt, pred_ts=pred_ts, gt_ts=gt_ts, q1_near=q1, q2_near=q2n, q1_far=q1, q2_far=q2f, t=np.linspace(0.0, 1.0, 5))


def main():
    out = {}
    base = inputs()
    for tag, dt in (('f64', torch.float64), ('f32', torch.float32)):
        t = {k: torch.as_tensor(v).to(dt) for k, v in base.items()}
        X, R = t['X'].clone().requires_grad_(True), t['R'].clone().requires_grad_(True)
        loss, loss_rot = ref.physics_loss([X, None, R], [t['Xgt'], None, t['Rgt']], t['pred_ts'], t['gt_ts'], gamma=GAMMA, rotation_loss=True)
        (loss + loss_rot).backward()
        assert torch.isfinite(X.grad).all() and torch.isfinite(R.grad).all()
        res = dict(t, loss=loss.detach(), loss_rot=loss_rot.detach(), g_X=X.grad, g_R=R.grad)
        for red in ('mean', 'sum', 'none'):
            res['rd_' + red] = ref.rotation_difference(t['R'][:, :T2], t['Rgt'], reduction=red)
            res['td_' + red] = ref.translation_difference(t['X'][:, :T2], t['Xgt'], reduction=red)
        res['slerp_near'] = ref.slerp(t['q1_near'], t['q2_near'], t['t'])
        res['slerp_far'] = ref.slerp(t['q1_far'], t['q2_far'], t['t'])
        for k, v in res.items():
            out[f'{tag}/{k}'] = v.detach().numpy()
    path = os.path.join(HERE, 'pose_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', 'loss', float(out['f64/loss']), 'loss_rot', float(out['f64/loss_rot']))


if __name__ == '__main__':
    main()
