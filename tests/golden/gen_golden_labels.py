#!/usr/bin/env python
"""Generate tests/golden/terrain_labels.npz by running the REAL reference functions on the CPU: `ego_to_cam` and `get_only_in_img_mask`
(models/terrain_encoder/utils.py), `transform_cloud` (transformations.py), `estimate_heightmap`, `filter_grid`, `hm_to_cloud` and
`within_bounds` (cloudproc.py), composed in the order of datasets/rough.py:545-649 (`get_semantic_cloud`, `get_footprint_traj_points`,
`get_terrain_height_map`) on synthetic inputs.

Runs only where the reference tree is present (`MONOFORCE_REFERENCE`); the modules are loaded by file path, unmodified.  (utils.py imports
torchvision at its top for functions not used here; where that package is absent a placeholder module stands in for the import, as in gen_golden.py.)

Why the inputs are constructed.  The reference projects with float32 `matmul` and aligns with numpy's float64 GEMM; neither fixes an operation
order, the definition in include/monoforce_hip.h does.  So every input point is kept away from every decision, checked in float64, and an
offending point (or pose) is drawn again from the seeded generator until none is left -- nothing is ever excluded from a comparison:
  camera depth   >= 0.5 m or <= -0.5 m
  u, v           >= 1/64 px from every integer (the mask bounds 1, Wi-1, Hi-1 are integers), |u|, |v| < 3000
  aligned x, y   >= 1e-4 m from every bin edge and from +-d_max;  z >= 1e-4 m from +-h_max
(The largest float32-versus-float64 difference of u, v measured on the host at depth >= 0.5 m and |u|, |v| < 3000 was 1.2e-3 px, for torch's
matmul and for the fixed order alike, over 200 000 points x 4 cameras: 1/64 px is thirteen times that.)

Asserted here: the referee (tests/terrain_labels_reference.py) reproduces the reference's per-point labels and mask channel exactly and its
heights to one float32 ulp.  The worst case is written to profiles/terrain_labels_errors.txt.

Stored (data only):
  points [sumN,3] f32, offsets [S+1], seg [S,C,Hi,Wi] u8, rots, trans, intrins (f32), pose_align [S,3,4] f64, poses [S,T,3,4] f64, rigid_labels,
  scalars (grid_res, d_max, h_max, width, length, clearance), hm_ref [S,2,n,n] f32, labels_ref [sumN,C] i16,
  sem_points / sem_labels / sem_offsets: the reference's concatenated semantic clouds (all labels), per sample,
  foot_ref [S,T*F,3] f64: the reference's footprint sweep,
  fg_*: filter_grid inputs and outputs, wb_*: within_bounds, hc_*: hm_to_cloud.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import terrain_labels_reference as referee  # noqa: E402

REF_ROOT = os.path.realpath(os.environ.get('MONOFORCE_REFERENCE', '/root/reference'))
PKG = os.path.join(REF_ROOT, 'monoforce', 'src', 'monoforce')


def load(name, rel):
    path = os.path.realpath(os.path.join(PKG, rel))
    assert path.startswith(REF_ROOT + os.sep) and os.path.isfile(path), path
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


try:
    import torchvision  # noqa: F401
except ImportError:
    class _Unused:                 # (utils.py builds a few torchvision transforms at import time; none is used here)
        def __init__(self, *args, **kwargs):
            pass
    _tv = types.ModuleType('torchvision')
    _tv.transforms = types.ModuleType('torchvision.transforms')
    for _name in ('Normalize', 'Compose', 'ToTensor', 'ToPILImage', 'Resize'):
        setattr(_tv.transforms, _name, _Unused)
    sys.modules['torchvision'], sys.modules['torchvision.transforms'] = _tv, _tv.transforms
ref_utils = load('reference_lss_utils', os.path.join('models', 'terrain_encoder', 'utils.py'))
ref_tf = load('reference_transformations', 'transformations.py')
ref_cp = load('reference_cloudproc', 'cloudproc.py')

S, C, HI, WI, T = 2, 3, 24, 32, 6
NS = (700, 500)
GRID_RES, D_MAX, H_MAX = 0.2, 3.2, 1.0
WIDTH, LENGTH, CLEARANCE = 0.7, 1.0, 0.132
RIGID = (1, 3, 4, 7)
N_LABELS = 9


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1.0, 0], [-np.sin(a), 0, np.cos(a)]])


def cameras(rng):
    """C cameras per sample fanned around the robot: camera axes (x right, y down, z forward) in the robot's frame (x forward, z up)."""
    base = np.array([[0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])
    rots = np.stack([np.stack([rot_z(2 * np.pi * c / C + 0.1 * s) @ rot_y(0.1) @ base for c in range(C)]) for s in range(S)])
    trans = 0.2 * rng.standard_normal((S, C, 3))
    K = np.array([[14.0, 0, 16.3], [0, 13.0, 11.7], [0, 0, 1.0]])
    intr = np.tile(K, (S, C, 1, 1)) + 0.2 * rng.standard_normal((S, C, 3, 3)) * (K != 0)
    return rots.astype(np.float32), trans.astype(np.float32), intr.astype(np.float32)


def near_integer(a, margin):
    return np.abs(a - np.round(a)) < margin


def offending_points(p, rots, trans, intr, A, bins):
    """float64 check of every decision a cloud point takes part in."""
    p64 = p.astype(np.float64)
    bad = np.zeros(p.shape[0], dtype=bool)
    for c in range(C):
        w = (intr[c].astype(np.float64) @ (rots[c].astype(np.float64).T @ (p64 - trans[c].astype(np.float64)).T)).T
        u, v = w[:, 0] / w[:, 2], w[:, 1] / w[:, 2]
        bad |= (np.abs(w[:, 2]) < 0.5) | near_integer(u, 1 / 64) | near_integer(v, 1 / 64) | (np.abs(u) >= 3000) | (np.abs(v) >= 3000)
    return bad | offending_aligned((A[:, :3] @ p64.T + A[:, 3:]).T, bins)


def offending_aligned(g, bins):
    edges = np.concatenate([bins.astype(np.float64), [D_MAX, -D_MAX]])
    bad = np.zeros(g.shape[0], dtype=bool)
    for k in (0, 1):
        bad |= (np.abs(g[:, k, None] - edges[None]) < 1e-4).any(axis=1)
    return bad | (np.abs(np.abs(g[:, 2]) - H_MAX) < 1e-4)


def draw_points(rng, n):
    p = rng.uniform(-4.0, 4.0, (n, 3))
    p[:, 2] = rng.uniform(-1.3, 1.3, n)
    return p.astype(np.float32)


def draw_pose(rng, t):
    P = np.zeros((3, 4))
    P[:, :3] = rot_z(0.15 * t + 0.05 * rng.standard_normal()) @ rot_y(0.05 * rng.standard_normal())
    P[:, 3] = [0.45 * t + 0.1 * rng.standard_normal(), 0.1 * t + 0.1 * rng.standard_normal(), 0.3 + 0.05 * rng.standard_normal()]
    return P


def reference_footprint(poses):
    """get_footprint_traj_points (rough.py:343-365) with the reference's transform_cloud; `poses` [T,4,4] float64 is changed in place, as there."""
    x = np.arange(-LENGTH / 2, LENGTH / 2, GRID_RES)
    y = np.arange(-WIDTH / 2, WIDTH / 2, GRID_RES)
    x, y = np.meshgrid(x, y)
    foot = np.asarray(np.stack([x, y, np.zeros_like(x)], axis=-1).reshape((-1, 3)), dtype=np.float32)
    poses[:, 2, 3] -= abs(np.float32(CLEARANCE))
    return np.concatenate([ref_tf.transform_cloud(foot, Tr) for Tr in poses], axis=0), foot


def reference_semantic_cloud(p, seg, rots, trans, intr):
    """get_semantic_cloud (rough.py:552-581) up to the class filter: per camera, in the order given, the points it sees and their labels."""
    pts, labs, per_point = [], [], np.full((p.shape[0], C), -1, dtype=np.int16)
    lidar = torch.as_tensor(p)
    for c in range(C):
        img = ref_utils.ego_to_cam(lidar.T, torch.as_tensor(rots[c]), torch.as_tensor(trans[c]), torch.as_tensor(intr[c])).T
        mask = ref_utils.get_only_in_img_mask(img.T, seg.shape[1], seg.shape[2])
        uv = img[mask][:, :2].numpy().astype(int)
        lab = seg[c][uv[:, 1], uv[:, 0]]
        pts.append(lidar[mask].numpy())
        labs.append(lab)
        per_point[mask.numpy(), c] = lab
    return np.concatenate(pts), np.concatenate(labs), per_point


def to44(P):
    out = np.tile(np.eye(4), P.shape[:-2] + (1, 1))
    out[..., :3, :] = P
    return out


def cloudproc_golden(rng, out):
    cells = rng.integers(-4, 4, (60, 3))
    xyz = ((cells + rng.uniform(0.05, 0.95, cells.shape)) * 0.25).astype(np.float32)        # 60 points in at most 512 cells of 0.25 m, off the cell borders
    xyz = np.concatenate([xyz, xyz[:15] + np.float32(0.01)]).astype(np.float32)             # ... and 15 certain repeats of a cell
    xyz = xyz[rng.permutation(xyz.shape[0])]
    structured = np.zeros(xyz.shape[0], dtype=[('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('i', 'f4')])
    for k, name in enumerate('xyz'):
        structured[name] = xyz[:, k]
    structured['i'] = rng.random(xyz.shape[0]).astype(np.float32)
    out['fg_xyz'], out['fg_intensity'], out['fg_grid_res'] = xyz, structured['i'], np.float64(0.25)
    for keep in ('first', 'last'):
        out[f'fg_plain_{keep}_ind'] = ref_cp.filter_grid(xyz.copy(), 0.25, keep=keep, only_mask=True)
        out[f'fg_plain_{keep}_rows'] = ref_cp.filter_grid(xyz.copy(), 0.25, keep=keep)
        out[f'fg_struct_{keep}_ind'] = ref_cp.filter_grid(structured.copy(), 0.25, keep=keep, only_mask=True)
        rows = ref_cp.filter_grid(structured.copy(), 0.25, keep=keep)
        out[f'fg_struct_{keep}_rows'] = np.stack([rows[n] for n in ('x', 'y', 'z', 'i')], axis=1)
        assert len(out[f'fg_plain_{keep}_ind']) < xyz.shape[0]
    x = rng.standard_normal((5, 7)).astype(np.float32)
    out['wb_x'] = x
    out['wb_min_max'] = ref_cp.within_bounds(torch.as_tensor(x), min=-0.5, max=0.8).numpy()
    out['wb_bounds'] = ref_cp.within_bounds(x, bounds=(-1.0, 0.2)).numpy()
    out['wb_max_only'] = ref_cp.within_bounds(torch.as_tensor(x), max=0.0).numpy()
    out['wb_inf'] = ref_cp.within_bounds(torch.as_tensor(x), min=-float('inf'), max=float('inf')).numpy()
    cfg = types.SimpleNamespace(d_max=D_MAX)
    h = rng.standard_normal((6, 6)).astype(np.float32)
    m = rng.random((6, 6)) < 0.5
    out['hc_height'], out['hc_mask'] = h, m
    out['hc_numpy'] = ref_cp.hm_to_cloud(h, cfg)
    out['hc_numpy_masked'] = ref_cp.hm_to_cloud(h, cfg, mask=m.astype(np.float32))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out['hc_torch'] = ref_cp.hm_to_cloud(torch.as_tensor(h), cfg).numpy()
        out['hc_torch_masked'] = ref_cp.hm_to_cloud(torch.as_tensor(h), cfg, mask=torch.as_tensor(m)).numpy()


def ulp_distance(a, b):
    """Distance of two float32 arrays in units of the last place (ordered bit patterns)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i >= 0, i, -(i & 0x7FFFFFFF))
    return np.abs(key(a) - key(b))


def main():
    rng = np.random.default_rng(2024)
    bins = torch.arange(-D_MAX, D_MAX, GRID_RES).numpy()
    assert bins.dtype == np.float32
    rots, trans, intr = cameras(rng)
    seg = rng.integers(0, N_LABELS, (S, C, HI, WI)).astype(np.uint8)
    pose_align = np.stack([np.hstack([rot_z(0.03 * (s + 1)) @ rot_y(0.04 - 0.02 * s), [[0.02], [-0.03], [0.05 * s]]]) for s in range(S)])
    redrawn_points = redrawn_poses = 0
    clouds, poses = [], []
    fx = np.arange(-LENGTH / 2, LENGTH / 2, GRID_RES).astype(np.float32)
    fy = np.arange(-WIDTH / 2, WIDTH / 2, GRID_RES).astype(np.float32)
    for s in range(S):
        p = draw_points(rng, NS[s])
        while True:
            bad = offending_points(p, rots[s], trans[s], intr[s], pose_align[s], bins)
            if not bad.any():
                break
            redrawn_points += int(bad.sum())
            p[bad] = draw_points(rng, int(bad.sum()))
        clouds.append(p)
        ps = []
        for t in range(T):
            while True:
                P = draw_pose(rng, t)
                lowered = P.copy()
                lowered[2, 3] -= abs(np.float32(CLEARANCE))
                X, Y = np.meshgrid(fx.astype(np.float64), fy.astype(np.float64))
                g = (lowered[:, :3] @ np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)]) + lowered[:, 3:]).T
                if not offending_aligned(g, bins).any():
                    break
                redrawn_poses += 1
            ps.append(P)
        poses.append(np.stack(ps))
    points = np.concatenate(clouds)
    offsets = np.concatenate([[0], np.cumsum(NS)]).astype(np.int32)
    poses = np.stack(poses)

    # ---- the reference, sample by sample (rough.py:621-649)
    hm_ref, labels_ref, sem_p, sem_l, sem_off, foot_ref = [], [], [], [], [0], []
    for s in range(S):
        traj_points, foot0 = reference_footprint(to44(poses[s]).copy())
        grid_xy = np.stack(np.meshgrid(fx, fy), axis=-1).reshape(-1, 2)
        assert np.array_equal(foot0, np.concatenate([grid_xy, np.zeros((grid_xy.shape[0], 1), dtype=np.float32)], axis=1))
        cloud, labs, per_point = reference_semantic_cloud(clouds[s], seg[s], rots[s], trans[s], intr[s])
        sem_p.append(cloud), sem_l.append(labs), sem_off.append(sem_off[-1] + len(labs))
        seg_points = ref_tf.transform_cloud(cloud[np.isin(labs, RIGID)], to44(pose_align[s]))
        both = torch.as_tensor(np.concatenate((seg_points, traj_points), axis=0), dtype=torch.float32)
        hm_ref.append(ref_cp.estimate_heightmap(both, d_max=D_MAX, grid_res=GRID_RES, h_max=H_MAX).numpy())
        labels_ref.append(per_point)
        foot_ref.append(traj_points)
    hm_ref, labels_ref = np.stack(hm_ref).astype(np.float32), np.concatenate(labels_ref)

    # ---- the referee against it
    hm, labels = referee.terrain_labels(points, offsets, seg, rots, trans, intr, RIGID, pose_align, poses, fx, fy, np.float32(CLEARANCE), bins, D_MAX, H_MAX)
    assert np.array_equal(labels, labels_ref), 'per-point labels differ'
    assert np.array_equal(hm[:, 1], hm_ref[:, 1]), 'mask channel differs'
    ulps = ulp_distance(hm[:, 0], hm_ref[:, 0])
    worst = int(ulps.max())
    at = np.unravel_index(int(ulps.argmax()), ulps.shape)
    assert worst <= 1, worst
    kept = int(np.isin(np.concatenate(sem_l), RIGID).sum())
    lines = ['# referee (tests/terrain_labels_reference.py) against the reference pipeline (rough.py:545-649 composed by tests/golden/gen_golden_labels.py), CPU',
             f'# S={S} samples of {NS} points, C={C} cameras of {HI}x{WI}, T={T} poses, footprint {fx.size}x{fy.size}, grid {bins.size}^2 at {GRID_RES} m',
             f'points redrawn to clear the margins: {redrawn_points}; poses redrawn: {redrawn_poses}',
             f'camera sightings: {len(np.concatenate(sem_l))}, of them rigid: {kept}; measured cells: {int(hm_ref[:, 1].sum())} of {hm_ref[:, 1].size}',
             'per-point labels: equal; mask channel: equal',
             f'heights: worst difference {worst} float32 ulp ({float(np.abs(hm[:, 0].astype(np.float64) - hm_ref[:, 0].astype(np.float64)).max()):.3g} m) at '
             f'(sample, ix, iy) = {tuple(int(v) for v in at)}; cells that differ: {int((ulps > 0).sum())}']
    with open(os.path.join(REPO, 'profiles', 'terrain_labels_errors.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))

    out = dict(points=points, offsets=offsets, seg=seg, rots=rots, trans=trans, intrins=intr, pose_align=pose_align, poses=poses,
               rigid_labels=np.asarray(RIGID, dtype=np.int32), grid_res=np.float64(GRID_RES), d_max=np.float64(D_MAX), h_max=np.float64(H_MAX),
               width=np.float64(WIDTH), length=np.float64(LENGTH), clearance=np.float32(CLEARANCE), hm_ref=hm_ref, labels_ref=labels_ref,
               sem_points=np.concatenate(sem_p), sem_labels=np.concatenate(sem_l), sem_offsets=np.asarray(sem_off, dtype=np.int32),
               foot_ref=np.stack(foot_ref))
    cloudproc_golden(rng, out)
    path = os.path.join(HERE, 'terrain_labels.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
