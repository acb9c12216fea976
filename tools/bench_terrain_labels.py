"""`rigid_terrain_heightmap` on the MI355X: the HIP route (`mf_terrain_labels_f32`: fill, one thread per item, finalize) against the ATen form on
the GPU (`rigid_terrain_heightmap_aten`: the same definition as elementwise tensor operations -- what a user would write without the kernel).

    python tools/bench_terrain_labels.py [--iters 30] [--warmup 5] [--out profiles/terrain_labels.txt]

Shapes: 131 072 cloud points per sample seen by 4 cameras with 1200 x 1920 label masks, T = 100 recorded poses under the default 0.7 x 1.0 m
footprint, a 256^2 grid of 0.1 m (d_max = 12.8), S = 1 and S = 8 samples, with and without the per-point label output.
    hip_launch    `terrain_labels_into` on tensors already on the GPU, into static buffers (three launches, nothing allocated)
    aten_launch   `rigid_terrain_heightmap_aten` on the same GPU tensors (it allocates its temporaries)
Method: HIP events around every call, the two forms alternating in one process after a warm-up of both; median, minimum and p90 over the
calls.  Before timing, the two forms' maps are compared (mask channel equal, heights to one float32 ulp).  The tool sets no bar: it records."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_map_losses import alternate, stats  # noqa: E402
from monoforce_amd import labels as L  # noqa: E402

DEV = 'cuda'
N, C, HI, WI, T = 131072, 4, 1200, 1920, 100
GRID_RES, D_MAX, H_MAX, ROBOT, CLEARANCE = 0.1, 12.8, 1.0, (0.7, 1.0), 0.132
RIGID = (1, 3, 4, 7, 9, 12)


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def inputs(S, rng):
    """A lidar-like cloud (uniform in a 30 m square, heights within +-1.5 m), four cameras looking forward, left, back and right."""
    pts = rng.uniform(-15.0, 15.0, (S * N, 3))
    pts[:, 2] = rng.uniform(-1.5, 1.5, S * N)
    base = np.array([[0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])
    rots = np.stack([rot_z(np.pi / 2 * c) @ base for c in range(C)])
    K = np.array([[1000.0, 0, WI / 2], [0, 1000.0, HI / 2], [0, 0, 1.0]])
    pose_align = np.stack([np.hstack([rot_z(0.02 * s), [[0.0], [0.0], [0.1]]]) for s in range(S)])
    poses = np.zeros((S, T, 3, 4))
    for t in range(T):
        poses[:, t, :, :3] = rot_z(0.01 * t)
        poses[:, t, :, 3] = [0.1 * t, 0.02 * t, 0.15]
    t = dict(points=torch.from_numpy(pts.astype(np.float32)), seg=torch.from_numpy(rng.integers(0, 15, (S, C, HI, WI), dtype=np.uint8)),
             rots=torch.from_numpy(rots.astype(np.float32)), trans=torch.from_numpy((0.3 * rng.standard_normal((C, 3))).astype(np.float32)),
             intrins=torch.from_numpy(np.broadcast_to(K, (C, 3, 3)).astype(np.float32).copy()), pose_align=torch.from_numpy(pose_align),
             poses=torch.from_numpy(poses), offsets=torch.arange(S + 1, dtype=torch.int32) * N)
    return {k: v.to(DEV) for k, v in t.items()}


def ulp_distance(a, b):
    def key(x):
        i = x.contiguous().view(torch.int32).long()
        return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))
    return int((key(a) - key(b)).abs().max())


def metadata_lines():
    try:
        import kernel_metadata
        return ['# ' + json.dumps(dict(kernel=name, **m)) for o, name, m in kernel_metadata.kernels() if o == 'terrain_labels.o']
    except Exception as e:      # (no LLVM tools, or the objects are not next to the library)
        return [f'# kernel metadata not available here: {type(e).__name__}']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'terrain_labels.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_terrain_labels needs the MI355X'
    lines = [f'# rigid_terrain_heightmap: S x {N} points x {C} cameras of {HI}x{WI}, T = {T} poses, footprint {ROBOT} m, grid {int(2 * D_MAX / GRID_RES)}^2 at {GRID_RES} m:',
             '# the HIP route (terrain_labels_into, static buffers) vs rigid_terrain_heightmap_aten on the GPU',
             f'# HIP events per call, forms alternating in one process, {args.warmup} warm-up + {args.iters} timed calls each; ms',
             f'# device: {torch.cuda.get_device_name(0)}']
    lines += metadata_lines()
    rng = np.random.default_rng(0)
    fx, fy = L._footprint_axes(ROBOT, GRID_RES, DEV)
    xb = L._bin_edges(D_MAX, GRID_RES, DEV)
    n = xb.numel()
    for S in (1, 8):
        t = inputs(S, rng)
        hm = torch.empty(S, 2, n, n, device=DEV)
        scratch = torch.empty(S * n * n, dtype=torch.int32, device=DEV)
        for want_labels in (False, True):
            lab = torch.empty(S * N, C, dtype=torch.int16, device=DEV) if want_labels else None

            def hip():
                return L.terrain_labels_into(t['points'], t['offsets'], t['seg'], t['rots'], t['trans'], t['intrins'], t['pose_align'], t['poses'], fx, fy,
                                             xb, xb, RIGID, CLEARANCE, D_MAX, -H_MAX, H_MAX, None, 1.0 / GRID_RES, scratch, hm, lab, N)

            def aten():
                return L.rigid_terrain_heightmap_aten(t['points'], t['seg'], t['rots'], t['trans'], t['intrins'], RIGID, t['pose_align'], t['poses'], GRID_RES,
                                                      D_MAX, H_MAX, robot_size=ROBOT, clearance=CLEARANCE, offsets=t['offsets'],
                                                      return_point_labels=want_labels)
            a = aten()
            a_hm = a[0] if want_labels else a
            hip()
            torch.cuda.synchronize()
            mask_equal = bool(torch.equal(a_hm[:, 1], hm[:, 1]))
            ulps = ulp_distance(a_hm[:, 0], hm[:, 0])
            labels_equal = bool(torch.equal(a[1], lab)) if want_labels else None
            del a, a_hm
            ms = alternate(dict(hip_launch=hip, aten_launch=aten), args.iters, args.warmup)
            for k in ('hip_launch', 'aten_launch'):
                row = dict(S=S, points=N, cameras=C, T=T, grid=n, point_labels=want_labels, form=k, **stats(ms[k]))
                if k == 'hip_launch':
                    row.update(mask_equal_to_aten=mask_equal, height_ulps_from_aten=ulps, labels_equal_to_aten=labels_equal,
                               measured_cells=int(hm[:, 1].sum()))
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
            ratio = float(np.median(ms['aten_launch']) / np.median(ms['hip_launch']))
            lines.append(f'# S={S} point_labels={int(want_labels)}: aten / hip = {ratio:.1f} (median)')
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
        del t
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
