"""Inputs shared by tests/test_terrain_labels_cpu.py and tests/test_terrain_labels_gpu.py: small cases where the label kernel can still go
wrong, as numpy arrays; `referee(case)` evaluates tests/terrain_labels_reference.py on one (once per case: the results are kept and must not
be changed), `api_args(case, device)` turns it into the arguments of `rigid_terrain_heightmap` / `rigid_terrain_heightmap_aten`."""
import numpy as np
import torch

from tests import terrain_labels_reference as ref

f32 = np.float32
CAM_BASE = np.array([[0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])      # camera axes (x right, y down, z forward) in the robot's frame
FOOT_1x1 = {0.2: (0.18, 0.18), 0.15: (0.13, 0.13)}                  # robot_size = (width, length) giving a 1 x 1 footprint grid
FOOT_5x7 = {0.2: (1.35, 0.95), 0.15: (1.0, 0.7)}                    # ... 5 points along x, 7 along y


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def axes(robot_size, grid_res):
    width, length = robot_size
    return np.arange(-length / 2, length / 2, grid_res).astype(f32), np.arange(-width / 2, width / 2, grid_res).astype(f32)


def random_case(seed, Ns, C, mask, T, foot, grid_res, d_max=2.0, labels=(1, 2, 5), n_labels=8, shared=False, clearance=0.1, r_min=None, h_min=None):
    """S = len(Ns) samples with Ns[s] points each, C cameras fanned around the robot with masks of `mask` = (Hi, Wi)."""
    rng = np.random.default_rng(seed)
    S, (Hi, Wi) = len(Ns), mask
    pts = rng.uniform(-3.0, 3.0, (sum(Ns), 3))
    pts[:, 2] = rng.uniform(-1.2, 1.2, sum(Ns))
    cams = (C,) if shared else (S, C)
    rots = np.zeros(cams + (3, 3))
    for idx in np.ndindex(*cams):
        rots[idx] = rot_z(2 * np.pi * idx[-1] / C + 0.2 * (0 if shared else idx[0])) @ CAM_BASE
    K = np.array([[0.45 * Wi, 0, 0.5 * Wi], [0, 0.45 * Wi, 0.5 * Hi], [0, 0, 1.0]])
    pose_align = np.stack([np.hstack([rot_z(0.05 * (s + 1)), [[0.1 * s], [-0.05], [0.02 * s]]]) for s in range(S)])
    poses = np.zeros((S, T, 3, 4))
    for s in range(S):
        for t in range(T):
            poses[s, t, :, :3] = rot_z(0.2 * t + 0.3 * s)
            poses[s, t, :, 3] = [0.25 * t - 0.5, 0.1 * t * (-1) ** s, 0.2 + 0.03 * t]
    return dict(points=pts.astype(f32), offsets=np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64),
                seg=rng.integers(0, n_labels, (S, C, Hi, Wi)).astype(np.uint8), rots=rots.astype(f32),
                trans=(0.1 * rng.standard_normal(cams + (3,))).astype(f32), intrins=np.broadcast_to(K, cams + (3, 3)).astype(f32).copy(),
                rigid_labels=tuple(labels), pose_align=pose_align, poses=poses, grid_res=grid_res, d_max=d_max, h_max=1.0, robot_size=foot,
                clearance=clearance, r_min=r_min, h_min=h_min)


def identity_camera_case(points, seg, pose_align, poses=None, grid_res=0.2, d_max=2.0, labels=(1,), foot=FOOT_1x1[0.2], clearance=0.0):
    """S samples sharing ONE camera with R = I, t = 0, K = I: w = p, so u = x / z and v = y / z are exact for z = 1.  `points` [S,N,3]."""
    points = np.asarray(points, dtype=f32)
    S, N = points.shape[:2]
    eye = np.eye(3, dtype=f32)[None]
    return dict(points=points.reshape(-1, 3), offsets=np.arange(S + 1, dtype=np.int64) * N, seg=np.asarray(seg, dtype=np.uint8), rots=eye, trans=np.zeros((1, 3), f32),
                intrins=eye, rigid_labels=tuple(labels), pose_align=np.asarray(pose_align, dtype=np.float64),
                poses=np.zeros((S, 0, 3, 4)) if poses is None else np.asarray(poses, dtype=np.float64), grid_res=grid_res, d_max=d_max, h_max=1.0,
                robot_size=foot, clearance=clearance, r_min=None, h_min=None)


def bins_of(case):
    return torch.arange(-case['d_max'], case['d_max'], case['grid_res'], dtype=torch.float32).numpy()


def boundary_case():
    """Identity camera, 17 x 23 masks of label 1 except column 5 (label 0): points exactly on u = 1, u = Wi-1, v = 1, v = Hi-1, one float32 step
    inside each, on integer pixel borders and one step below them, with w_2 = +0, -0 and a denormal; the seen ones land, through a pose_align
    whose x and y rows are pure translations, exactly on a bin edge / the box bound / one step beside it (one sample per landing place)."""
    Hi, Wi = 17, 23
    up, dn = (lambda v: np.nextafter(f32(v), f32(np.inf))), (lambda v: np.nextafter(f32(v), f32(-np.inf)))
    us = [1, up(1), dn(1), Wi - 1, dn(Wi - 1), up(Wi - 1), 5, dn(5), up(5), 6, dn(6), 2.5]
    vs = [1, up(1), Hi - 1, dn(Hi - 1), 3, dn(3), up(3), 7.25]
    rows = [(u, v, 1.0) for u in us for v in vs]
    rows += [(3.0, 3.0, 0.0), (3.0, 3.0, -0.0), (0.0, 0.0, 0.0), (3.0, 3.0, 1e-42), (-3.0, -3.0, -1.0), (6.5, 7.5, 0.5), (5.0, 4.0, 2.0)]
    seg = np.ones((1, Hi, Wi), dtype=np.uint8)
    seg[:, :, 5] = 0
    case = identity_camera_case(np.zeros((1, 1, 3)), seg[None], np.zeros((1, 3, 4)))
    b = bins_of(case)
    places = [(b[0], b[3]), (up(b[0]), b[3]), (b[7], b[0]), (b[7], up(b[7])), (dn(b[7]), dn(b[3])), (f32(2.0), b[1]), (dn(2.0), b[-1]), (b[-1], dn(2.0)),
              (b[1], f32(2.0))]
    S = len(places)
    A = np.zeros((S, 3, 4))
    for s, (x, y) in enumerate(places):
        A[s, 0, 3], A[s, 1, 3] = float(x), float(y)
        A[s, 2] = [0.01, 0.02, 0.0, 0.05 * s]                    # height = a function of the pixel
    pts = np.broadcast_to(np.asarray(rows, dtype=f32), (S, len(rows), 3))
    return identity_camera_case(pts, np.broadcast_to(seg, (S, 1, Hi, Wi)), A)


def footprint_boundary_case():
    """No cloud; a 1 x 1 footprint carried by poses whose translation puts its one point exactly on bin edges and box bounds (and one float32
    step beside them), and on the height bounds."""
    case = identity_camera_case(np.zeros((1, 0, 3)), np.ones((1, 1, 17, 23)), np.zeros((1, 3, 4)))
    b, (fx, fy) = bins_of(case), axes(case['robot_size'], case['grid_res'])
    up, dn = (lambda v: np.nextafter(f32(v), f32(np.inf))), (lambda v: np.nextafter(f32(v), f32(-np.inf)))
    targets = [(b[0], b[2], 0.1), (up(b[0]), b[2], 0.2), (b[4], b[4], 0.3), (up(b[4]), dn(b[4]), 0.4), (f32(2.0), b[3], 0.5), (dn(2.0), dn(2.0), 0.6),
               (b[6], b[6], 1.0), (b[6], b[6], float(dn(1.0))), (b[8], b[8], -1.0), (b[8], b[8], float(up(-1.0))), (b[-1], b[-1], 0.0), (b[-1], b[-1], -0.0)]
    poses = np.zeros((1, len(targets), 3, 4))
    for t, (x, y, z) in enumerate(targets):
        poses[0, t, :, :3] = np.eye(3)
        poses[0, t, :, 3] = [float(x) - float(fx[0]), float(y) - float(fy[0]), z]       # fx + (x - fx) = x exactly in float64
    case['poses'] = poses
    return case


def nonfinite_case():
    case = random_case(7, (257,), 2, (24, 32), 1, FOOT_1x1[0.2], 0.2)
    p = case['points']
    k = 0
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            p[k, col] = bad
            k += 3
    p[k] = [np.nan, np.nan, np.nan]
    p[k + 3] = [np.inf, -np.inf, np.inf]
    return case


def overlap_case():
    """Two cameras with the same pose: the first one's mask is soft (label 0) everywhere, the second one's rigid (label 1)."""
    case = random_case(11, (255,), 2, (24, 32), 0, FOOT_1x1[0.2], 0.2, labels=(1,))
    for name in ('rots', 'trans', 'intrins'):
        case[name][:, 1] = case[name][:, 0]
    case['seg'][:, 0], case['seg'][:, 1] = 0, 1
    return case


def contention_case(n=50_000):
    """n points all seen with a rigid label and all landing in ONE cell with n different heights."""
    rng = np.random.default_rng(5)
    x = rng.uniform(1.5, 30.5, n)
    pts = np.stack([x, np.full(n, 4.5), np.ones(n)], axis=1)[None]
    A = np.array([[[0, 0, 0, 0.31], [0, 0, 0, -0.77], [0.03, 0, 0, 0.0]]])
    return identity_camera_case(pts, np.ones((1, 1, 24, 32)), A)


def class_set_case(labels):
    case = random_case(3, (300,), 2, (17, 23), 1, FOOT_1x1[0.2], 0.2, labels=labels, n_labels=4)
    seg = case['seg']
    seg[seg == 3] = 255             # labels 0, 1, 2 and 255
    return case


# (name, builder): the shapes the issue lists -- cloud sizes 0, 1, 255, 257, 1000; 1, 2, 4 cameras; masks 24 x 32 and 17 x 23; 1 and 3 samples, ragged
# with an empty one; 0, 1, 7 poses; footprints 1 x 1 and 5 x 7; n = 20 and n = 27 (2 d_max / grid_res = 26.67)
SHAPES = {
    'N0_C1_T1_foot5x7_n20': lambda: random_case(20, (0,), 1, (24, 32), 1, FOOT_5x7[0.2], 0.2),
    'N1_C2_T0_n20': lambda: random_case(21, (1,), 2, (17, 23), 0, FOOT_1x1[0.2], 0.2),
    'N255_C4_T7_foot5x7_n27': lambda: random_case(22, (255,), 4, (24, 32), 7, FOOT_5x7[0.15], 0.15),
    'N257_C1_T1_foot1x1_n27': lambda: random_case(23, (257,), 1, (17, 23), 1, FOOT_1x1[0.15], 0.15, r_min=0.6, h_min=-0.5),
    'N1000_C2_T7_foot1x1_n20': lambda: random_case(24, (1000,), 2, (24, 32), 7, FOOT_1x1[0.2], 0.2),
    'S3_ragged_empty_C4_T7_n27': lambda: random_case(25, (257, 0, 1000), 4, (17, 23), 7, FOOT_5x7[0.15], 0.15),
    'S3_ragged_C2_T1_n20_shared': lambda: random_case(26, (1, 255, 0), 2, (24, 32), 1, FOOT_5x7[0.2], 0.2, shared=True),
    'S3_all_empty_T0': lambda: random_case(27, (0, 0, 0), 1, (17, 23), 0, FOOT_1x1[0.2], 0.2),
}
ADVERSARIAL = {
    'boundaries': boundary_case, 'footprint_boundaries': footprint_boundary_case, 'nonfinite': nonfinite_case, 'overlap': overlap_case,
    'classes_empty': lambda: class_set_case(()), 'classes_full': lambda: class_set_case(range(256)), 'classes_0': lambda: class_set_case((0,)),
    'classes_255': lambda: class_set_case((255,)),
}
ALL = dict(SHAPES, **ADVERSARIAL)

_REFEREE = {}


def referee(name, case):
    """(hm [S,2,n,n], labels [sumN,C]) of the referee, computed once per case name."""
    if name not in _REFEREE:
        fx, fy = axes(case['robot_size'], case['grid_res'])
        hm, lab = ref.terrain_labels(case['points'], case['offsets'], case['seg'], case['rots'], case['trans'], case['intrins'], case['rigid_labels'],
                                     case['pose_align'], case['poses'], fx, fy, case['clearance'], bins_of(case), case['d_max'], case['h_max'],
                                     h_min=case['h_min'], r_min=case['r_min'])
        hm.setflags(write=False), lab.setflags(write=False)
        _REFEREE[name] = (hm, lab)
    return _REFEREE[name]


def api_args(case, device='cpu'):
    """(args, kwargs) of rigid_terrain_heightmap(_aten) for a case, its arrays as tensors on `device`."""
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(device) for k in ('points', 'seg', 'rots', 'trans', 'intrins', 'pose_align', 'poses')}
    args = (t['points'], t['seg'], t['rots'], t['trans'], t['intrins'], case['rigid_labels'], t['pose_align'], t['poses'], case['grid_res'], case['d_max'],
            case['h_max'])
    kwargs = dict(robot_size=case['robot_size'], clearance=case['clearance'], r_min=case['r_min'], h_min=case['h_min'],
                  offsets=[int(v) for v in case['offsets']], return_point_labels=True)
    return args, kwargs


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
