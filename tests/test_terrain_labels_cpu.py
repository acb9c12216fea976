"""Rigid-terrain label maps without a GPU: the referee (tests/terrain_labels_reference.py) and the ATen form against the golden outputs of the
reference pipeline (tests/golden/terrain_labels.npz, written by tests/golden/gen_golden_labels.py), the ATen form against the referee bit for
bit on the adversarial cases, the three `monoforce.cloudproc` helpers against the reference's own outputs, the import surface, the
descriptor's size and the argument errors."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import terrain_labels_cases as cases
from tests import terrain_labels_reference as ref
from tests.conftest import REPO


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(REPO, 'tests', 'golden', 'terrain_labels.npz')))


def ulp_distance(a, b):
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i >= 0, i, -(i & 0x7FFFFFFF))
    return np.abs(key(a) - key(b))


def golden_args(g, as_tensor=True):
    conv = (lambda a: torch.from_numpy(a)) if as_tensor else (lambda a: a)
    args = tuple(conv(g[k]) for k in ('points', 'seg', 'rots', 'trans', 'intrins')) + (tuple(g['rigid_labels'].tolist()),) + \
        (conv(g['pose_align']), conv(g['poses']), float(g['grid_res']), float(g['d_max']), float(g['h_max']))
    kwargs = dict(robot_size=(float(g['width']), float(g['length'])), clearance=float(g['clearance']), offsets=g['offsets'].tolist(), return_point_labels=True)
    return args, kwargs


def test_referee_matches_the_reference_pipeline(golden):
    g = golden
    fx, fy = cases.axes((float(g['width']), float(g['length'])), float(g['grid_res']))
    bins = torch.arange(-float(g['d_max']), float(g['d_max']), float(g['grid_res']), dtype=torch.float32).numpy()
    hm, lab = ref.terrain_labels(g['points'], g['offsets'], g['seg'], g['rots'], g['trans'], g['intrins'], g['rigid_labels'], g['pose_align'], g['poses'],
                                 fx, fy, g['clearance'], bins, float(g['d_max']), float(g['h_max']))
    assert g['hm_ref'][:, 1].sum() > 100 and (g['labels_ref'] >= 0).sum() > 100
    assert np.array_equal(lab, g['labels_ref'])
    assert np.array_equal(hm[:, 1], g['hm_ref'][:, 1])
    worst = int(ulp_distance(hm[:, 0], g['hm_ref'][:, 0]).max())
    print('referee vs reference: worst height difference', worst, 'ulp')
    assert worst <= 1


def test_aten_form_matches_the_reference_pipeline(golden):
    from monoforce_amd.labels import rigid_terrain_heightmap_aten
    args, kwargs = golden_args(golden)
    hm, lab = rigid_terrain_heightmap_aten(*args, **kwargs)
    assert hm.dtype == torch.float32 and lab.dtype == torch.int16 and not hm.requires_grad
    assert np.array_equal(lab.numpy(), golden['labels_ref'])
    assert np.array_equal(hm[:, 1].numpy(), golden['hm_ref'][:, 1])
    worst = int(ulp_distance(hm[:, 0].numpy(), golden['hm_ref'][:, 0]).max())
    print('ATen form vs reference: worst height difference', worst, 'ulp')
    assert worst <= 1


def test_intermediate_clouds_match_the_reference(golden):
    from monoforce_amd.labels import footprint_traj_points, semantic_cloud
    g = golden
    for s in range(g['seg'].shape[0]):
        sl = slice(int(g['offsets'][s]), int(g['offsets'][s + 1]))
        pts, lab = semantic_cloud(torch.from_numpy(g['points'][sl]), torch.from_numpy(g['seg'][s]), torch.from_numpy(g['rots'][s]),
                                  torch.from_numpy(g['trans'][s]), torch.from_numpy(g['intrins'][s]))
        want = slice(int(g['sem_offsets'][s]), int(g['sem_offsets'][s + 1]))
        assert lab.dtype == torch.uint8 and np.array_equal(lab.numpy(), g['sem_labels'][want])
        assert cases.same_bits(pts.numpy(), g['sem_points'][want])
        rigid = g['rigid_labels'].tolist()
        pts_r, lab_r = semantic_cloud(torch.from_numpy(g['points'][sl]), torch.from_numpy(g['seg'][s]), torch.from_numpy(g['rots'][s]),
                                      torch.from_numpy(g['trans'][s]), torch.from_numpy(g['intrins'][s]), labels=rigid)
        keep = np.isin(g['sem_labels'][want], rigid)
        assert np.array_equal(lab_r.numpy(), g['sem_labels'][want][keep]) and cases.same_bits(pts_r.numpy(), g['sem_points'][want][keep])
        poses = g['poses'][s].copy()
        foot = footprint_traj_points(poses, (float(g['width']), float(g['length'])), float(g['grid_res']), float(g['clearance']))
        assert isinstance(foot, np.ndarray) and foot.shape == g['foot_ref'][s].shape and np.array_equal(poses, g['poses'][s])
        # numpy's float64 product fixes no operation order: a few units of the last place of the coordinates' scale
        assert np.abs(foot - g['foot_ref'][s]).max() <= 4 * np.finfo(np.float64).eps * np.abs(g['foot_ref'][s]).max()
        foot_t = footprint_traj_points(torch.from_numpy(poses), (float(g['width']), float(g['length'])), float(g['grid_res']), float(g['clearance']))
        assert isinstance(foot_t, torch.Tensor) and np.array_equal(foot_t.numpy(), foot)


@pytest.mark.parametrize('name', sorted(cases.ALL))
def test_aten_form_equals_the_referee_bit_for_bit(name):
    from monoforce_amd.labels import rigid_terrain_heightmap_aten
    case = cases.ALL[name]()
    hm_ref, lab_ref = cases.referee(name, case)
    args, kwargs = cases.api_args(case)
    hm, lab = rigid_terrain_heightmap_aten(*args, **kwargs)
    assert cases.same_bits(lab.numpy(), lab_ref)
    assert cases.same_bits(hm.numpy(), hm_ref)


def test_cases_are_what_their_names_say():
    """The adversarial cases decide what they were built to decide (checked on the referee's output)."""
    fx, fy = cases.axes(cases.FOOT_5x7[0.2], 0.2)
    assert (fx.size, fy.size) == (5, 7) and tuple(a.size for a in cases.axes(cases.FOOT_5x7[0.15], 0.15)) == (5, 7)
    assert tuple(a.size for a in cases.axes(cases.FOOT_1x1[0.2], 0.2)) == (1, 1) and tuple(a.size for a in cases.axes(cases.FOOT_1x1[0.15], 0.15)) == (1, 1)
    assert cases.bins_of(cases.SHAPES['N255_C4_T7_foot5x7_n27']()).size == 27 and cases.bins_of(cases.SHAPES['N1_C2_T0_n20']()).size == 20
    case = cases.overlap_case()
    hm, lab = cases.referee('overlap', case)
    both = (lab[:, 0] == 0) & (lab[:, 1] == 1)
    assert both.sum() > 20 and ((lab[:, 0] >= 0) == (lab[:, 1] >= 0)).all() and hm[0, 1].sum() > 5      # seen soft by one, rigid by the other: kept
    case = cases.boundary_case()
    hm, lab = cases.referee('boundaries', case)
    n = lab.shape[0] // case['seg'].shape[0]
    rows, lab0 = case['points'][:n], lab[:n, 0]
    on_border = (rows[:, 0] == 1) | (rows[:, 0] == 22) | (rows[:, 1] == 1) | (rows[:, 1] == 16)
    assert (lab0[on_border & (rows[:, 2] == 1)] == -1).all()                       # u = 1, u = Wi-1, v = 1, v = Hi-1 are outside
    assert (lab0[(rows[:, 0] == 5) & (rows[:, 2] == 1) & (rows[:, 1] > 1) & (rows[:, 1] < 16)] == 0).all()           # u = 5.0 is pixel 5 (label 0) ...
    below = rows[:, 0] == np.nextafter(np.float32(5), np.float32(0))
    assert below.any() and (lab0[below & (rows[:, 1] > 1) & (rows[:, 1] < 16)] == 1).all()                           # ... one step below is pixel 4
    assert (lab0[rows[:, 2] == 0] == -1).all()                                     # w_2 = +-0
    got = hm[:, 1].sum(axis=(1, 2))
    assert got.tolist() == [0, 1, 0, 1, 1, 0, 1, 1, 0], got                        # on -d_max / +d_max: dropped; on an inner edge: the cell below it
    hm, _ = cases.referee('footprint_boundaries', cases.footprint_boundary_case())
    assert hm[0, 1].sum() == 7, hm[0, 1].sum()        # twelve poses: five on a bound (dropped), two sharing a cell
    hm, lab = cases.referee('nonfinite', cases.nonfinite_case())
    bad = ~np.isfinite(cases.nonfinite_case()['points']).all(axis=1)
    assert bad.sum() == 11 and (lab[bad] == -1).all() and (lab[~bad] >= 0).any()
    for name, count in (('classes_empty', 0), ('classes_full', None)):
        case = cases.ALL[name]()
        hm, lab = cases.referee(name, case)
        seen = int((lab >= 0).any(axis=1).sum())
        assert seen > 50 and {0, 1, 2, 255} <= set(np.unique(lab).tolist())
    assert cases.referee('classes_empty', cases.ALL['classes_empty']())[0][0, 1].sum() == 1            # the footprint's one point only
    sizes = [cases.referee(n, cases.ALL[n]())[0][0, 1].sum() for n in ('classes_empty', 'classes_0', 'classes_255', 'classes_full')]
    assert sizes[0] < sizes[1] < sizes[3] and sizes[0] < sizes[2] < sizes[3], sizes


def test_single_sample_form_and_shared_cameras():
    from monoforce_amd.labels import rigid_terrain_heightmap_aten
    case = cases.random_case(31, (300, 200), 2, (24, 32), 3, cases.FOOT_5x7[0.2], 0.2, shared=True)
    args, kwargs = cases.api_args(case)
    hm, lab = rigid_terrain_heightmap_aten(*args, **kwargs)
    pts, seg, rots, trans, intr, labels, A, P = args[:8]
    for s, sl in enumerate((slice(0, 300), slice(300, 500))):
        one = rigid_terrain_heightmap_aten(pts[sl], seg[s], rots, trans, intr, labels, A[s], P[s], *args[8:], robot_size=kwargs['robot_size'],
                                           clearance=kwargs['clearance'])
        assert one.shape == hm.shape[1:] and torch.equal(one, hm[s])
    # 4 x 4 poses, per-sample copies of the shared cameras, points as [S,N,3]
    A4, P4 = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1), torch.eye(4, dtype=torch.float64).repeat(2, 3, 1, 1)
    A4[:, :3], P4[:, :, :3] = A, P
    copies = [t[None].repeat(2, *([1] * t.dim())) for t in (rots, trans, intr)]
    hm2 = rigid_terrain_heightmap_aten(pts[:400].reshape(2, 200, 3), seg, *copies, labels, A4, P4, *args[8:], robot_size=kwargs['robot_size'],
                                       clearance=kwargs['clearance'])
    hm3 = rigid_terrain_heightmap_aten(pts[:400], seg, rots, trans, intr, labels, A, P, *args[8:], robot_size=kwargs['robot_size'],
                                       clearance=kwargs['clearance'], offsets=torch.tensor([0, 200, 400]))
    assert torch.equal(hm2, hm3)


def test_cloudproc_helpers_match_the_reference(golden):
    from monoforce.cloudproc import filter_grid, hm_to_cloud, within_bounds
    import monoforce.cloudproc as shim
    import monoforce_amd.cloudproc as cp
    assert set(cp.__all__) == {'filter_grid', 'estimate_heightmap', 'hm_to_cloud', 'within_bounds'} and all(hasattr(shim, n) for n in cp.__all__)
    g = golden
    xyz, res = g['fg_xyz'], float(g['fg_grid_res'])
    structured = np.zeros(xyz.shape[0], dtype=[('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('i', 'f4')])
    for k, name in enumerate('xyz'):
        structured[name] = xyz[:, k]
    structured['i'] = g['fg_intensity']
    for keep in ('first', 'last'):
        assert np.array_equal(filter_grid(xyz.copy(), res, keep=keep, only_mask=True), g[f'fg_plain_{keep}_ind'])
        assert cases.same_bits(filter_grid(xyz.copy(), res, keep=keep), g[f'fg_plain_{keep}_rows'])
        assert np.array_equal(filter_grid(structured.copy(), res, keep=keep, only_mask=True), g[f'fg_struct_{keep}_ind'])
        rows = filter_grid(structured.copy(), res, keep=keep)
        assert rows.dtype == structured.dtype and cases.same_bits(np.stack([rows[n] for n in ('x', 'y', 'z', 'i')], axis=1), g[f'fg_struct_{keep}_rows'])
        ind = filter_grid(torch.from_numpy(xyz.copy()), res, keep=keep, only_mask=True)          # the torch route: the same indices
        assert isinstance(ind, torch.Tensor) and np.array_equal(ind.numpy(), g[f'fg_plain_{keep}_ind'])
        assert cases.same_bits(filter_grid(torch.from_numpy(xyz.copy()), res, keep=keep).numpy(), g[f'fg_plain_{keep}_rows'])
    shuffled = xyz.copy()
    kept = filter_grid(shuffled, res, keep='random', rng=np.random.default_rng(1))
    assert kept.shape == g['fg_plain_first_rows'].shape and not np.array_equal(shuffled, xyz)     # (shuffles in place, like the reference)
    x = g['wb_x']
    assert np.array_equal(within_bounds(torch.from_numpy(x), min=-0.5, max=0.8).numpy(), g['wb_min_max'])
    assert np.array_equal(within_bounds(x, bounds=(-1.0, 0.2)).numpy(), g['wb_bounds'])
    assert np.array_equal(within_bounds(torch.from_numpy(x), max=0.0).numpy(), g['wb_max_only'])
    assert np.array_equal(within_bounds(torch.from_numpy(x), min=-float('inf'), max=float('inf')).numpy(), g['wb_inf']) and g['wb_inf'].all()
    cfg = types.SimpleNamespace(d_max=float(g['d_max']))
    h, m = g['hc_height'], g['hc_mask']
    assert cases.same_bits(hm_to_cloud(h, cfg), g['hc_numpy'])
    assert cases.same_bits(hm_to_cloud(h, cfg, mask=m.astype(np.float32)), g['hc_numpy_masked'])
    assert cases.same_bits(hm_to_cloud(torch.from_numpy(h), cfg).numpy(), g['hc_torch'])
    assert cases.same_bits(hm_to_cloud(torch.from_numpy(h), cfg, mask=torch.from_numpy(m)).numpy(), g['hc_torch_masked'])


def test_transformations_shim():
    from monoforce.transformations import position, transform_cloud
    rng = np.random.default_rng(0)
    Tr = np.eye(4)
    Tr[:3, :3], Tr[:3, 3] = cases.rot_z(0.4), [1.0, -2.0, 0.5]
    cloud = rng.standard_normal((9, 3)).astype(np.float32)
    out = transform_cloud(cloud, Tr)
    assert out.shape == (9, 3) and out.dtype == np.float64 and np.allclose(out, cloud @ Tr[:3, :3].T + Tr[:3, 3])
    out_t = transform_cloud(torch.from_numpy(cloud), torch.from_numpy(Tr).float())
    assert isinstance(out_t, torch.Tensor) and np.allclose(out_t.numpy(), out, atol=1e-5)
    structured = np.zeros(9, dtype=[('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('i', 'f4')])
    for k, name in enumerate('xyz'):
        structured[name] = cloud[:, k]
    structured['i'] = 7
    moved = transform_cloud(structured, Tr)
    assert moved.dtype == structured.dtype and np.allclose(position(moved), out, atol=1e-5) and (moved['i'] == 7).all() and structured['x'][0] == cloud[0, 0]
    with pytest.raises(ImportError):
        from monoforce.transformations import rpy2rot  # noqa: F401


def test_struct_size_and_top_level_names():
    import __graft_entry__ as g
    g.build()
    import monoforce_amd
    from monoforce_amd import _lib, labels
    L = _lib.lib()
    L.mf_sizeof.restype = ctypes.c_int
    L.mf_sizeof.argtypes = [ctypes.c_char_p]
    assert L.mf_sizeof(b'MfTerrainLabelsDesc') == ctypes.sizeof(_lib.MfTerrainLabelsDesc) == 128
    assert 'mf_terrain_labels_f32' in _lib.SYMBOLS and hasattr(L, 'mf_terrain_labels_f32')
    for name in ('rigid_terrain_heightmap', 'rigid_terrain_heightmap_aten', 'semantic_cloud', 'footprint_traj_points'):
        assert getattr(monoforce_amd, name) is getattr(labels, name)
    # the descriptor is validated before any launch (no device needed)
    d = _lib.MfTerrainLabelsDesc(S=0, n=4)
    assert L.mf_terrain_labels_f32(ctypes.byref(d), *([None] * 16)) == 1 and b'bad sizes' in L.mf_last_error()
    d = _lib.MfTerrainLabelsDesc(S=1, n=4, C=1, Hi=2, Wi=8)
    assert L.mf_terrain_labels_f32(ctypes.byref(d), *([None] * 16)) == 1 and b'3 x 3' in L.mf_last_error()
    d = _lib.MfTerrainLabelsDesc(S=1, n=4)
    assert L.mf_terrain_labels_f32(ctypes.byref(d), *([None] * 16)) == 1 and b'null argument' in L.mf_last_error()
    assert labels.class_set_words([0, 31, 32, 255]) == [0x80000001, 1, 0, 0, 0, 0, 0, 0x80000000]


def test_argument_errors():
    from monoforce_amd import labels
    case = cases.random_case(1, (10,), 2, (24, 32), 1, cases.FOOT_1x1[0.2], 0.2)
    args, kwargs = cases.api_args(case)
    pts, seg, rots, trans, intr, rigid, A, P = args[:8]
    for fn in (labels.rigid_terrain_heightmap, labels.rigid_terrain_heightmap_aten):
        def call(*a, **kw):
            return fn(*a, **dict(kwargs, **kw))
        with pytest.raises(ValueError, match='0..255'):
            call(pts, seg, rots, trans, intr, (256,), A, P, *args[8:])
        with pytest.raises(ValueError, match='0..255'):
            call(pts, seg, rots, trans, intr, (1.5,), A, P, *args[8:])
        with pytest.raises(ValueError, match='positive'):
            call(pts, seg, rots, trans, intr, rigid, A, P, 0.0, 2.0, 1.0)
    aten = labels.rigid_terrain_heightmap_aten
    with pytest.raises(ValueError, match='seg must be'):
        aten(pts, seg[0, 0], *args[2:], **kwargs)
    with pytest.raises(TypeError, match='integer labels'):
        aten(pts, seg.float(), *args[2:], **kwargs)
    with pytest.raises(ValueError, match='rots must be'):
        aten(pts, seg, rots[:, :1], *args[3:], **kwargs)
    with pytest.raises(ValueError, match='offsets must be'):
        aten(*args, **dict(kwargs, offsets=[0, 5]))
    with pytest.raises(ValueError, match='offsets must be'):
        aten(*args, **dict(kwargs, offsets=[0, 11]))
    with pytest.raises(ValueError, match='without offsets'):
        aten(*args, **dict(kwargs, offsets=None))
    with pytest.raises(ValueError, match='offsets belong to a batch'):
        aten(pts, seg[0], rots[0], trans[0], intr[0], rigid, A[0], P[0], *args[8:], offsets=[0, 10])
    with pytest.raises(ValueError, match='pose_align must be'):
        aten(pts, seg, rots, trans, intr, rigid, A[:, :2], P, *args[8:], **kwargs)
    with pytest.raises(ValueError, match='outside 0..255'):
        aten(pts, seg.long() + 300, *args[2:], **kwargs)
    # the launch's own checks come before any device is touched: CPU tensors get as far as the device check, and no further
    xb = torch.arange(-2.0, 2.0, 0.2)
    S, n = 1, xb.numel()
    good = dict(points=pts, offsets=torch.tensor([0, 10], dtype=torch.int32), seg=seg, rots=rots, trans=trans, intrins=intr, pose_align=A, poses=P,
                fx=torch.zeros(1), fy=torch.zeros(1), x_bins=xb, y_bins=xb, rigid_labels=rigid, clearance=0.0, d_max=2.0, h_min=-1.0, h_max=1.0, r_min=None,
                inv_res=5.0, scratch=torch.empty(S * n * n, dtype=torch.int32), hm=torch.empty(S, 2, n, n))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        labels.terrain_labels_into(**good)
    for key, bad, err, match in (('points', pts.double(), ValueError, 'points must be float32'), ('offsets', good['offsets'].long(), ValueError, 'offsets must be int32'),
                                 ('seg', seg.long(), ValueError, 'seg must be uint8'), ('pose_align', A.float(), ValueError, 'pose_align must be float64'),
                                 ('poses', P[0], ValueError, 'poses must be float64'), ('hm', torch.empty(S, 2, n, n + 1), ValueError, 'hm must be float32'),
                                 ('scratch', torch.empty(3, dtype=torch.int32), ValueError, 'scratch must hold'),
                                 ('y_bins', xb[:-1], ValueError, 'same, positive length'), ('point_labels', torch.empty(10, 2, dtype=torch.int32), ValueError, 'point_labels must be int16'),
                                 ('max_points', 11, ValueError, 'max_points'), ('points', pts.t().contiguous().t(), ValueError, 'contiguous'),
                                 ('rigid_labels', (-1,), ValueError, '0..255')):
        with pytest.raises(err, match=match):
            labels.terrain_labels_into(**dict(good, **{key: bad}))
