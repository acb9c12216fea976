"""The rigid-terrain label kernel (monoforce_amd/csrc/terrain_labels.hip) on the MI355X against the referee (tests/terrain_labels_reference.py)
as BIT PATTERNS, `hm` and `point_labels`, on small cases where it can still go wrong (tests/terrain_labels_cases.py), and against the golden
outputs of the reference pipeline."""
import os

import numpy as np
import pytest
import torch

from tests import terrain_labels_cases as cases
from tests.conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def labels():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from monoforce_amd import labels
    return labels


def run(labels, case, device='cuda'):
    args, kwargs = cases.api_args(case, device)
    hm, lab = labels.rigid_terrain_heightmap(*args, **kwargs)
    torch.cuda.synchronize()
    return hm, lab


@pytest.mark.parametrize('name', sorted(cases.ALL))
def test_kernel_equals_the_referee_bit_for_bit(labels, name):
    case = cases.ALL[name]()
    hm_ref, lab_ref = cases.referee(name, case)
    hm, lab = run(labels, case)
    assert hm.is_cuda and lab.is_cuda and hm.dtype == torch.float32 and lab.dtype == torch.int16
    assert cases.same_bits(lab.cpu().numpy(), lab_ref)
    assert cases.same_bits(hm.cpu().numpy(), hm_ref)


def test_contention_for_one_cell(labels):
    """50 000 items, every one seen with a rigid label, all landing in one cell with different heights: the cell holds the largest."""
    case = cases.contention_case()
    hm_ref, lab_ref = cases.referee('contention', case)
    assert hm_ref[0, 1].sum() == 1 and (lab_ref == 1).all() and lab_ref.shape[0] == 50_000
    hm, lab = run(labels, case)
    assert cases.same_bits(lab.cpu().numpy(), lab_ref) and cases.same_bits(hm.cpu().numpy(), hm_ref)
    again, _ = run(labels, case)
    assert torch.equal(hm, again)


def test_shared_cameras_equal_per_sample_copies(labels):
    case = cases.SHAPES['S3_ragged_C2_T1_n20_shared']()
    assert case['rots'].ndim == 3
    hm_shared, lab_shared = run(labels, case)
    copies = dict(case)
    for name in ('rots', 'trans', 'intrins'):
        copies[name] = np.broadcast_to(case[name], (3,) + case[name].shape).copy()
    hm_copies, lab_copies = run(labels, copies)
    hm_ref, lab_ref = cases.referee('S3_ragged_C2_T1_n20_shared', case)
    assert torch.equal(hm_shared, hm_copies) and torch.equal(lab_shared, lab_copies)
    assert cases.same_bits(hm_shared.cpu().numpy(), hm_ref) and cases.same_bits(lab_shared.cpu().numpy(), lab_ref)


def test_host_inputs_come_home(labels):
    """CPU tensors are copied over and the results come back on the host; GPU tensors stay; offsets may be a device tensor (the host then
    sizes the grid from the total); without the per-point labels only the map is returned; the single-sample form drops the leading S."""
    case = cases.SHAPES['S3_ragged_empty_C4_T7_n27']()
    hm_ref, lab_ref = cases.referee('S3_ragged_empty_C4_T7_n27', case)
    hm, lab = run(labels, case, device='cpu')
    assert not hm.is_cuda and not lab.is_cuda
    assert cases.same_bits(hm.numpy(), hm_ref) and cases.same_bits(lab.numpy(), lab_ref)
    args, kwargs = cases.api_args(case, 'cuda')
    only = labels.rigid_terrain_heightmap(*args, **dict(kwargs, return_point_labels=False, offsets=torch.tensor(kwargs['offsets'], device='cuda')))
    assert isinstance(only, torch.Tensor) and only.is_cuda and cases.same_bits(only.cpu().numpy(), hm_ref)
    pts, seg, rots, trans, intr, rigid, A, P = args[:8]
    one = labels.rigid_terrain_heightmap(pts[:257], seg[0], rots[0], trans[0], intr[0], rigid, A[0], P[0], *args[8:], robot_size=kwargs['robot_size'],
                                         clearance=kwargs['clearance'])
    assert one.shape == (2, 27, 27) and cases.same_bits(one.cpu().numpy(), hm_ref[0])
    sem_p, sem_l = labels.semantic_cloud(pts[:257], seg[0], rots[0], trans[0], intr[0])
    want = [lab_ref[:257, c][lab_ref[:257, c] >= 0] for c in range(4)]
    assert sem_p.is_cuda and np.array_equal(sem_l.cpu().numpy(), np.concatenate(want).astype(np.uint8)) and sem_p.shape == (sem_l.shape[0], 3)


def test_golden_case(labels):
    g = dict(np.load(os.path.join(REPO, 'tests', 'golden', 'terrain_labels.npz')))
    dev = 'cuda'
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ('points', 'seg', 'rots', 'trans', 'intrins', 'pose_align', 'poses')}
    hm, lab = labels.rigid_terrain_heightmap(t['points'], t['seg'], t['rots'], t['trans'], t['intrins'], g['rigid_labels'].tolist(), t['pose_align'], t['poses'],
                                             float(g['grid_res']), float(g['d_max']), float(g['h_max']), robot_size=(float(g['width']), float(g['length'])),
                                             clearance=float(g['clearance']), offsets=g['offsets'].tolist(), return_point_labels=True)
    hm, lab = hm.cpu().numpy(), lab.cpu().numpy()
    assert np.array_equal(lab, g['labels_ref'])
    assert np.array_equal(hm[:, 1], g['hm_ref'][:, 1])

    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i >= 0, i, -(i & 0x7FFFFFFF))
    worst = int(np.abs(key(hm[:, 0]) - key(g['hm_ref'][:, 0])).max())
    print('kernel vs reference pipeline: worst height difference', worst, 'ulp')
    assert worst <= 1
    aten = labels.rigid_terrain_heightmap_aten(t['points'], t['seg'], t['rots'], t['trans'], t['intrins'], g['rigid_labels'].tolist(), t['pose_align'],
                                               t['poses'], float(g['grid_res']), float(g['d_max']), float(g['h_max']),
                                               robot_size=(float(g['width']), float(g['length'])), clearance=float(g['clearance']), offsets=g['offsets'].tolist())
    assert aten.is_cuda and np.array_equal(aten[:, 1].cpu().numpy(), hm[:, 1])         # the ATen form on the GPU: the benchmark's yardstick
    assert int(np.abs(key(aten[:, 0].cpu().numpy()) - key(hm[:, 0])).max()) <= 1


def test_missing_library_is_an_error_not_a_fallback(labels, monkeypatch, tmp_path):
    from monoforce_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    case = cases.SHAPES['N1_C2_T0_n20']()
    args, kwargs = cases.api_args(case, 'cuda')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        labels.rigid_terrain_heightmap(*args, **kwargs)
