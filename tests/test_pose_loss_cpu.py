"""physics_loss(rotation_loss=True), translation_difference and slerp against the reference's own results (tests/golden/pose_loss.npz,
written by tests/golden/gen_golden_pose_loss.py), and the C ABI of the pose-loss kernels as far as it goes without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as hp

T2 = 7


@pytest.fixture(scope='module')
def golden():
    return hp.load('pose_loss')


def _t(g, tag, k):
    return torch.as_tensor(g[f'{tag}/{k}'])


@pytest.mark.parametrize('tag,tol_value,tol_grad', [('f64', 1e-12, 1e-12), ('f32', 1e-6, 1e-5)])
def test_aten_pose_loss_matches_the_reference(golden, tag, tol_value, tol_grad):
    """`physics_loss_aten(rotation_loss=True)` == the reference's physics_loss on off-SO(3) rotations with two stamps on one step."""
    from monoforce_amd.losses import nearest_steps, physics_loss_aten
    g = golden
    near = nearest_steps(_t(g, tag, 'pred_ts'), _t(g, tag, 'gt_ts'))
    assert any(len(set(row)) < T2 for row in near.tolist())
    X, R = _t(g, tag, 'X').requires_grad_(True), _t(g, tag, 'R').requires_grad_(True)
    loss, loss_rot = physics_loss_aten([X, None, R], [_t(g, tag, 'Xgt'), None, _t(g, tag, 'Rgt')], _t(g, tag, 'pred_ts'), _t(g, tag, 'gt_ts'),
                                       gamma=0.9, rotation_loss=True)
    (loss + loss_rot).backward()
    for got, key in ((loss, 'loss'), (loss_rot, 'loss_rot')):
        want = float(g[f'{tag}/{key}'])
        assert abs(float(got.detach()) - want) <= tol_value * abs(want), key
    assert hp.rel_err(X.grad, g[f'{tag}/g_X']) <= tol_grad and hp.rel_err(R.grad, g[f'{tag}/g_R']) <= tol_grad


@pytest.mark.parametrize('tag,tol', [('f64', 1e-12), ('f32', 1e-6)])
def test_translation_difference_and_slerp_match_the_reference(golden, tag, tol):
    from monoforce_amd.losses import rotation_difference, slerp, translation_difference
    g = golden
    for red in ('mean', 'sum', 'none'):
        td = translation_difference(_t(g, tag, 'X')[:, :T2], _t(g, tag, 'Xgt'), reduction=red)
        rd = rotation_difference(_t(g, tag, 'R')[:, :T2], _t(g, tag, 'Rgt'), reduction=red)
        assert td.shape == g[f'{tag}/td_{red}'].shape and rd.shape == g[f'{tag}/rd_{red}'].shape
        assert hp.rel_err(td, g[f'{tag}/td_{red}']) <= tol and hp.rel_err(rd, g[f'{tag}/rd_{red}']) <= tol
    for pair in ('near', 'far'):
        q1, q2 = _t(g, tag, 'q1_' + pair), _t(g, tag, 'q2_' + pair)
        assert (float((q1 * q2).sum()) > 0.9995) == (pair == 'near')
        q = slerp(q1, q2, _t(g, tag, 't'))
        assert q.shape == (5, 4) and hp.rel_err(q, g[f'{tag}/slerp_{pair}']) <= tol
    # the reference's argument checks
    with pytest.raises(AssertionError):
        translation_difference(torch.zeros(2, 3), torch.zeros(3, 3))
    with pytest.raises(AssertionError):
        translation_difference(torch.zeros(2, 2), torch.zeros(2, 2))
    with pytest.raises(AssertionError):
        slerp(torch.zeros(3), torch.zeros(3), torch.zeros(2))
    with pytest.raises(AssertionError):
        slerp(torch.zeros(4), torch.zeros(4), 0.5)


def test_monoforce_losses_exports_the_references_names():
    import monoforce.losses as m
    names = ['rotation_difference', 'translation_difference', 'total_variation', 'hm_loss', 'slerp', 'physics_loss']
    assert sorted(m.__all__) == sorted(names)
    from monoforce_amd import losses as L
    for n in names:
        assert getattr(m, n) is getattr(L, n) and n in L.__all__


def test_row_overlap_check_for_rotation_rows():
    from monoforce_amd.losses import _rows_do_not_overlap
    R = torch.zeros(5, 4, 3, 3)
    assert _rows_do_not_overlap(R, 9) and _rows_do_not_overlap(R.transpose(0, 1), 9)
    assert not _rows_do_not_overlap(R[:1].expand(5, -1, -1, -1), 9)
    assert not _rows_do_not_overlap(torch.zeros(5, 4, 6).as_strided((5, 4, 3, 3), (12, 3, 3, 1)), 9)      # rows 3 apart, 9 wide
    assert _rows_do_not_overlap(torch.zeros(5, 4, 3)) and not _rows_do_not_overlap(torch.zeros(1, 4, 3).expand(5, -1, -1))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import _lib
    return _lib


def test_pose_loss_desc_size_matches_the_ctypes_mirror(lib):
    assert lib.lib().mf_sizeof(b'MfPoseLossDesc') == C.sizeof(lib.MfPoseLossDesc) == 56


@pytest.mark.parametrize('sfx', ['f32', 'f64'])
def test_pose_loss_entry_points_refuse_bad_arguments_without_a_gpu(lib, sfx):
    """Null pointers, non-positive sizes and B * T2 >= 2^31 come back as MF_ERR_INVALID with a message; nothing is launched (the
    pointers handed over are not device memory)."""
    L = lib.lib()
    value, bwd = getattr(L, 'mf_pose_loss_value_' + sfx), getattr(L, 'mf_pose_loss_bwd_' + sfx)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    zero = C.c_longlong(0)

    def call_value(desc, ptrs, zx=(None, zero), zr=(None, zero)):
        return value(desc, *ptrs, zx[0], zx[1], zr[0], zr[1], None)

    def good():
        return lib.MfPoseLossDesc(B=2, T1=5, T2=3, x_stride_b=15, x_stride_t=3, r_stride_b=45, r_stride_t=9, gamma=0.9)
    INVALID = 1
    assert call_value(None, [p] * 9) == INVALID and b'null' in L.mf_last_error()
    for k in range(9):                                   # Xs, Rs, Xgt, Rgt, gt_ts, nearest, partial, ticket, loss
        ptrs = [p] * 9
        ptrs[k] = None
        assert call_value(C.byref(good()), ptrs) == INVALID and b'null' in L.mf_last_error(), k
    for field in ('B', 'T1', 'T2'):
        for bad in (0, -3):
            d = good()
            setattr(d, field, bad)
            assert call_value(C.byref(d), [p] * 9) == INVALID and b'positive' in L.mf_last_error()
            assert bwd(C.byref(d), *([p] * 7), p, p, None) == INVALID and b'positive' in L.mf_last_error()
    d = good()
    d.B, d.T2 = 1 << 20, 1 << 11
    assert call_value(C.byref(d), [p] * 9) == INVALID and b'2^31' in L.mf_last_error()
    assert bwd(C.byref(d), *([p] * 7), p, p, None) == INVALID and b'2^31' in L.mf_last_error()
    assert call_value(C.byref(good()), [p] * 9, zx=(None, C.c_longlong(8))) == INVALID and b'zero_x' in L.mf_last_error()
    assert call_value(C.byref(good()), [p] * 9, zr=(None, C.c_longlong(8))) == INVALID and b'zero_r' in L.mf_last_error()
    assert call_value(C.byref(good()), [p] * 9, zr=(p, C.c_longlong(-1))) == INVALID
    assert bwd(None, *([p] * 7), p, p, None) == INVALID
    for k in range(7):                                   # Xs, Rs, Xgt, Rgt, gt_ts, nearest, gloss
        ptrs = [p] * 7
        ptrs[k] = None
        assert bwd(C.byref(good()), *ptrs, p, p, None) == INVALID and b'null' in L.mf_last_error(), k
    assert bwd(C.byref(good()), *([p] * 7), None, None, None) == INVALID and b'neither' in L.mf_last_error()


def test_pose_loss_kernels_use_no_scratch(lib):
    """Four kernels (value / backward x float32 / float64), none with a private segment, LDS for the wave sums only."""
    import os
    import sys
    from tests.conftest import REPO
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_metadata
    rows = [(n, m) for o, n, m in kernel_metadata.kernels() if o == 'pose_loss.o']
    assert len(rows) == 4, rows
    for n, m in rows:
        assert m['scratch'] == 0 and m['lds'] <= 2 * 4 * 8 + 8, (n, m)
