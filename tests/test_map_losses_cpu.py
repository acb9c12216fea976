"""The height-map losses (`hm_loss`, `total_variation`; mf_hm_loss_* / mf_total_variation_*) as far as they go without a GPU: the C ABI
(exports, struct layout, argument validation, no scratch), the ATen forms that CPU tensors keep taking against the float64 referee, the
layout folding of the Python layer, the registered ops, and the one documented difference from autograd."""
import ctypes as C
import math

import pytest
import torch

from tests import map_losses_cases as mc

SYMBOLS = [f'mf_{k}_{d}_{s}' for k in ('hm_loss', 'total_variation') for d in ('value', 'bwd') for s in ('f32', 'f64')]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import _lib
    return _lib


def test_the_eight_entry_points_are_exported_and_listed(lib):
    assert len(SYMBOLS) == 8
    for name in SYMBOLS:
        assert name in lib.SYMBOLS and hasattr(lib.lib(), name), name
        assert getattr(lib.lib(), name).restype is C.c_int
    import os
    from tests.conftest import REPO
    header = open(os.path.join(REPO, 'include', 'monoforce_hip.h')).read()
    for name in SYMBOLS:
        assert name + '(' in header
    # every declaration cites the reference lines it replaces
    assert 'losses.py:77-99' in header and 'losses.py:68-74' in header


def test_map_loss_desc_size_matches_the_ctypes_mirror(lib):
    assert lib.lib().mf_sizeof(b'MfMapLossDesc') == C.sizeof(lib.MfMapLossDesc) == 88
    assert lib.MfMapLossDesc.p_stride_m.offset == 16 and lib.MfMapLossDesc.o_stride_h.offset == 72 and lib.MfMapLossDesc.h_max.offset == 80


@pytest.mark.parametrize('sfx', ['f32', 'f64'])
def test_map_loss_entry_points_refuse_bad_arguments_without_a_gpu(lib, sfx):
    """Null pointers, non-positive sizes and M * H * W >= 2^31 come back as MF_ERR_INVALID with a message; nothing is launched (the pointers
    handed over are not device memory)."""
    L = lib.lib()
    hm_value, hm_bwd = getattr(L, 'mf_hm_loss_value_' + sfx), getattr(L, 'mf_hm_loss_bwd_' + sfx)
    tv_value, tv_bwd = getattr(L, 'mf_total_variation_value_' + sfx), getattr(L, 'mf_total_variation_bwd_' + sfx)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    INVALID = 1

    def good():
        return lib.MfMapLossDesc(M=2, H=3, W=4, p_stride_m=12, p_stride_h=4, g_stride_m=12, g_stride_h=4, w_stride_m=12, w_stride_h=4,
                                 o_stride_m=12, o_stride_h=4)
    # (pointer arguments after the descriptor; which of them may be NULL)
    entries = {'hm_loss_value': (hm_value, 8, {2}), 'hm_loss_bwd': (hm_bwd, 6, {2}), 'total_variation_value': (tv_value, 4, set()),
               'total_variation_bwd': (tv_bwd, 3, set())}
    for name, (fn, n, optional) in entries.items():
        assert fn(None, *([p] * n), None) == INVALID and b'null descriptor' in L.mf_last_error() and name.encode() in L.mf_last_error()
        for k in range(n):
            if k in optional:
                continue
            ptrs = [p] * n
            ptrs[k] = None
            assert fn(C.byref(good()), *ptrs, None) == INVALID and b'null argument' in L.mf_last_error(), (name, k)
        for field in ('M', 'H', 'W'):
            for bad in (0, -3):
                d = good()
                setattr(d, field, bad)
                assert fn(C.byref(d), *([p] * n), None) == INVALID and b'positive' in L.mf_last_error(), (name, field)
        for M, H, W in ((1 << 11, 1 << 10, 1 << 10), (1, 1 << 16, 1 << 15), (3, 46341, 46341)):
            d = good()
            d.M, d.H, d.W = M, H, W
            assert fn(C.byref(d), *([p] * n), None) == INVALID and b'2^31' in L.mf_last_error(), (name, M, H, W)


def test_map_loss_kernels_use_no_scratch(lib):
    """Eight kernels (hm_loss / total variation x value / backward x float32 / float64), none with a private segment, LDS for the wave
    sums only."""
    import os
    import sys
    from tests.conftest import REPO
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_metadata
    rows = [(n, m) for o, n, m in kernel_metadata.kernels() if o == 'map_losses.o']
    assert len(rows) == 8, rows
    for n, m in rows:
        assert m['scratch'] == 0 and m['lds'] <= 4 * 8 + 4 * 4 + 8, (n, m)


def test_aten_forms_exist_and_cpu_tensors_take_them(monkeypatch):
    from monoforce_amd import losses as L
    assert L._HIP_MAP_LOSS is True and callable(L.hm_loss_aten) and callable(L.total_variation_aten)
    assert 'hm_loss_aten' in L.__all__ and 'total_variation_aten' in L.__all__
    calls = []
    hm_aten, tv_aten = L.hm_loss_aten, L.total_variation_aten
    monkeypatch.setattr(L, 'hm_loss_aten', lambda *a, **k: (calls.append('hm'), hm_aten(*a, **k))[1])
    monkeypatch.setattr(L, 'total_variation_aten', lambda *a, **k: (calls.append('tv'), tv_aten(*a, **k))[1])
    p, g, w = mc.hm_inputs((3, 7, 13), torch.float32, 0)
    L.hm_loss(p, g, w)
    L.total_variation(p)
    assert calls == ['hm', 'tv']
    assert not L._hm_loss_takes_the_hip_route(p, g, w, None) and not L._map_dtype_ok(p)


@pytest.mark.parametrize('dtype,bar', [(torch.float64, mc.F64_BAR), (torch.float32, 2e-6)])
@pytest.mark.parametrize('shape', mc.SHAPES[:7], ids=mc.ids)
def test_cpu_hm_loss_equals_the_referee(shape, dtype, bar):
    """CPU tensors: `hm_loss` (the ATen form, a masked sum instead of the reference's boolean indexing) against the float64 referee on the
    same inputs, value and gradient, every NaN placement, with and without weights and `h_max`.  float32 bar 2e-6: a sum of up to 3855
    float32 squares (pairwise summation: a few ulps of 6e-8) and one tanh."""
    from monoforce_amd.losses import hm_loss
    for nan_mode in mc.NAN_MODES:
        for weighted in (True, False):
            for h_max in (None, 1.0):
                p, g, w = mc.hm_inputs(shape, dtype, 7, nan_mode, weighted=weighted)
                want, gwant, n_valid, pred_nan = mc.hm_loss_referee(p, g, w, h_max, upstream=3.0)
                pl = p.clone().requires_grad_(True)
                loss = hm_loss(pl, g, w, h_max=h_max)
                (3.0 * loss).backward()
                assert loss.dtype == dtype and loss.shape == ()
                exclude = pred_nan if h_max is not None else None
                assert mc.rel(loss.detach(), want) <= bar and mc.grad_err(pl.grad, gwant, exclude) <= bar, (nan_mode, weighted, h_max)
                assert n_valid >= 1 and (nan_mode == 'none' or p.numel() == 1 or n_valid < p.numel())


def test_nan_prediction_under_h_max_is_the_one_difference_from_autograd():
    """The documented difference, on the CPU: with `h_max` set autograd's gradient at a NaN PREDICTION is NaN (tanh's backward,
    0 * (1 - NaN^2)), in the referee and in the ATen form alike -- the kernels store 0 there (tests/test_map_losses_gpu.py).  Without
    `h_max` both are 0; a NaN LABEL never produces a NaN gradient; with every cell masked the value is NaN and the gradient all zeros."""
    from monoforce_amd.losses import hm_loss
    p, g, w = mc.hm_inputs((3, 7, 13), torch.float64, 3, 'both')
    only_pred = torch.isnan(p)
    assert int(only_pred.sum()) > 0 and int((torch.isnan(g) & ~only_pred).sum()) > 0
    for fn in ('referee', 'aten'):
        for h_max in (1.0, None):
            if fn == 'referee':
                grad = mc.hm_loss_referee(p, g, w, h_max)[1]
            else:
                pl = p.clone().requires_grad_(True)
                hm_loss(pl, g, w, h_max=h_max).backward()
                grad = pl.grad
            if h_max is not None:
                assert torch.isnan(grad[only_pred]).all() and torch.isfinite(grad[~only_pred]).all(), fn
            else:
                assert torch.isfinite(grad).all() and float(grad[only_pred].abs().max()) == 0.0, fn
            assert float(grad[torch.isnan(g) & ~only_pred].abs().max()) == 0.0
    nan = torch.full_like(g, float('nan'))
    loss, grad, n_valid, _ = mc.hm_loss_referee(torch.ones_like(g), nan, w)
    assert math.isnan(float(loss)) and n_valid == 0 and float(grad.abs().max()) == 0.0
    pl = torch.ones_like(g).requires_grad_(True)
    loss = hm_loss(pl, nan, w)
    loss.backward()
    assert math.isnan(float(loss.detach())) and float(pl.grad.abs().max()) == 0.0


@pytest.mark.parametrize('dtype,bar', [(torch.float64, mc.F64_BAR), (torch.float32, 2e-6)])
@pytest.mark.parametrize('shape', mc.SHAPES[:7], ids=mc.ids)
def test_cpu_total_variation_equals_the_referee(shape, dtype, bar):
    from monoforce_amd.losses import total_variation
    z = mc.tv_inputs(shape, dtype, 5)
    want, gwant = mc.total_variation_referee(z, upstream=3.0)
    zl = z.clone().requires_grad_(True)
    loss = total_variation(zl)
    (3.0 * loss).backward()
    assert mc.rel(loss.detach(), want) <= bar and mc.grad_err(zl.grad, gwant) <= bar
    flat = torch.full(shape, 0.37, dtype=dtype).requires_grad_(True)
    loss = total_variation(flat)
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(flat.grad.abs().max()) == 0.0
    if len(shape) == 3:          # M maps at different constants: no difference crosses a map boundary
        steps = (torch.arange(shape[0], dtype=dtype)[:, None, None] * 1.5).expand(shape).contiguous()
        assert float(total_variation(steps)) == 0.0 == float(mc.total_variation_referee(steps)[0])


def test_map_strides_folds_channel_views_and_crops_without_a_copy():
    """The layout rule of the Python layer, on the host: `[:, k:k+1]` and `[:, k]` views of a [B,2,H,W] tensor, a row-strided crop and an
    [H,W] map come back as they are with (stride_m, stride_h); a W-strided view and leading axes that do not fold are copied once."""
    from monoforce_amd.losses import map_strides
    t = torch.arange(3 * 2 * 6 * 8, dtype=torch.float32).view(3, 2, 6, 8)
    for view, want in ((t[:, 0:1], (96, 8)), (t[:, 1:2], (96, 8)), (t[:, 0], (96, 8)), (t[:, 1], (96, 8)), (t, (48, 8)),
                       (t[..., 2:-2, 1:-1], (48, 8)), (t[:, 1, 2:-2, 1:-1], (96, 8)), (t[0, 0], (0, 8)), (t[:1, :, :, :1], (48, 8))):
        got, sm, sh = map_strides(view)
        assert got is view and (sm, sh) == want, (view.shape, view.stride(), sm, sh)
        # ... and the addressing the kernels use reaches exactly the view's elements
        H, W = view.shape[-2:]
        M = view.numel() // (H * W)
        idx = (torch.arange(M)[:, None, None] * sm + torch.arange(H)[None, :, None] * sh + torch.arange(W)[None, None, :]).flatten()
        base = t.flatten()[view.storage_offset():]
        assert torch.equal(base[idx], view.reshape(-1))
    for view in (t[..., ::2], t[:, :, ::2].transpose(0, 1), t.transpose(0, 1), t.transpose(2, 3)):
        got, sm, sh = map_strides(view)
        assert got is not view and got.is_contiguous() and torch.equal(got, view)
        assert (sm, sh) == ((got.shape[-2] * got.shape[-1]) if got.numel() > got.shape[-2] * got.shape[-1] else 0, got.shape[-1])


def test_the_ops_are_registered_with_fake_implementations():
    from monoforce_amd import ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert torch.ops.monoforce.hm_loss.default._schema.returns[0].type.kind() == 'TensorType'
    assert len(torch.ops.monoforce.hm_loss.default._schema.returns) == 2 and len(torch.ops.monoforce.total_variation.default._schema.returns) == 1
    with FakeTensorMode():
        p = torch.empty(4, 1, 16, 16)
        loss, n_valid = torch.ops.monoforce.hm_loss(p, p, None, 1.0)
        tv = torch.ops.monoforce.total_variation(p)
    assert loss.shape == () and n_valid.shape == (1,) and n_valid.dtype == torch.int32 and tv.shape == () and tv.dtype == torch.float32
    # the ops delegate to losses.py and name no entry point themselves (tests/test_capi_cpu.py holds the whole tree to that)
    import ast
    import inspect
    names = {n.value for n in ast.walk(ast.parse(inspect.getsource(ops))) if isinstance(n, ast.Constant) and isinstance(n.value, str)
             and n.value.startswith(('mf_hm_loss', 'mf_total_variation'))}
    assert not names


def test_fit_problem_takes_a_tv_weight():
    import inspect
    from monoforce_amd.train import TerrainFitProblem
    assert inspect.signature(TerrainFitProblem.__init__).parameters['tv_weight'].default == 0.0
