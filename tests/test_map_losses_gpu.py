"""The height-map losses on the MI355X (mf_hm_loss_* / mf_total_variation_*: one value launch, one backward launch each) against the float64
referee of tests/map_losses_cases.py: values, gradients, NaN masking, strided views, determinism, capture, the shared ticket, the fit step's
`tv_weight` and the encoder train step.

Bars.  float64: 1e-11 relative on values, max-norm relative on gradients.  float32: for every case the error e32 of the ATen float32 form
(`hm_loss_aten` / `total_variation_aten`, on the GPU, same inputs) against the referee is measured, and the kernels are held to
max(1e-6, 2 e32).  Both errors are printed per case (lines starting with `map-loss-error`)."""
import math

import pytest
import torch

from tests import map_losses_cases as mc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float32, torch.float64]


def _bar(dtype, aten_err):
    return mc.F64_BAR if dtype == torch.float64 else max(mc.F32_FLOOR, 2 * aten_err)


def _report(what, shape, dtype, detail, errs, aten, bars):
    print('map-loss-error %-6s %-12s %-7s %-34s value hip %.3g aten %.3g bar %.3g | gradient hip %.3g aten %.3g bar %.3g'
          % (what, mc.ids(shape), str(dtype).replace('torch.', ''), detail, errs[0], aten[0], bars[0], errs[1], aten[1], bars[1]))


def _spy_on_copies(monkeypatch, L):
    """The list that receives the shape of every tensor `losses.map_strides` had to copy (`.contiguous()`) from now on."""
    copies, inner = [], L.map_strides

    def spy(t):
        out = inner(t)
        if out[0] is not t:
            copies.append(tuple(t.shape))
        return out
    monkeypatch.setattr(L, 'map_strides', spy)
    return copies


def _hm_run(fn, p, g, w, h_max, upstream=3.0):
    pl = p.detach().clone().requires_grad_(True)
    loss = fn(pl, g, w, h_max=h_max)
    (grad,) = torch.autograd.grad(upstream * loss, pl)
    return loss.detach(), grad, loss


def _tv_run(fn, z, upstream=3.0):
    zl = z.detach().clone().requires_grad_(True)
    loss = fn(zl)
    (grad,) = torch.autograd.grad(upstream * loss, zl)
    return loss.detach(), grad, loss


# ---- 1: hm_loss, every shape, NaN placement, weights and h_max ------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', mc.SHAPES, ids=mc.ids)
def test_hm_loss_equals_the_referee(shape, dtype):
    from monoforce_amd import losses as L
    from monoforce_amd import ops  # noqa: F401
    for nan_mode in mc.NAN_MODES:
        for weighted in (True, False):
            for h_max in (None, 1.0):
                p, g, w = (None if t is None else t.to(DEV) for t in mc.hm_inputs(shape, dtype, 11, nan_mode, weighted=weighted))
                want, gwant, n_valid, pred_nan = mc.hm_loss_referee(p, g, w, h_max, upstream=3.0)
                assert math.isfinite(float(want)) and n_valid >= 1
                exclude = pred_nan if h_max is not None else None        # the one documented difference: autograd's NaN, the kernel's 0
                loss, grad, out = _hm_run(L.hm_loss, p, g, w, h_max)
                assert type(out.grad_fn).__name__.startswith('_FusedHmLoss') and loss.dtype == dtype and loss.shape == () and grad.shape == p.shape
                a_loss, a_grad, a_out = _hm_run(L.hm_loss_aten, p, g, w, h_max)
                assert not type(a_out.grad_fn).__name__.startswith('_FusedHmLoss')
                errs = (mc.rel(loss, want), mc.grad_err(grad, gwant, exclude))
                aten = (mc.rel(a_loss, want), mc.grad_err(a_grad, gwant, exclude))
                bars = (_bar(dtype, aten[0]), _bar(dtype, aten[1]))
                _report('hm', shape, dtype, f'nan={nan_mode} w={int(weighted)} h_max={h_max}', errs, aten, bars)
                assert errs[0] <= bars[0] and errs[1] <= bars[1], (nan_mode, weighted, h_max, errs, bars)
                assert torch.isfinite(grad).all()
                if exclude is not None and bool(exclude.any()):
                    assert float(grad[exclude.to(DEV)].abs().max()) == 0.0
                # masked cells of either kind carry an exactly zero gradient
                masked = (torch.isnan(p) | torch.isnan(g))
                assert not bool(masked.any()) or float(grad[masked].abs().max()) == 0.0
                # the count is exact, and two calls are bit-equal
                l_op, n_op = torch.ops.monoforce.hm_loss(p, g, w, h_max)
                assert int(n_op) == n_valid and n_op.dtype == torch.int32
                loss2, grad2, _ = _hm_run(L.hm_loss, p, g, w, h_max)
                assert torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(l_op, loss)


@pytest.mark.parametrize('dtype', DTYPES)
def test_hm_loss_with_every_cell_masked(dtype):
    from monoforce_amd import losses as L
    for shape in ((1, 1), (3, 7, 13), (1, 256, 256)):
        p, g, w = (t.to(DEV) for t in mc.hm_inputs(shape, dtype, 2))
        for h_max in (None, 1.0):
            for nan_p, nan_g in ((False, True), (True, False), (True, True)):
                pp = torch.full_like(p, float('nan')) if nan_p else p
                gg = torch.full_like(g, float('nan')) if nan_g else g
                loss, grad, out = _hm_run(L.hm_loss, pp, gg, w, h_max)
                assert type(out.grad_fn).__name__.startswith('_FusedHmLoss')
                assert math.isnan(float(loss)) and float(grad.abs().max()) == 0.0
                assert int(torch.ops.monoforce.hm_loss(pp, gg, w, h_max)[1]) == 0


# ---- 2: views -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_hm_loss_reads_channel_views_and_crops_in_place(dtype, monkeypatch):
    """Labels as `[:, 0:1]` / `[:, 1:2]` and `[:, 0]` / `[:, 1]` views of a [B,2,H,W] tensor, a prediction that is a `[:, 0]` view, row-strided
    crops of all three: no `.contiguous()` is called and the numbers are the referee's; a W-strided view gives the same numbers through the
    one fallback copy.  The gradient arrives at the base tensor, in the view's cells only."""
    from monoforce_amd import losses as L
    B, H, W = 3, 21, 37
    p0, g0, w0 = mc.hm_inputs((B, H, W), dtype, 5, 'both')
    labels = torch.stack([g0, w0], dim=1).to(DEV)                      # [B,2,H,W]: value, weight (scripts/train.py:390)
    heads = torch.stack([p0, 0.1 * p0, p0 + 1], dim=1).to(DEV)         # the prediction is channel 0 of a [B,3,H,W] tensor
    copies = _spy_on_copies(monkeypatch, L)

    def check(pred_of, gt, w, what, n_copies):
        base = heads.clone().requires_grad_(True)
        pred = pred_of(base)
        del copies[:]
        loss = L.hm_loss(pred, gt, w, h_max=1.0)
        assert type(loss.grad_fn).__name__.startswith('_FusedHmLoss') and len(copies) == n_copies, (what, copies)
        (3.0 * loss).backward()
        want, gwant, n_valid, pred_nan = mc.hm_loss_referee(pred, gt, w, 1.0, upstream=3.0)
        a_loss, a_grad, _ = _hm_run(L.hm_loss_aten, pred.detach(), gt, w, 1.0)
        (gpred,) = torch.autograd.grad(pred_of(base), base, torch.ones_like(pred))      # 1 in the view's cells of the base tensor
        got = pred_of(base.grad)
        assert float((base.grad * (1 - gpred)).abs().max()) == 0.0                       # nothing outside the view
        errs = (mc.rel(loss.detach(), want), mc.grad_err(got, gwant, pred_nan))
        aten = (mc.rel(a_loss, want), mc.grad_err(a_grad, gwant, pred_nan))
        bars = (_bar(dtype, aten[0]), _bar(dtype, aten[1]))
        _report('hm', tuple(pred.shape), dtype, what, errs, aten, bars)
        assert errs[0] <= bars[0] and errs[1] <= bars[1] and float(got[pred_nan.to(DEV)].abs().max()) == 0.0, (what, errs, bars)
        return float(loss.detach())

    a = check(lambda t: t[:, 0:1], labels[:, 0:1], labels[:, 1:2], 'labels [:,0:1] / [:,1:2]', 0)
    b = check(lambda t: t[:, 0], labels[:, 0], labels[:, 1], 'labels [:,0] / [:,1], pred [:,0]', 0)
    assert a == b
    check(lambda t: t[:, 0], labels[:, 0], None, 'pred [:,0], weights=None', 0)
    check(lambda t: t[:, 0, 2:-2, 1:-1], labels[:, 0, 2:-2, 1:-1], labels[:, 1, 2:-2, 1:-1], 'crops [..., 2:-2, 1:-1]', 0)
    check(lambda t: t[..., 2:-2, 1:-1][:, 0:1], labels[..., 2:-2, 1:-1][:, 0:1], labels[..., 2:-2, 1:-1][:, 1:2], 'crops of [:,k:k+1]', 0)
    c = check(lambda t: t[:, 0, :, ::2], labels[:, 0, :, ::2], labels[:, 1, :, ::2], 'W-strided [..., ::2]', 3)
    d = check(lambda t: t[:, 0, :, ::2], labels[:, 0, :, ::2].contiguous(), labels[:, 1, :, ::2].contiguous(), 'W-strided pred, dense labels', 1)
    assert c == d


def test_backward_kernels_store_every_cell_of_a_strided_gradient_buffer():
    """`g_pred` / `g_z` need not be zero on entry and have their own strides: a `[:, 0]` channel of a buffer filled with 7 receives the
    gradient in every cell, masked ones included, and the other channel keeps its 7s."""
    from monoforce_amd import losses as L
    B, H, W = 3, 21, 37
    p, g, w = (t.to(DEV) for t in mc.hm_inputs((B, H, W), torch.float32, 9, 'both'))
    one = torch.ones(1, device=DEV)
    loss, n_valid, state = L.hm_loss_forward(p, g, w, 1.0)
    buf = torch.full((B, 2, H, W), 7.0, device=DEV)
    L.hm_loss_backward(*state, n_valid, one, buf[:, 0])
    assert torch.equal(buf[:, 0], L.hm_loss_grad(state, n_valid, one, p.shape)) and float((buf[:, 1] - 7).abs().max()) == 0.0
    assert float(buf[:, 0][torch.isnan(p) | torch.isnan(g)].abs().max()) == 0.0
    z = mc.tv_inputs((B, H, W), torch.float32, 9).to(DEV)
    loss, state = L.total_variation_forward(z)
    buf = torch.full((B, 2, H + 4, W + 2), 7.0, device=DEV)
    L.total_variation_backward(*state, one, buf[:, 1, 2:-2, 1:-1])
    assert torch.equal(buf[:, 1, 2:-2, 1:-1], L.total_variation_grad(state, one, z.shape))
    buf[:, 1, 2:-2, 1:-1] = 7.0
    assert float((buf - 7).abs().max()) == 0.0


# ---- 3: total variation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', mc.SHAPES, ids=mc.ids)
def test_total_variation_equals_the_referee(shape, dtype):
    from monoforce_amd import losses as L
    from monoforce_amd import ops  # noqa: F401
    for ties in (True, False):
        z = mc.tv_inputs(shape, dtype, 13, ties=ties).to(DEV)
        if ties and z.numel() > 64:
            d = z[..., :, 1:] - z[..., :, :-1]
            assert 0 < int((d == 0).sum()) < d.numel()                  # equal neighbours in places: sign(0) matters
        want, gwant = mc.total_variation_referee(z, upstream=3.0)
        loss, grad, out = _tv_run(L.total_variation, z)                 # a non-ones upstream gradient: (3 * loss).backward()
        assert type(out.grad_fn).__name__.startswith('_FusedTotalVariation') and loss.dtype == dtype and grad.shape == z.shape
        a_loss, a_grad, _ = _tv_run(L.total_variation_aten, z)
        errs = (mc.rel(loss, want), mc.grad_err(grad, gwant))
        aten = (mc.rel(a_loss, want), mc.grad_err(a_grad, gwant))
        bars = (_bar(dtype, aten[0]), _bar(dtype, aten[1]))
        _report('tv', shape, dtype, f'ties={int(ties)}', errs, aten, bars)
        assert errs[0] <= bars[0] and errs[1] <= bars[1], (ties, errs, bars)
        loss2, grad2, _ = _tv_run(L.total_variation, z)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2)    # deterministic
        zl = z.clone().requires_grad_(True)
        l_op = torch.ops.monoforce.total_variation(zl)
        (g_op,) = torch.autograd.grad(3.0 * l_op, zl)
        assert torch.equal(l_op.detach(), loss) and torch.equal(g_op, grad)
    # an exactly flat map -- where the terrain fit starts -- has value 0 and an all-zero gradient
    loss, grad, _ = _tv_run(L.total_variation, torch.full(shape, 0.37, dtype=dtype, device=DEV))
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize('dtype', DTYPES)
def test_total_variation_stays_inside_each_map_and_reads_views_in_place(dtype, monkeypatch):
    from monoforce_amd import losses as L
    # M = 3 maps at different constants: a difference across a map boundary would show
    for shape in ((3, 7, 13), (3, 1, 64, 64), (3, 257, 5)):
        steps = (torch.arange(3, dtype=dtype, device=DEV).view(3, *([1] * (len(shape) - 1))) * 1.5 + 0.25).expand(shape).contiguous()
        loss, grad, _ = _tv_run(L.total_variation, steps)
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    # the divisor is H * W whatever M is: M copies of one map give M times its value
    z = mc.tv_inputs((21, 37), dtype, 3).to(DEV)
    one, four = _tv_run(L.total_variation, z)[0], _tv_run(L.total_variation, z.expand(4, 21, 37).contiguous())[0]
    assert mc.rel(four, 4 * float(one)) <= _bar(dtype, 0.0)
    # a [:, 0] view, a row-strided crop (no copy), a W-strided view (one copy)
    base = mc.tv_inputs((3, 2, 25, 39), dtype, 4).to(DEV)
    copies = _spy_on_copies(monkeypatch, L)
    for view_of, what, n_copies in ((lambda t: t[:, 0], '[:, 0]', 0), (lambda t: t[..., 2:-2, 1:-1], 'crop [..., 2:-2, 1:-1]', 0),
                                    (lambda t: t[:, 1, 2:-2, 1:-1], 'crop of [:, 1]', 0), (lambda t: t[..., ::2], 'W-strided [..., ::2]', 1)):
        bl = base.clone().requires_grad_(True)
        del copies[:]
        loss = L.total_variation(view_of(bl))
        assert type(loss.grad_fn).__name__.startswith('_FusedTotalVariation') and len(copies) == n_copies, (what, copies)
        (3.0 * loss).backward()
        want, gwant = mc.total_variation_referee(view_of(base), upstream=3.0)
        a_loss, a_grad, _ = _tv_run(L.total_variation_aten, view_of(base))
        (inside,) = torch.autograd.grad(view_of(bl), bl, torch.ones_like(view_of(bl)))
        assert float((bl.grad * (1 - inside)).abs().max()) == 0.0
        errs = (mc.rel(loss.detach(), want), mc.grad_err(view_of(bl.grad), gwant))
        aten = (mc.rel(a_loss, want), mc.grad_err(a_grad, gwant))
        bars = (_bar(dtype, aten[0]), _bar(dtype, aten[1]))
        _report('tv', tuple(view_of(base).shape), dtype, what, errs, aten, bars)
        assert errs[0] <= bars[0] and errs[1] <= bars[1], (what, errs, bars)


# ---- 4: which calls take the HIP route ------------------------------------------------------------------------------------------------------
def test_public_losses_route_and_decline(monkeypatch):
    from monoforce.losses import hm_loss, total_variation
    from monoforce_amd import losses as L
    p, g, w = (t.to(DEV) for t in mc.hm_inputs((2, 1, 16, 16), torch.float32, 1, 'gt'))
    hm_aten, tv_aten = L.hm_loss_aten, L.total_variation_aten
    with monkeypatch.context() as m:
        m.setattr(L, 'hm_loss_aten', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the ATen form was called')))
        m.setattr(L, 'total_variation_aten', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the ATen form was called')))
        pl = p.clone().requires_grad_(True)
        assert type(hm_loss(pl, g, w).grad_fn).__name__.startswith('_FusedHmLoss')
        assert type(total_variation(pl).grad_fn).__name__.startswith('_FusedTotalVariation')
        with torch.no_grad():
            assert float(hm_loss(p, g, w)) == float(hm_loss(pl, g, w).detach()) and float(total_variation(p)) == float(total_variation(pl).detach())
    calls = []
    monkeypatch.setattr(L, 'hm_loss_aten', lambda *a, **k: (calls.append('hm'), hm_aten(*a, **k))[1])
    monkeypatch.setattr(L, 'total_variation_aten', lambda *a, **k: (calls.append('tv'), tv_aten(*a, **k))[1])
    declined = {'labels want a gradient': (p, g.clone().requires_grad_(True), w, None), 'weights want a gradient': (p, g, w.clone().requires_grad_(True), None),
                'half precision': (p.half(), g.half(), w.half(), None), 'mixed dtypes': (p, g.double(), w, None),
                'h_max on the device': (p, g, w, torch.tensor(1.0, device=DEV)), 'labels on the host': (p, g.cpu(), None, None)}
    for name, (pp, gg, ww, h_max) in declined.items():
        n = len(calls)
        try:
            hm_loss(pp.clone().requires_grad_(True), gg, ww, h_max=h_max)
        except RuntimeError:                             # (tensors on two devices: the ATen form's own error)
            assert name == 'labels on the host'
        assert calls[n:] == ['hm'], name
    total_variation(p.half())
    monkeypatch.setattr(L, '_HIP_MAP_LOSS', False)
    hm_loss(p, g, w)
    total_variation(p)
    assert calls[-3:] == ['tv', 'hm', 'tv']
    # a label that wants a gradient gets the ATen form's gradient
    gl = g.clone().nan_to_num(0.0).requires_grad_(True)
    L.hm_loss(p, gl, w).backward()
    assert float(gl.grad.abs().max()) > 0


# ---- 5: capture, and the ticket shared with the other loss kernels -----------------------------------------------------------------------------
def test_map_losses_replay_as_one_graph():
    """One `hm_loss` plus total variation, forward and backward, captured once and replayed three times with new prediction and label values
    copied in before each replay: the replay's results are the launch-by-launch results for those values, bit for bit (fixed summation order)."""
    from monoforce_amd.capture import capture
    from monoforce_amd import losses as L
    shape = (4, 1, 64, 64)
    p0, g0, w0 = (t.to(DEV) for t in mc.hm_inputs(shape, torch.float32, 20, 'gt'))      # (a NaN prediction would make the total variation NaN)
    labels = torch.stack([g0[:, 0], w0[:, 0]], dim=1).contiguous()
    pred = p0.clone().requires_grad_(True)

    def fwd_bwd():
        l_hm = L.hm_loss(pred, labels[:, 0:1], labels[:, 1:2], h_max=1.0)
        l_tv = L.total_variation(pred)
        (grad,) = torch.autograd.grad(2.0 * l_hm + 0.3 * l_tv, pred)
        return l_hm.detach(), l_tv.detach(), grad
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # warm-up on the capture stream: its ticket exists
        for _ in range(2):
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with capture(graph, stream=s, capture_error_mode='thread_local'):
        static = fwd_bwd()
    seen = set()
    for k in range(3):
        pn, gn, _ = (t.to(DEV) for t in mc.hm_inputs(shape, torch.float32, 30 + k, 'gt'))
        with torch.no_grad():
            pred.copy_(pn)
            labels[:, 0:1].copy_(gn)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        want = fwd_bwd()
        seen.add(float(got[0]))
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        ref, gref, _, _ = mc.hm_loss_referee(pn, gn, w0, 1.0, upstream=2.0)
        tv_ref, tv_gref = mc.total_variation_referee(pn, upstream=0.3)
        assert mc.rel(got[0], ref) <= 2e-6 and mc.rel(got[1], tv_ref) <= 2e-6 and mc.grad_err(got[2], gref + tv_gref) <= 2e-6
    assert len(seen) == 3                                # every replay read the values copied in before it


def test_ticket_is_shared_by_the_loss_kernels_of_one_stream():
    """hm_loss, total variation and physics_loss alternating on one stream: every value launch finds the ticket at zero and leaves it there."""
    from monoforce_amd import losses as L
    from tests.test_pose_loss_gpu import _problem
    p, g, w = (t.to(DEV) for t in mc.hm_inputs((4, 1, 256, 256), torch.float32, 40, 'gt'))
    z = mc.tv_inputs((1, 256, 256), torch.float32, 41).to(DEV)
    q = {k: (v.float().to(DEV) if v.is_floating_point() else v.to(DEV)) for k, v in _problem(300, 43, 20, 42).items()}
    rounds = []
    for _ in range(4):
        rounds.append((float(L.hm_loss(p, g, w)), float(L.total_variation(z)),
                       float(L.physics_loss_fused([q['X']], [q['Xgt']], None, q['gt_ts'], gamma=0.9, nearest=q['near'])),
                       float(L.total_variation(p)), float(L.hm_loss(p, g, None, h_max=1.0))))
    assert len(set(rounds)) == 1 and all(math.isfinite(v) for v in rounds[0]), rounds
    ticket = L._ticket(torch.device('cuda', torch.cuda.current_device()), torch.cuda.current_stream())
    assert int(ticket) == 0
    assert mc.rel(rounds[0][0], mc.hm_loss_referee(p, g, w)[0]) <= 2e-6 and mc.rel(rounds[0][1], mc.total_variation_referee(z)[0]) <= 2e-6


# ---- 6: the regularised terrain fit --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fit_steps():
    """One step of `TerrainFitProblem` at 64 rollouts x 100 steps on a 64 x 64 map, per (mode, tv_weight): (loss, z.grad, mu.grad, launches)."""
    from monoforce_amd import _timing
    from monoforce_amd import synthetic as syn
    from monoforce_amd.train import TerrainFitProblem
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    z_true = (syn.bump_terrain(syn.bump_params(3), 3.2, 0.1) * 0.3).to(DEV)
    mu = syn.wave_friction(3.2, 0.1).to(DEV)
    ctrl = syn.const_controls(64, 100, seed=2).to(DEV)
    assert z_true.shape == (64, 64)
    out = {}
    for mode, kw in (('eager', dict(loss_in_kernel=False)), ('loss_in_kernel', dict(loss_in_kernel=True)), ('graph', dict(graph=True))):
        for tv_weight in (0.0, 0.1, None):
            dp = make_dphysics(pts, masks, 1, 0.1, 3.2)
            prob = TerrainFitProblem(dp, z_true, mu, ctrl, **kw, **({} if tv_weight is None else dict(tv_weight=tv_weight)))
            z = (z_true * 0.5).clone().requires_grad_(True)
            m = mu.clone().requires_grad_(True)
            launches = None
            if mode != 'graph':
                _timing.start()
            vals = [float(prob.step(z, m)) for _ in range(2 if mode != 'graph' else 3)]
            if mode != 'graph':      # {bracket name: launches in the two steps}, {rollout launch: kernel template, grid, workgroup}
                launches = ({k: len(v) for k, v in _timing.stop().items()}, {k: v.split(' launches=')[0] for k, v in _timing.launches().items()})
            assert len(set(vals[-2:])) == 1 or abs(vals[-1] - vals[-2]) <= 2e-6 * abs(vals[-1]), vals
            out[mode, tv_weight] = (vals[-1], z.grad.clone(), m.grad.clone(), launches, z.detach().clone())
    return out


@pytest.mark.parametrize('mode', ['eager', 'loss_in_kernel', 'graph'])
def test_fit_step_with_tv_weight_adds_the_regulariser(fit_steps, mode):
    """loss(tv_weight=0.1) = loss(0) + 0.1 TV(z) and z.grad likewise, with the referee's TV value and gradient; mu.grad is unchanged.  Bar
    2e-5: two runs of the rollout backward differ by the arrival order of their float atomics, which tests/test_physics_loss_gpu.py holds
    to 2e-5 between routes; the TV term itself is exact to 1e-6 (above)."""
    from tests import helpers as hp
    l0, gz0, gm0, _, z = fit_steps[mode, 0.0]
    l1, gz1, gm1, _, _ = fit_steps[mode, 0.1]
    tv, gtv = mc.total_variation_referee(z)
    assert float(tv) > 0 and float(gtv.abs().max()) > 0
    want_l, want_g = l0 + 0.1 * float(tv), gz0.double().cpu() + 0.1 * gtv
    errs = (mc.rel(l1, want_l), hp.rel_err(gz1, want_g), hp.rel_err(gm1, gm0))
    print(f'fit step {mode}: loss err {errs[0]:.3g}, z.grad err {errs[1]:.3g}, mu.grad err {errs[2]:.3g}; TV share of z.grad '
          f'{0.1 * float(gtv.abs().max()) / float(want_g.abs().max()):.3g}')
    assert errs[0] <= 2e-5 and errs[1] <= 2e-5 and errs[2] <= 2e-5, errs
    assert hp.rel_err(gz1, gz0) > 1e-3                    # the regulariser is not lost in the comparison


@pytest.mark.parametrize('mode', ['eager', 'loss_in_kernel'])
def test_fit_step_without_tv_weight_launches_what_it_launched_before(fit_steps, mode):
    """tv_weight=0.0 (given or left out) brackets the same C-ABI launches as before the argument existed, none of them a map-loss launch;
    tv_weight=0.1 adds exactly the two total-variation launches (and, where the backward launch used to form the loss value, the one small
    value launch the sum needs in the forward)."""
    (base, base_k), (zero, zero_k), (reg, reg_k) = fit_steps[mode, None][3], fit_steps[mode, 0.0][3], fit_steps[mode, 0.1][3]
    # the step as it was: rollout forward and backward, between them the loss's own two launches unless the rollout carries it
    before = {'rollout_fwd_kernel': 2, 'rollout_bwd_kernel': 2}
    if mode == 'eager':
        before.update(physics_loss_fwd=2, physics_loss_bwd=2)
    assert base == zero == before and base_k == zero_k and len(zero_k) == 2, (base, zero, zero_k)
    assert fit_steps[mode, None][0] == fit_steps[mode, 0.0][0]
    added = {k: v for k, v in reg.items() if k not in zero}
    want = {'total_variation_fwd': 2, 'total_variation_bwd': 2}
    if mode == 'loss_in_kernel':
        want.update(physics_loss_fwd=2)
    assert added == want and all(reg[k] == v for k, v in zero.items()), (zero, reg)
    assert reg_k['rollout_fwd_kernel'] == zero_k['rollout_fwd_kernel']


# ---- 7: the encoder train step ------------------------------------------------------------------------------------------------------------------
def test_encoder_step_losses_and_gradients_agree_between_the_routes(monkeypatch):
    """`EncoderTrainStep.losses` with `_HIP_MAP_LOSS` on and off: the two height-map losses to 2e-6 (each route within 1e-6 of the exact
    value, see the bars above), the encoder's gradients of their sum to three times the spread of two runs of the ATen route (the splat
    backward adds with float atomics), 1e-5 at least."""
    from monoforce_amd import losses as L
    from tests import helpers as hp
    from tests.test_encoder_gpu import _stamp_rig
    enc, dp, step, b16 = _stamp_rig()
    params = [p for p in enc.parameters() if p.requires_grad]

    def run(hip):
        monkeypatch.setattr(L, '_HIP_MAP_LOSS', hip)
        l_geom, l_terr, _ = step.compute_losses(tuple(b16))
        assert type(l_geom.grad_fn).__name__.startswith('_FusedHmLoss') == hip and type(l_terr.grad_fn).__name__.startswith('_FusedHmLoss') == hip
        grads = torch.autograd.grad(l_geom + l_terr, params, allow_unused=True)
        return float(l_geom.detach()), float(l_terr.detach()), torch.cat([g.flatten() for g in grads if g is not None]).cpu()
    off, off2, on = run(False), run(False), run(True)
    spread = hp.rel_err(off2[2], off[2])
    errs = (mc.rel(on[0], off[0]), mc.rel(on[1], off[1]), hp.rel_err(on[2], off[2]))
    print(f'encoder step, hip vs aten: l_geom {errs[0]:.3g} l_terr {errs[1]:.3g} encoder gradients {errs[2]:.3g} (aten run-to-run {spread:.3g})')
    assert float(off[2].abs().max()) > 0 and errs[0] <= 2e-6 and errs[1] <= 2e-6 and errs[2] <= max(1e-5, 3 * spread), (errs, spread)


def test_graphed_encoder_step_equals_the_eager_one_with_the_map_loss_kernels():
    from tests.test_encoder_gpu import _stamp_rig
    from monoforce_amd import losses as L
    from monoforce_amd.train import synthetic_encoder_batch
    assert L._HIP_MAP_LOSS
    enc, dp, step, _ = _stamp_rig(graph=True)
    b9 = synthetic_encoder_batch(enc, dp, n_rollouts=32, device=DEV, img_hw=(64, 128))
    step.opt.param_groups[0]['lr'] = 0.0                 # the parameters stay put: every step scores the same encoder
    replayed = step.step(b9)
    assert step.graph and step._cap is not None
    replayed = [float(replayed[0])] + [float(v) for v in replayed[1]]
    eager = step.step(b9, eager=True)
    eager = [float(eager[0])] + [float(v) for v in eager[1]]
    errs = [mc.rel(a, b) for a, b in zip(replayed, eager)]
    print('graphed vs eager encoder step (loss, l_geom, l_terr, l_phys):', errs)
    assert all(math.isfinite(v) for v in replayed) and all(e <= 1e-5 for e in errs), (replayed, eager)
    assert errs[1] == 0.0 and errs[2] == 0.0 or max(errs[1], errs[2]) <= 2e-6      # the two height-map losses
