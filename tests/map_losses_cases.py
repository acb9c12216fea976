"""Shared cases and the float64 referee of the height-map loss tests (tests/test_map_losses_cpu.py, tests/test_map_losses_gpu.py).

The referee restates the reference's formulas (monoforce/losses.py:68-74 `total_variation`, :77-99 `hm_loss`) in float64 torch on the
CPU, boolean indexing included; its gradients are autograd's."""
import torch

# (1,257,3): rows of 3 cells against waves of 64 and workgroup rows of 256 threads -- every boundary falls mid-row; (3,257,5): the same
# over four workgroups; (1,256,256) and (4,1,256,256): 64 and 256 workgroups through the ticket finish
SHAPES = [(1, 1), (1, 5), (5, 1), (3, 7, 13), (2, 1, 64, 64), (1, 257, 3), (3, 257, 5), (1, 256, 256), (4, 1, 256, 256)]
NAN_MODES = ('none', 'gt', 'pred', 'both')
F64_BAR = 1e-11          # the project's float64 bar (tests/test_oracle_golden.py)
F32_FLOOR = 1e-6         # the pose-loss tests' float32 floor; the bar of a case is max(floor, 2 x the ATen float32 form's own error)


def ids(shape):
    return 'x'.join(str(v) for v in shape)


def hm_inputs(shape, dtype, seed, nan_mode='none', masked=0.3, weighted=True):
    """(pred, gt, weights) of `shape` in `dtype` on the CPU.  Predictions N(0, 0.7), labels N(0, 0.5); weights (`weighted`) U(0.2, 1.5) with
    about a fifth of the cells at exactly 0.  `nan_mode`: where the NaNs sit -- about `masked` of the cells in total ('both': a third of them
    in the labels only, a third in the predictions only, a third in both at once); at least one NaN whenever there are two cells or more."""
    g = torch.Generator().manual_seed(seed)
    pred = 0.7 * torch.randn(shape, generator=g, dtype=torch.float64)
    gt = 0.5 * torch.randn(shape, generator=g, dtype=torch.float64)
    weights = None
    if weighted:
        weights = 0.2 + 1.3 * torch.rand(shape, generator=g, dtype=torch.float64)
        weights[torch.rand(shape, generator=g) < 0.2] = 0.0
    if nan_mode != 'none' and pred.numel() > 1:
        u = torch.rand(shape, generator=g).flatten()
        u[int(torch.randint(pred.numel(), (1,), generator=g))] = 0.0                      # at least one
        u[(int(u.argmin()) + 1) % pred.numel()] = 1.0                                     # ... and at least one valid cell
        u = u.view(shape)
        hit = u < masked
        in_gt = hit if nan_mode == 'gt' else (hit & (u < masked * 2 / 3) if nan_mode == 'both' else torch.zeros_like(hit))
        in_pred = hit if nan_mode == 'pred' else (hit & (u >= masked / 3) if nan_mode == 'both' else torch.zeros_like(hit))
        gt[in_gt] = float('nan')
        pred[in_pred] = float('nan')
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    return cast(pred), cast(gt), cast(weights)


def tv_inputs(shape, dtype, seed, ties=True):
    """A map tensor of `shape`: N(0, 0.3) heights; `ties`: rounded to a 0.25 grid, so that many neighbours are EQUAL (sign(0) decides
    their gradient) while others differ."""
    g = torch.Generator().manual_seed(seed)
    z = 0.3 * torch.randn(shape, generator=g, dtype=torch.float64)
    if ties:
        z = torch.round(z * 4) / 4
    return z.to(dtype)


def hm_loss_referee(pred, gt, weights=None, h_max=None, upstream=1.0):
    """losses.py:77-99 in float64 with boolean indexing: (loss, d(upstream * loss) / d pred, n_valid, cells whose prediction is NaN)."""
    p = pred.detach().double().cpu().clone().requires_grad_(True)
    g = gt.detach().double().cpu()
    w = torch.ones_like(g) if weights is None else weights.detach().double().cpu()
    q = h_max * torch.tanh(p) if h_max is not None else p
    ok = ~(torch.isnan(q) | torch.isnan(g))
    loss = ((q[ok] * w[ok] - g[ok] * w[ok]) ** 2).mean()
    (grad,) = torch.autograd.grad(upstream * loss, p)
    return loss.detach(), grad, int(ok.sum()), torch.isnan(p.detach())


def total_variation_referee(z, upstream=1.0):
    """losses.py:68-74 in float64: (loss, d(upstream * loss) / d z)."""
    x = z.detach().double().cpu().clone().requires_grad_(True)
    h, w = x.shape[-2:]
    tv = torch.sum(torch.abs(x[..., :, :-1] - x[..., :, 1:])) + torch.sum(torch.abs(x[..., :-1, :] - x[..., 1:, :]))
    tv = tv / (h * w)
    (grad,) = torch.autograd.grad(upstream * tv, x)
    return tv.detach(), grad


def rel(a, b):
    """|a - b| / |b| of two scalars (0 when both are exactly equal, also at b == 0)."""
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / max(abs(b), 1e-300)


def grad_err(a, b, exclude=None):
    """max |a - b| / max |b| over the cells not in `exclude` (0 when both are all zeros there)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if exclude is not None:
        keep = ~exclude.cpu()
        a, b = a[keep], b[keep]
    if a.numel() == 0:
        return 0.0
    d, s = float((a - b).abs().max()), float(b.abs().max())
    return 0.0 if d == 0.0 else d / max(s, 1e-300)
