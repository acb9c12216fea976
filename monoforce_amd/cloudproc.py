"""`estimate_heightmap` of the reference's label generation (`/root/reference/monoforce/src/monoforce/cloudproc.py:88-148`)
on the MI355X: per-cell maximum height of a point cloud plus the measurement mask, `mf_estimate_heightmap_f32`
(csrc/heightmap.hip; include/monoforce_hip.h).  Same signature, same `[2, H, W]` float32 result (height, mask; first grid
axis = x).  The cloud may live on the host (it is copied to the GPU, the result comes back on the cloud's device) or on the
GPU; there is no CPU implementation.

`filter_grid`, `hm_to_cloud` and `within_bounds` are the other three names of the reference's module (cloudproc.py:24-86, :151-173): small
host-side helpers with its signatures and its results, restated here; `filter_grid` additionally takes a torch tensor on any device.
"""
import numpy as np
import torch
from numpy.lib.recfunctions import structured_to_unstructured

from . import _lib

__all__ = ['filter_grid', 'estimate_heightmap', 'hm_to_cloud', 'within_bounds']

default_rng = np.random.default_rng(135)

_BINS = {}


def _bin_edges(d_max, grid_res, device):
    """The reference's bin edges: `torch.arange(-d_max, d_max, grid_res)` in the default dtype (float32), built on the host
    exactly like there -- the edges, not a formula, decide which cell a point on a boundary falls into."""
    key = (float(d_max), float(grid_res), str(device))
    if key not in _BINS:
        _BINS[key] = torch.arange(-d_max, d_max, grid_res, dtype=torch.float32).to(device)
    return _BINS[key]


def estimate_heightmap(points, grid_res, d_max, h_max, r_min=None, h_min=None):
    """points [N, 3] (x, y, z) float32 -> hm [2, H, W]: hm[0] = max z per cell (0 where no point fell), hm[1] = 1.0 where
    measured.  Rows with NaNs, points closer than `r_min` to the origin (xy) and points outside the open box
    (-d_max, d_max)^2 x (h_min, h_max) are ignored; `h_min` defaults to -h_max."""
    assert points.dim() == 2 and points.shape[1] >= 3
    if not torch.cuda.is_available():
        raise RuntimeError('estimate_heightmap runs on the MI355X HIP path only (no CPU fallback)')
    home = points.device
    dev = home if points.is_cuda else torch.device('cuda', torch.cuda.current_device())
    pts = points.detach()[:, :3].to(device=dev, dtype=torch.float32).contiguous()
    if points.shape[1] > 3:
        # the reference drops a row when ANY of its columns is NaN (cloudproc.py:90: `~torch.isnan(points).any(dim=1)`), the extra
        # fields (intensity, ...) included: such a row gets a NaN x here, which the kernel's own filter then discards
        extra_nan = torch.isnan(points.detach()[:, 3:]).any(dim=1).to(dev)
        pts[:, 0] = torch.where(extra_nan, torch.full_like(pts[:, 0], float('nan')), pts[:, 0])
    xb = _bin_edges(d_max, grid_res, dev)
    n = xb.numel()
    desc = _lib.MfHeightmapDesc(n_points=pts.shape[0], nx=n, ny=n, d_max=float(d_max), h_min=float(-h_max if h_min is None else h_min),
                                h_max=float(h_max), r_min=float(-1.0 if r_min is None else r_min), inv_res=float(1.0 / grid_res))
    scratch = torch.empty(n * n, dtype=torch.int32, device=dev)
    hm = torch.empty(2, n, n, dtype=torch.float32, device=dev)
    _lib.launch('mf_estimate_heightmap', dev, desc, pts, xb, xb, scratch, hm, dtype=torch.float32)
    return hm.to(home)


def position(cloud):
    """The xyz columns of a structured cloud as a plain array; a plain array is returned as it is (ALL of its columns)."""
    return structured_to_unstructured(cloud[['x', 'y', 'z']]) if cloud.dtype.names else cloud


def within_bounds(x, min=None, max=None, bounds=None, log_variable=None):
    """Flat boolean mask of `min <= x <= max` over the elements of x (a tensor, or anything `torch.tensor` takes).  `bounds=(min, max)`
    instead of the two; a bound of None or of infinite size is no bound.  `log_variable`: print the kept fraction under that name."""
    x = x if isinstance(x, torch.Tensor) else torch.tensor(x)
    if bounds:
        assert min is None and max is None, 'give bounds or min / max, not both'
        min, max = bounds
    flat = x.flatten()
    keep = torch.ones(flat.shape, dtype=torch.bool, device=x.device)
    if min is not None and min > -float('inf'):
        keep &= flat >= (min if isinstance(min, torch.Tensor) else torch.tensor(min))
    if max is not None and max < float('inf'):
        keep &= flat <= (max if isinstance(max, torch.Tensor) else torch.tensor(max))
    if log_variable is not None:
        print('%.3f = %i / %i points kept (%.3g <= %s <= %.3g).'
              % (keep.double().mean(), keep.sum(), keep.numel(), float('nan') if min is None else min, log_variable,
                 float('nan') if max is None else max))
    return keep


def filter_grid(cloud, grid_res, keep='first', log=False, rng=default_rng, only_mask=False):
    """One point per occupied cell of a grid of `grid_res`: the cells are `floor(position / grid_res)` over every column of the positions,
    and each cell keeps its first point.  `keep='last'` walks the cloud backwards and `keep='random'` shuffles it IN PLACE first, as the
    reference does; the result follows the sorted order of the cells, not the cloud's.  `only_mask`: return the row indices instead of the
    rows -- indices into the cloud AS WALKED (reversed for 'last').

    `cloud`: a numpy array, structured (fields x, y, z) or plain, like the reference's; or a torch tensor [N,D] on any device, where the
    cells come from `torch.unique(dim=0)` and the first row of each from `scatter_reduce('amin')` of the row numbers -- the same indices."""
    assert isinstance(grid_res, (float, int)) and grid_res > 0.0
    assert keep in ('first', 'random', 'last')
    if isinstance(cloud, torch.Tensor):
        assert cloud.dim() == 2 and cloud.shape[0] > 0, tuple(cloud.shape)
        if keep == 'random':
            cloud.copy_(cloud[torch.from_numpy(rng.permutation(cloud.shape[0])).to(cloud.device)])
        elif keep == 'last':
            cloud = cloud.flip(0)
        cells = torch.floor(cloud / grid_res).long()
        _, inverse = torch.unique(cells, dim=0, return_inverse=True)
        rows = torch.arange(cloud.shape[0], device=cloud.device)
        ind = torch.full((int(inverse.max()) + 1,), cloud.shape[0], dtype=torch.long, device=cloud.device)
        ind = ind.scatter_reduce(0, inverse, rows, 'amin', include_self=True)
    else:
        assert isinstance(cloud, np.ndarray), type(cloud)
        if cloud.dtype.names:
            cloud = cloud.ravel()
        if keep == 'random':
            rng.shuffle(cloud)
        elif keep == 'last':
            cloud = cloud[::-1]
        cells = np.floor(position(cloud) / grid_res).astype(int)
        assert cells.size > 0
        ind = np.unique(cells, return_index=True, axis=0)[1]
    if log:
        print('%.3f = %i / %i points kept (grid res. %.3f m).' % (len(ind) / len(cells), len(ind), len(cells), grid_res))
    return ind if only_mask else cloud[ind]


def hm_to_cloud(height, cfg, mask=None):
    """A height map [H,W] as a cloud [H*W,3] (or the rows where `mask` is set): x and y are `linspace(-cfg.d_max, cfg.d_max, .)` over the
    two axes, z the heights.  Like the reference, a numpy map pairs its coordinates through `np.meshgrid`'s default 'xy' indexing (x varies
    along the SECOND axis) and a torch map through `torch.meshgrid`'s 'ij' (x along the first)."""
    assert isinstance(height, (np.ndarray, torch.Tensor)) and height.ndim == 2
    if mask is not None:
        assert isinstance(mask, (np.ndarray, torch.Tensor)) and mask.ndim == 2 and mask.shape == height.shape
        mask = mask.bool() if isinstance(mask, torch.Tensor) else mask.astype(bool)
    if isinstance(height, np.ndarray):
        xs, ys = (np.linspace(-cfg.d_max, cfg.d_max, k) for k in height.shape)
        gx, gy = np.meshgrid(xs, ys)
        cloud = np.stack([gx, gy, height], axis=2)
    else:
        xs, ys = (torch.linspace(-cfg.d_max, cfg.d_max, k).to(height.device) for k in height.shape)
        gx, gy = torch.meshgrid(xs, ys, indexing='ij')
        cloud = torch.stack([gx, gy, height], dim=2)
    if mask is not None:
        cloud = cloud[mask]
    return cloud.reshape([-1, 3])
