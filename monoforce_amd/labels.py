"""Rigid-terrain label maps for training: `rigid_terrain_heightmap` builds the `hm_terrain` label of the reference's dataset classes
(`get_terrain_height_map`, datasets/rough.py:621-649) for one sample or a batch of samples on the GPU.

Per sample the reference projects the lidar cloud into every camera's segmentation mask (`get_semantic_cloud`, :545-601), keeps the points
whose label is a rigid class, gravity-aligns them, sweeps the robot's footprint along the recorded poses (`get_footprint_traj_points`,
:343-365) and takes `estimate_heightmap` of the two clouds together -- five host stages.  Here that is ONE launch sequence of
monoforce_amd/csrc/terrain_labels.hip (`mf_terrain_labels_f32`, marshalled here and nowhere else): sentinel fill, one thread per cloud or
footprint point, finalize; no cloud is materialised in between, nothing is allocated by the launch and the host reads nothing back.  The full
definition -- every float32 operation and its order -- is the comment of `MfTerrainLabelsDesc` in include/monoforce_hip.h.

`rigid_terrain_heightmap_aten` is the same definition as an elementwise ATen composition (no `matmul`: the operation order is the
definition's): it runs on any device, is the route for machines without the kernel, and the yardstick of tests and
tools/bench_terrain_labels.py.  `semantic_cloud` and `footprint_traj_points` are the two intermediate clouds of the reference for callers that
want them.

NOT DIFFERENTIABLE: labels are data.  Nothing here has a backward and no result requires grad."""
import numpy as np
import torch

from . import _lib

__all__ = ['rigid_terrain_heightmap', 'rigid_terrain_heightmap_aten', 'terrain_labels_into', 'semantic_cloud', 'footprint_traj_points',
           'class_set_words']

_CACHE = {}


def _bin_edges(d_max, grid_res, device):
    """`torch.arange(-d_max, d_max, grid_res)` in float32, built on the host like the reference's and kept per device: the edges, not a
    formula, decide which cell a point on a boundary falls into."""
    key = ('bins', float(d_max), float(grid_res), str(device))
    if key not in _CACHE:
        _CACHE[key] = torch.arange(-d_max, d_max, grid_res, dtype=torch.float32).to(device)
    return _CACHE[key]


def _footprint_axes(robot_size, grid_res, device):
    """(fx, fy): `np.arange(-length/2, length/2, grid_res)` and `np.arange(-width/2, width/2, grid_res)` cast to float32 (rough.py:345-351;
    `robot_size` = (width, length)), built on the host and kept per device."""
    width, length = (float(v) for v in robot_size)
    key = ('foot', width, length, float(grid_res), str(device))
    if key not in _CACHE:
        _CACHE[key] = tuple(torch.from_numpy(np.arange(-e / 2, e / 2, grid_res).astype(np.float32)).to(device) for e in (length, width))
    return _CACHE[key]


def class_set_words(rigid_labels):
    """The 256-bit membership set of the labels as eight 32-bit words: bit (l & 31) of word l >> 5."""
    words = [0] * 8
    for v in (rigid_labels.tolist() if hasattr(rigid_labels, 'tolist') else rigid_labels):
        if int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f'terrain_labels: a label is an integer in 0..255, got {v!r}')
        words[int(v) >> 5] |= 1 << (int(v) & 31)
    return words


def _check_launch(points, offsets, seg, rots, trans, intrins, pose_align, poses, fx, fy, x_bins, y_bins, scratch, hm, point_labels, max_points):
    """Argument errors of the launch (raised before any device is touched).  Returns (S, C, Hi, Wi, T, n, strides)."""
    if seg.dim() != 4 or seg.dtype != torch.uint8:
        raise ValueError(f'terrain_labels: seg must be uint8 [S,C,Hi,Wi], got {seg.dtype} {tuple(seg.shape)}')
    S, C, Hi, Wi = seg.shape
    if S < 1 or (C > 0 and (Hi < 3 or Wi < 3)):
        raise ValueError(f'terrain_labels: at least one sample and masks of at least 3 x 3 are needed, got seg {tuple(seg.shape)}')
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f'terrain_labels: points must be float32 [sum N,3], got {points.dtype} {tuple(points.shape)}')
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (S + 1,):
        raise ValueError(f'terrain_labels: offsets must be int32 [{S + 1}], got {offsets.dtype} {tuple(offsets.shape)}')
    strides = []
    for name, t, tail in (('rots', rots, (3, 3)), ('trans', trans, (3,)), ('intrins', intrins, (3, 3))):
        if t.dtype != torch.float32 or tuple(t.shape) not in ((S, C) + tail, (C,) + tail):
            raise ValueError(f'terrain_labels: {name} must be float32 {(S, C) + tail} or, shared, {(C,) + tail}; got {t.dtype} {tuple(t.shape)}')
        strides.append(C * int(np.prod(tail)) if t.dim() == len(tail) + 2 else 0)
    if pose_align.dtype != torch.float64 or tuple(pose_align.shape) != (S, 3, 4):
        raise ValueError(f'terrain_labels: pose_align must be float64 [{S},3,4], got {pose_align.dtype} {tuple(pose_align.shape)}')
    if poses.dtype != torch.float64 or poses.dim() != 4 or poses.shape[0] != S or tuple(poses.shape[2:]) != (3, 4):
        raise ValueError(f'terrain_labels: poses must be float64 [{S},T,3,4], got {poses.dtype} {tuple(poses.shape)}')
    for name, t in (('fx', fx), ('fy', fy), ('x_bins', x_bins), ('y_bins', y_bins)):
        if t.dtype != torch.float32 or t.dim() != 1:
            raise ValueError(f'terrain_labels: {name} must be a float32 vector, got {t.dtype} {tuple(t.shape)}')
    n = x_bins.numel()
    if n < 1 or y_bins.numel() != n:
        raise ValueError(f'terrain_labels: x_bins and y_bins must have the same, positive length; got {n} and {y_bins.numel()}')
    if hm.dtype != torch.float32 or tuple(hm.shape) != (S, 2, n, n):
        raise ValueError(f'terrain_labels: hm must be float32 [{S},2,{n},{n}], got {hm.dtype} {tuple(hm.shape)}')
    if scratch.dtype != torch.int32 or scratch.numel() < S * n * n:
        raise ValueError(f'terrain_labels: scratch must hold {S * n * n} int32, got {scratch.dtype} x {scratch.numel()}')
    if point_labels is not None and (point_labels.dtype != torch.int16 or tuple(point_labels.shape) != (points.shape[0], C)):
        raise ValueError(f'terrain_labels: point_labels must be int16 [{points.shape[0]},{C}], got {point_labels.dtype} {tuple(point_labels.shape)}')
    if max_points is not None and not 0 <= int(max_points) <= points.shape[0]:
        raise ValueError(f'terrain_labels: max_points must be in 0..{points.shape[0]}, got {max_points}')
    named = dict(points=points, offsets=offsets, seg=seg, rots=rots, trans=trans, intrins=intrins, pose_align=pose_align, poses=poses, fx=fx, fy=fy,
                 x_bins=x_bins, y_bins=y_bins, scratch=scratch, hm=hm, point_labels=point_labels)
    for name, t in named.items():
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError(f'terrain_labels: {name} must be contiguous')
        if t.device != points.device:
            raise TypeError(f'terrain_labels: {name} is on {t.device}, points on {points.device}')
    return S, C, Hi, Wi, poses.shape[1], n, strides


def terrain_labels_into(points, offsets, seg, rots, trans, intrins, pose_align, poses, fx, fy, x_bins, y_bins, rigid_labels, clearance, d_max,
                        h_min, h_max, r_min, inv_res, scratch, hm, point_labels=None, max_points=None):
    """The launch.  GPU tensors, contiguous: `points` float32 [sum N,3]; `offsets` int32 [S+1]; `seg` uint8 [S,C,Hi,Wi]; `rots` / `intrins`
    float32 [S,C,3,3] and `trans` [S,C,3], or without the leading S when the samples share their cameras; `pose_align` float64 [S,3,4];
    `poses` float64 [S,T,3,4]; `fx`, `fy`, `x_bins`, `y_bins` float32 vectors; `scratch` int32, S*n*n words; writes `hm` float32 [S,2,n,n]
    and, when given, `point_labels` int16 [sum N,C].  `rigid_labels`: the labels 0..255 that count as rigid.  `r_min` None: no inner radius.
    `max_points`: an upper bound of the largest sample's point count known on the host (default: sum N) -- the offsets are read on the
    device only.  Returns (hm, point_labels).  No allocation, no host read."""
    S, C, Hi, Wi, T, n, strides = _check_launch(points, offsets, seg, rots, trans, intrins, pose_align, poses, fx, fy, x_bins, y_bins, scratch, hm,
                                                point_labels, max_points)
    words = class_set_words(rigid_labels)
    _lib.require_hip_tensor(points, 'points')
    d = _lib.MfTerrainLabelsDesc(S=S, C=C, Hi=Hi, Wi=Wi, T=T, Fx=fx.numel(), Fy=fy.numel(), n=n, n_points=points.shape[0],
                                 max_points=points.shape[0] if max_points is None else int(max_points),
                                 rots_stride_s=strides[0], trans_stride_s=strides[1], intrins_stride_s=strides[2],
                                 class_set=(_lib.C.c_uint32 * 8)(*words), clearance=float(clearance), d_max=float(d_max), h_min=float(h_min),
                                 h_max=float(h_max), r_min=float(-1.0 if r_min is None else r_min), inv_res=float(inv_res))
    _lib.launch('mf_terrain_labels', points.device, d, points, offsets, seg, rots, trans, intrins, pose_align, poses, fx, fy, x_bins, y_bins,
                scratch, hm, point_labels, dtype=torch.float32, timer='terrain_labels_kernel')
    return hm, point_labels


def _pose34(t, name, lead):
    """[.., 3, 4] float64 from [.., 3, 4] or [.., 4, 4] with `lead` leading dimensions."""
    t = torch.as_tensor(t).detach()
    if t.dim() != lead + 2 or t.shape[-1] != 4 or t.shape[-2] not in (3, 4):
        raise ValueError(f'terrain_labels: {name} must be {lead} leading dimension(s) of [3,4] or [4,4] matrices, got {tuple(t.shape)}')
    return t[..., :3, :].to(torch.float64)


def _normalised(points, seg, rots, trans, intrins, pose_align, poses, offsets, device):
    """The user-facing arguments in the launch's shapes and dtypes on `device` (argument errors are raised before anything is moved).
    Returns (tensors dict, single, max_points)."""
    seg = torch.as_tensor(seg).detach()
    if seg.dim() not in (3, 4):
        raise ValueError(f'terrain_labels: seg must be [C,Hi,Wi] or [S,C,Hi,Wi], got {tuple(seg.shape)}')
    if seg.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.bool):
        raise TypeError(f'terrain_labels: seg holds integer labels 0..255, got {seg.dtype}')
    single = seg.dim() == 3
    points = torch.as_tensor(points).detach()
    lead = 0 if single else 1
    if single:
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f'terrain_labels: points of one sample must be [N,3], got {tuple(points.shape)}')
        if offsets is not None:
            raise ValueError('terrain_labels: offsets belong to a batch of samples ([S,C,Hi,Wi] masks)')
        seg = seg[None]
        off, max_points = [0, points.shape[0]], points.shape[0]
    else:
        S = seg.shape[0]
        if offsets is None:
            if points.dim() != 3 or points.shape[0] != S or points.shape[2] != 3:
                raise ValueError(f'terrain_labels: without offsets the points of {S} samples must be [{S},N,3], got {tuple(points.shape)}')
            off, max_points = [s * points.shape[1] for s in range(S + 1)], points.shape[1]
            points = points.reshape(-1, 3)
        else:
            if points.dim() != 2 or points.shape[1] != 3:
                raise ValueError(f'terrain_labels: with offsets the points must be [sum N,3], got {tuple(points.shape)}')
            off = offsets
            if isinstance(off, torch.Tensor) and off.is_cuda:
                if tuple(off.shape) != (S + 1,):
                    raise ValueError(f'terrain_labels: offsets must have {S + 1} entries, got {tuple(off.shape)}')
                max_points = points.shape[0]           # (a device tensor is not read here: the loosest bound)
            else:
                off = [int(v) for v in (off.tolist() if hasattr(off, 'tolist') else off)]
                if len(off) != S + 1 or off[0] != 0 or off[-1] != points.shape[0] or any(b < a for a, b in zip(off, off[1:])):
                    raise ValueError(f'terrain_labels: offsets must be {S + 1} non-decreasing row indices from 0 to {points.shape[0]}, got {off}')
                max_points = max(b - a for a, b in zip(off, off[1:]))
    S, C = seg.shape[0], seg.shape[1]
    cams = {}
    for name, t, tail in (('rots', rots, (3, 3)), ('trans', trans, (3,)), ('intrins', intrins, (3, 3))):
        t = torch.as_tensor(t).detach()
        if tuple(t.shape) == (C,) + tail:
            pass                                        # one sample's cameras, or cameras the samples share
        elif single or tuple(t.shape) != (S, C) + tail:
            raise ValueError(f'terrain_labels: {name} must be {(C,) + tail}' + ('' if single else f' or {(S, C) + tail}') + f', got {tuple(t.shape)}')
        cams[name] = t
    pose_align = _pose34(pose_align, 'pose_align', lead)
    poses = torch.as_tensor(poses).detach()
    if poses.numel() == 0 and poses.dim() <= lead + 1:
        poses = poses.new_zeros((S, 0, 3, 4) if not single else (0, 3, 4), dtype=torch.float64)
    poses = _pose34(poses, 'poses', lead + 1)
    if single:
        pose_align, poses = pose_align[None], poses[None]
    if pose_align.shape[0] != S or poses.shape[0] != S:
        raise ValueError(f'terrain_labels: pose_align and poses must lead with the {S} samples, got {tuple(pose_align.shape)} and {tuple(poses.shape)}')
    if seg.numel() and seg.dtype != torch.uint8 and (int(seg.min()) < 0 or int(seg.max()) > 255):
        raise ValueError('terrain_labels: seg holds labels outside 0..255')
    t = dict(points=points.to(device=device, dtype=torch.float32).contiguous(),
             offsets=torch.as_tensor(off, dtype=torch.int32).to(device).contiguous(),
             seg=seg.to(device=device, dtype=torch.uint8).contiguous(),
             pose_align=pose_align.to(device).contiguous(), poses=poses.to(device).contiguous())
    for name, c in cams.items():
        t[name] = c.to(device=device, dtype=torch.float32).contiguous()
    return t, single, max_points


def _grid_scalars(grid_res, d_max, h_max, h_min, r_min):
    if not float(grid_res) > 0 or not float(d_max) > 0:
        raise ValueError(f'terrain_labels: grid_res and d_max must be positive, got {grid_res} and {d_max}')
    return float(-h_max if h_min is None else h_min), (None if r_min is None else float(r_min))


def rigid_terrain_heightmap(points, seg, rots, trans, intrins, rigid_labels, pose_align, poses, grid_res, d_max, h_max, robot_size=(0.7, 1.0),
                            clearance=0.0, r_min=None, h_min=None, offsets=None, return_point_labels=False):
    """The rigid-terrain label map `hm` [2,n,n] of one sample, or [S,2,n,n] of a batch: hm[0] = the largest height per cell (0 where nothing
    fell) of the cloud's rigid points and the footprint sweep, hm[1] = 1.0 where something fell; first grid axis = x, as `estimate_heightmap`.

    One sample: `points` [N,3] in the robot's frame; `seg` [C,Hi,Wi] integer label masks (0..255); `rots` [C,3,3], `trans` [C,3], `intrins`
    [C,3,3] the cameras as `ego_to_cam` takes them; `pose_align` [3|4,4] the gravity alignment of the cloud; `poses` [T,3|4,4] the recorded
    poses, already aligned (T may be 0).  A batch: `seg` [S,C,Hi,Wi], `pose_align` [S,..], `poses` [S,T,..]; `points` [S,N,3], or [sum N,3] with
    `offsets` ([S+1] row indices, a sample may be empty); the cameras [S,C,..] or, shared, [C,..].  `rigid_labels`: the labels that count as
    rigid.  `robot_size` = (width, length) in metres and `grid_res` give the footprint grid; `clearance`: |clearance| is taken off every
    pose's height.  `r_min`, `h_min` as in `estimate_heightmap` (h_min defaults to -h_max).  The poses are computed with in float64.

    Inputs on the host are copied to the GPU and the result comes back on the points' device.  With `return_point_labels` also the int16
    [N,C] (or [sum N,C]) labels each camera sees at each point, -1 where it does not see it.  The kernel route only: without the GPU or the
    library a RuntimeError (use `rigid_terrain_heightmap_aten` there).  Not differentiable."""
    h_lo, r_lo = _grid_scalars(grid_res, d_max, h_max, h_min, r_min)
    class_set_words(rigid_labels)
    home = torch.as_tensor(points).device
    if not torch.cuda.is_available():
        raise RuntimeError('rigid_terrain_heightmap runs on the MI355X HIP path only (no CPU fallback); rigid_terrain_heightmap_aten is the host form')
    dev = home if home.type == 'cuda' else torch.device('cuda', torch.cuda.current_device())
    t, single, max_points = _normalised(points, seg, rots, trans, intrins, pose_align, poses, offsets, dev)
    fx, fy = _footprint_axes(robot_size, grid_res, dev)
    xb = _bin_edges(d_max, grid_res, dev)
    n, S = xb.numel(), t['seg'].shape[0]
    hm = torch.empty(S, 2, n, n, dtype=torch.float32, device=dev)
    scratch = torch.empty(S * n * n, dtype=torch.int32, device=dev)
    lab = torch.empty(t['points'].shape[0], t['seg'].shape[1], dtype=torch.int16, device=dev) if return_point_labels else None
    terrain_labels_into(t['points'], t['offsets'], t['seg'], t['rots'], t['trans'], t['intrins'], t['pose_align'], t['poses'], fx, fy, xb, xb,
                        rigid_labels, clearance, d_max, h_lo, h_max, r_lo, 1.0 / grid_res, scratch, hm, lab, max_points)
    hm = (hm[0] if single else hm).to(home)
    return (hm, lab.to(home)) if return_point_labels else hm


def _point_labels_aten(t):
    """int16 [sum N,C] labels and the sample index of every row, by the definition's float32 operations (elementwise, in its order)."""
    p, seg, off = t['points'], t['seg'], t['offsets']
    S, C, Hi, Wi = seg.shape
    dev = p.device
    rows = torch.arange(p.shape[0], device=dev)
    sid = torch.searchsorted(off[1:].long(), rows, right=True).clamp_(max=S - 1)
    owned = (rows >= off[0]) & (rows < off[S])
    nan_row = torch.isnan(p).any(dim=1)
    lab = torch.full((p.shape[0], C), -1, dtype=torch.int16, device=dev)
    one = torch.ones((), dtype=torch.float32, device=dev)
    for c in range(C):
        R, tr, K = ((a[c][None] if a.dim() == b else a[sid, c]) for a, b in ((t['rots'], 3), (t['trans'], 2), (t['intrins'], 3)))
        a = [p[:, k] - tr[:, k] for k in range(3)]
        q = [(R[:, 0, i] * a[0] + R[:, 1, i] * a[1]) + R[:, 2, i] * a[2] for i in range(3)]
        w = [(K[:, i, 0] * q[0] + K[:, i, 1] * q[1]) + K[:, i, 2] * q[2] for i in range(3)]
        u, v = w[0] / w[2], w[1] / w[2]
        seen = (w[2] > 0) & (u > one) & (u < one * (Wi - 1)) & (v > one) & (v < one * (Hi - 1)) & owned & ~nan_row
        ui, vi = torch.where(seen, u, one).long(), torch.where(seen, v, one).long()          # (.long() truncates)
        lab[:, c] = torch.where(seen, seg[sid, c, vi, ui].to(torch.int16), lab[:, c])
    return lab, sid, owned


def _rigid_rows(P, x, y, z, tz):
    """((r0 x + r1 y) + r2 z) + t per row of the float64 poses P [..,3,4], `tz` the z row's translation; float64, stacked last."""
    ts = (P[..., 0, 3], P[..., 1, 3], tz)
    return torch.stack([(((P[..., r, 0] * x + P[..., r, 1] * y) + P[..., r, 2] * z) + ts[r]) for r in range(3)], dim=-1)


def _footprint_aten(poses, fx, fy, clearance):
    """poses [..,T,3,4] float64 -> [..,T,Fy,Fx,3] float64 (rough.py:343-365; meshgrid rows are y)."""
    P = poses[..., None, None, :, :]
    X, Y = fx.double()[None, :], fy.double()[:, None]
    return _rigid_rows(P, X, Y, torch.zeros((), dtype=torch.float64, device=poses.device), P[..., 2, 3] - abs(float(clearance)))


def rigid_terrain_heightmap_aten(points, seg, rots, trans, intrins, rigid_labels, pose_align, poses, grid_res, d_max, h_max, robot_size=(0.7, 1.0),
                                 clearance=0.0, r_min=None, h_min=None, offsets=None, return_point_labels=False):
    """`rigid_terrain_heightmap` as an ATen composition on the points' device (same arguments, same result): the definition's operations
    elementwise and in its order -- no `matmul`, whose order is the library's -- the per-cell maximum as `scatter_reduce('amax')` on the ordered
    integer keys.  The route for the host, and what the kernel is measured against.  Not differentiable."""
    h_lo, r_lo = _grid_scalars(grid_res, d_max, h_max, h_min, r_min)
    words = class_set_words(rigid_labels)
    dev = torch.as_tensor(points).device
    with torch.no_grad():
        t, single, _ = _normalised(points, seg, rots, trans, intrins, pose_align, poses, offsets, dev)
        fx, fy = _footprint_axes(robot_size, grid_res, dev)
        xb = _bin_edges(d_max, grid_res, dev)
        n, S = xb.numel(), t['seg'].shape[0]
        p = t['points']
        lab, sid, owned = _point_labels_aten(t)
        member = torch.tensor([(words[v >> 5] >> (v & 31)) & 1 for v in range(256)], dtype=torch.bool).to(dev)
        kept = ((lab >= 0) & member[lab.clamp(min=0).long()]).any(dim=1) & owned
        A = t['pose_align'][sid]
        g = _rigid_rows(A, p[:, 0].double(), p[:, 1].double(), p[:, 2].double(), A[:, 2, 3]).float()
        foot = _footprint_aten(t['poses'], fx, fy, clearance).float().reshape(S, -1, 3)
        g = torch.cat([g, foot.reshape(-1, 3)])
        sid = torch.cat([sid, torch.arange(S, device=dev).repeat_interleave(foot.shape[1])])
        ok = torch.cat([kept, torch.ones(S * foot.shape[1], dtype=torch.bool, device=dev)])
        x, y, z = g[:, 0].contiguous(), g[:, 1].contiguous(), g[:, 2].contiguous()
        ok = ok & ~torch.isnan(g).any(dim=1)
        if r_lo is not None and r_lo >= 0:
            ok = ok & ((x.double() * x.double() + y.double() * y.double()).sqrt().float() > r_lo)
        ok = ok & (x > -d_max) & (x < d_max) & (y > -d_max) & (y < d_max) & (z > h_lo) & (z < h_max)
        ix, iy = torch.bucketize(x, xb) - 1, torch.bucketize(y, xb) - 1
        ok = ok & (ix >= 0) & (iy >= 0)
        cells = S * n * n
        flat = torch.where(ok, (sid * n + iy.clamp(0, n - 1)) * n + ix.clamp(0, n - 1), torch.full_like(sid, cells))     # (rejected: a spare cell)
        b = z.view(torch.int32)
        key = torch.where(b >= 0, b, b ^ 0x7FFFFFFF)
        lowest = torch.iinfo(torch.int32).min
        top = torch.full((cells + 1,), lowest, dtype=torch.int32, device=dev).scatter_reduce(0, flat, key, 'amax', include_self=True)[:cells]
        got = (top != lowest).view(S, n, n).transpose(1, 2)
        val = torch.where(top >= 0, top, top ^ 0x7FFFFFFF).view(torch.float32).view(S, n, n).transpose(1, 2)
        hm = torch.stack([torch.where(got, val, torch.zeros((), dtype=torch.float32, device=dev)), got.float()], dim=1).contiguous()
        hm = hm[0] if single else hm
    return (hm, lab) if return_point_labels else hm


def semantic_cloud(points, seg, rots, trans, intrins, labels=None):
    """The labelled cloud of ONE sample as the reference concatenates it (`get_semantic_cloud`, rough.py:553-588): for every camera in the
    order given (the reference walks its camera list backwards), the points it sees and the labels it sees there, one camera after the other --
    a point seen by two cameras appears twice.  `labels`: keep only these labels (the reference's `classes=`).  Returns (points [M,3], labels
    [M] uint8) on the points' device; the points are NOT gravity-aligned (`monoforce.transformations.transform_cloud` does that).  GPU tensors
    go through the kernel, host tensors through the ATen form; the cloud is then built from the per-point labels with boolean indexing."""
    points = torch.as_tensor(points).detach()
    if torch.as_tensor(seg).dim() != 3:
        raise ValueError('semantic_cloud: one sample at a time ([C,Hi,Wi] masks)')
    if points.is_cuda:
        dev = points.device
        t, single, max_points = _normalised(points, seg, rots, trans, intrins, torch.eye(4, dtype=torch.float64), torch.zeros(0, 3, 4), None, dev)
        edge = _bin_edges(1.0, 2.0, dev)                # one cell: the map is not what is asked for
        none = torch.zeros(0, dtype=torch.float32, device=dev)
        lab = torch.empty(t['points'].shape[0], t['seg'].shape[1], dtype=torch.int16, device=dev)
        terrain_labels_into(t['points'], t['offsets'], t['seg'], t['rots'], t['trans'], t['intrins'], t['pose_align'], t['poses'], none, none, edge, edge,
                            (), 0.0, 1.0, -1.0, 1.0, None, 0.5, torch.empty(1, dtype=torch.int32, device=dev),
                            torch.empty(1, 2, 1, 1, dtype=torch.float32, device=dev), lab, max_points)
    else:
        t, single, _ = _normalised(points, seg, rots, trans, intrins, torch.eye(4, dtype=torch.float64), torch.zeros(0, 3, 4), None, points.device)
        with torch.no_grad():
            lab = _point_labels_aten(t)[0]
    pts, out_p, out_l = t['points'], [], []
    for c in range(lab.shape[1]):
        m = lab[:, c] >= 0
        out_p.append(pts[m])
        out_l.append(lab[m, c].to(torch.uint8))
    out_p = torch.cat(out_p) if out_p else pts[:0]
    out_l = torch.cat(out_l) if out_l else torch.zeros(0, dtype=torch.uint8, device=pts.device)
    if labels is not None:
        words = class_set_words(labels)
        member = torch.tensor([(words[v >> 5] >> (v & 31)) & 1 for v in range(256)], dtype=torch.bool).to(pts.device)
        m = member[out_l.long()]
        out_p, out_l = out_p[m], out_l[m]
    return out_p, out_l


def footprint_traj_points(poses, robot_size, grid_res, clearance):
    """The footprint sweep of the reference (`get_footprint_traj_points`, rough.py:343-365) for `poses` [T,3|4,4]: the footprint grid of
    `robot_size` = (width, length) at `grid_res`, on the plane z = 0, carried through every pose with |clearance| taken off its height.
    Returns [T*F,3] float64, like the reference (the label map rounds them to float32), pose after pose, rows of the grid along y; a numpy
    array for numpy poses, else a tensor on the poses' device.  The poses are not changed (the reference subtracts the clearance in place)."""
    as_numpy = isinstance(poses, np.ndarray)
    P = _pose34(torch.from_numpy(poses) if as_numpy else poses, 'poses', 1)
    fx, fy = _footprint_axes(robot_size, grid_res, P.device)
    with torch.no_grad():
        out = _footprint_aten(P, fx, fy, clearance).reshape(-1, 3)
    return out.numpy() if as_numpy else out
