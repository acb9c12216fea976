"""Losses that sit directly on top of the rollout / encoder outputs (plain torch; they run on whatever device the
tensors are on).  Semantics of `/root/reference/monoforce/src/monoforce/losses.py`: `physics_loss` :102-138, `hm_loss`
:77-99, `total_variation` :68-74, `rotation_difference` :48-65, `translation_difference` :36-45, `slerp` :14-34.

The loss kernels of the C ABI (`mf_physics_loss_*`, `mf_pose_loss_*`, `mf_nearest_steps_*`) are marshalled here and nowhere else: one
function per entry point (`loss_value`, `loss_backward`, `pose_loss_value`, `pose_loss_backward`, `nearest_steps_hip`) builds the
descriptor, sizes the partial sums and launches through `_lib.launch`; the autograd functions below and the rollout's fused-loss route
(dphysics.py) call them.  Likewise the two losses on a terrain map, `mf_hm_loss_*` and `mf_total_variation_*` (`hm_loss_value`,
`hm_loss_backward`, `total_variation_value`, `total_variation_backward`).
"""
import ctypes as C

import torch

from . import _lib

_HIP_LOSS = True      # physics_loss on GPU tensors runs on the mf_physics_loss_* kernels (False: the reference's ATen form)
_HIP_MAP_LOSS = True  # hm_loss / total_variation on GPU tensors run on the mf_hm_loss_* / mf_total_variation_* kernels (False: the ATen forms)

__all__ = ['nearest_steps', 'nearest_steps_hip', 'physics_loss', 'physics_loss_aten', 'physics_loss_fused', 'hm_loss', 'hm_loss_aten',
           'total_variation', 'total_variation_aten', 'rotation_difference', 'translation_difference', 'slerp']


def _map_dtype_ok(t):
    return t.is_cuda and t.dtype in (torch.float32, torch.float64) and t.dim() >= 2 and 0 < t.numel() < 2 ** 31


def total_variation(heightmap):
    """(sum |d/dy| + sum |d/dx|) / (h w) (losses.py:68-74) of a map [...,h,w]; the differences stay inside each map, the divisor is h w
    however many maps there are.  A float32 / float64 map on the MI355X: one `mf_total_variation_value_*` launch, and one
    `mf_total_variation_bwd_*` launch for the gradient (`_FusedTotalVariation`), instead of the eleven ATen launches of
    `total_variation_aten` and as many again backward; channel views, row-strided crops and [h,w] maps are read in place.  `sign(0) = 0`
    as in torch's `abs` backward.  `monoforce_amd.losses._HIP_MAP_LOSS = False` keeps the ATen form everywhere."""
    if _HIP_MAP_LOSS and _map_dtype_ok(heightmap):
        return _FusedTotalVariation.apply(heightmap)
    return total_variation_aten(heightmap)


def total_variation_aten(heightmap):
    """The reference's formulation (losses.py:68-74) in plain torch ops, on whatever device the tensor is on."""
    h, w = heightmap.shape[-2:]
    dv = (heightmap[..., :, 1:] - heightmap[..., :, :-1]).abs().sum()
    dh = (heightmap[..., 1:, :] - heightmap[..., :-1, :]).abs().sum()
    return (dv + dh) / (h * w)


def hm_loss(height_pred, height_gt, weights=None, h_max=None):
    """Weighted MSE between height maps over the cells where both are finite (losses.py:77-99).
    Tensors on the MI355X: one `mf_hm_loss_value_*` launch (the masked sum, the count of valid cells and their quotient) and one
    `mf_hm_loss_bwd_*` launch for the gradient (`_FusedHmLoss`) instead of about a dozen ATen launches each way -- where that IS the
    reference's result: float32 / float64 tensors of one dtype on one device, labels and weights that do not require grad, `h_max` a
    number.  Channel views of a [B,2,H,W] label tensor (`hm_geom[:, 0:1]`, `hm_geom[:, 1]`), row-strided crops and [H,W] maps are read in
    place; any other layout through one `.contiguous()`.  One documented difference from autograd: with `h_max` set, a NaN PREDICTION
    gets a NaN gradient at that cell from torch's tanh backward (0 * (1 - NaN^2)); the kernel's gradient is 0 there, like at every other
    masked cell.  Everything else takes `hm_loss_aten`.  `monoforce_amd.losses._HIP_MAP_LOSS = False` keeps the ATen form everywhere."""
    assert height_pred.shape == height_gt.shape, 'Height prediction and ground truth must have the same shape'
    assert weights is None or weights.shape == height_gt.shape, 'Weights and height ground truth must have the same shape'
    if _HIP_MAP_LOSS and _hm_loss_takes_the_hip_route(height_pred, height_gt, weights, h_max):
        return _FusedHmLoss.apply(height_pred, height_gt, weights, h_max)
    return hm_loss_aten(height_pred, height_gt, weights=weights, h_max=h_max)


def _hm_loss_takes_the_hip_route(height_pred, height_gt, weights, h_max):
    """`hm_loss`'s route decision (the kernels return the loss in the prediction's dtype and send no gradient to labels or weights)."""
    if not (_map_dtype_ok(height_pred) and (h_max is None or isinstance(h_max, (int, float)))):
        return False
    for t in (height_gt,) if weights is None else (height_gt, weights):
        if not (torch.is_tensor(t) and t.device == height_pred.device and t.dtype == height_pred.dtype and not t.requires_grad):
            return False
    return True


def hm_loss_aten(height_pred, height_gt, weights=None, h_max=None):
    """The reference's formulation (losses.py:77-99) in plain torch ops, on whatever device the tensors are on -- what `hm_loss` runs on CPU
    tensors and for everything its HIP route declines."""
    assert height_pred.shape == height_gt.shape, 'Height prediction and ground truth must have the same shape'
    if weights is None:
        weights = torch.ones_like(height_gt)
    assert weights.shape == height_gt.shape, 'Weights and height ground truth must have the same shape'
    if h_max is not None:
        height_pred = h_max * torch.tanh(height_pred)
    ok = ~(torch.isnan(height_pred) | torch.isnan(height_gt))
    # mean over the valid cells, written without boolean indexing: `x[ok]` is a `nonzero` plus a host synchronisation (four
    # per call in the reference's form); the masked sum differs from it only in float summation order
    diff = torch.where(ok, height_pred * weights - height_gt * weights, torch.zeros((), dtype=height_pred.dtype, device=height_pred.device))
    return (diff ** 2).sum() / ok.sum()


def nearest_steps(pred_ts, gt_ts):
    """Index of the predicted step closest in time to every ground-truth stamp, [N,T2] (losses.py:116)."""
    return (pred_ts.unsqueeze(1) - gt_ts.unsqueeze(2)).abs().argmin(dim=2)


def nearest_steps_hip(pred_ts, gt_ts):
    """`nearest_steps` as ONE launch (`mf_nearest_steps_*`: a thread per (rollout, stamp) scans its rollout's predicted stamps) instead
    of sub / abs / argmin over two [N,T2,T1] temporaries -- 25.6 M elements and 76 us of GPU time at the BASELINE shape for 51 200
    indices.  Same indices (the first minimum, like torch.argmin); int32 [N,T2].  Expanded (stride-0) stamp rows are read as they are.
    One documented difference: a NaN among the differences is SKIPPED here (index 0 only when every difference is NaN), where
    torch.argmin returns the first NaN's index -- stamps are finite in every caller of the reference."""
    _lib.require_hip_tensor(pred_ts, 'pred_ts')
    dt = torch.promote_types(pred_ts.dtype, gt_ts.dtype)
    if dt not in (torch.float32, torch.float64):
        dt = torch.float32
    N, T2 = gt_ts.shape
    T1 = pred_ts.shape[1]
    assert pred_ts.shape[0] == N and pred_ts.dim() == 2, f'pred_ts {tuple(pred_ts.shape)} and gt_ts {tuple(gt_ts.shape)} disagree'

    def rows(t):      # dtype, unit stride inside a row; the row stride may be 0 (one row expanded over the rollouts)
        t = t.detach().to(dt)
        return t if t.stride(1) == 1 or t.shape[1] == 1 else t.contiguous()
    p, g = rows(pred_ts), rows(gt_ts)
    out = torch.empty(N, T2, dtype=torch.int32, device=pred_ts.device)
    _lib.launch('mf_nearest_steps', pred_ts.device, C.c_int32(N), C.c_int32(T1), C.c_int32(T2), p, C.c_longlong(p.stride(0)), g,
                C.c_longlong(g.stride(0)), out, dtype=dt)
    return out


def physics_loss(states_pred, states_gt, pred_ts, gt_ts, gamma=0.9, rotation_loss=False, nearest=None):
    """Time-discounted position MSE at the predicted steps closest to the ground-truth stamps (losses.py:102-138).

    states_*[0]: positions [N,T1,3] / [N,T2,3]; pred_ts [N,T1]; gt_ts [N,T2]; weight 1 / (1 + gamma t).
    Tensors on the MI355X: the same value and gradient from the hand-written kernels (`physics_loss_fused`: one gather-reduce launch
    forward, one scatter launch backward, the index table from `mf_nearest_steps_*`) instead of ~25 ATen launches -- the reference's
    own form (`physics_loss_aten`) costs 0.29 ms of GPU time per call at the BASELINE shape, as much as the rollout's forward and
    half its backward (a sort inside `index_put_`'s backward, two 25.6 M-element temporaries for the argmin).
    `rotation_loss=True` (scripts/eval.py:151-153) returns `(loss, loss_rot)`, the second the time-discounted squared geodesic angle between
    states_*[2] ([N,T,3,3], losses.py:129-136).  On the MI355X both come from ONE launch and their gradients from another (`mf_pose_loss_*`,
    `_FusedPoseLoss`) under the conditions of the position route plus: rotations on the device in X_pred's dtype with their inner 3x3
    contiguous, an `R_gt` that does not require grad, rows of `R_pred` that do not alias.  One documented difference from autograd: where
    `(tr - 1) / 2` is exactly +-1 (identical rotations, or an angle of exactly pi) torch's `arccos` backward yields 0 * inf = NaN / inf;
    the kernel's rotation gradient is 0 there.  Outside the clip range both are 0.
    `monoforce_amd.losses._HIP_LOSS = False` keeps the ATen form everywhere."""
    X_gt, X_pred = states_gt[0], states_pred[0]
    # the cached drop-in step (api_cache.py): these ARE the states a replayed step handed out and this IS the call it was captured with ->
    # the graph's loss, whose backward hands out the graph's gradients; a launch-by-launch forward's states are observed instead
    tag = getattr(X_pred, '_mf_step', None)
    if tag is not None:
        hit = tag[0].cached_loss(tag, states_pred, states_gt, pred_ts, gt_ts, gamma, rotation_loss, nearest)
        if hit is not None:
            return hit
    else:
        tag = getattr(X_pred, '_mf_obs', None)
        if tag is not None:
            tag[0].observe_loss(tag, states_pred, states_gt, pred_ts, gt_ts, gamma, rotation_loss, nearest)
    # (the HIP route returns the loss in X_pred's dtype, sends no gradient to X_gt / gt_ts and stores -- not adds -- a row's gradient: it takes
    #  the call only where that IS the reference's result -- same dtypes, constants that do not require grad, a non-empty batch, rows of
    #  X_pred that do not alias each other -- and leaves the rest to the ATen form.  ADVICE r5.)
    if (_HIP_LOSS and not rotation_loss and X_pred.is_cuda and X_pred.dtype in (torch.float32, torch.float64) and X_pred.dim() == 3
            and X_pred.stride(2) == 1 and X_gt.is_cuda and gt_ts.is_cuda and (nearest is not None or pred_ts.is_cuda)
            and X_gt.dtype == X_pred.dtype and gt_ts.dtype == X_pred.dtype and not X_gt.requires_grad and not gt_ts.requires_grad
            and X_pred.numel() > 0 and X_gt.numel() > 0 and _rows_do_not_overlap(X_pred)):
        if nearest is None:
            nearest = nearest_steps_hip(pred_ts, gt_ts)
        return _FusedPhysicsLoss.apply(X_pred, X_gt, gt_ts, nearest, gamma)
    if (_HIP_LOSS and rotation_loss and X_pred.is_cuda and X_pred.dtype in (torch.float32, torch.float64) and X_pred.dim() == 3
            and X_pred.stride(2) == 1 and X_gt.is_cuda and gt_ts.is_cuda and (nearest is not None or pred_ts.is_cuda)
            and X_gt.dtype == X_pred.dtype and gt_ts.dtype == X_pred.dtype and not X_gt.requires_grad and not gt_ts.requires_grad
            and X_pred.numel() > 0 and X_gt.numel() > 0 and _rows_do_not_overlap(X_pred) and _rotations_take_the_hip_route(states_pred, states_gt)):
        if nearest is None:
            nearest = nearest_steps_hip(pred_ts, gt_ts)
        return _FusedPoseLoss.apply(X_pred, states_pred[2], X_gt, states_gt[2], gt_ts, nearest, gamma)
    return physics_loss_aten(states_pred, states_gt, pred_ts, gt_ts, gamma=gamma, rotation_loss=rotation_loss, nearest=nearest)


def _rows_do_not_overlap(X, width=3):
    """True when no two (rollout, step) rows of X[B,T,...] (`width` contiguous scalars each: 3 for positions, 9 for rotations) share memory
    (an `expand`ed / stride-0 X_pred aliases rows: the scatter kernel's plain stores would then drop contributions that the reference's
    index_put_ adds up)."""
    (lo, nlo), (hi, nhi) = sorted([(abs(X.stride(0)), X.shape[0]), (abs(X.stride(1)), X.shape[1])])
    if nlo > 1 and lo < width:
        return False
    return not (nhi > 1 and hi < lo * (nlo - 1) + width)


def _rotations_take_the_hip_route(states_pred, states_gt):
    """The rotation half of `physics_loss`'s route decision: states_*[2] on the device, in the positions' dtype, [B,T,3,3] with the inner
    3x3 contiguous, a ground truth that needs no gradient and predicted rows that do not alias."""
    if len(states_pred) < 3 or len(states_gt) < 3:
        return False
    X_pred, X_gt, R_pred, R_gt = states_pred[0], states_gt[0], states_pred[2], states_gt[2]
    for R, X in ((R_pred, X_pred), (R_gt, X_gt)):
        if not (torch.is_tensor(R) and R.is_cuda and R.device == X_pred.device and R.dtype == X_pred.dtype and R.dim() == 4
                and tuple(R.shape) == (*X.shape[:2], 3, 3) and R.stride(3) == 1 and R.stride(2) == 3):
            return False
    return not R_gt.requires_grad and _rows_do_not_overlap(R_pred, 9)


def physics_loss_aten(states_pred, states_gt, pred_ts, gt_ts, gamma=0.9, rotation_loss=False, nearest=None):
    """The reference's formulation (losses.py:102-138) in plain torch ops, on whatever device the tensors are on -- what `physics_loss`
    runs on CPU tensors and for the rotation term, and what the tests hold the HIP loss kernels to."""
    X_gt, X_pred = states_gt[0], states_pred[0]
    if nearest is None:     # callers with fixed time stamps may pass the cached result of nearest_steps()
        nearest = nearest_steps(pred_ts, gt_ts)
    rows = torch.arange(X_gt.shape[0], device=nearest.device).unsqueeze(1)
    X_sel = X_pred[rows, nearest]
    wt = 1. / (1. + gamma * gt_ts.unsqueeze(2))
    loss = ((X_sel * wt - X_gt * wt) ** 2).mean()
    if not rotation_loss:
        return loss
    R_gt, R_sel = states_gt[2], states_pred[2][rows, nearest]
    return loss, (rotation_difference(R_sel, R_gt, reduction='none') * wt).mean()


def translation_difference(x1, x2, reduction='mean'):
    """Euclidean distance between positions [...,3]: its mean, its sum, or (any other `reduction`) the distances themselves (losses.py:36-45)."""
    assert isinstance(x1, torch.Tensor) and isinstance(x2, torch.Tensor)
    assert x1.shape == x2.shape
    assert x1.shape[-1] == 3
    dist = torch.norm(x1 - x2, dim=-1)
    if reduction == 'mean':
        return dist.mean()
    if reduction == 'sum':
        return dist.sum()
    return dist


def slerp(q1, q2, t_interval, diff_thresh=0.9995):
    """Quaternion interpolation at the fractions `t_interval` [K] -> [K,4] (losses.py:14-34).  As the reference: above `diff_thresh` of the
    dot product the quaternions are blended linearly and the whole [K,4] result is divided by ITS norm (one scalar, not one per row);
    below, spherical interpolation with every row normalised; the shorter arc is not chosen (no sign flip for a negative dot product)."""
    assert isinstance(q1, torch.Tensor) and isinstance(q2, torch.Tensor)
    assert q1.shape == q2.shape == (4,)
    assert isinstance(t_interval, torch.Tensor)
    dot = (q1 * q2).sum()
    if dot > diff_thresh:
        q = (q1.unsqueeze(1) + t_interval * (q2 - q1).unsqueeze(1)).T
        return q / torch.norm(q)
    theta_0 = torch.acos(dot)
    theta = theta_0 * t_interval
    sin_t, sin_0 = torch.sin(theta), torch.sin(theta_0)
    s0 = torch.cos(theta) - dot * sin_t / sin_0
    s1 = sin_t / sin_0
    q = s0.unsqueeze(1) * q1 + s1.unsqueeze(1) * q2
    return q / torch.norm(q, dim=1, keepdim=True)


def rotation_difference(R1, R2, reduction='mean'):
    """Squared geodesic angle between rotations, theta = arccos((tr(R1 R2^T) - 1) / 2) (losses.py:48-65)."""
    assert R1.shape == R2.shape and R1.shape[-2:] == (3, 3)
    tr = (R1 @ R2.transpose(-2, -1)).diagonal(dim1=-2, dim2=-1).sum(dim=-1, keepdim=True)
    theta2 = torch.arccos(torch.clip((tr - 1) / 2., min=-1, max=1.)) ** 2
    if reduction == 'mean':
        return theta2.mean()
    if reduction == 'sum':
        return theta2.sum()
    return theta2


_TICKETS = {}
_CAPTURED_TICKETS = []      # counters whose ADDRESS a captured hipGraph replays into: never freed (4 bytes each), whatever the LRU / reset does


def _ticket(device, stream):
    """The zero-initialised counter `mf_physics_loss_value_*` needs, one per (device, stream): launches ordered on one stream
    share it (the kernel resets it)."""
    key = (device.index, stream.cuda_stream)
    t = _TICKETS.pop(key, None)
    if t is None:
        while len(_TICKETS) >= 32:                 # stream handles come and go: the oldest counters leave first
            _TICKETS.pop(next(iter(_TICKETS)))
        t = torch.zeros(1, dtype=torch.int32, device=device)
    _TICKETS[key] = t                              # re-inserted last = most recently used
    if torch.cuda.is_current_stream_capturing() and not any(t is c for c in _CAPTURED_TICKETS):
        _CAPTURED_TICKETS.append(t)                # a replay ticks this address long after the LRU dropped the entry
    return t


def _reset_tickets():
    """After a failed launch: a counter some blocks already ticked would never reach gridDim - 1 again, and every later loss on
    that stream would stay unwritten.  Dropping the counters makes the next call start from fresh zeros."""
    _TICKETS.clear()


def _register_reset():
    if _reset_tickets not in _lib.ON_ERROR:
        _lib.ON_ERROR.append(_reset_tickets)


def _numel(g):
    return C.c_longlong(0 if g is None else g.numel())


def loss_value(X_pred, X_gt, gt_ts, near, gamma, ticket, loss, gX=None):
    """One `mf_physics_loss_value_*` launch: `loss` (a scalar tensor) <- physics_loss of X_pred [B,T1,3] (any strides with xyz dense) against
    X_gt [B,T2,3], gt_ts [B,T2] and near [B,T2] int32, all contiguous in X_pred's dtype; `ticket`: `_ticket`'s counter of the current
    stream; `gX`: a gradient buffer with X_pred's strides that the same launch clears.  Returns the descriptor, which the backward takes."""
    (B, T1, _), T2 = X_pred.shape, X_gt.shape[1]
    desc = _lib.MfLossDesc(B=B, T1=T1, T2=T2, x_stride_b=X_pred.stride(0), x_stride_t=X_pred.stride(1), gamma=float(gamma))
    partial = torch.empty((B * T2 + 255) // 256, dtype=X_pred.dtype, device=X_pred.device)
    _lib.launch('mf_physics_loss_value', X_pred.device, desc, X_pred, X_gt, gt_ts, near, partial, ticket, loss, gX, _numel(gX),
                dtype=X_pred.dtype, timer='physics_loss_fwd')
    return desc


def loss_backward(desc, X_pred, X_gt, gt_ts, near, gloss, gX):
    """One `mf_physics_loss_bwd_*` launch: the rows of the zeroed `gX` that `near` names <- gloss [1] x d loss / d X_pred."""
    _lib.launch('mf_physics_loss_bwd', X_pred.device, desc, X_pred, X_gt, gt_ts, near, gloss, gX, dtype=X_pred.dtype, timer='physics_loss_bwd')


def pose_loss_value(X_pred, R_pred, X_gt, R_gt, gt_ts, near, gamma, ticket, out, gX=None, gR=None):
    """One `mf_pose_loss_value_*` launch: out [2] <- (loss, loss_rot); arguments as `loss_value` plus the rotations [B,T,3,3] (inner 3x3
    dense) and their gradient buffer.  Returns the descriptor."""
    (B, T1, _), T2 = X_pred.shape, X_gt.shape[1]
    desc = _lib.MfPoseLossDesc(B=B, T1=T1, T2=T2, x_stride_b=X_pred.stride(0), x_stride_t=X_pred.stride(1),
                               r_stride_b=R_pred.stride(0), r_stride_t=R_pred.stride(1), gamma=float(gamma))
    partial = torch.empty(2 * ((B * T2 + 255) // 256), dtype=X_pred.dtype, device=X_pred.device)
    _lib.launch('mf_pose_loss_value', X_pred.device, desc, X_pred, R_pred, X_gt, R_gt, gt_ts, near, partial, ticket, out, gX, _numel(gX),
                gR, _numel(gR), dtype=X_pred.dtype, timer='pose_loss_fwd')
    return desc


def pose_loss_backward(desc, X_pred, R_pred, X_gt, R_gt, gt_ts, near, gl, gX, gR):
    """One `mf_pose_loss_bwd_*` launch: gl [2] = the two upstream gradients; `gX` / `gR` zeroed, None = that half is not formed."""
    _lib.launch('mf_pose_loss_bwd', X_pred.device, desc, X_pred, R_pred, X_gt, R_gt, gt_ts, near, gl, gX, gR, dtype=X_pred.dtype,
                timer='pose_loss_bwd')


_MAP_CHUNK = 1024     # cells per workgroup of the map-loss kernels (map_losses.hip): one partial sum each


def map_strides(t):
    """A map tensor [...,H,W] as the map-loss kernels address it, [M][H][W] with unit stride along W: (tensor, stride_m, stride_h) in
    elements.  The leading axes must fold into ONE axis with one stride (axes of size 1 do not count): channel views of a [B,2,H,W]
    tensor, row-strided crops and [H,W] maps come back as they are, everything else (a strided W, leading axes that do not fold) as
    one `.contiguous()` copy."""
    for _ in range(2):
        lead = [(n, s) for n, s in zip(t.shape[:-2], t.stride()[:-2]) if n != 1]
        if (t.shape[-1] == 1 or t.stride(-1) == 1) and all(s0 == s1 * n1 for (_n0, s0), (n1, s1) in zip(lead, lead[1:])):
            return t, (lead[-1][1] if lead else 0), t.stride(-2)
        t = t.contiguous()
    raise AssertionError('a contiguous tensor folds')


def _map_desc(shape, **kw):
    H, W = shape[-2:]
    n = 1
    for v in shape:
        n *= v
    return _lib.MfMapLossDesc(M=n // (H * W), H=H, W=W, **kw), (n + _MAP_CHUNK - 1) // _MAP_CHUNK


def _grad_strides(g, like):
    """(stride_m, stride_h) of a gradient buffer the backward kernels store into: the shape, dtype and device of the tensor they read, and a
    layout they address without a copy (a copy would receive the stores instead of the buffer)."""
    assert g.shape == like.shape and g.dtype == like.dtype and g.device == like.device, 'the gradient buffer must match the map tensor'
    view, sm, sh = map_strides(g)
    assert view is g, f'a gradient buffer of strides {g.stride()} is not addressable as [M][H][W] with unit stride along W'
    return sm, sh


def hm_loss_state(pred, gt, weights, h_max):
    """What both `mf_hm_loss_*` launches take: (descriptor, pred, gt, weights) -- map tensors of one shape [...,H,W] and one dtype
    (weights None: all ones) as the kernels read them, each in place where `map_strides` returns it unchanged."""
    (pred, psm, psh), (gt, gsm, gsh) = map_strides(pred), map_strides(gt)
    weights, wsm, wsh = (None, 0, 0) if weights is None else map_strides(weights)
    desc, _ = _map_desc(pred.shape, use_h_max=int(h_max is not None), h_max=0.0 if h_max is None else float(h_max), p_stride_m=psm,
                        p_stride_h=psh, g_stride_m=gsm, g_stride_h=gsh, w_stride_m=wsm, w_stride_h=wsh)
    return desc, pred, gt, weights


def hm_loss_value(pred, gt, weights, h_max, ticket, loss, n_valid):
    """One `mf_hm_loss_value_*` launch: `loss` (a scalar tensor) <- hm_loss of pred against gt and weights; `n_valid` (int32 [1]) <- the
    number of cells that count; `ticket`: `_ticket`'s counter of the current stream.  Returns `hm_loss_state`, which the backward takes."""
    desc, pred, gt, weights = state = hm_loss_state(pred, gt, weights, h_max)
    blocks = _map_desc(pred.shape)[1]
    partial = torch.empty(blocks, dtype=pred.dtype, device=pred.device)
    counts = torch.empty(blocks, dtype=torch.int32, device=pred.device)
    _lib.launch('mf_hm_loss_value', pred.device, desc, pred, gt, weights, partial, counts, ticket, loss, n_valid, dtype=pred.dtype,
                timer='hm_loss_fwd')
    return state


def hm_loss_backward(desc, pred, gt, weights, n_valid, gloss, g_pred):
    """One `mf_hm_loss_bwd_*` launch: every cell of `g_pred` (pred's shape, its own strides, in a layout `map_strides` returns unchanged;
    no need to clear it) <- gloss [1] x d loss / d pred; (desc, pred, gt, weights) as `hm_loss_value` returned them."""
    desc.o_stride_m, desc.o_stride_h = _grad_strides(g_pred, pred)
    _lib.launch('mf_hm_loss_bwd', pred.device, desc, pred, gt, weights, n_valid, gloss, g_pred, dtype=pred.dtype, timer='hm_loss_bwd')


def total_variation_state(z):
    """What both `mf_total_variation_*` launches take: (descriptor, z as the kernels read it -- in place, or its contiguous copy)."""
    z, sm, sh = map_strides(z)
    return _map_desc(z.shape, p_stride_m=sm, p_stride_h=sh)[0], z


def total_variation_value(z, ticket, loss):
    """One `mf_total_variation_value_*` launch: `loss` (a scalar tensor) <- total_variation of the map tensor z [...,H,W].  Returns
    `total_variation_state`, which the backward takes."""
    desc, z = state = total_variation_state(z)
    partial = torch.empty(_map_desc(z.shape)[1], dtype=z.dtype, device=z.device)
    _lib.launch('mf_total_variation_value', z.device, desc, z, partial, ticket, loss, dtype=z.dtype, timer='total_variation_fwd')
    return state


def total_variation_backward(desc, z, gloss, g_z):
    """One `mf_total_variation_bwd_*` launch: every cell of `g_z` (z's shape, its own strides, no need to clear it) <- gloss [1] x d loss / d z."""
    desc.o_stride_m, desc.o_stride_h = _grad_strides(g_z, z)
    _lib.launch('mf_total_variation_bwd', z.device, desc, z, gloss, g_z, dtype=z.dtype, timer='total_variation_bwd')


def hm_loss_forward(height_pred, height_gt, weights=None, h_max=None):
    """`hm_loss` on the HIP kernels without autograd: (loss, n_valid, state); `n_valid` is the int32 [1] device count of the cells that
    entered the mean, `state` what `hm_loss_grad` takes."""
    _lib.require_hip_tensor(height_pred, 'height_pred')
    _register_reset()
    dev, dt = height_pred.device, height_pred.dtype
    loss = torch.empty((), dtype=dt, device=dev)
    n_valid = torch.empty(1, dtype=torch.int32, device=dev)
    state = hm_loss_value(height_pred.detach(), height_gt.detach().to(dt), None if weights is None else weights.detach().to(dt), h_max,
                          _ticket(dev, torch.cuda.current_stream(dev)), loss, n_valid)
    return loss, n_valid, state


def hm_loss_grad(state, n_valid, gloss, shape):
    """d hm_loss / d height_pred x gloss (a device scalar), a fresh contiguous tensor of `shape`: one launch, every cell stored."""
    desc, pred, gt, weights = state
    g_pred = torch.empty(shape, dtype=pred.dtype, device=pred.device)
    hm_loss_backward(desc, pred, gt, weights, n_valid, gloss.detach().to(pred.dtype).reshape(1), g_pred)
    return g_pred


class _FusedHmLoss(torch.autograd.Function):
    """`mf_hm_loss_value/bwd_*`: `hm_loss` as one masked-reduce kernel forward (sum, count and quotient) and one kernel backward that stores
    every cell; the count stays on the device between the two.  A NaN prediction under `h_max` has gradient 0 (torch's tanh backward: NaN),
    see `hm_loss`."""

    @staticmethod
    def forward(ctx, height_pred, height_gt, weights, h_max):
        loss, n_valid, (desc, pred, gt, w) = hm_loss_forward(height_pred, height_gt, weights, h_max)
        if ctx.needs_input_grad[0]:
            ctx.desc, ctx.has_w, ctx.shape = desc, w is not None, height_pred.shape
            ctx.save_for_backward(pred, gt, n_valid, *(() if w is None else (w,)))
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if gloss is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        pred, gt, n_valid = ctx.saved_tensors[:3]
        w = ctx.saved_tensors[3] if ctx.has_w else None
        return hm_loss_grad((ctx.desc, pred, gt, w), n_valid, gloss, ctx.shape), None, None, None


def total_variation_forward(heightmap):
    """`total_variation` on the HIP kernels without autograd: (loss, state); `state` is what `total_variation_grad` takes."""
    _lib.require_hip_tensor(heightmap, 'heightmap')
    _register_reset()
    dev = heightmap.device
    loss = torch.empty((), dtype=heightmap.dtype, device=dev)
    return loss, total_variation_value(heightmap.detach(), _ticket(dev, torch.cuda.current_stream(dev)), loss)


def total_variation_grad(state, gloss, shape):
    """d total_variation / d heightmap x gloss (a device scalar), a fresh contiguous tensor of `shape`: one launch, every cell stored."""
    desc, z = state
    g_z = torch.empty(shape, dtype=z.dtype, device=z.device)
    total_variation_backward(desc, z, gloss.detach().to(z.dtype).reshape(1), g_z)
    return g_z


class _FusedTotalVariation(torch.autograd.Function):
    """`mf_total_variation_value/bwd_*`: one reduce kernel forward, one gather kernel backward (the signed sum of a cell's up to four
    neighbour terms, sign(0) = 0; no atomics)."""

    @staticmethod
    def forward(ctx, heightmap):
        loss, (desc, z) = total_variation_forward(heightmap)
        if ctx.needs_input_grad[0]:
            ctx.desc, ctx.shape = desc, heightmap.shape
            ctx.save_for_backward(z)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if gloss is None or not ctx.needs_input_grad[0]:
            return None
        return total_variation_grad((ctx.desc, ctx.saved_tensors[0]), gloss, ctx.shape)


class _FusedPhysicsLoss(torch.autograd.Function):
    """`mf_physics_loss_value/bwd_*`: one gather-reduce kernel forward, one scatter kernel backward; the gradient comes back
    with the SAME strides as `X_pred` (for the rollout's time-major outputs: ready for `mf_rollout_bwd_*` without a copy)."""

    @staticmethod
    def forward(ctx, X_pred, X_gt, gt_ts, nearest, gamma):
        _lib.require_hip_tensor(X_pred, 'X_pred')
        _register_reset()
        assert X_pred.stride(2) == 1, 'positions must have their xyz components contiguous'
        Xg = X_gt.to(X_pred.dtype).contiguous()
        ts = gt_ts.to(X_pred.dtype).contiguous()
        near = nearest if nearest.dtype == torch.int32 else nearest.to(torch.int32)
        near = near.contiguous()
        loss = torch.empty((), dtype=X_pred.dtype, device=X_pred.device)
        # the mean is finished inside the launch (no `partial.sum() * c`: two launches fewer forward, two fewer backward)
        # when a backward will follow and X_pred is a dense view (the rollout's outputs are), its gradient buffer is allocated now
        # and cleared by the same launch
        gX = None
        if ctx.needs_input_grad[0] and X_pred.numel() > 0:
            gX = torch.empty_like(X_pred)                  # preserve_format: the strides of X_pred
            if gX.stride() != X_pred.stride():
                gX = None
        ctx.desc = loss_value(X_pred, Xg, ts, near, gamma, _ticket(X_pred.device, torch.cuda.current_stream(X_pred.device)), loss, gX)
        ctx.save_for_backward(X_pred, Xg, ts, near)
        ctx.gX = gX
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if gloss is None:
            return None, None, None, None, None
        X_pred, Xg, ts, near = ctx.saved_tensors
        gX, ctx.gX = ctx.gX, None                         # cleared by the forward launch; a second backward (retain_graph) refills
        if gX is None:
            gX = torch.zeros_like(X_pred)                 # preserve_format: same (dense) strides as X_pred
            if gX.stride() != X_pred.stride():
                gX = torch.empty_strided(X_pred.shape, X_pred.stride(), dtype=X_pred.dtype, device=X_pred.device).zero_()
        gl = gloss.to(X_pred.dtype).reshape(1).contiguous()
        loss_backward(ctx.desc, X_pred, Xg, ts, near, gl, gX)
        return gX, None, None, None, None


class _FusedPoseLoss(torch.autograd.Function):
    """`mf_pose_loss_value/bwd_*`: `physics_loss(..., rotation_loss=True)` as one gather-reduce kernel forward (both scalars) and one
    scatter kernel backward; the gradients of `X_pred` and `R_pred` come back with the SAME strides as their inputs (the rollout's
    time-major outputs: `mf_rollout_bwd_*` takes them as its gXs / gRs without a copy).  Where `(tr - 1) / 2` is exactly +-1 the rotation
    gradient is 0 (torch's arccos backward: NaN / inf), see `physics_loss`."""

    @staticmethod
    def forward(ctx, X_pred, R_pred, X_gt, R_gt, gt_ts, nearest, gamma):
        _lib.require_hip_tensor(X_pred, 'X_pred')
        _lib.require_hip_tensor(R_pred, 'R_pred')
        _register_reset()
        B, T1, _ = X_pred.shape
        T2 = X_gt.shape[1]
        dt = X_pred.dtype
        assert X_pred.stride(2) == 1, 'positions must have their xyz components contiguous'
        assert tuple(R_pred.shape) == (B, T1, 3, 3) and R_pred.dtype == dt and R_pred.stride(3) == 1 and R_pred.stride(2) == 3, \
            'rotations must be [B,T1,3,3] in the dtype of the positions with their 3x3 contiguous'
        assert tuple(R_gt.shape) == (B, T2, 3, 3), f'R_gt {tuple(R_gt.shape)} != {(B, T2, 3, 3)}'
        Xg = X_gt.to(dt).contiguous()
        Rg = R_gt.to(dt).contiguous()
        ts = gt_ts.to(dt).contiguous()
        near = nearest if nearest.dtype == torch.int32 else nearest.to(torch.int32)
        near = near.contiguous()
        out = torch.empty(2, dtype=dt, device=X_pred.device)
        # when a backward will follow and the inputs are dense views (the rollout's outputs are), their gradient buffers are allocated now
        # and cleared by the same launch

        def grad_buffer(k, t):
            if not ctx.needs_input_grad[k]:
                return None
            g = torch.empty_like(t)                        # preserve_format: the strides of the input
            return g if g.stride() == t.stride() else None
        gX, gR = grad_buffer(0, X_pred), grad_buffer(1, R_pred)
        ctx.desc = pose_loss_value(X_pred, R_pred, Xg, Rg, ts, near, gamma, _ticket(X_pred.device, torch.cuda.current_stream(X_pred.device)),
                                   out, gX, gR)
        ctx.save_for_backward(X_pred, R_pred, Xg, Rg, ts, near)
        ctx.gX, ctx.gR = gX, gR
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, gloss, grot):
        none = (None,) * 7
        X_pred, R_pred, Xg, Rg, ts, near = ctx.saved_tensors
        # a None upstream is a zero for that half: its gradient is not formed at all
        want_x = gloss is not None and ctx.needs_input_grad[0]
        want_r = grot is not None and ctx.needs_input_grad[1]
        if not (want_x or want_r):
            return none
        (gX, gR), ctx.gX, ctx.gR = (ctx.gX, ctx.gR), None, None      # cleared by the forward launch; a second backward (retain_graph) refills

        def zeroed(g, t):
            if g is not None:
                return g
            g = torch.zeros_like(t)                       # preserve_format: same (dense) strides as the input
            if g.stride() != t.stride():
                g = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device).zero_()
            return g
        gX = zeroed(gX, X_pred) if want_x else None
        gR = zeroed(gR, R_pred) if want_r else None
        zero = None
        if gloss is None or grot is None:
            zero = torch.zeros((), dtype=X_pred.dtype, device=X_pred.device)
        gl = torch.stack([(zero if g is None else g.to(X_pred.dtype).reshape(())) for g in (gloss, grot)])
        pose_loss_backward(ctx.desc, X_pred, R_pred, Xg, Rg, ts, near, gl, gX, gR)
        return (gX, gR) + none[2:]


def physics_loss_fused(states_pred, states_gt, pred_ts, gt_ts, gamma=0.9, nearest=None, rotation_loss=False):
    """`physics_loss` on the HIP kernels: the position term on `mf_physics_loss_*`; with `rotation_loss=True` the pair
    `(loss, loss_rot)` on `mf_pose_loss_*` (`_FusedPoseLoss`).  Same values and gradients, up to the rotation gradient's |cos| == 1
    rule (`physics_loss`)."""
    if nearest is None:
        nearest = nearest_steps(pred_ts, gt_ts)
    X_pred = states_pred[0]
    if X_pred.dim() != 3 or X_pred.numel() == 0 or not _rows_do_not_overlap(X_pred):      # (aliased rows: the scatter kernel stores, the reference adds)
        return physics_loss_aten(states_pred, states_gt, pred_ts, gt_ts, gamma=gamma, rotation_loss=rotation_loss, nearest=nearest.long())
    if not rotation_loss:
        return _FusedPhysicsLoss.apply(X_pred, states_gt[0], gt_ts, nearest, gamma)
    R_pred = states_pred[2]
    if R_pred.stride(3) != 1 or R_pred.stride(2) != 3:
        R_pred = R_pred.contiguous()
    if not _rows_do_not_overlap(R_pred, 9):
        return physics_loss_aten(states_pred, states_gt, pred_ts, gt_ts, gamma=gamma, rotation_loss=True, nearest=nearest.long())
    return _FusedPoseLoss.apply(X_pred, R_pred.to(X_pred.dtype), states_gt[0], states_gt[2], gt_ts, nearest, gamma)
