"""Every `mf_rollout_*` entry point of the C ABI (include/monoforce_hip.h), marshalled in ONE place.

Everything that builds an `MfRolloutDesc`, `MfRolloutFwdBufs`, `MfRolloutBwdBufs` or `MfRolloutLoss`, or that calls the rollout
launches (`mf_rollout_fwd_*`, `mf_rollout_bwd_*`, `mf_rollout_default_state_*`), their sizing and policy queries
(`mf_rollout_force_stride`, `mf_rollout_record_bytes[_f64]`, `mf_rollout_loss_fusable`, `mf_rollout_bwd_window`,
`mf_rollout_bwd_wants_gcontrols`, `mf_rollout_fwd_stages_zmu`) and the reduction over the gradient copies
(`mf_reduce_grad_copies_*`), is here; a new buffer or descriptor field is threaded through this file alone.  The launches go through
`_lib.launch`.  The callers -- `DPhysics` (dphysics.py, dphysics_bwd.py) and the registered ops (ops.py) -- decide WHAT they want
(options, gradient-copy count, which outputs) and shape what they hand out (transposes, `[:N]` slices); nothing here knows who calls.

The queries read the CU count of the CURRENT device, so a caller enters `torch.cuda.device` once around its whole launch
path, queries included.

Imports without a GPU (the library is loaded at the first launch); `canonical_maps` and `time_grid` are plain torch.
"""
import ctypes as C
import os
from typing import NamedTuple, Optional

import torch

from . import _lib, _timing


# ------------------------------------------------------------------------------------------------------------
# descriptor, maps, time grid
# ------------------------------------------------------------------------------------------------------------
def rollout_desc(B, T, N, H, W, integrator, *, consts=None, Iinv=None, n_tracks=0, layout=_lib.MF_LAYOUT_BATCH_MAJOR, map_shared=0,
                 block=0, skip_snap=0, points_per_lane=0, math_mode=_lib.MF_MATH_FAST, force_stride=0):
    """`MfRolloutDesc` from explicit arguments.  `consts`: the physics constants by the struct's field names (mass, gravity, stiffness,
    damping, omega_max, grid_res, d_max, dt, robot_size_y); `Iinv`: nine host scalars, row-major.  A descriptor that only asks a policy
    query leaves both out.  The per-launch fields (strides of the controls, default_state, joints, path cost, grad_copies) are the
    caller's to set on the result."""
    d = _lib.MfRolloutDesc(B=B, T=T, N=N, H=H, W=W, n_tracks=n_tracks, integrator=integrator, layout=layout, map_shared=map_shared,
                           block=block, skip_snap=skip_snap, points_per_lane=points_per_lane, math_mode=math_mode,
                           force_stride=force_stride, **(consts or {}))
    if Iinv is not None:
        for i, v in enumerate(Iinv):
            d.Iinv[i] = v
    return d


def is_shared_map(t):
    """True if a [B,H,W] map is one [H,W] map broadcast over the batch (`expand`, stride 0) -- read once, not B times."""
    return t.dim() == 3 and (t.shape[0] == 1 or t.stride(0) == 0)


def canonical_maps(z, mu, B):
    """(z, mu, B) -> (z_kernel, mu_kernel, shared): ONE [H,W] map pair when both maps are shared by the B rollouts ([1,H,W], or an
    `expand` of it: stride 0), else contiguous [B,H,W] maps; `mu` may be None."""
    assert z.dim() == 3, f'z_grid must be [B,H,W] (or [1,H,W] = one map shared by all rollouts), got {tuple(z.shape)}'
    _, H, W = z.shape
    for name, m in (('z_grid', z), ('friction', mu)):
        if m is None:
            continue
        assert m.dim() == 3 and tuple(m.shape[-2:]) == (H, W), \
            f'{name} shape {tuple(m.shape)} does not match the {H}x{W} height grid'
        assert m.shape[0] in (1, B), f'{name} batch {m.shape[0]} is neither 1 (shared map) nor the {B} rollouts of controls'
    if is_shared_map(z) and (mu is None or is_shared_map(mu)):
        return z[0].contiguous(), (None if mu is None else mu[0].contiguous()), True
    # one map shared, the other per rollout: the kernels index both at b*H*W, so the shared one is expanded for real
    return z.expand(B, H, W).contiguous(), (None if mu is None else mu.expand(B, H, W).contiguous()), False


_TIME_GRIDS = {}


def time_grid(t_sim, full_len, n, dtype, dev):
    """The reference's grid: linspace(0, t_sim, full_len)[:n] (dphysics.py:166-167, 581).  Built once per configuration: a
    host-to-device copy is not allowed while a stream is capturing."""
    key = (float(t_sim), int(full_len), int(n), dtype, str(dev))
    if key not in _TIME_GRIDS:
        _TIME_GRIDS[key] = torch.linspace(0, t_sim, full_len, dtype=dtype)[:n].to(dev).contiguous()
    return _TIME_GRIDS[key]


# ------------------------------------------------------------------------------------------------------------
# the gradient copies of a shared map
# ------------------------------------------------------------------------------------------------------------
# private copies of a shared map's gradient (2 x 256 KiB each at 256x256); MF_GRAD_COPIES overrides (tuning)
# (c3, 1024 rollouts x 4 points, streaming backward: 16 / 32 / 64 copies -> kernel 0.218 / 0.210 / 0.207 ms, step 0.3865 / 0.3831 /
#  0.3887 ms -- the reduction over the copies grows with them: 32)
GRAD_COPIES = int(os.environ.get('MF_GRAD_COPIES', '32'))


def grad_copies_for(B, N):
    """Private gradient copies of a shared map for B rollouts of an N-point body.  Bodies of up to 4 points: ~64 rollouts per copy
    between GRAD_COPIES (32) and 256.  Larger bodies put N points of every
    rollout on nearly the same cells (the rollouts of a batch start from one pose): at least 64 copies -- measured with
    tools/ab_grad_copies.py, backward kernel at 16 / 64 / 256 copies: 256 x 223 points 1.20 / 0.94 / 0.88 ms, 1024 x 32 points
    0.98 / 0.81 / 0.78 ms, 64 x 223 0.91 / 0.85 / 0.85 ms (one copy per rollout) -- 64, not 256: the zero fill and the
    reduction over the copies grow with them (2 x 256 KiB each at 256 x 256)."""
    # (... and more with the number of points in flight: 2048 x 32 points 1.33 ms at 64 copies, 1.19 at 256; 1024 x 64: 0.86 / 0.77)
    floor = GRAD_COPIES if N <= 4 else max(GRAD_COPIES, min(256, max(64, (B * N) // 512)))
    return max(1, min(max(floor, B // 64), 256, B))


class GradPool:
    """The private gradient copies of a shared-map backward, [n_maps][copies][H*W] + 16 zeros (the row absent upstream
    gradients point at), kept ZEROED between steps: `mf_reduce_grad_copies_*` sums the copies and clears them in one launch, so a
    step pays neither the zero fill nor a separate reduction (~10 us of dependent-launch latency each at the BASELINE shape).
    `busy` is set while a backward is between its kernel launch and the reduction; a pool found busy (an exception in between,
    or two streams at once) is not trusted and gets refilled.
    `pinned`: a hipGraph capture used this pool -- its address is baked into the graph, so the pool must outlive every replay
    (`grad_pool` never evicts it).  `done` is an event recorded behind the last reduction: a later acquire on ANOTHER stream
    waits for it before it clears the buffer."""

    def __init__(self, n_maps, copies, n, dt, dev):
        self.n_maps, self.copies, self.n = n_maps, copies, n
        self.buf = torch.zeros(n_maps * copies * n + 16, dtype=dt, device=dev)
        self.busy = False
        self.stream = None
        self.pinned = False
        self.done = None

    def acquire(self):
        cur_s = torch.cuda.current_stream(self.buf.device)
        cur = cur_s.cuda_stream
        capturing = torch.cuda.is_current_stream_capturing()
        self.pinned = self.pinned or capturing
        if self.busy or (self.stream is not None and self.stream != cur):
            if self.done is not None and not capturing:
                cur_s.wait_event(self.done)       # the other stream's scatter / reduction may still be in flight
            self.buf.zero_()
        self.busy, self.stream = True, cur

    def reduce(self, map_shape):
        # one spare scalar behind the maps: a data-parallel caller puts its loss there and exchanges gradients and loss with
        # ONE collective on this buffer, no pack / unpack (train.py::TerrainFitProblem)
        flat = torch.empty(self.n_maps * self.n + 1, dtype=self.buf.dtype, device=self.buf.device)
        out = flat[:-1].view((self.n_maps,) + tuple(map_shape))
        # (a direct call, not `_lib.launch`: the reduction goes on the stream taken at `acquire` -- the one the scatter ran on --, not the current one)
        fn = getattr(_lib.lib(), 'mf_reduce_grad_copies_' + _lib.scalar_suffix(self.buf.dtype))
        _lib.check(fn(*_lib.c_args(self.buf, self.n_maps, self.copies, C.c_longlong(self.n), out), C.c_void_p(self.stream)),
                   'mf_reduce_grad_copies')
        if not torch.cuda.is_current_stream_capturing():
            if self.done is None:
                self.done = torch.cuda.Event()
            self.done.record(torch.cuda.current_stream(self.buf.device))
        self.busy = False
        return out


MAX_IDLE_POOLS = 4      # per owner; pools a captured graph references are kept on top of these


def grad_pool(owner, n_maps, copies, n, dt, dev):
    """The owner's (a DPhysics module's) pool for this shape, acquired for one backward.  Shapes come and go (tests, sweeps), so
    the least recently used pools beyond MAX_IDLE_POOLS are dropped -- never one a hipGraph capture has used (`pinned`: the
    graph replays into its address) and never one between its scatter and its reduction."""
    pools = owner.__dict__.setdefault('_grad_pools', {})
    key = (n_maps, copies, n, dt, dev)
    p = pools.pop(key, None)
    if p is None:
        idle = [k for k, q in pools.items() if not q.pinned and not q.busy]
        for k in idle[:max(len(idle) - (MAX_IDLE_POOLS - 1), 0)]:       # dicts keep insertion order: oldest first
            del pools[k]
        p = GradPool(n_maps, copies, n, dt, dev)
    pools[key] = p                                 # (re-)inserted last = most recently used
    p.acquire()
    return p


# ------------------------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------------------------
def loss_struct(spec, X_gt=None, flags=0, **tensors):
    """`MfRolloutLoss` for a `LossSpec`: the named tensors (partial, ticket, loss, gloss, Xs) become its pointers; with `X_gt` the
    ground truth and the spec's stamp tables ride along.  The struct keeps its tensors alive."""
    s = _lib.MfRolloutLoss(T2=spec.T2, flags=flags, **{k: _lib.ptr(t) for k, t in tensors.items()})
    if X_gt is not None:
        s.gt, s.near, s.w, s.row_stamp, s.row_w = (_lib.ptr(t) for t in (X_gt, spec.near, spec.w, spec.row_stamp, spec.row_w))
    s.keep = (X_gt, tensors)
    return s


def record_bytes(desc, dtype):
    """Bytes of the per-step record the forward of `desc` keeps for its backward (MfRolloutFwdBufs.rec); 0: this launch keeps none.
    (float64: the validation build of the component-parallel kernels, 32-byte quads)"""
    rb = _lib.lib().mf_rollout_record_bytes if dtype == torch.float32 else _lib.lib().mf_rollout_record_bytes_f64
    return int(rb(C.byref(desc)))


def loss_fusable(desc):
    """Which launches of `desc` can carry physics_loss themselves: one of the MF_LOSS_FUSE_* answers of _lib.py."""
    return int(_lib.lib().mf_rollout_loss_fusable(C.byref(desc)))


def bwd_window(desc):
    """True if the backward of `desc` sends its cell gradients through per-workgroup LDS windows (saturated positions-only launches)."""
    return bool(_lib.lib().mf_rollout_bwd_window(C.byref(desc)))


def bwd_wants_gcontrols(desc):
    """True if the backward kernels chosen for `desc` cannot leave the control gradient out."""
    return bool(_lib.lib().mf_rollout_bwd_wants_gcontrols(C.byref(desc)))


def fwd_stages_zmu(desc):
    """True if the forward of `desc` fills `zmu_scratch` with the interleaved (z, mu) pair: its backward may read it as `zmu`."""
    return bool(_lib.lib().mf_rollout_fwd_stages_zmu(C.byref(desc)))


def default_state(controls, x, xd, R, w):
    """One `mf_rollout_default_state_*` launch: the start state of contiguous `controls` [B,T,2] (x = 0, xd = (v_0, 0, 0), R = I,
    omega = (0, 0, w_0)) written into the four buffers."""
    _lib.launch('mf_rollout_default_state', controls.device, C.c_int32(x.shape[0]), C.c_int32(controls.shape[1]), controls, x, xd, R, w,
                dtype=controls.dtype)


class ForwardBufs(NamedTuple):
    """What one forward launch wrote, in the descriptor's layout and at the kernel's force stride; None = not asked for."""
    Xs: torch.Tensor
    Rs: torch.Tensor
    Xds: Optional[torch.Tensor] = None
    Om: Optional[torch.Tensor] = None
    Fs: Optional[torch.Tensor] = None
    Ff: Optional[torch.Tensor] = None
    Xraw: Optional[torch.Tensor] = None
    rec: Optional[torch.Tensor] = None
    cost_rows: Optional[torch.Tensor] = None
    path_cost: Optional[torch.Tensor] = None


def launch_forward(desc, z, mu, controls, ts, points, part, state, *, want_forces=True, want_xraw=False, want_rec=False,
                   joint_angles=None, zmu_scratch=None, zmu=None, pose_rows=0, loss=None):
    """One `mf_rollout_fwd_*` launch.  `z`, `mu`: the maps as `canonical_maps` returns them; `state` = (x0, xd0, R0, w0), x0
    receives the snapped height.  `want_rec`: keep the per-step record for the backward where the library says it pays
    (MfRolloutFwdBufs.rec; 1 KiB per rollout and step for the component-parallel kernels).  `pose_rows` > 0 is the path-cost mode
    (desc.pose_stride): the launch writes cost rows, the path cost and `pose_rows` poses instead of the states and forces.
    `loss`: a `loss_struct`.  Reads the force stride into the descriptor, allocates, launches; returns `ForwardBufs`."""
    dt, dev = z.dtype, z.device
    B, T = desc.B, desc.T
    lead = (T, B) if desc.layout == _lib.MF_LAYOUT_TIME_MAJOR else (B, T)
    new = lambda *tail: torch.empty(*lead, *tail, dtype=dt, device=dev)  # noqa: E731
    if pose_rows:
        out = ForwardBufs(Xs=torch.empty(pose_rows, B, 3, dtype=dt, device=dev), Rs=torch.empty(pose_rows, B, 3, 3, dtype=dt, device=dev),
                          cost_rows=new(4), path_cost=torch.empty(B, dtype=dt, device=dev))
    else:
        Np = _lib.lib().mf_rollout_force_stride(C.byref(desc))      # point slots per force row the chosen kernel writes
        if Np < desc.N:
            raise RuntimeError('mf_rollout_force_stride rejected the descriptor')
        desc.force_stride = Np
        nbytes = record_bytes(desc, dt) if want_rec else 0
        rec = torch.empty(nbytes // dt.itemsize, dtype=dt, device=dev) if nbytes > 0 else None
        out = ForwardBufs(Xs=new(3), Rs=new(3, 3), Xds=new(3), Om=new(3), Fs=new(Np, 3) if want_forces else None,
                          Ff=new(Np, 3) if want_forces else None, Xraw=new(3) if want_xraw else None, rec=rec)
    x0, xd0, R0, w0 = state
    p = _lib.ptr
    bufs = _lib.MfRolloutFwdBufs(
        z=p(z), mu=p(mu), controls=p(controls), ts=p(ts), points=p(points), part=p(part), x0=p(x0), xd0=p(xd0), R0=p(R0), w0=p(w0),
        Xs=p(out.Xs), Xds=p(out.Xds), Rs=p(out.Rs), Omegas=p(out.Om), Fs=p(out.Fs), Ff=p(out.Ff), Xraw=p(out.Xraw),
        joint_angles=p(joint_angles), cost_rows=p(out.cost_rows), path_cost=p(out.path_cost), zmu_scratch=p(zmu_scratch), zmu=p(zmu),
        rec=p(out.rec), loss=None if loss is None else C.addressof(loss))       # (`loss` stays alive until the call below returns)
    _lib.launch('mf_rollout_fwd', dev, desc, bufs, dtype=dt, timer='rollout_fwd_kernel')
    _timing.note_launch('rollout_fwd_kernel')
    return out


class BackwardGrads(NamedTuple):
    """What one backward launch wrote: `gz` / `gmu` [H,W] (shared maps, summed over the copies) or [B,H,W]; None = not asked for."""
    gz: torch.Tensor
    gmu: Optional[torch.Tensor]
    gcontrols: Optional[torch.Tensor]
    gx0: Optional[torch.Tensor]
    gxd0: torch.Tensor
    gR0: torch.Tensor
    gw0: torch.Tensor
    gjoint_angles: Optional[torch.Tensor]


def launch_backward(desc, z, mu, controls, ts, points, part, state, saved, ups, *, pool_owner, want_gmu=True, want_gcontrols=True,
                    want_gx0=True, joint_angles=None, want_gjoint_angles=False, rec=None, zmu_scratch=None, zmu=None, loss=None):
    """One `mf_rollout_bwd_*` launch (+ the reduction over a shared map's gradient copies).  `state` = (x_init, xd0, R0, w0) with
    the SNAPPED start position; `saved` = (Xraw, Xds, Rs, Om) in the descriptor's layout; `ups` = the six upstream gradients
    (gXs, gXds, gRs, gOm, gFs, gFf) as autograd hands them out, [B,T,...], None = absent (NULL = zeros).  Shared maps: the launch
    scatters into `desc.grad_copies` private copies -- the CALLER's count -- taken from `pool_owner`'s `GradPool`.  Returns
    `BackwardGrads`."""
    dt, dev = controls.dtype, controls.device
    tm = desc.layout == _lib.MF_LAYOUT_TIME_MAJOR
    # upstream gradient -> the kernel's layout, contiguous; None stays NULL (= zeros)
    ups = [None if g is None else (g.to(dt).transpose(0, 1) if tm else g.to(dt)).contiguous() for g in ups]
    want_gmu = want_gmu and mu is not None
    if desc.map_shared:
        # private gradient copies: rollout b scatters into copy b % copies, summed below (same-address atomics serialise)
        # one zero fill for [gz copies | gmu copies | the zero row absent upstream gradients point at]
        n_maps, copies = (2 if want_gmu else 1), desc.grad_copies
        pool = grad_pool(pool_owner, n_maps, copies, z.numel(), dt, dev)
        maps = pool.buf[:n_maps * copies * z.numel()].view((n_maps, copies) + tuple(z.shape))
        gz, gmu, zero_row = maps[0], (maps[1] if want_gmu else None), pool.buf[-16:]
    else:
        gz = torch.zeros_like(z)
        gmu = torch.zeros_like(mu) if want_gmu else None
        zero_row = torch.zeros(16, dtype=dt, device=dev)
    x_init, xd0, R0, w0 = state
    gcontrols = torch.empty_like(controls) if want_gcontrols else None
    gxd0, gR0, gw0 = torch.empty_like(xd0), torch.empty_like(R0), torch.empty_like(w0)
    gx0 = torch.empty_like(xd0) if want_gx0 else None
    # (zeros: the default integrator never reads its last row of angles, and the kernel does not write that gradient row)
    gja = torch.zeros_like(joint_angles) if want_gjoint_angles and joint_angles is not None else None
    p = _lib.ptr
    bufs = _lib.MfRolloutBwdBufs(
        z=p(z), mu=p(mu), controls=p(controls), ts=p(ts), points=p(points), part=p(part), x_init=p(x_init), xd0=p(xd0), R0=p(R0),
        w0=p(w0), Xraw=p(saved[0]), Xds=p(saved[1]), Rs=p(saved[2]), Omegas=p(saved[3]),
        gXs=p(ups[0]), gXds=p(ups[1]), gRs=p(ups[2]), gOmegas=p(ups[3]), gFs=p(ups[4]), gFf=p(ups[5]), zeros=p(zero_row),
        gz=p(gz), gmu=p(gmu), gcontrols=p(gcontrols), gx0=p(gx0), gxd0=p(gxd0), gR0=p(gR0), gw0=p(gw0),
        joint_angles=p(joint_angles), gjoint_angles=p(gja), rec=p(rec), zmu_scratch=p(zmu_scratch), zmu=p(zmu),
        loss=None if loss is None else C.addressof(loss))
    _lib.launch('mf_rollout_bwd', dev, desc, bufs, dtype=dt, timer='rollout_bwd_kernel')
    _timing.note_launch('rollout_bwd_kernel')
    if desc.map_shared:
        summed = pool.reduce(z.shape)          # one launch: both maps summed over their copies, the pool left zeroed
        gz, gmu = summed[0], (summed[1] if want_gmu else None)
    return BackwardGrads(gz, gmu, gcontrols, gx0, gxd0, gR0, gw0, gja)
