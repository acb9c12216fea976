"""Backward of the fused rollout on the module path: hands `_RolloutFn`'s saved tensors to `rollout_launch.launch_backward`
(`mf_rollout_bwd_*`, include/monoforce_hip.h) and maps the map gradients back to the inputs' own shapes.

Replaces the T x ~300-node autograd graph of the reference (`loss.backward()` through
`/root/reference/monoforce/src/monoforce/models/traj_predictor/dphysics.py:172-272,467-528`) with one kernel launch.
"""
import os

import torch

from . import _lib, rollout_launch as rl
from .rollout_launch import grad_copies_for      # (read through this module's name: tools/ab_grad_copies.py patches it here)

# LDS-window launches (0: as everywhere else).  Fit step at 16 384 / 32 768 rollouts, backward kernel at 256 / 64 / 32 copies: 0.969 / 1.004 /
# 1.059 and 1.524 / 1.536 / 1.632 ms (the windows' final adds meet in fewer copies) against 0.125 / 0.035 / 0.02 ms of reduction: 64
# (profiles/r6c_ab_step_copies.txt)
WIN_GRAD_COPIES = int(os.environ.get('MF_GRAD_COPIES_WIN', '64'))


def to_input_shape(g, shape, expanded):
    """Gradient of a map input in that input's own shape.  A per-rollout map given where the kernels ran shared maps
    cannot happen (`canonical_maps` expands); what can: a shared run ([H,W] gradient g) whose input was [1,H,W] -> g[None],
    or ONE map expanded over the batch (stride 0) -> autograd's ExpandBackward sums whatever [B,H,W] gradient it is
    handed, so it gets g/B as a stride-0 expand when B is a power of two (the division is then exact, and so is the
    B-fold sum where it runs pairwise; a row-by-row sum comes back within B - 1 roundings), and otherwise g in row 0
    and zeros elsewhere (exact for every B, costs the B x H x W buffer).  A per-rollout run whose input was one shared
    map (the other map was per-rollout) gets the sum over the rollouts."""
    if g is None:
        return None
    Bm = shape[0]
    if g.dim() == 3:                         # per-rollout gradient [B,H,W]
        if Bm == g.shape[0] and not expanded:
            return g
        gs_ = g.sum(0)                       # the input was ONE map ([1,H,W] or an expand of it)
        if Bm == 1:
            return gs_.unsqueeze(0)
        g = gs_
    if Bm == 1:
        return g.unsqueeze(0)
    if Bm & (Bm - 1) == 0:
        return (g / Bm).unsqueeze(0).expand(shape)
    full = torch.zeros(shape, dtype=g.dtype, device=g.device)
    full[0] = g
    return full


def rollout_backward(ctx, ups, gloss=None):
    """Gradients of (z, mu, controls, x, xd0, R0, w0, joint_angles) -- the tensor arguments of `_RolloutFn.apply`, in its order -- from
    the six upstream gradients `ups`, or from `gloss` when the forward carried physics_loss itself."""
    controls, x_init, xd0, R0, w0, ts, Xraw, Xds, Rs, Om, _z_in, _mu_in = ctx.saved_tensors      # (the maps as given: saved for their version check)
    desc, mod = ctx.desc, ctx.mod
    z, mu, points = ctx.maps
    dev, dt = controls.device, controls.dtype
    _, need_z, need_mu, need_controls, need_x, need_xd0, need_R0, need_w0, need_ja = ctx.needs_input_grad
    # (policy queries -- mf_rollout_bwd_wants_gcontrols, mf_rollout_bwd_window -- read the CU count of the CURRENT device: the tensors' device, throughout)
    with torch.cuda.device(dev):
        if desc.map_shared:
            # ~64 rollouts per copy (same-address atomics serialise), between GRAD_COPIES and 256 copies
            copies = grad_copies_for(desc.B, desc.N)
            # ... unless the launch sends its cell gradients through per-workgroup LDS windows (mf_rollout_bwd_window: saturated positions-only
            # launches): a workgroup adds its window to ONE copy once, at its end -- 256 copies cost a 0.125 ms reduction for 0.035 ms of kernel time
            if (WIN_GRAD_COPIES and dt == torch.float32 and (gloss is not None or ups[0] is not None) and all(u is None for u in ups[1:])
                    and rl.bwd_window(desc)):
                copies = min(copies, WIN_GRAD_COPIES)
            desc.grad_copies = copies
        # the control gradient is skipped where nobody wants it and the chosen kernels can leave it out (mf_rollout_bwd_wants_gcontrols)
        need_gc = need_controls or rl.bwd_wants_gcontrols(desc)      # (round 6: never forced by the library)
        lstruct = None
        if gloss is not None:       # the forward carried physics_loss itself (MfRolloutLoss): the kernel forms dL/dXs from Xs and the ground truth
            spec, X_gt, Xs_rows, loss_out = ctx.loss
            value = {}
            if loss_out is not None:       # MF_LOSS_VALUE_IN_BACKWARD: this launch also forms the value the forward left as NaN
                value = dict(flags=_lib.MF_LOSS_VALUE_IN_BACKWARD, partial=loss_out[1], ticket=spec.ticket(dev, torch.cuda.current_stream(dev)),
                             loss=loss_out[0])
            lstruct = rl.loss_struct(spec, X_gt, gloss=gloss.to(dt).reshape(1).contiguous(), Xs=Xs_rows, **value)
        g = rl.launch_backward(desc, z, mu, controls, ts, points, mod._part_dev(dev), (x_init, xd0, R0, w0), (Xraw, Xds, Rs, Om), ups,
                               pool_owner=mod, want_gmu=need_mu, want_gcontrols=need_gc, want_gx0=need_x, joint_angles=ctx.joint_angles,
                               want_gjoint_angles=need_ja, rec=ctx.rec, zmu_scratch=ctx.zmu[0], zmu=ctx.zmu[1], loss=lstruct)
    return (to_input_shape(g.gz, ctx.z_shape, ctx.z_expanded) if need_z else None, to_input_shape(g.gmu, ctx.mu_shape, ctx.mu_expanded),
            g.gcontrols if need_controls else None, g.gx0, g.gxd0 if need_xd0 else None, g.gR0 if need_R0 else None,
            g.gw0 if need_w0 else None, g.gjoint_angles)
