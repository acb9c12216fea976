"""Cases, referee and harness of tests/test_state_grads_gpu.py: the gradients every rollout backward route hands back for the START state
(gx0, gxd0, gR0, gw0 -- the epilogues of rollout_bwd_kernel.h, rollout_bwd_mw_kernel.h and rollout_bwd_cp_kernel.h, each with the adjoint of
the terrain snap) against the float64 oracle's autograd over the same four leaves.

State gradients are per rollout, so the oracle differentiates n <= 8 DISTINCT rollouts (their own start state from `given_state(n)`, controls,
and map pair where the maps are per rollout); HIP rollout b is a copy of distinct rollout b mod n, the upstream weights are generated for
(n, T, ...) and indexed the same way, and ALL B rollouts are compared with oracle row b mod n.

A case names the route of tests/golden/rollout_routes_gpu.json whose backward kernel it must run; B is the smallest batch that reaches the
route on the MI355X (the thresholds of csrc/rollout_route.hip) plus a ragged tail, so that the last wave or workgroup is partial.
Importable without a GPU."""
import contextlib
import functools
import json
import os

import numpy as np
import torch

from oracle import dphysics_oracle as orc
from tests import helpers as hp
from tests.golden_state import given_state

DEV = 'cuda'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, 'tests', 'golden', 'rollout_routes_gpu.json')
GRID_RES, D_MAX = 0.1, 3.2      # 64 x 64 maps
GRADS = ('gx0', 'gxd0', 'gR0', 'gw0')
F64_BAR, F32_FLOOR, ENVELOPE = 1e-8, 2e-4, 3.0
STREAM_T, OTHER_T = (1, 2, 14), (1, 6)

# Thresholds of rollout_route.hip on the MI355X (256 CUs, 1024 SIMDs), in rollouts of the <= 4-point body (four per wave):
#   <= 1024 (256 workgroups, one per CU): twelve-slot ring       <= 2048 (512 workgroups): six-slot ring
#   <= 4096 (1024 waves): a record is kept / late recompute      <= 8192 (2048 waves): end of the component-parallel backward
#   beyond (xs_bwd_min_waves = 512 waves = 8192 rollouts x 4 lanes): the one-point-per-lane kernels, XS_ONLY for a positions-only upstream
# +1: one rollout in the last wave.  The component-parallel window form takes whole 512-thread workgroups only (32 rollouts; the planner
# asks threads % 512 == 0): 4128 is the smallest such B beyond 4096.  The one-point-per-lane windows take a partial workgroup.
# `rec=False`: the forward keeps no record (MfRolloutFwdBufs.rec = NULL, what a C-ABI caller may do): the module always offers one, and with
# it an 8-point body goes to the multi-wave kernels and the float64 validation build to its streaming form.
# `interleave=False` (DPhysics.interleave_maps): the shared maps are read as they are, the route the fixture names; the module's default
# offers the interleaved (z, mu) copy, which the saturated positions-only kernels take (ZMU: `xs_win256_zmu`).
_CP, _P1 = 'rollout_bwd_cp_kernel', 'rollout_bwd_kernel'
CASES = {
    # component-parallel, float32
    'cp_rec_stream12': dict(B=5, T=STREAM_T, integ=(1,)),
    'cp_rec_stream12_n3': dict(route='cp_rec_stream12', B=5, N=3, T=STREAM_T, integ=(1,)),      # an absent point in the 16-lane row
    'cp_rec_stream12_xs': dict(B=5, T=STREAM_T, integ=(1,), up='xs', shared=True),
    'cp_rec_stream6': dict(B=1025, T=STREAM_T, integ=(1,)),
    'cp_rec_stream_dyn': dict(B=5, T=STREAM_T, integ=(0,), shared=True),
    'cp_rec_saved': dict(B=2049, integ=(1,)),
    'cp_rec_saved_zmu': dict(B=2049, integ=(1,), shared=True),
    'cp_dyn_late': dict(B=1025, integ=(0,)),
    'cp_early': dict(B=4097),
    'cp_early_win': dict(B=4128, shared=True),          # whole workgroups: the smallest admissible B
    'cp_early_win_xs': dict(B=4128, shared=True, up='xs'),
    'cp_loss_in_bwd_euler': dict(B=5, T=STREAM_T, integ=(1,), up='loss', shared=True),
    'cp_loss_in_bwd': dict(B=5, T=STREAM_T, integ=(0,), up='loss', shared=True),
    'cp_loss_one1': dict(B=4097, up='loss'),
    'cp_loss_one1_win': dict(B=4128, up='loss', shared=True),      # whole workgroups: the smallest admissible B
    # one point per lane, float32 fast math
    'fast_general': dict(B=5, N=8, rec=False),
    'ppl4_fast': dict(B=5, N=8, ppl=4),
    'split_carry': dict(B=8193),
    'xs': dict(B=8193, up='xs'),
    'xs_win256': dict(B=8193, up='xs', shared=True, interleave=False),
    'xs_win256_zmu': dict(route='py_mod_xs_saturated', B=8193, up='xs', shared=True),      # ... as the module runs it: the shared maps interleaved
    'xs_win512': dict(B=32769, up='xs', shared=True, interleave=False),
    'xs_loss': dict(B=8193, up='loss'),
    'xs_win_loss': dict(B=8193, up='loss', shared=True, interleave=False),
    'xs_ppl': dict(B=513, N=223, up='xs'),
    'carry_ppl': dict(B=513, N=223),
    # articulated (marv body, non-zero joint angles)
    'joints_fast': dict(B=5, N=8, joints=True),
    'joints_exact': dict(B=5, N=8, joints=True, precise=True),
    'f64_joints': dict(B=5, N=8, joints=True, f64=True),
    # exact
    'exact': dict(B=5, precise=True),
    'f64_exact': dict(B=5, f64=True),
    # one rollout over several lanes / waves from the forward's record
    'mw_rec': dict(B=3, N=32),
    'mw_rec_xs': dict(B=3, N=32, up='xs'),
    'mw_rec_tile': dict(B=3, N=223),
    'mw_rec_dyn': dict(B=3, N=16, integ=(0,)),
    # float64 validation builds of the fast kernels (points_per_lane = 16)
    'f64_cp_stream': dict(B=5, T=STREAM_T, integ=(1,), f64=True, ppl=16),
    'f64_cp_saved': dict(B=5, integ=(0,), f64=True, ppl=16),
    'f64_cp_late': dict(B=5, f64=True, ppl=16, rec=False),
    'f64_cp_states': dict(B=5, f64=True, ppl=16, rec=False, up='xs', forces=False),
    'f64_mw': dict(B=3, N=32, f64=True, ppl=16),
}
_DEFAULTS = dict(route=None, N=4, T=OTHER_T, integ=(1, 0), up='all', shared=False, ppl=0, rec=True, joints=False, precise=False, f64=False,
                 forces=True, snap=True, interleave=True)


def case(name, **over):
    c = dict(_DEFAULTS, name=name)
    c.update(CASES[name])
    c.update(over)
    c['route'] = c['route'] or name
    return c


def case_ids():
    """(name, T, integ) of every parametrised run."""
    return [(name, T, integ) for name in CASES for integ in case(name)['integ'] for T in case(name)['T']]


# ----------------------------------------------------------------------------------------------------------------------------------
# the route a case must take
# ----------------------------------------------------------------------------------------------------------------------------------
def _template(launch):
    """('rollout_bwd_cp_kernel', [template arguments]) of an mf_last_launch() text or a fixture entry's kernel name."""
    head = launch.split(' grid=')[0]
    kern, args = head.split('<')
    return kern.split('::')[-1], args.rstrip('>').split(', ')


def expected_template(c, integ):
    """The fixture's kernel template for the case's route with this run's integrator.  The component-parallel kernels' fourth argument
    (GCTRL: a control gradient is wanted) is not part of the route -- the module asks for it whenever the controls require grad, the
    fixture's C-ABI launches do not -- and reads '*'."""
    entry = json.load(open(FIXTURE))[c['route']]['bwd']
    kern, args = _template(entry['launch'] if isinstance(entry, dict) else entry[1])      # (the module's own cases keep 'kernel<..> grid=.. block=..')
    args[{_CP: 1, _P1: 3}.get(kern, 4)] = str(integ)      # rollout_bwd_mw_kernel<S, G, XS_ONLY, TILE, INTEG>
    if kern == _CP:
        args[3] = '*'
    return kern, args


def assert_route(c, integ, launch):
    kern, args = _template(launch)
    if kern == _CP:
        args[3] = '*'
    assert (kern, args) == expected_template(c, integ), (c['name'], launch, 'expected', expected_template(c, integ))


# ----------------------------------------------------------------------------------------------------------------------------------
# the problem: n distinct rollouts in float64, cast and tiled for the device
# ----------------------------------------------------------------------------------------------------------------------------------
def body(c):
    from monoforce_amd import synthetic as syn
    if c['joints']:
        pts, masks = syn.robot_points_box(c["N"], seed=15, n_tracks=4)      # (a seed that puts a point on every flipper)
        assert all(int(m.sum()) >= 1 for m in masks)
        return pts, masks
    if c['N'] <= 4:
        pts, masks = syn.robot_points_4()
        return pts[:c['N']], [m[:c['N']] for m in masks]
    return syn.robot_points_box(c['N'], seed=c['N'], n_tracks=2)


def make_spec(c, integ):
    pts, masks = body(c)
    spec = hp.spec_from(pts, masks, integ, GRID_RES, D_MAX)
    if c['joints']:
        from monoforce_amd.dphys_config import DPhysConfig
        cfg = DPhysConfig(robot='marv', grid_res=GRID_RES, robot_points=pts, driving_parts=np.stack(masks))
        spec.joint_positions = [list(v) for v in cfg.joint_positions.values()]
    return spec


def make_module(c, integ, **kw):
    """The DPhysics module of a case (a marv body for the articulated ones)."""
    from monoforce_amd.dphys_config import DPhysConfig
    from monoforce_amd.dphysics import DPhysics
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = body(c)
    opts = dict(points_per_lane=c['ppl'], precise=c['precise'], return_forces=c['forces'], snap_to_terrain=c['snap'])
    opts.update(kw)
    if not c['joints']:
        dp = make_dphysics(pts, masks, integ, GRID_RES, D_MAX, **opts)
        dp.interleave_maps = c['interleave']
        return dp
    cfg = DPhysConfig(robot='marv', grid_res=GRID_RES, robot_points=pts, driving_parts=np.stack(masks))
    cfg.robot_mass = 40.0
    cfg.damping = float(np.sqrt(4 * cfg.robot_mass * cfg.stiffness))
    cfg.d_max, cfg.use_odeint = D_MAX, (integ == 1)
    return DPhysics(cfg, device=DEV, **opts)


def stamps_of(T):
    """Output rows that carry a ground-truth stamp: always row 0 -- with the default integrator the start state itself, whose dL/dXs goes
    straight into the epilogue -- and the last row."""
    return sorted({0, T // 3, T - 1})


@functools.lru_cache(maxsize=None)
def _problem(n, T, shared, joints, snap, N):
    from monoforce_amd import synthetic as syn
    m = 1 if shared else n
    z = torch.stack([syn.bump_terrain(syn.bump_params(20 + k), D_MAX, GRID_RES, torch.float64) * 0.3 for k in range(m)])
    mu = torch.stack([syn.wave_friction(D_MAX, GRID_RES, 0.5, 1.0, 1.0 + 0.2 * k, 0.8, torch.float64) for k in range(m)])
    ctrl = syn.varying_controls(n, max(T, 2), seed=4, dtype=torch.float64)[:, :T].contiguous()
    state = [s.clone() for s in given_state(n)]
    if not snap:     # the start height is the caller's: half a centimetre above where the snap would have put the 4-point body in this pose
        x = state[0]
        P = torch.as_tensor(syn.robot_points_4()[0], dtype=torch.float64)
        p0 = P.unsqueeze(0) @ state[2].transpose(1, 2) + x.unsqueeze(1)
        x[:, 2] = orc.sample_grid(z.expand(n, -1, -1), p0[..., 0], p0[..., 1], D_MAX, GRID_RES).mean(1) + 0.005
    ja = None
    if joints:
        tt = torch.linspace(0, 1, max(T, 2), dtype=torch.float64).view(1, -1, 1)[:, :T]
        ja = 0.5 * torch.sin(2 * np.pi * (tt * torch.tensor([0.9, 1.2, 0.6, 1.5]) + torch.arange(n).view(n, 1, 1) * 0.15)) + 0.1
    gen = torch.Generator().manual_seed(7)
    gt = state[0].unsqueeze(1) + 0.2 * (torch.rand(n, len(stamps_of(T)), 3, generator=gen, dtype=torch.float64) - 0.5)
    return dict(z=z, mu=mu, ctrl=ctrl, state=tuple(state), ja=ja, gt=gt)


def problem(c, T):
    """The n = min(B, 8) distinct rollouts of a case in float64 (cached; nobody writes into it)."""
    return _problem(min(c['B'], 8), T, c['shared'], c['joints'], c['snap'], c['N'])


def upstream_weights(n, T, N, dtype):
    """probe_loss's weights for the six outputs of n rollouts: (n, T, ...) each."""
    from monoforce_amd import synthetic as syn
    shapes = [(n, T, 3), (n, T, 3), (n, T, 3, 3), (n, T, 3), (n, T, N, 3), (n, T, N, 3)]
    return [syn.probe_weights(s, phase=0.5 + i, dtype=dtype) for i, s in enumerate(shapes)]


def upstream_loss(outs, up, idx, n, T, N, dtype):
    """'all': helpers.probe_loss over the six outputs; 'xs': probe weights on Xs only.  Row b of the outputs meets the weights of distinct
    rollout idx[b]."""
    from monoforce_amd import synthetic as syn
    dev = outs[0].device
    if up == 'xs':
        return (outs[0] * syn.probe_weights((n, T, 3), phase=0.4, dtype=dtype)[idx].to(dev)).sum()
    scales = [1.0, 1.0, 1.0, 1.0, 1e-3, 1e-3]
    loss = 0
    for o, w, s in zip(outs, upstream_weights(n, T, N, dtype), scales):
        loss = loss + (o * w[idx].to(dev)).sum() * s
    return loss


# ----------------------------------------------------------------------------------------------------------------------------------
# the referee
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(name, over, T, integ, f32):
    c = case(name, **dict(over))
    dtype = torch.float32 if f32 else torch.float64
    p = problem(c, T)
    n = p['ctrl'].shape[0]
    spec = make_spec(c, integ)
    leaves = [t.clone().to(dtype).requires_grad_(True) for t in p['state']]
    st = [leaves[0] * 1.0] + leaves[1:]                      # non-leaf: the in-place snap is legal on it
    ja = None if p['ja'] is None else p['ja'].to(dtype)
    so, fo = orc.rollout(spec, p['z'].to(dtype).expand(n, -1, -1), p['ctrl'].to(dtype), state=tuple(st),
                         friction=p['mu'].to(dtype).expand(n, -1, -1), joint_angles=ja, snap=c['snap'])
    if c['up'] == 'loss':        # physics_loss on the stamped rows: the weighted mean over ALL B rollouts' terms (the copies' are equal)
        stamps = stamps_of(T)
        full_ts = torch.linspace(0, 5.0, 500)[:T]
        w = (1. / (1. + 0.9 * full_ts[stamps].to(dtype))).view(1, -1, 1)
        loss = ((so[0][:, stamps] * w - p['gt'].to(dtype) * w) ** 2).sum() / (c['B'] * len(stamps) * 3)
    else:
        loss = upstream_loss(list(so) + list(fo), c['up'], torch.arange(n), n, T, c['N'], dtype)
    loss.backward()
    return tuple((torch.zeros_like(l) if l.grad is None else l.grad).double() for l in leaves)


def oracle_grads(c, T, integ, dtype=torch.float64):
    """(gx0, gxd0, gR0, gw0) [n, ...] of the oracle's autograd in `dtype`, as float64 tensors (cached)."""
    over = tuple(sorted((k, v) for k, v in c.items() if k != 'name' and CASES[c['name']].get(k, _DEFAULTS.get(k)) != v
                        and not (k == 'route' and v == c['name'])))
    return _oracle(c['name'], over, T, integ, dtype == torch.float32)


# ----------------------------------------------------------------------------------------------------------------------------------
# the harness
# ----------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _no_record(off):
    """The forward launches inside keep no per-step record for their backward."""
    from monoforce_amd import rollout_launch as rl
    if not off:
        yield
        return
    keep = rl.record_bytes
    rl.record_bytes = lambda desc, dtype: 0
    try:
        yield
    finally:
        rl.record_bytes = keep


def run_hip(c, T, integ, *, leaves=(True, True, True, True), controls_grad=True, entry='module', dp=None):
    """One forward + backward of a case through DPhysics (entry='ops': monoforce_amd.ops.rollout on the same module).
    Returns ([gx0, gxd0, gR0, gw0] on the host, None where the tensor did not require grad; the backward's mf_last_launch() text)."""
    from monoforce_amd import _timing, ops
    dtype = torch.float64 if c['f64'] else torch.float32
    p = problem(c, T)
    B, n = c['B'], p['ctrl'].shape[0]
    idx = torch.arange(B) % n
    dp = dp or make_module(c, integ)
    tile = lambda t: t.to(dtype).to(DEV)[idx.to(DEV)].contiguous()      # noqa: E731
    maps = lambda t: t.to(dtype).to(DEV) if c['shared'] else tile(t)    # noqa: E731  ([1,H,W]: one pair shared by all rollouts)
    z, mu = maps(p['z']), maps(p['mu'])
    ctrl = tile(p['ctrl']).requires_grad_(controls_grad)
    ja = None if p['ja'] is None else tile(p['ja'])
    lv = [tile(t).requires_grad_(need) for t, need in zip(p['state'], leaves)]
    st = [lv[0] * 1.0 if leaves[0] else lv[0]] + lv[1:]      # x0 as a non-leaf: the forward writes the snapped height into it
    _timing.start(capacity=16)
    with _no_record(not c['rec']):
        if c['up'] == 'loss':
            stamps = stamps_of(T)
            lspec = dp.loss_spec(torch.linspace(0, 5.0, 500)[:T][stamps], gamma=0.9, n_steps=T, dtype=dtype)
            loss = dp.physics_loss_rollout(z, ctrl, tile(p['gt']), lspec, state=tuple(st), friction=mu, value_in_backward=True)[0]
        else:
            if entry == 'ops':
                states, forces = ops.rollout(dp, z, ctrl, tuple(st), friction=mu)
            else:
                states, forces = dp(z, ctrl, joint_angles=ja, state=tuple(st), friction=mu)
            outs = list(states) + ([] if forces[0] is None else list(forces))
            loss = upstream_loss(outs, c['up'], idx, n, T, c['N'], dtype)
    loss.backward()
    launch = _timing.launches()['rollout_bwd_kernel']
    _timing.stop()
    return [None if l.grad is None else l.grad.double().cpu() for l in lv], launch


# ----------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------------------------------------------------------------
def _parts(gname, T, c):
    """The pieces of a gradient tensor held to the bar on their own, as (label, index into [B, ...]): the whole tensor; at T = 1 -- where
    the snap term is at least ~1e-2 of the gradient and a whole-tensor bar would hide it -- every row of gR0 and every component of gx0;
    without the snap the components of gx0 at every T (gx0.z must match)."""
    out = [(gname, (Ellipsis,))]
    if gname == 'gx0' and (T == 1 or not c['snap']):
        out += [(f'gx0.{"xyz"[k]}', (Ellipsis, k)) for k in range(3)]
    if gname == 'gR0' and T == 1:
        out += [(f'gR0[{k}]', (Ellipsis, k, slice(None))) for k in range(3)]
    return out


def compare(c, T, integ, got):
    """Rows (label, error of HIP vs the float64 oracle, the float32 oracle's own error -- None for a float64 run --, bar, ok) for the
    four gradients of ALL B rollouts; each rollout against oracle row b mod n.  An oracle piece that is exactly zero (gx0.z under the
    snap; gxd0 and gw0 when only row 0 of Xs carries gradient) must be exactly zero here."""
    r64 = oracle_grads(c, T, integ)
    r32 = None if c['f64'] else oracle_grads(c, T, integ, torch.float32)
    n = r64[0].shape[0]
    idx = torch.arange(c['B']) % n
    rows = []
    for k, gname in enumerate(GRADS):
        assert got[k] is not None and got[k].shape == r64[k][idx].shape, (gname, None if got[k] is None else got[k].shape)
        finite = bool(torch.isfinite(got[k]).all())
        for label, sel in _parts(gname, T, c):
            a, ref = got[k][sel], r64[k][idx][sel]
            if float(ref.abs().max()) == 0.0:
                err = float(a.abs().max())
                rows.append((label, err, None if r32 is None else float(r32[k][sel].abs().max()), 0.0, finite and err == 0.0))
                continue
            err = hp.rel_err(a, ref)
            env = None if r32 is None else hp.rel_err(r32[k][sel], r64[k][sel])
            bar = F64_BAR if r32 is None else max(F32_FLOOR, ENVELOPE * env)
            rows.append((label, err, env, bar, finite and err <= bar))
    if c['snap']:
        z = float(got[0][:, 2].abs().max())
        rows.append(('gx0.z == 0', z, None, 0.0, z == 0.0))
    return rows
