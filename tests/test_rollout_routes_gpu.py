"""Which kernel each rollout launch takes on the MI355X, pinned: one small launch (T = 3 or 16 on a 64^2 / 100^2 map) per branch of
mf_rollout_fwd_f32/f64 and mf_rollout_bwd_f32/f64 through the C ABI, and after each call the return code, mf_last_launch() -- the kernel
template, grid and workgroup -- and how many rollout kernels the call launched; and the routes the Python wrappers pick from the policy
queries (physics_loss_rollout by mf_rollout_loss_fusable's answer, rollout_costs).  The fixture, tests/golden/rollout_routes_gpu.json, was
recorded on the MI355X; regenerate it only for an intended change of the routing:  python -m tests.test_rollout_routes_gpu --record PATH"""
import ctypes as C
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, 'tests', 'golden', 'rollout_routes_gpu.json')
COMPONENT = 16      # MF_LANES_COMPONENT

# up: the backward's upstream -- 'all' six gradients, 'xs' positions only, 'loss' the fused physics loss, None no backward
CASES = {
    # component-parallel (<= 4 points): forward forms, then the backward's stream (12 / 6 ring slots) / saved (+- zmu) / late / early (+- window) / ONE1
    'cp_states': dict(B=64, forces=False, up='xs'),
    'cp_forces': dict(B=64),
    'cp_forces_gcontrols': dict(B=1024, gcontrols=True),
    'cp_zmu_pass': dict(B=2048, shared=1, zmu_scratch=True, up='xs'),
    'cp_zmu_staged': dict(B=64, shared=1, zmu=True),
    'cp_rec_stream12': dict(B=1024, rec=True),
    'cp_rec_stream12_xs': dict(B=1024, rec=True, up='xs'),
    'cp_rec_stream6': dict(B=2048, rec=True),
    'cp_rec_stream_dyn': dict(B=1024, rec=True, integ=0),
    'cp_rec_saved': dict(B=4096, rec=True),
    'cp_rec_saved_zmu': dict(B=4096, rec=True, shared=1, zmu_scratch=True, bwd_zmu_scratch=True),
    'cp_dyn_late': dict(B=2048, rec=True, integ=0),
    'cp_early': dict(B=8192),
    'cp_early_win': dict(B=8192, shared=1),
    'cp_early_win_xs': dict(B=8192, shared=1, up='xs'),
    'cp_loss_fwd': dict(B=256, rec=True, forces=False, loss='fwd', up='loss'),
    'cp_loss_in_bwd': dict(B=256, rec=True, forces=False, loss='in_bwd', up='loss', integ=0),
    'cp_loss_in_bwd_euler': dict(B=1024, rec=True, forces=False, loss='in_bwd', up='loss'),
    'cp_loss_one1': dict(B=6144, forces=False, side=100, up='loss'),
    'cp_loss_one1_win': dict(B=6144, forces=False, shared=1, up='loss'),
    # one point per lane
    'split_carry': dict(B=16384),
    'zmu_split_xs_zmu': dict(B=16384, shared=1, side=100, zmu_scratch=True, bwd_zmu_scratch=True, up='xs'),
    'zmu_cost1': dict(B=16384, shared=1, zmu_scratch=True, cost=1, up=None),
    'zmu_cost2': dict(B=16384, shared=1, zmu_scratch=True, cost=2, up=None),
    'cost': dict(B=64, cost=1, up=None),
    'fast_general': dict(B=64, N=8),
    'fast_states': dict(B=64, N=8, forces=False, up='xs'),
    'chunked': dict(B=40000),
    'ppl4_fast': dict(B=64, N=8, ppl=4),
    'joints_fast': dict(B=64, N=8, joints=1),
    'joints_exact': dict(B=64, N=8, joints=1, math=0),
    'exact': dict(B=64, math=0),
    'mw_rec': dict(B=64, N=32, rec=True),
    'mw_rec_xs': dict(B=64, N=32, rec=True, up='xs'),
    'mw_rec_tile': dict(B=64, N=223, rec=True),
    'mw_rec_dyn': dict(B=1024, N=16, rec=True, integ=0),
    'xs': dict(B=16384, side=100, up='xs'),
    'xs_win256': dict(B=16384, shared=1, up='xs'),
    'xs_win512': dict(B=32768, shared=1, up='xs'),
    'xs_loss': dict(B=16384, side=100, forces=False, up='loss'),
    'xs_win_loss': dict(B=16384, shared=1, forces=False, up='loss'),
    'xs_ppl': dict(B=2048, N=223, up='xs'),
    'carry_ppl': dict(B=2048, N=223),
    # the edges of the instantiated lane maps (tests/test_rollout_instances_cpu.py): an articulated body inside a wave and over four waves, a
    # states-only launch that asks for four points per lane (the planner re-chooses one), projected cost rows under dynamics() (the COST = 1 kernel)
    'joints_fast_ppl4_n4': dict(B=8, T=16, joints=1),
    'joints_fast_multiwave': dict(B=4, T=16, N=223, joints=1),
    'ppl4_states': dict(B=8, T=16, N=16, ppl=4, forces=False, up='xs'),
    'cost2_dynamics': dict(B=8, T=16, cost=2, integ=0, up=None),
    # the float64 validation builds and the exact float64 kernels
    'f64_cp_stream': dict(f64=True, ppl=COMPONENT, B=64, rec=True),
    'f64_cp_saved': dict(f64=True, ppl=COMPONENT, B=64, rec=True, integ=0),
    'f64_cp_late': dict(f64=True, ppl=COMPONENT, B=64),
    'f64_cp_states': dict(f64=True, ppl=COMPONENT, B=64, forces=False, up='xs'),
    'f64_mw': dict(f64=True, ppl=COMPONENT, B=64, N=32, rec=True),
    'f64_exact': dict(f64=True, B=64),
    'f64_joints': dict(f64=True, B=64, N=8, joints=1),
}


def _last(L):
    t = L.mf_last_launch().decode()
    if not t:
        return '', 0, 0, 0
    name, rest = t.split(' grid=')
    grid, rest = rest.split(' block=')
    block, n = rest.split(' launches=')
    return name, int(grid), int(block), int(n)


def _outcome(L, rc, n0):
    if rc != 0:
        return [rc, L.mf_last_error().decode()]
    name, grid, block, n = _last(L)
    return [rc, name, grid, block, n - n0]


def run_case(spec, rows=None):
    """[rc, kernel, grid, block, launches] of the forward and (unless up is None) the backward of one case; `rows`: a list that receives
    the forward's cost rows."""
    import torch
    from monoforce_amd import _lib
    L = _lib.lib()
    L.mf_rollout_record_bytes.restype = C.c_longlong
    L.mf_rollout_record_bytes_f64.restype = C.c_longlong
    c = dict(B=64, T=3, N=4, side=64, integ=1, math=1, ppl=0, shared=0, joints=0, f64=False, forces=True, zmu_scratch=False, zmu=False,
             rec=False, cost=0, loss=None, up='all', bwd_zmu_scratch=False, gcontrols=False)
    c.update(spec)
    dt = torch.float64 if c['f64'] else torch.float32
    sfx = 'f64' if c['f64'] else 'f32'
    B, T, N, H = c['B'], c['T'], c['N'], c['side']      # (the loss tables below are those of T = 3)
    keep = []

    def put(t):
        t = t.cuda().contiguous()
        keep.append(t)
        return t.data_ptr()

    def buf(n, fill=0.0, dtype=dt):
        return put(torch.full((max(int(n), 1),), fill, dtype=dtype))

    d = _lib.MfRolloutDesc(B=B, T=T, N=N, H=H, W=H, n_tracks=4 if c['joints'] else 2, integrator=c['integ'], layout=1,
                           map_shared=c['shared'], points_per_lane=c['ppl'], math_mode=c['math'], has_joints=c['joints'],
                           pose_stride=1 if c['cost'] else 0, cost_project=1 if c['cost'] == 2 else 0, mass=40.0, gravity=9.81,
                           stiffness=5000.0, damping=250.0, omega_max=3.0, grid_res=0.1, d_max=H * 0.05, dt=0.01, robot_size_y=0.5)
    for i in (0, 4, 8):
        d.Iinv[i] = 0.1
    d.force_stride = fs = L.mf_rollout_force_stride(C.byref(d))
    nmap = H * H * (1 if c['shared'] else B)
    pts = torch.zeros(N, 3, dtype=dt)
    pts[:, 0] = torch.linspace(-0.4, 0.4, N, dtype=dt)
    pts[:, 1] = 0.25 * (1 - 2 * (torch.arange(N) % 2)).to(dt)
    part = torch.arange(N, dtype=torch.int32) % d.n_tracks
    f = _lib.MfRolloutFwdBufs(z=buf(nmap), mu=buf(nmap, 0.8), controls=buf(B * T * 2, 0.5), ts=put(torch.arange(T, dtype=dt) * 0.01),
                              points=put(pts), part=put(part), x0=buf(B * 3), xd0=buf(B * 3),
                              R0=put(torch.eye(3, dtype=dt).repeat(B, 1, 1)), w0=buf(B * 3), Xs=buf(B * T * 3), Rs=buf(B * T * 9))
    if c['cost']:
        f.cost_rows, f.path_cost = buf(T * B * 4), buf(B)
        cost_rows = keep[-2]
    else:
        f.Xds, f.Omegas, f.Xraw = buf(B * T * 3), buf(B * T * 3), buf(B * (T + 1) * 3)
        if c['forces']:
            f.Fs, f.Ff = buf(B * T * fs * 3), buf(B * T * fs * 3)
    if c['joints']:
        f.joint_angles = buf(B * T * 4, 0.1)
    if c['zmu_scratch']:
        f.zmu_scratch = buf(2 * H * H)
    if c['zmu']:
        f.zmu = put(torch.tensor([0.0, 0.8], dtype=dt).repeat(H * H))
    if c['rec']:
        nb = (L.mf_rollout_record_bytes_f64 if c['f64'] else L.mf_rollout_record_bytes)(C.byref(d))
        f.rec = buf(nb, 0, torch.uint8) if nb > 0 else None
    tables = dict(T2=2, gt=buf(B * 2 * 3), near=put(torch.tensor([0, 2], dtype=torch.int32)), w=put(torch.tensor([1.0, 0.9], dtype=dt)),
                  row_stamp=put(torch.tensor([0, -1, 1], dtype=torch.int32)), row_w=put(torch.tensor([1.0, 0.0, 0.9], dtype=dt)))
    flags = 1 if c['loss'] == 'in_bwd' else 0
    if c['loss']:
        lf = _lib.MfRolloutLoss(flags=flags, partial=buf(B + 64), ticket=buf(1, 0, torch.int32), loss=buf(1), **tables)
        f.loss = C.addressof(lf)
    out = {}
    n0 = _last(L)[3]
    rc = getattr(L, 'mf_rollout_fwd_' + sfx)(C.byref(d), C.byref(f), None)
    out['fwd'] = _outcome(L, rc, n0)
    torch.cuda.synchronize()
    if rows is not None:
        rows.append(cost_rows.cpu())
    if c['up'] is None or rc != 0:
        return out
    g = _lib.MfRolloutBwdBufs(z=f.z, mu=f.mu, controls=f.controls, ts=f.ts, points=f.points, part=f.part, x_init=f.x0, xd0=f.xd0, R0=f.R0,
                              w0=f.w0, Xraw=f.Xraw, Xds=f.Xds, Rs=f.Rs, Omegas=f.Omegas, zeros=buf(16), gz=buf(nmap), gmu=buf(nmap),
                              gx0=buf(B * 3), gxd0=buf(B * 3), gR0=buf(B * 9), gw0=buf(B * 3), rec=f.rec, joint_angles=f.joint_angles)
    if c['up'] in ('all', 'xs'):
        g.gXs = buf(B * T * 3, 1e-3)
    if c['up'] == 'all':
        g.gXds, g.gRs, g.gOmegas = buf(B * T * 3, 1e-3), buf(B * T * 9, 1e-3), buf(B * T * 3, 1e-3)
        g.gFs, g.gFf = buf(B * T * fs * 3, 1e-3), buf(B * T * fs * 3, 1e-3)
    if c['up'] == 'loss':
        lb = _lib.MfRolloutLoss(flags=flags, gloss=buf(1, 1.0), Xs=f.Xs, partial=buf(B + 64), ticket=buf(1, 0, torch.int32), loss=buf(1),
                                **tables)
        g.loss = C.addressof(lb)
    if c['gcontrols']:
        g.gcontrols = buf(B * T * 2)
    if c['joints']:
        g.gjoint_angles = buf(B * T * 4)
    if c['bwd_zmu_scratch']:
        g.zmu_scratch = buf(2 * H * H)
    n0 = _last(L)[3]
    rc = getattr(L, 'mf_rollout_bwd_' + sfx)(C.byref(d), C.byref(g), None)
    out['bwd'] = _outcome(L, rc, n0)
    torch.cuda.synchronize()
    return out


# The Python wrappers that pick a route from a policy query: physics_loss_rollout (dphysics.py: mf_rollout_loss_fusable's answer 1, 2 or 3 --
# and 0, the unfused route of its own loss launches) and rollout_costs (path-cost rows, the shared maps interleaved from half a wave per SIMD)
PY_CASES = {
    'py_loss1': dict(B=256),
    'py_loss1_value_in_backward': dict(B=256, value_in_backward=True),
    'py_loss1_dynamics': dict(B=256, integ=0, value_in_backward=True),
    'py_loss0': dict(B=3072),
    'py_loss3': dict(B=6144),
    'py_loss2': dict(B=16384),
    'py_loss2_value_in_backward': dict(B=16384, value_in_backward=True),
    'py_costs': dict(B=64, costs=True),
    'py_costs_zmu': dict(B=16384, costs=True),
    # every other entry point of the Python layer (`entry`), with what crossed the C ABI: the descriptor and the non-NULL buffers of each
    # launch, the gradient pool's copies, whether a record was passed
    # (recorded with the library code of commit ab3e796, before monoforce_amd/rollout_launch.py existed: they pin that refactor)
    'py_mod_all': dict(entry='module'),
    'py_mod_mixed_maps': dict(entry='module', B=8, maps='mixed'),
    'py_mod_expand8': dict(entry='module', B=8, maps='expand'),
    'py_mod_expand6': dict(entry='module', B=6, maps='expand'),
    'py_mod_xs_saturated': dict(entry='module', B=16384, up='xs', kw=dict(return_forces=False)),
    'py_mod_contiguous': dict(entry='module', kw=dict(contiguous_outputs=True)),
    'py_mod_precise': dict(entry='module', kw=dict(precise=True)),
    'py_mod_f64_cp': dict(entry='module', f64=True, up='states', kw=dict(points_per_lane=COMPONENT, return_forces=False)),
    'py_mod_default_state': dict(entry='module', up=None, controls='time_constant'),
    'py_ops_shared': dict(entry='ops'),
    'py_ops_per_rollout': dict(entry='ops', maps='per_rollout'),
    'py_ops_f64': dict(entry='ops', f64=True),
    'py_planner_no_forces': dict(entry='planner', cost='inclination'),
    'py_planner_forces': dict(entry='planner', cost='force'),
}


class _AbiSpy:
    """Stands in for mf_rollout_fwd_* / mf_rollout_bwd_* on the loaded library while one entry point runs: notes, per launch, the
    descriptor, the names of the non-NULL buffers and -- on the launching thread, the backward's is autograd's -- mf_last_launch()."""

    def __init__(self, L):
        self.L, self.seen, self.orig = L, {}, {}

    def __enter__(self):
        for way in ('fwd', 'bwd'):
            for sfx in ('f32', 'f64'):
                name = f'mf_rollout_{way}_{sfx}'
                self.orig[name] = getattr(self.L, name)
                setattr(self.L, name, self._wrap(way, self.orig[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.L, name, fn)

    def _wrap(self, way, fn):
        def call(desc, bufs, stream):
            rc = fn(desc, bufs, stream)
            d, b = desc._obj, bufs._obj
            r9 = lambda v: float('%.9g' % v) if isinstance(v, float) else v  # noqa: E731  (Iinv comes from a host LAPACK inverse: not to the last bit)
            fields = {n: ([r9(v) for v in getattr(d, n)] if n in ('Iinv', 'joint_xyz') else r9(getattr(d, n))) for n, _ in d._fields_}
            assert way not in self.seen, f'two {way} launches in one case'
            self.seen[way] = dict(launch=self.L.mf_last_launch().decode().split(' launches=')[0], rc=rc,
                                  desc={n: v for n, v in fields.items() if v and (not isinstance(v, list) or any(v))},
                                  bufs=sorted(n for n, _ in b._fields_ if getattr(b, n)))
            return rc
        return call


def run_entry_case(c):
    """One entry point of the Python layer other than the fused loss and the path costs: what its forward and backward launch (kernel,
    descriptor, non-NULL buffers), the timed names, the gradient pool's copies and whether a record was passed."""
    import torch
    from monoforce_amd import _lib, _timing, ops, synthetic as syn
    from monoforce_amd.planner import TrajectoryShooter
    from tests.test_rollout_gpu import DEV, make_dphysics
    B, T = c['B'], 20
    dt = torch.float64 if c.get('f64') else torch.float32
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 3.2, **c.get('kw', {}))
    dp.dphys_cfg.traj_sim_time = 5.0
    z1 = syn.bump_terrain(syn.bump_params(5), 3.2, 0.1, dt).to(DEV).unsqueeze(0).requires_grad_(True)
    mu1 = syn.wave_friction(3.2, 0.1, dtype=dt).to(DEV).unsqueeze(0).requires_grad_(True)
    maps = c.get('maps', 'shared')
    z = {'shared': z1, 'expand': z1.expand(B, -1, -1)}.get(maps)
    if z is None:       # 'mixed' (z per rollout, mu shared) and 'per_rollout': a [B,H,W] leaf
        z = z1.detach().repeat(B, 1, 1).requires_grad_(True)
    mu = mu1.detach().repeat(B, 1, 1).requires_grad_(True) if maps == 'per_rollout' else mu1
    ctrl = syn.const_controls(B, T, seed=2, dtype=dt).to(DEV)
    if c.get('controls') == 'time_constant':
        ctrl = ctrl[:, 0][:, None].expand(B, T, 2)
    elif c['entry'] != 'planner':
        ctrl.requires_grad_(True)
    up = c.get('up', 'all')
    pools = None
    _timing.start()
    with _AbiSpy(_lib.lib()) as spy:
        if c['entry'] == 'planner':
            TrajectoryShooter(dp, cost=c['cost'], fused=False).shoot(z.detach(), friction=mu.detach(), controls=ctrl)
        elif up is None:
            with torch.no_grad():
                dp(z.detach(), ctrl, friction=mu.detach())
        else:
            if c['entry'] == 'ops':
                eye = torch.eye(3, dtype=dt, device=DEV).repeat(B, 1, 1)
                state = tuple(torch.zeros(B, 3, dtype=dt, device=DEV) for _ in range(2)) + (eye, torch.zeros(B, 3, dtype=dt, device=DEV))
                states, forces = ops.rollout(dp, z, ctrl, state, friction=mu)
                pools = ops._POOL_OWNER
            else:
                states, forces = dp(z, ctrl, friction=mu)
                pools = dp
            outs = {'all': list(states) + list(forces), 'states': list(states), 'xs': list(states)[:1]}[up]
            sum(o.sum() for o in outs).backward()
        torch.cuda.synchronize()
    out = dict(timed=sorted(_timing.stop()), **spy.seen)
    out['rec'] = 'rec' in out['fwd']['bufs']
    if pools is not None and out['bwd']['desc'].get('map_shared'):
        out['copies'] = list(pools._grad_pools.values())[-1].copies       # (the pool used last is the dict's last entry)
    return out


def run_py_case(spec):
    """The loss answer, the forward / backward kernel (template, grid, workgroup) and the names of the timed launches of one wrapper call."""
    import torch
    from monoforce_amd import _lib, _timing, synthetic as syn
    from tests.test_rollout_gpu import DEV, make_dphysics
    c = dict(B=64, integ=1, value_in_backward=False, costs=False)
    c.update(spec)
    if 'entry' in c:
        return run_entry_case(c)
    B, T = c['B'], 20
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, c['integ'], 0.1, 3.2)
    dp.dphys_cfg.traj_sim_time = 5.0
    z = syn.bump_terrain(syn.bump_params(5), 3.2, 0.1).to(DEV).unsqueeze(0)
    mu = syn.wave_friction(3.2, 0.1).to(DEV).unsqueeze(0)
    ctrl = syn.const_controls(B, T, seed=2).to(DEV)
    strip = lambda t: t.split(' launches=')[0]      # noqa: E731  (the count runs over the whole process)
    if c['costs']:
        _timing.start()
        dp.rollout_costs(z, ctrl, friction=mu, pose_stride=5)
        fwd = strip(_lib.lib().mf_last_launch().decode())
        return dict(fwd=fwd, timed=sorted(_timing.stop()))
    d = _lib.MfRolloutDesc(B=B, T=T, N=4, H=z.shape[-2], W=z.shape[-1], integrator=c['integ'], math_mode=_lib.MF_MATH_FAST, force_stride=4,
                           map_shared=1, layout=_lib.MF_LAYOUT_TIME_MAJOR)
    fus = int(_lib.lib().mf_rollout_loss_fusable(C.byref(d)))
    full_ts = torch.linspace(0, 5.0, 500)[:T]
    lspec = dp.loss_spec(full_ts[torch.arange(4, T, 5)], gamma=0.9, n_steps=T)
    X_gt = torch.zeros(B, lspec.T2, 3, device=DEV)
    zd, md, cd = z.clone().requires_grad_(True), mu.clone().requires_grad_(True), ctrl.clone().requires_grad_(True)
    _timing.start()
    loss = dp.physics_loss_rollout(zd, cd, X_gt, lspec, friction=md, value_in_backward=c['value_in_backward'])[0]
    loss.backward()
    ln = _timing.launches()
    timed = sorted(_timing.stop())
    return dict(loss_fusable=fus, fwd=strip(ln.get('rollout_fwd_kernel', '')), bwd=strip(ln.get('rollout_bwd_kernel', '')), timed=timed)


def test_fixture_covers_every_case():
    assert sorted(json.load(open(FIXTURE))) == sorted(list(CASES) + list(PY_CASES))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_route_is_the_recorded_one(name):
    assert run_case(CASES[name]) == json.load(open(FIXTURE))[name]


@pytest.mark.gpu
def test_projected_cost_rows_under_dynamics_are_the_plain_ones():
    """cost_project = 1 under dynamics(), whose rotation cannot drift, runs the COST = 1 kernel: the rows of cost_project = 0, bit for bit."""
    import torch
    rows = []
    plain = run_case(dict(CASES['cost2_dynamics'], cost=1), rows)
    assert run_case(CASES['cost2_dynamics'], rows) == plain
    assert ', 0, true, false, false, 1, false, false, false>' in plain['fwd'][1]      # (INTEG = dynamics(), ..., COST = 1, ...)
    assert rows[0].abs().max() > 0 and torch.equal(rows[0], rows[1])


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(PY_CASES))
def test_wrapper_route_is_the_recorded_one(name):
    assert run_py_case(PY_CASES[name]) == json.load(open(FIXTURE))[name]


if __name__ == '__main__' and len(sys.argv) == 3 and sys.argv[1] == '--record':
    table = {}
    for name in sorted(CASES):
        table[name] = run_case(CASES[name])
        print(name, table[name], flush=True)
    for name in sorted(PY_CASES):
        table[name] = run_py_case(PY_CASES[name])
        print(name, table[name], flush=True)
    with open(sys.argv[2], 'w') as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
