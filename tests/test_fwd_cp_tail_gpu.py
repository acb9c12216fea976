"""The component-parallel forward's step loop (rollout_fwd_cp_kernel.h) runs its steps two per trip WITHOUT clamps on the offsets it
prefetches through -- the trips whose time stamps all exist -- and finishes with one or two clamped steps; it reads three stamps with one
load, the second step's controls through a base pointer one row on, clamps the flat cell index with one instruction, and exists twice
(with and without a friction map).  What can go wrong there shows at the smallest shapes:
  T = 1 .. 5       no step; an empty main loop with a tail of one and of two steps; the first trip, with a tail of one and of two
  B = 1, 3, 4, 5   a partial wave, a full one, a trailing workgroup of one rollout
  8 x 8 and 16 x 16 maps, start poses inside, on the edge and well outside (negative cell coordinates, the flat-index clamp)
  both integrators, with and without a friction map, with and without the record (then followed by the backward), both layouts,
  non-uniform time stamps, controls contiguous / with another stride over time / one pair per rollout (stride 0).
Every forward is held to the float64 oracle and to the one-point-per-lane kernels (float32 sums in another order) at the tolerances of
tests/test_rollout_gpu.py; the backward to the one-point-per-lane kernels and the oracle at those of tests/test_stream_scatter_gpu.py.
The over-read test hands the kernel controls and stamps as views into larger tensors whose remainder is NaN: a prefetch past a row that
reached any result would show as NaN, and everything the launch writes equals the run on plain tensors bit for bit."""
import functools
import math

import pytest
import torch

from oracle import dphysics_oracle as orc
from tests import helpers as hp
from tests.test_rollout_gpu import make_dphysics

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RES = 0.1
TOL_STATE, TOL_FORCE, TOL_MAPPING = 2e-4, {0: 1e-2, 1: 2e-3}, 5e-5      # test_large_bodies_fast_f32_multi_wave_kernels
TOL_GRAD_MAPPING, TOL_GRAD_ORACLE = 2e-5, 2e-4                          # test_stream_scatter_gpu


@functools.lru_cache(maxsize=None)
def _module(integ, side, ppl, batch_major):
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    return make_dphysics(pts, masks, integ, RES, side * RES / 2, points_per_lane=ppl, contiguous_outputs=batch_major)


@functools.lru_cache(maxsize=None)
def _inputs(B, T, side, friction, const=False):
    """Float32 inputs on the host: a map pair per rollout, time-varying controls, non-uniform stamps, start poses inside the map, on
    its edge and well outside it (rollout b: b % 3), yawed and moving.  `const`: the first (v, w) of each rollout at every step."""
    from monoforce_amd import synthetic as syn
    d_max = side * RES / 2
    z = torch.stack([syn.bump_terrain(syn.bump_params(20 + k), d_max, RES) * 0.3 for k in range(B)])
    mu = torch.stack([syn.wave_friction(d_max, RES, 0.5, 1.0, 1.1 + 0.2 * k, 0.8) for k in range(B)]) if friction else None
    ctrl = syn.varying_controls(B, max(T, 2), seed=3 + T)[:, :T].contiguous()
    if const:
        ctrl = ctrl[:, :1].expand(-1, T, -1).contiguous()
    k = torch.arange(T, dtype=torch.float64)
    ts = (0.01 * k + 0.002 * torch.sin(1.7 * k)).float()          # steps of 0.008 .. 0.012 s
    x = torch.zeros(B, 3)
    R = torch.zeros(B, 3, 3)
    for b in range(B):
        x[b, :2] = torch.tensor([[0.013 + 0.02 * b, -0.031], [-d_max + 0.013, d_max - 0.017], [d_max + 0.37, -d_max - 0.21 - 0.1 * b]][b % 3])
        yaw = 0.3 + 0.5 * b
        R[b] = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    xd = torch.stack([ctrl[:, 0, 0] * R[:, 0, 0], ctrl[:, 0, 0] * R[:, 1, 0], torch.zeros(B)], 1)
    w = torch.stack([torch.zeros(B), torch.zeros(B), ctrl[:, 0, 1]], 1)
    return z, mu, ctrl, ts, (x, xd, R, w)


@functools.lru_cache(maxsize=None)
def _oracle(B, T, side, friction, integ, grads, const=False):
    """The float64 oracle on the same float32 values: the six outputs, and (grads) dL/dz, dL/dmu of the probe loss `_ups` defines."""
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    z, mu, ctrl, ts, state = _inputs(B, T, side, friction, const)
    z64 = z.double().requires_grad_(grads)
    mu64 = None if mu is None else mu.double().requires_grad_(grads)
    spec = hp.spec_from(pts, masks, integ, RES, side * RES / 2)
    with torch.set_grad_enabled(grads):
        st, fo = orc.rollout(spec, z64, ctrl.double(), state=tuple(s.double().clone() for s in state), friction=mu64, ts=ts.double())
        outs = list(st) + list(fo)
        gz = gmu = None
        if grads:
            sum((o * u.double()).sum() for o, u in zip(outs[:4], _ups(B, T))).backward()
            gz, gmu = z64.grad, (None if mu64 is None else mu64.grad)
    return [o.detach() for o in outs], gz, gmu


def _ups(B, T):
    from monoforce_amd import synthetic as syn
    return [syn.probe_weights((B, T) + tail, phase=0.3 + i) for i, tail in enumerate(((3,), (3,), (3, 3), (3,)))]


def _launch(integ, side, ppl, batch_major, B, T, friction, record, controls=None, ts=None, stride=(0, 0), const=False):
    """One forward through the C ABI (and, with `record`, the backward of the probe loss).  `controls` / `ts`: device tensors -- or views
    -- the kernel reads instead of the plain ones; `stride`: (controls_stride_b, controls_stride_t) in elements.  Returns the six
    outputs [B,T,...], the snapped start position, the record, (gz, gmu) and the forward kernel's name, all on the host."""
    from monoforce_amd import _lib, rollout_launch as rl
    dp = _module(integ, side, ppl, batch_major)
    z, mu, ctrl, ts0, state = _inputs(B, T, side, friction, const)
    zd, mud = z.to(DEV), (None if mu is None else mu.to(DEV))
    cd = ctrl.to(DEV) if controls is None else controls
    td = ts0.to(DEV) if ts is None else ts
    sd = tuple(s.to(DEV).clone() for s in state)
    desc, (zc, muc, points) = dp._make_desc(zd, mud, ctrl)
    desc.controls_stride_b, desc.controls_stride_t = stride
    if desc.map_shared:      # (B = 1: one map pair is a shared one)
        desc.grad_copies = rl.grad_copies_for(B, 4)
    f = rl.launch_forward(desc, zc, muc, cd, td, points, dp._part_dev(torch.device(DEV)), sd, want_forces=True, want_xraw=record, want_rec=record)
    name = _lib.lib().mf_last_launch().decode()
    outs = [f.Xs, f.Xds, f.Rs, f.Om, f.Fs[..., :4, :], f.Ff[..., :4, :]]
    if not batch_major:
        outs = [o.transpose(0, 1) for o in outs]
    grads = (None, None)
    if record:
        desc.controls_stride_b = desc.controls_stride_t = 0      # (the backward takes contiguous [B][T][2] controls only: the plain tensor)
        g = rl.launch_backward(desc, zc, muc, ctrl.to(DEV), ts0.to(DEV), points, dp._part_dev(torch.device(DEV)), sd, (f.Xraw, f.Xds, f.Rs, f.Om),
                               [u.to(DEV) for u in _ups(B, T)] + [None, None], pool_owner=dp, want_gcontrols=False, rec=f.rec)
        grads = (g.gz.cpu().reshape(z.shape), None if g.gmu is None else g.gmu.cpu().reshape(z.shape))
    torch.cuda.synchronize()
    # (the record: one slab per STEP -- the default integrator takes T - 1 of them and leaves the last slab of the buffer unwritten)
    rec = None if f.rec is None else f.rec.cpu().view(T, -1)[:T - 1 if integ == 1 else T]
    return [o.contiguous().cpu() for o in outs], sd[0].cpu(), rec, grads, name


def _close(got, ref, tol, tag):
    assert torch.isfinite(got).all(), tag
    if float(ref.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, tag
    else:
        assert hp.rel_err(got, ref) <= tol, (tag, hp.rel_err(got, ref), 'bar', tol)


def _check(integ, side, batch_major, B, T, friction, record, const=False, **views):
    tag = dict(integ=integ, side=side, batch_major=batch_major, B=B, T=T, friction=friction, record=record, **{k: True for k in views if k != 'stride'})
    outs, x0, rec, grads, name = _launch(integ, side, 0, batch_major, B, T, friction, record, const=const, **views)
    assert 'rollout_fwd_cp_kernel<float' in name, name
    if record and integ == 1:
        assert rec is not None and ', true, false>' in name.split(' grid=')[0], name      # <float, 1, FORCES, ZMU, REC = true, LOSS = false>
    lane, x0_lane, _, grads_lane, name_lane = _launch(integ, side, 1, batch_major, B, T, friction, False, const=const)
    assert 'rollout_fwd_kernel<' in name_lane, name_lane
    ref, gz64, gmu64 = _oracle(B, T, side, friction, integ, record, const)
    for k, a, b, r in zip(hp.OUT_KEYS, outs, lane, ref):
        assert tuple(a.shape) == tuple(r.shape), (tag, k)
        _close(a, r.float(), TOL_FORCE[integ] if k in ('Fs', 'Ff') else TOL_STATE, (tag, k, 'vs oracle'))
        _close(a, b, TOL_MAPPING, (tag, k, 'vs one point per lane'))
    _close(x0, x0_lane, TOL_MAPPING, (tag, 'snapped start'))
    if record:
        lane_g = _launch(integ, side, 1, batch_major, B, T, friction, True, const=const)[3]
        for k, a, b, r in zip(('gz', 'gmu'), grads, lane_g, (gz64, gmu64)):
            if r is None:      # (no friction map, or T = 1: nothing depends on the map)
                assert a is None or float(a.abs().max()) == 0.0, (tag, k)
                continue
            _close(a, b, TOL_GRAD_MAPPING, (tag, k, 'vs one point per lane'))
            _close(a, r.float(), TOL_GRAD_ORACLE, (tag, k, 'vs oracle'))
    return outs, x0, rec


@pytest.mark.parametrize('integ', [1, 0])
@pytest.mark.parametrize('T', [1, 2, 3, 4, 5])
def test_every_tail_and_ragged_batch(T, integ):
    """T x B x integrator in full; map size, friction map, record (+ backward) and layout cycle through their sixteen combinations over
    the cases, so each value meets every horizon."""
    for i, B in enumerate((1, 3, 4, 5)):
        k = 4 * (T - 1) + i + 8 * integ
        _check(integ, side=16 if k & 1 else 8, batch_major=bool(k & 2), B=B, T=T, friction=bool(k & 4), record=bool(k & 8))
        _check(integ, side=8 if k & 1 else 16, batch_major=not k & 2, B=B, T=T, friction=not k & 4, record=not k & 8)


def _nan_backed(t, lead, trail):
    """`t` as a view into a larger NaN-filled device tensor, `lead` / `trail` elements in front of / behind its contiguous values."""
    big = torch.full((lead + t.numel() + trail,), float('nan'), dtype=t.dtype, device=DEV)
    view = big[lead:lead + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize('integ', [1, 0])
@pytest.mark.parametrize('mode', ['contiguous', 'strided', 'one_pair'])
def test_no_prefetch_past_a_row_reaches_a_result(mode, integ):
    """Controls and stamps as views into NaN-filled tensors (an odd element offset: rows that are 4-byte aligned only): contiguous rows,
    rows 5 elements apart with NaN between them, one (v, w) per rollout (stride 0 over time).  All outputs, the snapped start and the
    record are finite and equal the run on plain tensors bit for bit -- and meet the oracle and the one-point-per-lane kernels."""
    side, friction, B = 16, True, 5
    for T in (1, 2, 3, 4, 5):
        for record in (False, True):
            const = mode == 'one_pair'
            z, mu, ctrl, ts, state = _inputs(B, T, side, friction, const)
            ts_v = _nan_backed(ts.to(DEV), 5, 9)
            if mode == 'contiguous':
                views = dict(controls=_nan_backed(ctrl.to(DEV), 7, 16), ts=ts_v)
            elif mode == 'strided':
                big = torch.full((B, 3 + 5 * T + 8), float('nan'), device=DEV)
                for t in range(T):
                    big[:, 3 + 5 * t:5 + 5 * t] = ctrl[:, t].to(DEV)
                views = dict(controls=big[:, 3:], ts=ts_v, stride=(big.stride(0), 5))
            else:
                big = torch.full((B, 9), float('nan'), device=DEV)
                big[:, 3:5] = ctrl[:, 0].to(DEV)
                views = dict(controls=big[:, 3:], ts=ts_v, stride=(big.stride(0), 0))
            plain = _launch(integ, side, 0, False, B, T, friction, record, const=const)
            got = _check(integ, side, False, B, T, friction, record, const=const, **views)
            for k, a, b in zip(hp.OUT_KEYS, got[0], plain[0]):
                assert torch.isfinite(a).all() and torch.equal(a, b), (mode, integ, T, record, k)
            assert torch.isfinite(got[1]).all() and torch.equal(got[1], plain[1]), (mode, integ, T, record, 'snapped start')
            if plain[2] is not None:
                assert torch.equal(got[2].contiguous().view(torch.int32), plain[2].contiguous().view(torch.int32)), (mode, integ, T, record, 'record')
