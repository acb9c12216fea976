"""The cached drop-in step (monoforce_amd/api_cache.py) held to eager autograd's contract, beyond the straight loop of tests/test_api_cache_gpu.py:
losses and gradients that are kept, outputs that are held, backwards that come late or twice, in-place edits between forward and backward,
module scalars changed after arming, maps that are no leaves, and the private torch call the buffer guard leans on being absent.

Every test runs ONE script twice, `api_cache.ENABLED` off and then on (a fresh `_problem` each time).  The launch-by-launch run is the
referee (other files hold that route to the oracle).  Each outcome of the script must be the same in both runs: values equal within the
tolerance of tests/test_api_cache_gpu.py (`_same`, 2e-5: float-atomic ordering), or both runs raise RuntimeError.  Every test that claims to
exercise the cache asserts a minimum of `cache.replays`."""
import warnings

import pytest
import torch

from tests import helpers as hp
from tests.test_api_cache_gpu import _problem, _same

gpu = pytest.mark.gpu
DEV = 'cuda'
TOL = 2e-5          # `_same`'s default, restated for the "the referee did move" assertions
RAISED = 'RuntimeError'
WARM = 6            # iterations before the step under test: three launch by launch, the capture in the fourth call, replays from there on


def _run(script, enabled, **kw):
    """(outcomes of `script` on a fresh problem, that problem's cache or None)."""
    from monoforce_amd import api_cache
    keep, api_cache.ENABLED = api_cache.ENABLED, enabled
    try:
        prob = _problem(B=64, T=60, **kw)
        out = script(*prob)
        torch.cuda.synchronize()
        return out, prob[0].__dict__.get('_api_step_cache')
    finally:
        api_cache.ENABLED = keep


def _both(script, **kw):
    ref, c0 = _run(script, False, **kw)
    got, c1 = _run(script, True, **kw)
    assert c0 is None or c0.replays == 0
    return ref, got, c1


def _rec(loss, *tensors):
    """One record in the layout `_same` compares: (loss, four tensors) -- fewer tensors are repeated."""
    ts = [t.detach() for t in tensors]
    return (float(loss),) + tuple(ts[min(k, len(ts) - 1)] for k in range(4))


def _agree(got, ref):
    """Every outcome the same in both runs (keys that begin with '_' carry counters for the test itself)."""
    assert got.keys() == ref.keys()
    for k in ref:
        if k.startswith('_'):
            continue
        if isinstance(ref[k], str) or isinstance(got[k], str):
            assert got[k] == ref[k], (k, got[k] if isinstance(got[k], str) else 'values', ref[k] if isinstance(ref[k], str) else 'values')
        else:
            _same(got[k], ref[k])


def _attempt(fn):
    """fn()'s result, or RAISED for autograd's refusal of a modified saved tensor (any other error is the test's failure)."""
    try:
        return fn()
    except RuntimeError as e:
        if 'modified by an inplace operation' not in str(e):
            raise
        return RAISED


def _leaves(z0, mu0):
    return z0.clone().unsqueeze(0).requires_grad_(True), mu0.clone().unsqueeze(0).requires_grad_(True)


def _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts):
    from monoforce.losses import physics_loss          # the reference's import path
    states, forces = dp(z_grid=z, controls=ctrl, friction=mu)
    return physics_loss(states_pred=states, states_gt=states_gt, pred_ts=pred_ts, gt_ts=gt_ts, gamma=0.9), states, forces


def _drift(z, mu, i):
    """A deterministic in-place parameter update, the same in both runs."""
    with torch.no_grad():
        z += 0.002
        mu -= 0.0005


def _warm(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts, extra=None, iters=WARM):
    for i in range(iters):
        z.grad = mu.grad = None
        loss, states, forces = _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
        if extra is not None:
            loss = loss + extra(states, forces)
        loss.backward()
        _drift(z, mu, i)
    z.grad = mu.grad = None


# -- kept losses / gradients ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('keep', ['detached', 'with_graph'])
def test_kept_losses_and_gradients_keep_their_values(keep):
    """`hist.append(loss.detach())` (or `loss` itself) and `z.grad` without a clone, read only after the loop: every kept tensor still holds
    ITS iteration's value.  (The terrain drifts by 2 mm per iteration: on the referee consecutive losses differ by more than ten times the
    tolerance, so a loss that aliases the graph's scalar cannot pass.)"""
    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        z, mu = _leaves(z0, mu0)
        kept, gz, gmu = [], [], []
        for i in range(10):
            z.grad = mu.grad = None
            loss, states, forces = _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
            loss.backward()
            kept.append(loss.detach() if keep == 'detached' else loss)
            gz.append(z.grad); gmu.append(mu.grad)          # (not cloned)
            _drift(z, mu, i)
        vals = torch.stack([k.detach() for k in kept]).tolist()          # nothing was read until here
        return {'kept': [_rec(v, a, b) for v, a, b in zip(vals, gz, gmu)]}
    ref, got, cache = _both(script)
    L = [r[0] for r in ref['kept']]
    for a, b in zip(L, L[1:]):
        assert abs(b - a) > 10 * TOL * abs(a), L
    assert cache.replays >= 6, cache.replays
    _agree(got, ref)


@gpu
def test_a_held_view_and_held_forces_are_never_overwritten():
    """Between iterations only `states[0][:, -1]` (a view) and `forces[1]` of the previous iteration stay referenced: neither changes while
    it is held, the other buffer set keeps replaying, and every iteration equals the referee's."""
    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        z, mu = _leaves(z0, mu0)
        hist, held, intact = [], None, []
        for i in range(12):
            z.grad = mu.grad = None
            loss, states, forces = _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
            loss.backward()
            hist.append(_rec(loss.detach(), z.grad, mu.grad, states[0].detach().clone(), forces[0].detach().clone()))
            if held is not None:          # the previous iteration's, through this iteration's forward and backward
                intact.append(all(torch.equal(h.detach(), c) for h, c in zip(held[0], held[1])))
            held = ((states[0][:, -1], forces[1]), (states[0][:, -1].detach().clone(), forces[1].detach().clone()))
            del states, forces, loss
            _drift(z, mu, i)
        return {'hist': hist, '_intact': intact}
    ref, got, cache = _both(script)
    assert len(got['_intact']) == 11 and all(got['_intact']) and all(ref['_intact']), (got['_intact'], ref['_intact'])
    assert cache.replays >= 8, cache.replays          # (one set held at a time: the other one is free in every iteration)
    _agree(got, ref)


# -- in-place edits between forward and backward ------------------------------------------------------------------------------------------
def _edit(what, z, mu, ctrl, states_gt):
    with torch.no_grad():
        if what == 'z_grid':
            z += 0.01
        elif what == 'friction':
            mu *= 0.9
        elif what == 'controls':
            ctrl *= 0.9
        else:
            states_gt[0] += 0.01


def _other_loss(states, forces, gt_rows, X_gt):
    """A loss on the handed-out states that is not `physics_loss`: its gradient reaches the cached step's own backward."""
    return 1e-3 * (states[1] ** 2).mean() + ((states[0][:, gt_rows] - X_gt) ** 2).mean()


@gpu
@pytest.mark.parametrize('late', [False, True], ids=['at_once', 'two_forwards_later'])
@pytest.mark.parametrize('what', ['z_grid', 'friction', 'controls', 'states_gt'])
@pytest.mark.parametrize('route', ['module', 'cached_loss', 'cached_step', 'ops'])
def test_in_place_edit_between_forward_and_backward(route, what, late):
    """Autograd's contract for saved tensors on every HIP route: a map edited in place between forward and backward makes the backward raise
    (as it does on the float64 oracle, test_oracle_raises_for_a_map_edited_in_place) instead of meeting the old states with new contacts; for
    the controls and the ground truth the cached routes do what launch by launch does."""
    from monoforce_amd import ops
    rows = torch.arange(9, 60, 10, device=DEV)

    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        z, mu = _leaves(z0, mu0)
        args = (dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
        extra = (lambda s, f: _other_loss(s, f, rows, states_gt[0])) if route == 'cached_step' else None
        if route in ('cached_loss', 'cached_step'):
            _warm(*args, extra=extra)
        if route == 'ops':
            from monoforce.losses import physics_loss
            x0 = torch.zeros(ctrl.shape[0], 3, device=DEV)
            state = (x0, torch.zeros_like(x0), torch.eye(3, device=DEV).repeat(ctrl.shape[0], 1, 1), torch.zeros_like(x0))

            def forward():
                states, forces = ops.rollout(dp, z, ctrl, tuple(s.clone() for s in state), friction=mu)
                return physics_loss(states_pred=states, states_gt=states_gt, pred_ts=pred_ts, gt_ts=gt_ts, gamma=0.9), states, forces
        else:
            def forward():
                return _step(*args)
        loss, states, forces = forward()
        target = extra(states, forces) if extra is not None else loss
        del states, forces, loss
        _edit(what, z, mu, ctrl, states_gt)
        if late:
            for _ in range(2):
                forward()
        cache = dp.__dict__.get('_api_step_cache')
        n = cache.replays if cache is not None else 0

        def backward():
            target.backward()
            return [_rec(target.detach(), z.grad, mu.grad)]
        return {'backward': _attempt(backward), '_replays': n}
    ref, got, cache = _both(script)
    if route in ('cached_loss', 'cached_step'):          # (three replays in the warm-up, one for the forward under test)
        assert got['_replays'] >= 4 and ref['_replays'] == 0, (got['_replays'], ref['_replays'])
    if what in ('z_grid', 'friction'):
        assert ref['backward'] == RAISED, 'launch by launch: the backward went through on an edited map'
        assert got['backward'] == RAISED, 'cache on: the backward went through on an edited map'
    _agree(got, ref)


def test_oracle_raises_for_a_map_edited_in_place():
    """The referee of the expectation above, on the CPU: the float64 oracle (plain torch autograd) refuses a backward after either map was
    modified in place."""
    from monoforce_amd import synthetic as syn
    from oracle import dphysics_oracle as orc
    pts, masks = syn.robot_points_4()
    for integ in (0, 1):
        spec = hp.spec_from(pts, masks, integ, 0.1, 1.6)
        spec.traj_sim_time = 0.1
        for what in ('z_grid', 'friction'):
            z = (syn.bump_terrain(syn.bump_params(30), 1.6, 0.1, torch.float64) * 0.3).unsqueeze(0).repeat(2, 1, 1).requires_grad_(True)
            mu = syn.wave_friction(1.6, 0.1, dtype=torch.float64).unsqueeze(0).repeat(2, 1, 1).requires_grad_(True)
            ctrl = syn.const_controls(2, 10, seed=1, dtype=torch.float64)
            (Xs, _, _, _), _ = orc.rollout(spec, z, ctrl, friction=mu)
            loss = Xs.square().mean()
            with torch.no_grad():
                if what == 'z_grid':
                    z += 0.01
                else:
                    mu *= 0.9
            with pytest.raises(RuntimeError, match='inplace operation'):
                loss.backward()


# -- late and repeated backwards ------------------------------------------------------------------------------------------------------------
@gpu
def test_late_backward_with_nothing_edited():
    """Three forward + loss calls, then the backward of the FIRST loss: nothing was edited, so it is legal, and the gradients are the referee's."""
    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        z, mu = _leaves(z0, mu0)
        args = (dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
        _warm(*args)
        losses = [_step(*args)[0] for _ in range(3)]
        losses[0].backward()
        return {'first': [_rec(losses[0].detach(), z.grad, mu.grad)]}
    ref, got, cache = _both(script)
    assert cache.replays >= 5, cache.replays
    _agree(got, ref)


@gpu
def test_retain_graph_and_two_backwards_accumulate():
    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        z, mu = _leaves(z0, mu0)
        args = (dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
        _warm(*args)
        loss = _step(*args)[0]
        loss.backward(retain_graph=True)
        once = _rec(loss.detach(), z.grad.clone(), mu.grad.clone())
        loss.backward()
        return {'once': [once], 'twice': [_rec(loss.detach(), z.grad, mu.grad)]}
    ref, got, cache = _both(script)
    assert cache.replays >= 3, cache.replays
    for k in (1, 2):          # (the second backward did add: the accumulated gradient is twice the first, on the referee)
        assert float((ref['twice'][0][k] - 2 * ref['once'][0][k]).abs().max()) <= TOL * float(ref['twice'][0][k].abs().max())
    _agree(got, ref)


@gpu
def test_no_grad_forward_on_the_same_tensors_every_third_iteration():
    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        z, mu = _leaves(z0, mu0)
        hist, plain, trace = [], [], []
        for i in range(12):
            z.grad = mu.grad = None
            loss, states, forces = _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
            loss.backward()
            hist.append(_rec(loss.detach(), z.grad, mu.grad, states[0].detach().clone(), forces[0].detach().clone()))
            if i % 3 == 2:
                with torch.no_grad():
                    s, f = dp(z_grid=z, controls=ctrl, friction=mu)
                plain.append(_rec(0.0, s[0].clone(), s[2].clone(), f[0].clone(), f[1].clone()))
            cache = dp.__dict__.get('_api_step_cache')
            trace.append(cache.replays if cache is not None else 0)
            _drift(z, mu, i)
        return {'hist': hist, 'plain': plain, '_trace': trace}
    ref, got, cache = _both(script)
    trace = got['_trace']
    assert trace[-1] >= 8 and trace[-1] > trace[8], trace          # (... and the replays went on after the inference calls)
    _agree(got, ref)


# -- what the captured launches bake in ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', ['robot_mass', 'gravity', 'omega_max', 'robot_size'])
def test_module_scalar_changed_after_arming(name):
    """`DPhysics._make_desc` reads these on every launch-by-launch call; a captured step that went on replaying the old value would not move.
    (No parameter update in this loop: on the referee the loss is constant up to the change and moves by more than ten tolerances with it.)"""
    AT = 8

    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        z, mu = _leaves(z0, mu0)
        cfg, hist = dp.dphys_cfg, []
        for i in range(16):
            if i == AT:
                cache = dp.__dict__.get('_api_step_cache')
                armed = cache.replays if cache is not None else 0
                if name == 'robot_size':
                    cfg.robot_size = (cfg.robot_size[0], 1.5 * cfg.robot_size[1])
                elif name == 'omega_max':
                    cfg.omega_max = 0.25 * cfg.omega_max
                else:
                    setattr(cfg, name, 1.5 * getattr(cfg, name))
            z.grad = mu.grad = None
            loss, states, forces = _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
            loss.backward()
            hist.append(_rec(loss.detach(), z.grad, mu.grad, states[0].detach().clone(), forces[0].detach().clone()))
        return {'hist': hist, '_armed': armed}
    ref, got, cache = _both(script)
    assert got['_armed'] >= 4 and ref['_armed'] == 0, (got['_armed'], ref['_armed'])
    L = [r[0] for r in ref['hist']]
    assert abs(L[AT] - L[AT - 1]) > 10 * TOL * abs(L[AT - 1]), (name, L)
    _agree(got, ref)
    assert cache.replays >= 8 and cache.captures == 2, (cache.replays, cache.captures)          # launch by launch for three cycles, captured again


@gpu
def test_non_leaf_maps_do_not_capture_again_and_again():
    """scripts/train.py: the map is the encoder's output, a fresh tensor in every iteration.  The graph reads its inputs by address, so such a
    loop must not capture a step every few iterations that nothing ever replays.  (Before maps had to be leaves, this loop stayed idle only
    by the allocator's doing: the module's `z_grid` attribute still holds the previous map when the next one is made, so the addresses
    alternate and no three cycles look alike.  test_leaves_that_keep_moving_switch_the_cache_off is the case that did capture for ever.)"""
    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        zp, mp = _leaves(z0, mu0)
        hist = []
        for i in range(20):
            zp.grad = mp.grad = None
            z, mu = zp * 1.0, mp * 1.0
            loss, states, forces = _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
            loss.backward()
            hist.append(_rec(loss.detach(), zp.grad, mp.grad, states[0].detach().clone(), forces[0].detach().clone()))
            _drift(zp, mp, i)
        return {'hist': hist}
    ref, got, cache = _both(script)
    _agree(got, ref)
    assert cache.replays >= 10 or (cache.entry is None and cache.pending is None), cache.replays
    assert cache.captures <= 2, cache.captures


@gpu
def test_leaves_that_keep_moving_switch_the_cache_off():
    """Leaf maps in another buffer every four iterations: each capture is replayed by its own first forward only.  After two such captures the
    cache gives up (one warning) instead of capturing for ever; the results stay the referee's."""
    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        pairs = [_leaves(z0 + 0.01 * k, mu0) for k in range(4)]
        hist = []
        for i in range(16):
            z, mu = pairs[i // 4]
            z.grad = mu.grad = None
            loss, states, forces = _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
            loss.backward()
            hist.append(_rec(loss.detach(), z.grad, mu.grad, states[0].detach().clone(), forces[0].detach().clone()))
        return {'hist': hist}
    ref, _ = _run(script, False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        got, cache = _run(script, True)
    _agree(got, ref)
    assert len([x for x in w if 'DPhysics' in str(x.message)]) == 1, [str(x.message) for x in w]
    assert cache.captures == 2 and cache.replays == 2 and cache.failed, (cache.captures, cache.replays, cache.failed)


# -- the private call -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('how', ['absent', 'raises', 'raises_after_arming'])
def test_private_use_count_call_absent_or_raising(how, monkeypatch):
    """`torch._C._storage_Use_Count` is private: without it `forward` must not die -- the cache switches itself off with ONE warning and
    every iteration stays the referee's."""
    def boom(*a, **k):
        raise AttributeError('gone')

    def script(dp, z0, mu0, ctrl, states_gt, pred_ts, gt_ts):
        z, mu = _leaves(z0, mu0)
        hist = []
        for i in range(10):
            if how == 'raises_after_arming' and i == 6:
                monkeypatch.setattr(torch._C, '_storage_Use_Count', boom)
            z.grad = mu.grad = None
            loss, states, forces = _step(dp, z, mu, ctrl, states_gt, pred_ts, gt_ts)
            loss.backward()
            hist.append(_rec(loss.detach(), z.grad, mu.grad, states[0].detach().clone(), forces[0].detach().clone()))
            _drift(z, mu, i)
        return {'hist': hist}
    ref, _ = _run(script, False)
    monkeypatch.undo()
    if how == 'absent':
        monkeypatch.delattr(torch._C, '_storage_Use_Count')
    elif how == 'raises':
        monkeypatch.setattr(torch._C, '_storage_Use_Count', boom)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        got, cache = _run(script, True)
    monkeypatch.undo()
    assert len([x for x in w if 'DPhysics' in str(x.message)]) == 1, [str(x.message) for x in w]
    assert cache.failed and cache.entry is None
    assert cache.replays == (3 if how == 'raises_after_arming' else 0), cache.replays
    _agree(got, ref)
