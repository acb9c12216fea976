"""The traversability kernel on the MI355X (mf_traversability_*: one launch) against the float64 referee of tests/traversability_reference.py:
terms, cost, the known / unknown pattern, strided views, in-place buffers, determinism, capture, the torch op and the planner.

Bars.  float64: 1e-12 absolute.  float32: for every case the error e32 of the ATen float32 form (`traversability_map_aten`, on the GPU, same
inputs) against the referee is measured per term layer and for the cost, and the kernel is held to max(2 e32, 1e-6) absolute.  The ramps of
the cost check are the 20 % / 80 % quantiles of each term over the referee's known cells; on the referee alone at least 30 % of the known
cells then have a cost strictly inside (0,1) and each term decides at least 3 % of those (asserted).  Where the window covers the whole map
the quantiles coincide: the terms are checked there and the cost ramp is not.  All errors are printed per case (lines starting with
`traversability-error`; profiles/traversability_errors.txt is that output)."""
import pytest
import torch

from tests import traversability_reference as tr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float32, torch.float64]
DEFAULT = ([0.2, 0.02, 0.10], [0.6, 0.10, 0.30])
SHAPES = list(tr.SIZES)
ids = lambda s: f'{s[0]}x{s[1]}'  # noqa: E731


def _ramps(th):
    lo, hi = th
    return dict(slope=(lo[0], hi[0]), roughness=(lo[1], hi[1]), step=(lo[2], hi[2]))


def _errors(cost, terms, c, want_cost):
    """max |x - referee| over the known cells per term layer, and over every cell for the cost (None without a cost check)."""
    k = c['known']
    e = [float((terms[:, j].double().cpu() - c['terms'][:, j])[k].abs().max()) if bool(k.any()) else 0.0 for j in range(3)]
    return e + [None if want_cost is None else float((cost.double().cpu() - want_cost).abs().max())]


def _check_case(c, dtype, r, what, view=None):
    """One case through the kernel (and, float32, the ATen form), with and without `base`; `view`: maps a dense CPU tensor to the GPU tensor
    the kernel reads (default: a plain copy)."""
    from monoforce_amd import costmap as cm
    put = (lambda t: t.to(DEV)) if view is None else view
    z = put(c['z'].to(dtype))
    valid = None if c['valid'] is None else put(c['valid'].to(dtype))
    lo, hi = c['th'] if c['th'] is not None else DEFAULT
    if c['th'] is not None:
        inside, shares = tr.deciding_shares(c['terms'], c['known'], lo, hi)
        assert inside >= 0.30 and min(shares) >= 0.03, (what, inside, shares)
    for with_base in (False, True):
        base = put(c['base'].to(dtype)) if with_base else None
        cost, terms = cm.traversability_map(z, 0.1, radius_cells=r, valid=valid, base=base, return_terms=True, **_ramps((lo, hi)))
        assert cost.dtype == dtype and cost.shape == z.shape and terms.shape == (z.shape[0], 3) + tuple(z.shape[1:]) and cost.is_contiguous()
        assert torch.equal(torch.isnan(terms).cpu(), torch.isnan(c['terms'])), what                 # the known / unknown pattern, exactly
        want = tr.cost_from_terms(c['terms'], c['known'], lo, hi, 0.5, c['base'] if with_base else None)
        assert torch.equal(cost.double().cpu()[~c['known']], want[~c['known']]), what               # `unknown` exactly, after `base`
        errs = _errors(cost, terms, c, want if c['th'] is not None else None)
        if dtype == torch.float32:
            a_cost, a_terms = cm.traversability_map_aten(z, 0.1, radius_cells=r, valid=valid, base=base, return_terms=True, **_ramps((lo, hi)))
            aten = _errors(a_cost, a_terms, c, want if c['th'] is not None else None)
            bars = [None if a is None else max(2 * a, 1e-6) for a in aten]
        else:
            aten, bars = [None] * 4, [1e-12] * 3 + [None if errs[3] is None else 1e-12]
        f = lambda v: '   -    ' if v is None else '%.2e' % v  # noqa: E731
        print('traversability-error %-7s %-22s base=%d | %s' % (str(dtype).replace('torch.', ''), what, with_base, ' | '.join(
            '%s hip %s aten %s bar %s' % (n, f(e), f(a), f(b)) for n, e, a, b in zip(('slope', 'rough', 'step', 'cost'), errs, aten, bars))))
        for n, e, b in zip(('slope', 'roughness', 'step', 'cost'), errs, bars):
            assert e is None or e <= b, (what, with_base, n, e, b)
        if with_base and bool(torch.isnan(c['base']).logical_not().any()):
            assert float((cost.double().cpu() - c['base'])[~torch.isnan(c['base'])].min()) >= 0      # the keep-out map is a floor


# ---- 1. every size, radius and hole pattern ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('r', tr.RADII)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_kernel_equals_the_referee(shape, r, dtype):
    from monoforce_amd import costmap as cm
    assert cm.TILE == tr.TILE
    for pattern in tr.HOLES:
        _check_case(tr.case(shape, r, pattern), dtype, r, f'{ids(shape)} r={r} S={tr.batch_of(pattern)} {pattern}')


# ---- 2. views read in place -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('r', [2, 7])
def test_channel_views_and_row_strided_crops_are_read_in_place(r, dtype):
    shape = (tr.TILE + 1, 2 * tr.TILE - 1)

    def channel(t):        # [:, 0] of a [S,2,H,W] tensor whose other channel is poison
        buf = torch.full((t.shape[0], 2) + tuple(t.shape[1:]), 1e30, dtype=t.dtype, device=DEV)
        buf[:, 0] = t.to(DEV)
        return buf[:, 0]

    def crop(t):           # a row-strided crop of a larger poisoned tensor
        buf = torch.full((t.shape[0], t.shape[1] + 5, t.shape[2] + 7), 1e30, dtype=t.dtype, device=DEV)
        buf[:, 2:-3, 3:-4] = t.to(DEV)
        return buf[:, 2:-3, 3:-4]
    for pattern in ('random', 'valid'):
        c = tr.case(shape, r, pattern)
        for name, view in (('[S,1,H,W] channel', channel), ('row-strided crop', crop)):
            v = view(c['z'].to(dtype))
            assert v.stride(-1) == 1 and (v.shape[0] == 1 or not v.is_contiguous())      # (a [1,2,H,W][:, 0] view counts as contiguous)
            _check_case(c, dtype, r, f'{ids(shape)} r={r} {pattern} {name}', view=view)
    # a plain [H,W] map is the S = 1 case
    from monoforce_amd import costmap as cm
    c = tr.case(shape, r, 'none')
    cost2, terms2 = cm.traversability_map(c['z'][0].to(dtype).to(DEV), 0.1, radius_cells=r, return_terms=True)
    cost3, terms3 = cm.traversability_map(c['z'].to(dtype).to(DEV), 0.1, radius_cells=r, return_terms=True)
    assert cost2.shape == shape and terms2.shape == (3,) + shape and torch.equal(cost2, cost3[0]) and torch.equal(terms2, terms3[0])


# ---- 3. buffers, determinism, the op ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_in_place_buffers_determinism_and_the_op(dtype):
    from monoforce_amd import costmap as cm
    from monoforce_amd import ops
    from monoforce_amd.dphys_config import DPhysConfig
    from monoforce_amd import synthetic as syn
    c = tr.case((70, 37), 7, 'random')
    z, base = c['z'].to(dtype).to(DEV), c['base'].to(dtype).to(DEV)
    lo, hi = c['th']
    cost, terms = cm.traversability_map(z, 0.1, radius_cells=7, base=base, return_terms=True, **_ramps((lo, hi)))
    again = cm.traversability_map(z, 0.1, radius_cells=7, base=base, return_terms=True, **_ramps((lo, hi)))
    assert torch.equal(cost, again[0]) and torch.equal(terms.isnan(), again[1].isnan()) and torch.equal(terms.nan_to_num(0.0), again[1].nan_to_num(0.0))
    # out=: the caller's buffer is written, whatever it held
    out = torch.full_like(z, 7.0)
    ptr = out.data_ptr()
    got = cm.traversability_map(z, 0.1, radius_cells=7, base=base, out=out, **_ramps((lo, hi)))
    assert got is out and out.data_ptr() == ptr and torch.equal(out, cost)
    # the torch op and its _into form
    o_cost, o_terms = torch.ops.monoforce.traversability(z, None, base, 0.1, 7, lo, hi, 0.5, 3, True)
    assert torch.equal(o_cost, cost) and torch.equal(o_terms.nan_to_num(0.0), terms.nan_to_num(0.0))
    o_cost, o_terms = torch.ops.monoforce.traversability(z, None, base, 0.1, 7, lo, hi, 0.5, 3, False)
    assert torch.equal(o_cost, cost) and o_terms.numel() == 0
    b_cost, b_terms = torch.full_like(cost, 3.0), torch.full_like(terms, 3.0)
    ops.traversability_into(z, None, base, 0.1, 7, lo, hi, 0.5, 3, b_cost, b_terms)
    assert torch.equal(b_cost, cost) and torch.equal(b_terms.nan_to_num(0.0), terms.nan_to_num(0.0))
    # TraversabilityMap: static buffers, rewritten in place by every call
    pts, masks = syn.robot_points_4()
    cfg = DPhysConfig(robot='tradr', grid_res=0.1, robot_points=pts, driving_parts=masks)
    tm = cm.TraversabilityMap(cfg, radius=0.7, slope=(lo[0], hi[0]), roughness=(lo[1], hi[1]), step=(lo[2], hi[2]))
    first = tm(z, base=base)
    assert first is tm.cost and torch.equal(tm.cost, cost) and torch.equal(tm.terms.nan_to_num(0.0), terms.nan_to_num(0.0))
    ptrs = (tm.cost.data_ptr(), tm.terms.data_ptr())
    other = tr.case((70, 37), 7, 'inf')['z'].to(dtype).to(DEV).expand(3, 70, 37).contiguous()
    second = tm(other)
    assert second is tm.cost and (tm.cost.data_ptr(), tm.terms.data_ptr()) == ptrs
    assert torch.equal(tm.cost, cm.traversability_map(other, 0.1, radius_cells=7, **_ramps((lo, hi)))) and not torch.equal(tm.cost, cost)
    with pytest.raises(TypeError, match='float32 or float64'):
        cm.traversability_map(z.half(), 0.1, radius_cells=7)


# ---- 4. capture ------------------------------------------------------------------------------------------------------------------------------
def _poses(B, Tp, seed):
    g = torch.Generator().manual_seed(seed)
    Xs = torch.cat([(torch.rand(B, Tp, 2, generator=g) - 0.5) * 5.0, 0.1 * torch.randn(B, Tp, 1, generator=g)], -1)
    yaw = torch.rand(B, Tp, generator=g) * 6.28
    Rs = torch.zeros(B, Tp, 3, 3)
    Rs[..., 0, 0], Rs[..., 0, 1], Rs[..., 1, 0], Rs[..., 1, 1], Rs[..., 2, 2] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw), 1.0
    pts = torch.tensor([[0.3, 0.2, 0.0], [0.3, -0.2, 0.0], [-0.3, 0.2, 0.0], [-0.3, -0.2, 0.0]])
    return Xs, Rs, pts


def test_map_then_pose_costs_replay_as_one_graph():
    """`tm(z)` followed by `pose_costs` on `tm.cost`, captured once: after `z.copy_(other)` a replay gives what the eager calls give on `other`."""
    from monoforce_amd import costmap as cm
    from monoforce_amd import ops  # noqa: F401
    from monoforce_amd.capture import capture
    from monoforce_amd.dphys_config import DPhysConfig
    from monoforce_amd import synthetic as syn
    pts4, masks = syn.robot_points_4()
    cfg = DPhysConfig(robot='tradr', grid_res=0.1, robot_points=pts4, driving_parts=masks)
    H = W = 64
    z0, z1 = (tr.terrain(1, H, W, s)[0].float().to(DEV) for s in (11, 12))
    z1[5:9, 7] = float('nan')
    Xs, Rs, pts = (t.to(DEV) for t in _poses(32, 6, 3))
    tm = cm.TraversabilityMap(cfg, radius=0.3)
    z = z0.clone()

    def run():
        cost = tm(z)
        return torch.ops.monoforce.pose_costs(Xs, Rs, pts, cost, None, None, 0.1, 3.2, 2.0, 1.0, [1.0, 0.0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with capture(graph, stream=s, capture_error_mode='thread_local'):
        static = run()
    ptr = tm.cost.data_ptr()
    z.copy_(z1)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in static] + [tm.cost.clone()]
    assert tm.cost.data_ptr() == ptr
    tm2 = cm.TraversabilityMap(cfg, radius=0.3)
    want_map = tm2(z1).clone()
    want = torch.ops.monoforce.pose_costs(Xs, Rs, pts, want_map, None, None, 0.1, 3.2, 2.0, 1.0, [1.0, 0.0])
    assert torch.equal(got[2], want_map) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(want_map, cm.traversability_map(z0, 0.1, 0.3)) and float(want[0].abs().max()) > 0


# ---- 5. the planner ----------------------------------------------------------------------------------------------------------------------------
def test_planner_step_scores_on_the_traversability_map():
    """`MPPIPlanner.step(cost_map=tm.cost)` on a 64 x 64 map, 64 samples x 20 steps: its `pose_terms` are those of the REFEREE's map run through
    tests/pose_costs_reference.py on the step's own poses, within the pose-cost kernel's own bar (tests/test_pose_costs_gpu.py)."""
    from monoforce_amd import MPPIPlanner, costmap as cm
    from monoforce_amd import synthetic as syn
    from tests import helpers as hp
    from tests import pose_costs_reference as pref
    from tests.test_rollout_gpu import make_dphysics
    pts, masks = syn.robot_points_4()
    dp = make_dphysics(pts, masks, 1, 0.1, 3.2)
    dp.dphys_cfg.traj_sim_time = 0.2
    dp = type(dp)(dp.dphys_cfg, device=DEV)                      # rebuild the time grid: T = 20
    B = 64
    mp = MPPIPlanner(dp, n_trajs=B, weights=dict(inclination=1.0, force=0.02, goal=1.0, map=0.5, path=0.0), lethal=2.0)
    z64 = tr.terrain(1, 64, 64, 21)[0] * 0.5
    z64 = z64.float().double()
    z = z64.float().to(DEV)
    tm = cm.TraversabilityMap(dp)
    g = torch.Generator().manual_seed(5)
    noise = (torch.randn(B, 20, 2, generator=g) + 2.0 * torch.randn(B, 1, 2, generator=g)).to(DEV)
    out = mp.step(z, torch.tensor([1.0, 0.5], device=DEV), noise=noise, cost_map=tm(z))
    assert out['controls'].shape == (B, 20, 2) and out['pose_terms'].shape == (B, 2)
    ref_map, _, known = tr.traversability(z64, 0.1, tm.r, tm.lo, tm.hi, tm.unknown, tm.min_valid)
    assert bool(known.all()) and float(ref_map.max()) > float(ref_map.min()) and float(ref_map.max()) <= 1.0
    args = (out['Xs'].cpu(), out['Rs'].cpu(), mp.footprint.cpu(), None, None, None)
    scal = (0.1, 3.2, 2.0, float('inf'))
    _, t32 = pref.pose_costs(args[0], args[1], args[2], ref_map.float(), None, None, *scal, (0.5, 0.0))
    _, t64 = pref.pose_costs(args[0].double(), args[1].double(), args[2].double(), ref_map, None, None, *scal, (0.5, 0.0))
    got = out['pose_terms'][:, 0].cpu()
    assert bool(torch.isfinite(t64[:, 0]).all()) and float(t64[:, 0].max()) > 0
    err, bar = hp.rel_err(got, t64[:, 0]), max(1e-5, 3 * hp.rel_err(t32[:, 0], t64[:, 0]))
    print(f'planner step on the traversability map: map term err {err:.3g} bar {bar:.3g}')
    assert err <= bar
