"""No-GPU checks of the traversability feature (monoforce_amd/costmap.py, mf_traversability_*): the ATen form against the float64 referee of
tests/traversability_reference.py, the known / unknown rule on constructed maps, argument errors, the C ABI through ctypes, and the new
kernels' code-object metadata."""
import ctypes
import os
import re
import sys

import pytest
import torch

from tests import traversability_reference as tr
from tests.conftest import REPO

NAN = float('nan')
RAMPS = dict(slope=(0.2, 0.6), roughness=(0.02, 0.10), step=(0.10, 0.30))


def _aten(z, r, th=None, **kw):
    from monoforce_amd import costmap as cm
    ramps = RAMPS if th is None else dict(slope=(th[0][0], th[1][0]), roughness=(th[0][1], th[1][1]), step=(th[0][2], th[1][2]))
    return cm.traversability_map_aten(z, 0.1, radius_cells=r, return_terms=True, **ramps, **kw)


# ---- 1. the ATen form against the referee -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', tr.RADII)
@pytest.mark.parametrize('shape', list(tr.SIZES), ids=lambda s: f'{s[0]}x{s[1]}')
def test_aten_form_equals_the_referee(shape, r):
    """float32 ATen against the float64 referee: the NaN pattern of the terms and the unknown cells' cost exactly, the numbers to 2e-5
    absolute on terms of order 0.01 .. 1 (float32 sums of up to 805 heights of up to ~1 m, centred: ~1e-7 per term, amplified in the cost
    by 1 / (hi - lo) of the quantile ramps, 1e-6 measured)."""
    from monoforce_amd import costmap as cm
    assert cm.TILE == tr.TILE
    for pattern in tr.HOLES:
        c = tr.case(shape, r, pattern)
        z32, v32 = c['z'].float(), None if c['valid'] is None else c['valid'].float()
        if c['th'] is not None:
            inside, shares = tr.deciding_shares(c['terms'], c['known'], *c['th'])
            assert inside >= 0.30 and min(shares) >= 0.03, (pattern, inside, shares)
        for base in (None, c['base']):
            cost, terms = _aten(z32, r, c['th'], valid=v32, base=None if base is None else base.float())
            assert cost.dtype == torch.float32 and cost.shape == z32.shape and terms.shape == (z32.shape[0], 3) + z32.shape[1:]
            assert torch.equal(torch.isnan(terms), torch.isnan(c['terms']))
            k = c['known']
            for j in range(3 if bool(k.any()) else 0):
                assert float((terms[:, j].double() - c['terms'][:, j])[k].abs().max()) <= 2e-5
            lo, hi = c['th'] if c['th'] is not None else ([v[0] for v in RAMPS.values()], [v[1] for v in RAMPS.values()])
            want = tr.cost_from_terms(c['terms'], k, lo, hi, 0.5, base)
            assert torch.equal(cost.double()[~k], want[~k])
            if c['th'] is not None:
                assert float((cost.double() - want).abs().max()) <= 2e-5


def test_public_function_on_cpu_tensors_and_shapes():
    import monoforce_amd
    from monoforce_amd import costmap as cm
    c = tr.case((70, 37), 2, 'random')
    z = c['z']
    cost3, terms3 = monoforce_amd.traversability_map(z, 0.1, 0.2, return_terms=True)          # 0.2 m = 2 cells
    assert cost3.dtype == torch.float64 and cost3.shape == z.shape and terms3.shape == (3, 3, 70, 37) and not cost3.requires_grad
    cost2, terms2 = cm.traversability_map(z[1].float(), 0.1, 0.2, return_terms=True)
    assert cost2.shape == (70, 37) and terms2.shape == (3, 70, 37) and torch.equal(cost2, cost3[1].float())
    assert float(cost3.min()) >= 0 and float(cost3.max()) <= 1
    assert torch.equal(torch.isnan(terms3), torch.isnan(c['terms']))
    out = torch.full((70, 37), 7.0)
    assert cm.traversability_map(z[1].float(), 0.1, 0.2, out=out) is out and torch.equal(out, cost2)
    assert cm.cells_of_radius(0.04, 0.1) == 1 and cm.cells_of_radius(0.25, 0.1) == 2 and cm.cells_of_radius(1.6, 0.1) == 16
    with pytest.raises(ValueError, match='limited to 16 cells'):
        cm.traversability_map(z, 0.1, 1.7)
    # the owner of static buffers takes its radius from the robot: half the shorter side of robot_size
    from monoforce_amd.dphys_config import DPhysConfig
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    cfg = DPhysConfig(robot='tradr', grid_res=0.1, robot_points=pts, driving_parts=masks)
    tm = cm.TraversabilityMap(cfg)
    assert tm.radius == 0.5 * min(cfg.robot_size) and tm.r == cm.cells_of_radius(tm.radius, 0.1) and tm.cost is None
    assert cm.TraversabilityMap(cfg, radius=0.7).r == 7


# ---- 2. the unknown rule on constructed maps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fn', ['aten', 'referee'])
def test_unknown_rule_on_constructed_maps(fn):
    def run(z, r, min_valid=3, valid=None):
        if fn == 'aten':
            cost, terms = _aten(z.float(), r, min_valid=min_valid, valid=valid)
            return cost.double(), ~torch.isnan(terms[0])
        cost, terms, known = tr.traversability(z, 0.1, r, [v[0] for v in RAMPS.values()], [v[1] for v in RAMPS.values()], min_valid=min_valid, valid=valid)
        assert torch.equal(known, ~torch.isnan(terms[0])) and torch.equal(known, ~torch.isnan(terms[2]))
        return cost, known
    H, W, r = 9, 11, 2
    g = torch.Generator().manual_seed(0)
    full = (0.1 * torch.randn(H, W, generator=g, dtype=torch.float64)).float().double()
    # one valid row only: every window is collinear
    row = torch.full((H, W), NAN, dtype=torch.float64)
    row[4] = full[4]
    cost, known = run(row, r)
    assert not bool(known.any()) and torch.equal(cost, torch.full((H, W), 0.5, dtype=torch.float64))
    # ... given through `valid` instead, over arbitrary heights
    v = torch.zeros(H, W)
    v[4] = 1.0
    assert not bool(run(full, r, valid=v.double() if fn == 'referee' else v)[1].any())
    # that row plus one off-row cell: exactly the cells whose window holds the cell AND at least two cells of the row
    row[2, 5] = full[2, 5]
    cost, known = run(row, r)
    want = torch.zeros(H, W, dtype=torch.bool)
    for i in range(H):
        for j in range(W):
            in_row = sum(1 for dj in range(-r, r + 1) if (4 - i) ** 2 + dj * dj <= r * r and 0 <= j + dj < W)
            want[i, j] = (2 - i) ** 2 + (5 - j) ** 2 <= r * r and in_row >= 2
    assert bool(want.any()) and torch.equal(known, want) and torch.equal(cost[~known], torch.full((int((~known).sum()),), 0.5, dtype=torch.float64))
    assert bool(known[3, 5]) and not bool(row[3, 5] == row[3, 5])          # known depends on the window, not on the centre cell's own validity
    # an all-NaN map
    cost, known = run(torch.full((H, W), NAN, dtype=torch.float64), r)
    assert not bool(known.any()) and float(cost.min()) == float(cost.max()) == 0.5
    # n = min_valid - 1 against n = min_valid: an L of three cells, then a fourth; windows of radius 1 around (4, 5)
    few = torch.full((H, W), NAN, dtype=torch.float64)
    few[4, 5], few[4, 6], few[5, 5] = 0.1, 0.2, 0.3
    assert bool(run(few, 1, min_valid=3)[1][4, 5]) and not bool(run(few, 1, min_valid=4)[1][4, 5])
    few[3, 5] = 0.15
    assert bool(run(few, 1, min_valid=4)[1][4, 5]) and not bool(run(few, 1, min_valid=5)[1][4, 5])
    # a single-row map can never be known
    assert not bool(run(full[:1], 2)[1].any())


# ---- 3. argument errors -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_each_have_their_own_message():
    from monoforce_amd import costmap as cm
    z = torch.zeros(8, 9)
    for form in (cm.traversability_map, cm.traversability_map_aten):
        with pytest.raises(ValueError, match=r'radius must be 1\.\.16 cells, got 0'):
            form(z, 0.1, radius_cells=0)
        with pytest.raises(ValueError, match=r'radius must be 1\.\.16 cells, got 17'):
            form(z, 0.1, radius_cells=17)
        with pytest.raises(ValueError, match='roughness ramp needs hi > lo'):
            form(z, 0.1, 0.2, roughness=(0.05, 0.05))
        with pytest.raises(ValueError, match='slope ramp needs hi > lo'):
            form(z, 0.1, 0.2, slope=(0.5, 0.1))
        with pytest.raises(ValueError, match=r'valid has shape \(8, 8\), z has \(8, 9\)'):
            form(z, 0.1, 0.2, valid=torch.ones(8, 8))
        with pytest.raises(ValueError, match=r'base has shape \(1, 8, 9\), z has \(8, 9\)'):
            form(z, 0.1, 0.2, base=torch.ones(1, 8, 9))
        with pytest.raises(ValueError, match='z must have unit stride along W'):
            form(torch.zeros(8, 18)[:, ::2], 0.1, 0.2)
        with pytest.raises(ValueError, match='min_valid must be at least 3'):
            form(z, 0.1, 0.2, min_valid=2)
        with pytest.raises(ValueError, match=r'\[H,W\] or \[S,H,W\]'):
            form(torch.zeros(2, 1, 8, 9), 0.1, 0.2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        cm.traversability_into(z, None, None, 0.1, 2, [0, 0, 0], [1, 1, 1], 0.5, 3, torch.empty(8, 9))


# ---- 4. the C ABI without a GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def built_lib():
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import _lib
    return _lib.lib()


def test_c_abi_symbol_struct_and_validation(built_lib):
    from monoforce_amd import _lib, costmap as cm
    header = open(os.path.join(REPO, 'include', 'monoforce_hip.h')).read()
    assert int(re.search(r'#define MF_TRAVERSABILITY_TILE (\d+)', header).group(1)) == cm.TILE == _lib.MF_TRAVERSABILITY_TILE
    assert int(re.search(r'#define MF_TRAVERSABILITY_MAX_RADIUS (\d+)', header).group(1)) == cm.MAX_RADIUS_CELLS
    for name in ('mf_traversability_f32', 'mf_traversability_f64'):
        assert hasattr(built_lib, name) and name in _lib.SYMBOLS and getattr(built_lib, name).restype is ctypes.c_int
    built_lib.mf_sizeof.restype = ctypes.c_int
    built_lib.mf_sizeof.argtypes = [ctypes.c_char_p]
    assert built_lib.mf_sizeof(b'MfTraversabilityDesc') == ctypes.sizeof(_lib.MfTraversabilityDesc) == 104
    f3 = lambda *v: (ctypes.c_float * 3)(*v)  # noqa: E731

    def call(fn=built_lib.mf_traversability_f32, z=1, cost=1, **kw):
        d = dict(S=1, H=8, W=9, r=2, min_valid=3, grid_res=0.1, unknown=0.5, lo=f3(0, 0, 0), hi=f3(1, 1, 1), z_stride_h=9)
        d.update(kw)
        p = lambda a: ctypes.c_void_p(0x1000) if a else None  # noqa: E731      (never dereferenced: validation fails before any launch)
        rc = fn(ctypes.byref(_lib.MfTraversabilityDesc(**d)), p(z), None, None, p(cost), None, None)
        return rc, built_lib.mf_last_error().decode()
    for fn in (built_lib.mf_traversability_f32, built_lib.mf_traversability_f64):
        assert fn(None, None, None, None, None, None, None) == 1 and 'null descriptor' in built_lib.mf_last_error().decode()
        for kw, text in ((dict(z=0), 'null input'), (dict(cost=0), 'null input'), (dict(r=0), 'radius r must be in 1..16 cells, got 0'),
                         (dict(r=17), 'radius r must be in 1..16 cells, got 17'), (dict(hi=f3(1, 0, 1)), 'hi must be above lo'),
                         (dict(lo=f3(0, 0, 1)), 'hi must be above lo'), (dict(min_valid=2), 'min_valid must be at least 3'),
                         (dict(H=0), 'must be positive'), (dict(S=-1), 'must be positive'), (dict(W=0), 'must be positive'),
                         (dict(grid_res=0.0), 'grid_res must be positive')):
            rc, msg = call(fn, **kw)
            assert rc == 1 and text in msg, (kw, rc, msg)


# ---- 5. kernel metadata -------------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_fit_the_lds():
    """Code-object metadata only (tools/kernel_metadata.py, as tests/test_no_scratch_cpu.py): both instantiations, no scratch, the halo image of
    the largest radius -- (TILE + 32)^2 scalars -- plus the disc's row table within 64 KB."""
    import __graft_entry__ as g
    g.build()
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_metadata
    rows = {name: m for o, name, m in kernel_metadata.kernels() if o == 'traversability.o'}
    assert set(rows) == {'mf::traversability_kernel<float>', 'mf::traversability_kernel<double>'}, rows
    for name, m in rows.items():
        size = 4 if 'float' in name else 8
        assert m['scratch'] == 0 and m['agpr'] == 0 and m['vgpr'] <= 128, (name, m)
        assert (tr.TILE + 32) ** 2 * size <= m['lds'] <= min(64 * 1024, (tr.TILE + 32) ** 2 * size + 512), (name, m)
