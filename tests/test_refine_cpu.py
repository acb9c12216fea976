"""No-GPU checks of the control refiner's pieces (monoforce_amd/refine.py, csrc/traj_objective.hip, csrc/control_refine.hip): the two descriptors
and their validation texts, `trajectory_objective_aten` against the float64 referee of tests/traj_objective_reference.py -- the gradient rules
at the documented kinks included --, the shape table of the GPU tests against the kernel's source, and the share of rows the referee takes out
of the gradient comparison."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

from tests import traj_objective_reference as tr
from tests.conftest import REPO

INF = float('inf')


@pytest.fixture(scope='module')
def built_lib():
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import _lib
    return _lib.lib()


def test_descriptor_mirrors_match_the_header(built_lib):
    from monoforce_amd import _lib
    built_lib.mf_sizeof.restype = ctypes.c_int
    built_lib.mf_sizeof.argtypes = [ctypes.c_char_p]
    assert built_lib.mf_sizeof(b'MfTrajObjDesc') == ctypes.sizeof(_lib.MfTrajObjDesc) == 96
    assert built_lib.mf_sizeof(b'MfRefineDesc') == ctypes.sizeof(_lib.MfRefineDesc) == 72
    assert built_lib.mf_sizeof(b'MfPoseCostDesc') == 80 and built_lib.mf_sizeof(b'MfFitDesc') == 96           # untouched
    for name in ('mf_traj_objective_f32', 'mf_control_refine_update_f32'):
        assert name in _lib.SYMBOLS and hasattr(built_lib, name)


def test_objective_validation_without_gpu(built_lib):
    """Every rejected argument is reported before any launch: an error code and a message, on a box without a GPU."""
    from monoforce_amd import _lib
    p = ctypes.c_void_p(1 << 20)       # never dereferenced: validation fails first
    nan = float('nan')

    def desc(**kw):
        d = dict(B=8, T=50, N=4, P=3, H=16, W=16, pose_stride=7, x_stride_b=3, x_stride_t=24, r_stride_b=9, r_stride_t=72, grid_res=0.1, d_max=0.8,
                 lethal=INF, off_map=INF, w_map=1.0, w_path=1.0, w_goal=1.0, w_incl=1.0)
        d.update(kw)
        return _lib.MfTrajObjDesc(**d)

    def call(d, Xs=p, Rs=p, points=p, cost_map=p, path=p, goal=p, gcosts=p, costs=p, terms=p, gXs=p, gRs=p):
        return built_lib.mf_traj_objective_f32(ctypes.byref(d) if d is not None else None, Xs, Rs, points, cost_map, path, goal, gcosts, costs, terms,
                                               gXs, gRs, None)

    INVALID, UNSUPPORTED = 1, 2
    cases = [(dict(d=None), INVALID, b'null descriptor'),
             (dict(d=desc(), Xs=None), INVALID, b'null'), (dict(d=desc(), Rs=None), INVALID, b'null'), (dict(d=desc(), points=None), INVALID, b'null'),
             (dict(d=desc(), goal=None), INVALID, b'null'), (dict(d=desc(), costs=None), INVALID, b'null'),
             (dict(d=desc(), gXs=None), INVALID, b'both'), (dict(d=desc(), gRs=None), INVALID, b'both'),
             (dict(d=desc(B=0)), INVALID, b'positive'), (dict(d=desc(T=0)), INVALID, b'positive'), (dict(d=desc(N=0)), INVALID, b'positive'),
             (dict(d=desc(pose_stride=0)), INVALID, b'pose_stride'),
             (dict(d=desc(N=1025)), UNSUPPORTED, b'1024'), (dict(d=desc(P=257)), UNSUPPORTED, b'256'),
             (dict(d=desc(P=-1)), INVALID, b'negative'), (dict(d=desc(H=1)), INVALID, b'H >= 2'), (dict(d=desc(W=1)), INVALID, b'W >= 2'),
             (dict(d=desc(x_stride_b=-3)), INVALID, b'stride'), (dict(d=desc(r_stride_t=-1)), INVALID, b'stride'),
             (dict(d=desc(grid_res=0.0)), INVALID, b'grid_res'), (dict(d=desc(grid_res=nan)), INVALID, b'grid_res'),
             (dict(d=desc(lethal=nan)), INVALID, b'NaN'), (dict(d=desc(off_map=nan)), INVALID, b'NaN'),
             (dict(d=desc(), cost_map=None), INVALID, b'w_map'),                                   # a weight without its input
             (dict(d=desc(P=0), path=None), INVALID, b'w_path'),
             (dict(d=desc(P=0, w_path=0.0)), INVALID, b'path must be NULL'),                       # a path without P
             (dict(d=desc(), path=None), INVALID, b'path must be NULL'),                           # P without a path
             (dict(d=desc(H=1 << 16, W=1 << 15)), UNSUPPORTED, b'2^31'),
             (dict(d=desc(B=1 << 20, x_stride_b=1 << 12)), UNSUPPORTED, b'2^31'), (dict(d=desc(T=1 << 20, r_stride_t=1 << 12)), UNSUPPORTED, b'2^31'),
             (dict(d=desc(x_stride_t=1 << 31)), UNSUPPORTED, b'2^31')]
    for kw, code, word in cases:
        rc = call(**kw)
        assert rc == code and word in built_lib.mf_last_error(), (kw, rc, built_lib.mf_last_error())
        assert built_lib.mf_last_error().startswith(b'traj_objective: ')


def test_update_validation_without_gpu(built_lib):
    from monoforce_amd import refine
    p = ctypes.c_void_p(1 << 20)
    good = dict(K=4, T=50, max_iters=10, lr=(0.05, 0.1), betas=(0.9, 0.999), eps=1e-8, lo=(-1.0, -2.0), hi=(1.0, 2.0))

    def call(d, **null):
        names = ('controls', 'grad', 'costs', 'm', 'v', 'best_controls', 'best_cost', 'best_iter', 'history', 'state')
        return built_lib.mf_control_refine_update_f32(ctypes.byref(d) if d is not None else None, *[None if n in null else p for n in names], None)

    INVALID, UNSUPPORTED = 1, 2
    cases = [(None, {}, INVALID, b'null descriptor'), (dict(K=0), {}, INVALID, b'positive'), (dict(T=0), {}, INVALID, b'positive'),
             (dict(max_iters=-1), {}, INVALID, b'max_iters'), (dict(betas=(1.0, 0.999)), {}, INVALID, b'beta'), (dict(betas=(0.9, -0.1)), {}, INVALID, b'beta'),
             (dict(eps=0.0), {}, INVALID, b'eps'), (dict(lr=(-0.1, 0.1)), {}, INVALID, b'lr'), (dict(lo=(1.5, -2.0)), {}, INVALID, b'lo <= hi'),
             (dict(hi=(1.0, math.nan)), {}, INVALID, b'lo <= hi'), (dict(K=1 << 20, T=1 << 11), {}, UNSUPPORTED, b'2^31'),
             ({}, dict(controls=1), INVALID, b'null argument'), ({}, dict(state=1), INVALID, b'null argument'), ({}, dict(history=1), INVALID, b'null argument')]
    for change, null, code, word in cases:
        d = None if change is None else refine.refine_desc(**{**good, **change})
        rc = call(d, **null)
        assert rc == code and word in built_lib.mf_last_error(), (change, null, rc, built_lib.mf_last_error())
    assert tuple(refine.refine_desc(**good).lr) == (0.05, 0.1)


def test_both_kernels_use_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_metadata
    rows = {n: m for o, n, m in kernel_metadata.kernels() if o in ('traj_objective.o', 'control_refine.o')}
    names = ' '.join(rows)
    assert 'traj_objective_kernel' in names and 'control_refine_update_kernel' in names, names
    assert all(m['scratch'] == 0 for m in rows.values()), rows


# ---- the ATen form against the referee ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 50, 7, 4, 2), (65, 50, 7, 17, 18), (1, 1, 1, 1, 0), (3, 50, 2, 65, 18)])
def test_aten_form_matches_the_referee(shape):
    """float64 against float64: the same formulas twice, to rounding; infinite and finite off_map, a lethal threshold, an upstream gradient."""
    from monoforce_amd import refine
    case = tr.make_case(*shape)
    gc = torch.rand(shape[0], generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 1
    for sc in (dict(), dict(off_map=1.5), dict(off_map=1.5, lethal=1.2)):
        want = tr.gradients(case, gcosts=gc, **sc)
        got = tr.gradients(case, gcosts=gc, fn=refine.trajectory_objective_aten, **sc)
        inf = torch.isinf(want[0])
        assert torch.equal(torch.isinf(got[0]), inf) and torch.equal(torch.isinf(got[1][:, 0]), torch.isinf(want[1][:, 0]))
        assert float((got[0][~inf] - want[0][~inf]).abs().max() if bool((~inf).any()) else 0.0) <= 1e-12
        fin = torch.isfinite(want[1])
        assert float((got[1][fin] - want[1][fin]).abs().max()) <= 1e-12
        assert float((got[2] - want[2]).abs().max()) <= 1e-12 and float((got[3] - want[3]).abs().max()) <= 1e-12
        if 'lethal' in sc and shape[0] >= 3:
            assert bool(inf.any()) and bool(want[3][inf][:, :, :2].any())          # a lethal rollout keeps the gradient of its finite map term
    # float32 stays within float32 of it
    g32 = tr.gradients(case, dtype=torch.float32, fn=refine.trajectory_objective_aten)
    want = tr.gradients(case)
    mask = tr.row_mask(case, tr.excluded_rows(case))
    assert float((g32[2].double() - want[2])[mask].abs().max()) <= 1e-5 and float((g32[3].double() - want[3])[mask].abs().max()) <= 1e-5
    # the public entry sends CPU tensors here
    w = dict(zip(refine.TERM_NAMES, tr.case_weights(case)))
    a = refine.trajectory_objective(case['Xs'], case['Rs'], case['goal'], points=case['points'], cost_map=case['cost_map'], path=case['path'], weights=w,
                                    pose_stride=case['pose_stride'], grid_res=0.1, d_max=3.2)
    b = refine.trajectory_objective_aten(case['Xs'], case['Rs'], case['goal'], points=case['points'], cost_map=case['cost_map'], path=case['path'], weights=w,
                                         pose_stride=case['pose_stride'], grid_res=0.1, d_max=3.2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_aten_gradient_rules_at_the_kinks():
    """Exact ties and exact zeros (tr.kink_case: dyadic numbers), by hand: the FIRST of two tied footprint points takes the gradient; an off-map
    maximum has none; a zero path distance, a zero goal distance and a zero roll / pitch have derivative 0 -- and nothing is NaN."""
    from monoforce_amd import refine
    case, sc = tr.kink_case()
    for dtype in (torch.float64, torch.float32):
        costs, terms, gX, gR = tr.gradients(case, dtype=dtype, fn=refine.trajectory_objective_aten, **sc)
        assert bool(torch.isfinite(gX).all()) and bool(torch.isfinite(gR).all()) and bool(torch.isfinite(costs).all())
        w = [float(torch.tensor(v, dtype=torch.float32)) for v in tr.WEIGHTS]
        c_map = w[0] / 3 / 0.25                              # w_map / Tp / grid_res, times ds/du = 1
        tol = 1e-12 if dtype == torch.float64 else 1e-6
        # pose 0: points 0 and 1 tie at u = 6; the gradient carries point 0's y = -0.125, not point 1's +0.25
        assert abs(float(gR[0, 0, 0, 0]) - c_map * 0.5) <= tol and abs(float(gR[0, 0, 0, 1]) - c_map * -0.125) <= tol
        # ... and that is all of pose 0: on a path vertex (distance 0), third row (0, 0, 1) (roll = pitch = 0)
        assert abs(float(gX[0, 0, 0]) - c_map) <= tol and float(gX[0, 0, 1]) == 0.0 and not bool(gR[0, 0, 1:].any())
        # pose 1: the maximum is off the map (off_map = 100): only the path pulls, by w_path / Tp along the unit offset (1, -1) / sqrt(2)
        assert not bool(gR[0, 1].any())
        assert abs(float(gX[0, 1, 0]) - w[1] / 3 / math.sqrt(2)) <= tol and abs(float(gX[0, 1, 1]) + w[1] / 3 / math.sqrt(2)) <= tol
        # pose 2: on the goal -- the goal term adds nothing; roll = 0 exactly: no gradient to r1
        assert float(gR[0, 2, 2, 1]) == 0.0 and float(gR[0, 2, 2, 0]) != 0.0
        assert abs(float(terms[0, 2])) == 0.0 and abs(float(terms[0, 0]) - (6 + 100 + 4) / 3) <= 1e-5
    want = tr.gradients(case, **sc)
    got = tr.gradients(case, fn=refine.trajectory_objective_aten, **sc)
    assert float((got[2] - want[2]).abs().max()) <= 1e-12 and float((got[3] - want[3]).abs().max()) <= 1e-12


def test_kept_steps_follow_rollout_costs():
    from monoforce_amd import refine
    assert refine.kept_steps(1, 1) == [0] and refine.kept_steps(50, 50) == [0, 49] and refine.kept_steps(50, 7) == [0, 7, 14, 21, 28, 35, 42, 49]
    assert refine.kept_steps(50, 49) == [0, 49] and refine.kept_steps(51, 50) == [0, 50] and refine.kept_steps(52, 50) == [0, 50, 51]
    for T, ps in ((100, 10), (500, 50), (40, 7)):
        assert refine.kept_steps(T, ps) == tr.kept_steps(T, ps).tolist() and len(refine.kept_steps(T, ps)) == 1 + (T - 1 + ps - 1) // ps
    with pytest.raises(ValueError, match='pose_stride'):
        refine.kept_steps(10, 0)


# ---- the shape table of the GPU tests against the kernel's source -----------------------------------------------------------------------
MOVE = ('the launch configuration is chosen differently now: move tr.CASES (tests/traj_objective_reference.py) and the T list of '
        'tests/test_control_refine_gpu.py with it, then the restatement in this file')


def _source(name):
    with open(os.path.join(REPO, 'monoforce_amd', 'csrc', name)) as f:
        return re.sub(r'\s+', ' ', f.read())


@pytest.mark.parametrize('name,text', [('traj_objective.hip', 'constexpr int kObjBlock = 256;'), ('traj_objective.hip', 'constexpr int kObjRows = kObjBlock / 16;'),
                                        ('traj_objective.hip', 'for (int p = row; p < Tp; p += kObjRows)'), ('traj_objective.hip', 'for (int n = l; n < d.N; n += 16)'),
                                        ('traj_objective.hip', 'for (int k = l; k < nseg; k += 16)'), ('traj_objective.hip', 'for (int t = threadIdx.x; t < d.T; t += kObjBlock)'),
                                        ('traj_objective.hip', 'dim3(d->B), dim3(mf::kObjBlock)'), ('traj_objective.hip', 'constexpr int kObjPointsMax = 1024;'),
                                        ('traj_objective.hip', 'constexpr int kObjPathMax = 256;'),
                                        ('control_refine.hip', 'constexpr int kRefineBlock = 256;'), ('control_refine.hip', 'dim3(d->K), dim3(mf::kRefineBlock)')])
def test_the_selectors_are_the_ones_the_shape_tables_were_chosen_for(name, text):
    assert _source(name).count(text) == 1, f'{text!r} is no longer in {name}: {MOVE}'
    assert _source('control_refine.hip').count('i += kRefineBlock') == 2, MOVE


def test_gradient_cases_reach_every_configuration():
    """ONE mapping (a 16-lane row per kept pose, 16 rows per workgroup, one workgroup per rollout): what can differ between launches is the trip
    count of the pose loop (Tp against 16 rows), of the point loop and the segment loop (N, P - 1 against 16 lanes), and of the zeroing loop (T
    against 256 threads: one trip at every T a test can afford -- T = 300 would only repeat it)."""
    rows, lanes = 16, 16
    Tps = {1 + (T - 1 + ps - 1) // ps for _, T, ps, _, _ in tr.CASES}
    assert {1, 2, 8, 9} <= Tps and any(tp > rows and tp % rows for tp in Tps), MOVE                   # a second, ragged trip of the pose loop
    assert {(T, ps) for _, T, ps, _, _ in tr.CASES} >= {(1, 1), (50, 7), (50, 50)}, MOVE            # the last kept step is the clamp T - 1
    assert all((T - 1) % ps for _, T, ps, _, _ in tr.CASES if (T, ps) in ((51, 7), (50, 3), (50, 2))), MOVE   # ... behind the last multiple
    bodies = {N for *_, N, _ in tr.CASES}
    assert {1, 4, 8, 9, lanes, lanes + 1, 4 * lanes + 1} <= bodies, MOVE                             # either side of a row; a fifth trip of lane 0
    assert {P for *_, P in tr.CASES} == {0, 1, 2, lanes + 2}, MOVE                                    # no path, a point, a segment, 17 segments
    assert {B for B, *_ in tr.CASES} == {1, 3, 65}, MOVE
    from tests import test_control_refine_gpu as tc
    Ts = [m.args[1] for m in tc.test_update_kernel_against_torch_adam.pytestmark if m.name == 'parametrize' and m.args[0] == 'T'][0]
    assert {2 * T for T in Ts} >= {2, 256, 258} and any(2 * T > 512 and (2 * T) % 256 for T in Ts), MOVE


@pytest.mark.parametrize('shape', tr.CASES)
def test_few_rows_lie_next_to_a_kink(shape):
    """The referee alone, in float64: at most 5 % of a case's kept pose rows are taken out of the gradient comparison (the seeds of
    tr.SEEDS were chosen for it), under an infinite and under a finite off_map."""
    case = tr.make_case(*shape)
    for off_map in (INF, 1.5):
        bad = tr.excluded_rows(case, off_map=off_map)
        assert bad.shape == (shape[0], 1 + (shape[1] - 1 + shape[2] - 1) // shape[2])
        assert float(bad.float().mean()) <= 0.05, (shape, off_map, int(bad.sum()), bad.numel())
