"""The kernels around the rollout pick their workgroup shape on the host from B and N, and nothing reports which one a launch took.  The shape
tables of their GPU tests (tests/pose_costs_cases.py, tests/test_mppi_gpu.py, the loss tests) were chosen for the thresholds written in
monoforce_amd/csrc/pose_costs.hip, mppi.hip, physics_loss.hip and pose_loss.hip; this test reads those expressions as text and restates them, so
that a changed threshold cannot leave a configuration silently untested."""
import os
import re

import pytest

from tests import pose_costs_cases as pc
from tests.conftest import REPO

MOVE = ('the launch configuration is chosen differently now: move the shapes of the GPU tests with it (tests/pose_costs_cases.py CONFIG_SHAPES, '
        'tests/test_mppi_gpu.py SHAPES, the (B, T2) lists of the two loss value tests), then the restatement in this file')


def _source(name):
    with open(os.path.join(REPO, 'monoforce_amd', 'csrc', name)) as f:
        return re.sub(r'\s+', ' ', f.read())


POSE, MPPI = _source('pose_costs.hip'), _source('mppi.hip')
S_SELECTOR = 'const int S = d->B <= 8192 ? 16 : (d->B <= 16384 ? 8 : 4);'
WAVES_SELECTOR = 'const int waves = d->B <= 1024 ? 4 : (d->B <= 4096 ? 2 : 1);'


def _slices(B):
    return 16 if B <= 8192 else (8 if B <= 16384 else 4)


def _row_waves(B):
    return 4 if B <= 1024 else (2 if B <= 4096 else 1)


@pytest.mark.parametrize('text,where', [(S_SELECTOR, POSE), (WAVES_SELECTOR, POSE), ('constexpr int kLaneBodyMax = 8;', POSE),
                                         ('if (d->N <= mf::kLaneBodyMax) {', POSE), ('constexpr int kPosePointsMax = 1024;', POSE),
                                         ('constexpr int kPosePathMax = 256;', POSE), ('for (int p = s; p < d.Tp; p += S)', POSE),
                                         ('for (int p = row; p < d.Tp; p += rows)', POSE), ('for (int n = l; n < d.N; n += 16)', POSE),
                                         ('for (int k = l; k < nseg; k += 16)', POSE),
                                         (S_SELECTOR, MPPI), ('constexpr int kUpdChunk = 64;', MPPI), ('constexpr int kFinishSlices = 16;', MPPI),
                                         ('per = (n_chunks + kFinishSlices - 1) / kFinishSlices;', MPPI), ('t_tiles = (d->T + 63) / 64;', MPPI)])
def test_the_selectors_are_the_ones_the_shape_tables_were_chosen_for(text, where):
    assert where.count(text) == 1, f'{text!r} is no longer in the source: {MOVE}'


@pytest.mark.parametrize('name', ['physics_loss.hip', 'pose_loss.hip'])
def test_the_loss_value_kernels_finish_in_trips_of_256(name):
    src = _source(name)
    assert src.count('for (unsigned k = threadIdx.x; k < gridDim.x; k += 256)') == 1, MOVE
    assert 'dim3(256)' in src and '+ 255) / 256' in src, MOVE
    if name == 'physics_loss.hip':
        assert src.count('for (; t + 8 <= T1; t += 8) {') == 1 and src.count('for (; t < T1; ++t) {') == 1, MOVE


def test_pose_cost_shapes_reach_every_configuration():
    reached = set()
    for B, Tp, N in pc.SHAPES + pc.CONFIG_SHAPES:
        if N <= 8:
            reached.add(('lanes', _slices(B), 'ragged' if Tp > _slices(B) and Tp % _slices(B) else 'one trip'))
        else:
            rows = 4 * _row_waves(B)
            reached.add(('points', rows, 'ragged' if Tp > rows and Tp % rows else 'one trip'))
    for kind, widths in (('lanes', (16, 8, 4)), ('points', (16, 8, 4))):
        for w in widths:
            assert any(k == kind and v == w for k, v, _ in reached), f'no shape runs {kind} at width {w}: {MOVE}'
    # a second, ragged trip of the pose loop in each kernel, and in every width of the points kernel
    assert ('lanes', 4, 'ragged') in reached and ('lanes', 16, 'ragged') in reached, MOVE
    assert all(('points', w, 'ragged') in reached for w in (16, 8, 4)), MOVE
    bodies = {N for _, _, N in pc.CONFIG_SHAPES}
    assert {8, 9, 16, 17, 65, 1024} <= bodies, MOVE                  # either side of kLaneBodyMax, of a 16-lane row, of a wave; the full table
    assert 1 in pc.PATH_LENGTHS and 2 in pc.PATH_LENGTHS and {17, 18, 256} <= set(pc.PATH_LENGTHS), MOVE
    assert pc.RECT[0] != pc.RECT[1]


def test_mppi_and_loss_shapes_reach_every_configuration():
    from tests import test_mppi_gpu as tm
    assert {_slices(B) for B, _ in tm.SHAPES} == {16, 8, 4}, MOVE
    assert any(_slices(B) == 4 and T % 4 for B, T in tm.SHAPES) and any(_slices(B) == 8 and T % 8 for B, T in tm.SHAPES), MOVE
    per = {B: ((B + 63) // 64 + 15) // 16 for B, _ in tm.SHAPES}
    assert max(per.values()) >= 17 and any(3 <= p <= 16 for p in per.values()), MOVE            # README's 4096 / 16 384 rollouts: per = 4 / 16
    assert any(16 * per[B] - (B + 63) // 64 >= per[B] for B in per if per[B] > 1), MOVE         # a wave whose slice is empty
    assert any(T > 64 and T % 64 for _, T in tm.SHAPES), MOVE                                   # a second, partial 64-step tile
    # the loss value kernels: grids of 257 (a second trip of the finishing loop, one thread) and of more than 768 blocks (four trips)
    import inspect
    from tests import test_physics_loss_gpu as tl, test_pose_loss_gpu as tp
    for fn in (tl.test_loss_value_is_finished_inside_the_launch_and_reusable, tp.test_pose_loss_value_is_finished_inside_the_launch_and_reusable):
        shapes = [m.args[1] for m in fn.pytestmark if m.name == 'parametrize'][0]
        blocks = {(B * T2 + 255) // 256 for B, T2 in shapes}
        assert 257 in blocks and any(b > 768 and b % 256 for b in blocks) and 1 in blocks, (inspect.getsourcefile(fn), MOVE)
