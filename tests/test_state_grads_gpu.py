"""Gradients with respect to the START state -- gx0, gxd0, gR0, gw0, what `state=` tensors that require grad receive and
torch.ops.monoforce.dphys_rollout_bwd returns -- on every rollout backward route, against the float64 oracle's autograd over the same four
leaves (tests/state_grad_cases.py: the cases, the referee, the harness).  Three epilogues write them (rollout_bwd_kernel.h,
rollout_bwd_mw_kernel.h, rollout_bwd_cp_kernel.h), each with the adjoint of the terrain snap of the start height.

Bars: float64 runs 1e-8 per gradient tensor; float32 runs max(2e-4, 3 x the float32 oracle's own distance from the float64 one) per tensor,
and at T = 1 per row of gR0 and per component of gx0 as well.  Every case must run the kernel its route names.

The measured table:  python -m tests.test_state_grads_gpu --report profiles/state_grads_errors.txt"""
import sys

import pytest
import torch

from tests import state_grad_cases as sg

pytestmark = pytest.mark.gpu

STREAM_SHAPE, FAST_SHAPE = ('cp_rec_stream12', 14, 1), ('fast_general', 6, 1)


def _check(c, T, integ, **kw):
    got, launch = sg.run_hip(c, T, integ, **kw)
    sg.assert_route(c, integ, launch)
    rows = sg.compare(c, T, integ, got)
    for row in rows:
        print(c['name'], T, integ, *row)
    bad = [r for r in rows if not r[-1]]
    assert not bad, (c['name'], T, integ, bad)
    return got


@pytest.mark.parametrize('name,T,integ', sg.case_ids(), ids=lambda v: str(v))
def test_start_state_gradients_on_every_route(name, T, integ):
    """All four gradients of all B rollouts == the oracle's, gx0.z exactly zero under the snap, on the kernel the route names."""
    _check(sg.case(name), T, integ)


@pytest.mark.parametrize('name,T,integ', [STREAM_SHAPE, FAST_SHAPE, ('f64_cp_stream', 14, 1), ('f64_exact', 6, 1), ('f64_exact', 6, 0)],
                         ids=lambda v: str(v))
def test_without_the_terrain_snap(name, T, integ):
    """snap_to_terrain=False against oracle.rollout(snap=False): gx0.z is the raw adjoint (non-zero, held to the bar on its own) and the
    rows of gR0 carry no snap term."""
    c = sg.case(name, snap=False)
    assert float(sg.oracle_grads(c, T, integ)[0][:, 2].abs().min()) > 0.0
    _check(c, T, integ)


@pytest.mark.parametrize('integ', [1, 0])
@pytest.mark.parametrize('name', ['fast_general', 'split_carry', 'xs'])
def test_gw0_survives_being_the_control_gradient_dump(name, integ):
    """Controls that do not require grad, on the families whose kernels then send every step's control-gradient pair to the rollout's own
    gw0 row (rollout_bwd.hip), which the final store overwrites: gw0 == the oracle's, and bit for bit the gw0 of the same problem run
    with controls that do require grad (the same kernel, the same per-rollout arithmetic)."""
    c, T = sg.case(name), 6
    dumped = _check(c, T, integ, controls_grad=False)
    wanted, launch = sg.run_hip(c, T, integ)
    sg.assert_route(c, integ, launch)
    for a, b in zip(dumped, wanted):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', ['cp_rec_stream12', 'f64_exact'])
def test_ops_entry_returns_the_module_paths_gradients(name):
    """monoforce_amd.ops.rollout (torch.ops.monoforce.dphys_rollout_fwd / _bwd) with the four state tensors as leaves: the four gradients
    bit for bit those of the module path, in float32 and float64."""
    c, T, integ = sg.case(name), 14, 1
    mod = _check(c, T, integ)
    op, launch = sg.run_hip(c, T, integ, entry='ops')
    sg.assert_route(c, integ, launch)
    for gname, a, b in zip(sg.GRADS, op, mod):
        assert torch.equal(a, b), (gname, float((a - b).abs().max()))


@pytest.mark.parametrize('only', range(4), ids=sg.GRADS)
@pytest.mark.parametrize('name,T,integ', [STREAM_SHAPE, FAST_SHAPE], ids=lambda v: str(v))
def test_only_one_state_tensor_requires_grad(name, T, integ, only):
    """The need_* branches of dphysics_bwd.py: that tensor's gradient is the one of the run where all four require grad, bit for bit, and
    the others get none."""
    c = sg.case(name)
    full, _ = sg.run_hip(c, T, integ)
    got, launch = sg.run_hip(c, T, integ, leaves=tuple(k == only for k in range(4)))
    sg.assert_route(c, integ, launch)
    for k in range(4):
        if k == only:
            assert torch.equal(got[k], full[k]), sg.GRADS[k]
        else:
            assert got[k] is None, sg.GRADS[k]


def _report(path):
    """Every parametrised case (and the runs without the snap): per gradient the measured error against the float64 oracle, the float32
    oracle's own error, the bar."""
    runs = [(sg.case(name), T, integ) for name, T, integ in sg.case_ids()]
    runs += [(sg.case(name, snap=False), T, integ) for name, T, integ in (STREAM_SHAPE, FAST_SHAPE, ('f64_cp_stream', 14, 1), ('f64_exact', 6, 1))]
    fmt = lambda v: '-' if v is None else '%.2e' % v      # noqa: E731
    lines = ['# start-state gradients, HIP vs the float64 oracle (rel. to the absolute maximum; all B rollouts): python -m tests.test_state_grads_gpu --report',
             '# %-26s %5s %2s %5s  %-11s %9s %9s %9s  %s' % ('case', 'B', 'T', 'integ', 'gradient', 'error', 'oracle32', 'bar', 'kernel')]
    misses = 0
    for c, T, integ in runs:
        got, launch = sg.run_hip(c, T, integ)
        for label, err, env, bar, ok in sg.compare(c, T, integ, got):
            misses += not ok
            lines.append('%-28s %5d %2d %5d  %-11s %9s %9s %9s  %s%s' % (c['name'] + ('' if c['snap'] else '/nosnap'), c['B'], T, integ, label, fmt(err),
                                                                         fmt(env), fmt(bar), launch.split(' grid=')[0].replace('mf::', ''), '' if ok else '  MISS'))
        print(lines[-1], flush=True)
    lines.append('# %d rows, %d over their bar' % (len(lines) - 2, misses))
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__' and len(sys.argv) == 3 and sys.argv[1] == '--report':
    _report(sys.argv[2])
