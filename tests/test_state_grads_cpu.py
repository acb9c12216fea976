"""Pins the referee of tests/test_state_grads_gpu.py: the oracle's `snap=False` mode is the snapped mode continued from the snapped height,
bit for bit, and the oracle's autograd gradients with respect to the start state agree with central differences to the difference
quotient's own truncation error (measured by halving the step, not assumed)."""
import pytest
import torch

from oracle import dphysics_oracle as orc
from tests import helpers as hp
from tests.golden_state import given_state

B, T, GRID_RES, D_MAX = 2, 6, 0.1, 3.2


def _inputs():
    from monoforce_amd import synthetic as syn
    pts, masks = syn.robot_points_4()
    z = torch.stack([syn.bump_terrain(syn.bump_params(20 + b), D_MAX, GRID_RES, torch.float64) * 0.3 for b in range(B)])
    mu = torch.stack([syn.wave_friction(D_MAX, GRID_RES, 0.5, 1.0, 1.0 + 0.2 * b, 0.8, torch.float64) for b in range(B)])
    ctrl = syn.varying_controls(B, T, seed=4, dtype=torch.float64)
    return pts, masks, z, mu, ctrl


@pytest.mark.parametrize('integ', [0, 1])
def test_snap_false_continues_from_the_snapped_height_bit_for_bit(integ):
    pts, masks, z, mu, ctrl = _inputs()
    spec = hp.spec_from(pts, masks, integ, GRID_RES, D_MAX)
    st = tuple(s.clone() for s in given_state(B))
    so, fo = orc.rollout(spec, z, ctrl, state=st, friction=mu)            # writes the snapped height into st[0]
    assert float((st[0][:, 2] - given_state(B)[0][:, 2]).abs().min()) > 0.0
    st2 = tuple(s.clone() for s in given_state(B))
    st2[0][:, 2] = st[0][:, 2]
    kept = st2[0].clone()
    so2, fo2 = orc.rollout(spec, z, ctrl, state=st2, friction=mu, snap=False)
    assert torch.equal(st2[0], kept)                                      # ... and snap=False leaves the caller's start position alone
    for k, a, b in zip(hp.OUT_KEYS, list(so) + list(fo), list(so2) + list(fo2)):
        assert torch.equal(a, b), k


def _cells(spec, pts, x0, R0, outs):
    """Cell index (trunc, as sample_grid) of every contact point at the start pose and at every output row."""
    Xs, _, Rs, _ = outs
    sink = spec.mass * spec.gravity / (spec.stiffness + 1e-6)
    x = torch.cat([x0.unsqueeze(1), Xs - Rs[:, :, :3, 2] * sink], 1)      # (Xs carries the sink offset along the body's z axis)
    R = torch.cat([R0.unsqueeze(1), Rs], 1)
    p = torch.einsum('btij,nj->btni', R, torch.as_tensor(pts, dtype=torch.float64)) + x.unsqueeze(2)
    return ((p[..., :2] + spec.d_max) / spec.grid_res).long()


# (leaf, index of the perturbed entry, snap): one entry each of xd0, w0, an off-diagonal entry of R0 and x0.x under the snap; x0.z without it
ENTRIES = [('xd0', 1, (1, 1), True), ('w0', 3, (0, 2), True), ('R0', 2, (1, 0, 1), True), ('x0.x', 0, (1, 0), True), ('x0.z', 0, (1, 2), False)]


@pytest.mark.parametrize('integ', [0, 1])
@pytest.mark.parametrize('label,leaf,entry,snap', ENTRIES, ids=[e[0] for e in ENTRIES])
def test_oracle_state_gradient_vs_central_differences(label, leaf, entry, snap, integ):
    """float64, 4-point body, B = 2, T = 6, the yawed / pitched / moving / spinning start of golden_state.  The model has kinks at cell
    edges, so the step keeps every sampled contact point in its cell (asserted: at the start pose and at every output row, for all four
    perturbed runs).  The bar is the quotient's own error: |D(h/2) - D(h)| bounds the truncation error of D(h/2) (which is a third of it
    for a smooth function), plus the rounding of the two loss values over the step (float64 eps x the sum of the loss's terms in
    magnitude; at h = 1e-4 the truncation error of most entries is below it)."""
    pts, masks, z, mu, ctrl = _inputs()
    spec = hp.spec_from(pts, masks, integ, GRID_RES, D_MAX)

    def start():
        st = [s.clone() for s in given_state(B)]
        if not snap:
            st[0][:, 2] = torch.tensor([0.13, 0.21], dtype=torch.float64)
        return st

    def run(delta, grad=False):
        st = start()
        st[leaf][entry] += delta
        leaves = [s.requires_grad_(True) for s in st] if grad else st
        state = [leaves[0] * 1.0] + list(leaves[1:]) if grad else leaves
        so, fo = orc.rollout(spec, z, ctrl, state=tuple(state), friction=mu, snap=snap)
        outs = list(so) + list(fo)
        loss = hp.probe_loss(outs, torch.float64)
        cells = _cells(spec, pts, state[0].detach(), state[2].detach(), [o.detach() for o in so])
        if grad:
            loss.backward()
            return float(loss.detach()), cells, float(leaves[leaf].grad[entry])
        return float(loss), cells

    def abs_sum():      # sum of |term| of the loss: what one rounding of every term is relative to
        from monoforce_amd import synthetic as syn
        st = start()
        so, fo = orc.rollout(spec, z, ctrl, state=tuple(st), friction=mu, snap=snap)
        return sum(float((o * syn.probe_weights(o.shape, phase=0.5 + i, dtype=torch.float64)).abs().sum()) * s_
                   for i, (o, s_) in enumerate(zip(list(so) + list(fo), [1.0, 1.0, 1.0, 1.0, 1e-3, 1e-3])))

    _, cells0, g = run(0.0, grad=True)
    h = 1e-4
    vals = {}
    for d in (h, -h, h / 2, -h / 2):
        vals[d], cells = run(d)
        assert torch.equal(cells, cells0), (label, d)      # no contact point changed cell: the quotient differentiates one smooth piece
    d_h, d_half = (vals[h] - vals[-h]) / (2 * h), (vals[h / 2] - vals[-h / 2]) / h
    rounding = 4 * 2.2e-16 * abs_sum() / h       # two loss values, each off by ~eps x the sum of its terms' magnitudes, over the step h/2 x 2
    bar = abs(d_h - d_half) + rounding
    print(label, integ, 'autograd', g, 'D(h/2)', d_half, 'D(h)', d_h, 'bar', bar)
    assert g != 0.0
    assert bar <= 1e-5 * abs(g), (label, bar, g)           # the quotient itself is sharp here (else the comparison below says nothing)
    assert abs(d_half - g) <= bar, (label, g, d_half, d_h, bar)
