"""The pure-host pieces of the rollout's marshalling layer on CPU tensors: which maps the kernels get for which inputs
(`rollout_launch.canonical_maps`) and how a map gradient goes back to its input's own shape (`dphysics_bwd.to_input_shape`)."""
import pytest
import torch

from monoforce_amd.dphysics_bwd import to_input_shape
from monoforce_amd.rollout_launch import canonical_maps, time_grid

H, W = 5, 7


def _map(B, seed):
    return torch.randn(B, H, W, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('with_mu', [True, False])
def test_one_map_pair_shared_by_all_rollouts(with_mu):
    z, mu = _map(1, 0), (_map(1, 1) if with_mu else None)
    zc, muc, shared = canonical_maps(z, mu, 6)
    assert shared is True and zc.shape == (H, W) and zc.is_contiguous() and torch.equal(zc, z[0])
    assert (muc is None) if not with_mu else (muc.shape == (H, W) and muc.is_contiguous() and torch.equal(muc, mu[0]))


def test_strided_shared_map_is_made_contiguous():
    z = _map(1, 0).transpose(1, 2)[:, :H, :H]
    zc, _, shared = canonical_maps(z, None, 3)
    assert shared is True and zc.is_contiguous() and torch.equal(zc, z[0])


def test_per_rollout_maps_stay_per_rollout():
    z, mu = _map(6, 0), _map(6, 1)
    zc, muc, shared = canonical_maps(z, mu, 6)
    assert shared is False and zc.shape == muc.shape == (6, H, W) and zc.is_contiguous() and muc.is_contiguous()
    assert torch.equal(zc, z) and torch.equal(muc, mu)


@pytest.mark.parametrize('z_shared', [True, False])
def test_mixed_maps_expand_the_shared_one_for_real(z_shared):
    z, mu = _map(1 if z_shared else 6, 0), _map(6 if z_shared else 1, 1)
    zc, muc, shared = canonical_maps(z, mu, 6)
    assert shared is False and zc.shape == muc.shape == (6, H, W)
    assert zc.is_contiguous() and muc.is_contiguous() and zc.stride(0) == muc.stride(0) == H * W
    assert torch.equal(zc, z.expand(6, H, W)) and torch.equal(muc, mu.expand(6, H, W))


def test_stride_0_expand_counts_as_shared():
    z, mu = _map(1, 0).expand(6, H, W), _map(1, 1)
    zc, muc, shared = canonical_maps(z, mu, 6)
    assert shared is True and zc.shape == muc.shape == (H, W) and zc.is_contiguous() and torch.equal(zc, z[0])
    # ... next to a per-rollout map it is one more map to expand for real
    zc, muc, shared = canonical_maps(z, _map(6, 2), 6)
    assert shared is False and zc.shape == (6, H, W) and zc.stride(0) == H * W and torch.equal(zc, z)


def test_maps_that_do_not_fit_are_refused():
    with pytest.raises(AssertionError):
        canonical_maps(_map(1, 0)[0], None, 6)              # [H,W]
    with pytest.raises(AssertionError):
        canonical_maps(_map(1, 0), _map(1, 1)[:, :, :W - 1], 6)
    with pytest.raises(AssertionError):
        canonical_maps(_map(4, 0), None, 6)


@pytest.mark.parametrize('B', [1, 8, 6])
def test_to_input_shape_sums_back_to_the_shared_gradient(B):
    """A shared run's [H,W] gradient handed to an input that was [1,H,W], or an expand of it to B = 8 (a power of two: g / B as a
    stride-0 expand) or B = 6 (g in row 0): summed over the batch by ExpandBackward it is the gradient again, exactly.
    (Gradients of 16 significant bits: every partial sum k g / 8 is then a float32 whatever the order of the sum.  With full 24-bit
    mantissas the B-fold sum of g / B is exact only where it runs pairwise; the CPU's row-by-row sum rounds 3 g / 8, 5 g / 8, ... and
    comes back up to 7.5e-8 relative off at B = 8 -- within the (B - 1) roundings of 2^-24 each that the second half allows.)"""
    def through_expand_backward(g):
        leaf = _map(1, 0).requires_grad_(True)
        inp = leaf if B == 1 else leaf.expand(B, H, W)
        out = to_input_shape(g, inp.shape, B > 1)
        assert out.shape == inp.shape
        inp.backward(out)
        return leaf.grad[0]

    g16 = torch.randint(-2 ** 15, 2 ** 15, (H, W), generator=torch.Generator().manual_seed(3)).float() / 64.
    assert torch.equal(through_expand_backward(g16), g16)
    g24 = _map(1, 3)[0] * 1e3 + 0.1
    back = through_expand_backward(g24)
    if B & (B - 1):
        assert torch.equal(back, g24)           # g in row 0, zeros elsewhere: exact for every order
    else:
        assert float(((back - g24) / g24).abs().max()) <= (B - 1) * 2. ** -24


def test_to_input_shape_of_a_per_rollout_run():
    g = _map(6, 4)
    assert to_input_shape(g, (6, H, W), False) is g                                   # a per-rollout input gets its rows
    assert torch.equal(to_input_shape(g, (1, H, W), False), g.sum(0, keepdim=True))   # one shared map beside a per-rollout one
    assert to_input_shape(None, (1, H, W), False) is None


def test_time_grid_is_the_truncated_linspace_and_cached():
    ts = time_grid(5.0, 500, 20, torch.float64, 'cpu')
    assert torch.equal(ts, torch.linspace(0, 5.0, 500, dtype=torch.float64)[:20]) and ts.is_contiguous()
    assert time_grid(5.0, 500, 20, torch.float64, 'cpu') is ts
    assert time_grid(5.0, 500, 20, torch.float32, 'cpu').dtype == torch.float32
