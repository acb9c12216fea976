"""Referee of the MPPI kernels (monoforce_amd/csrc/mppi.hip): the three formulas of include/monoforce_hip.h restated in plain torch, in the
dtype of their tensor arguments (float32 or float64).  Test code: the product never imports it.

The scalars of the launch descriptor (sigma, limits, cost weights, lambda) are C floats: every function rounds them to float32 first, so a
float64 evaluation differs from the kernels by their arithmetic alone."""
import torch


def _f32(v, dtype):
    return torch.tensor(v, dtype=torch.float32).to(dtype)


def perturb(nominal, noise, sigma, lo, hi, keep_nominal):
    """nominal [T,2], noise [B,T,2] -> controls [B,T,2] = min(max(nominal + sigma * noise, lo), hi); row 0 = clamp(nominal) with keep_nominal."""
    dt = noise.dtype
    u = nominal.to(dt).unsqueeze(0) + _f32(sigma, dt) * noise      # two ops, two roundings
    if keep_nominal:
        u = u.clone()
        u[0] = nominal.to(dt)
    return torch.minimum(torch.maximum(u, _f32(lo, dt)), _f32(hi, dt))


def path_costs(cost_rows, force_cost, x_last, goal, weights):
    """cost_rows [B,T,4], force_cost [B] or None, x_last [B,>=2], goal [2], weights (inclination, force, goal) -> costs [B], terms [B,3]."""
    dt = cost_rows.dtype
    pitch = torch.asin(torch.clamp(-cost_rows[..., 0], -1.0, 1.0))
    roll = torch.atan2(cost_rows[..., 1], cost_rows[..., 2])
    incl = roll.abs().mean(dim=-1) + pitch.abs().mean(dim=-1)
    force = torch.zeros_like(incl) if force_cost is None else force_cost.to(dt)
    d = x_last[:, :2].to(dt) - goal.to(dt)
    dist = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    w = _f32(list(weights), dt)
    return w[0] * incl + w[1] * force + w[2] * dist, torch.stack([incl, force, dist], dim=-1)


def update(costs, controls, nominal, lam):
    """costs [B], controls [B,T,2], nominal [T,2] -> (nominal_out [T,2], weights [B], best, n_valid); best / n_valid are Python ints."""
    dt = controls.dtype
    costs = costs.to(dt)
    finite = torch.isfinite(costs)
    n_valid = int(finite.sum())
    if n_valid == 0:
        return nominal.to(dt).clone(), torch.zeros_like(costs), -1, 0
    c = torch.where(finite, costs, torch.full_like(costs, float('inf')))
    best = int(torch.argmin(c))
    e = torch.where(finite, torch.exp(-(c - c[best]) / _f32(lam, dt)), torch.zeros_like(c))
    w = e / e.sum()
    return torch.einsum('b,btk->tk', w, controls), w, best, n_valid
