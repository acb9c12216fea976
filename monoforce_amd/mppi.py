"""MPPI (model-predictive path integral) trajectory optimisation on top of the path-cost rollout.

`TrajectoryShooter` (planner.py) does what the reference's node does: constant-in-time (v, w) samples, one scoring pass, argmin.
`MPPIPlanner` adds the loop a goal-directed planner needs: a time-varying nominal control sequence [T,2] is perturbed with Gaussian
noise into B sequences, the B sequences are rolled out on one terrain (`DPhysics.rollout_costs`, the kernel's path-cost mode), scored

    cost = w_inclination (mean|roll| + mean|pitch|) + w_force std_t(std_points |F_spring|) + w_goal |x_T[0:2] - goal|

and the nominal is replaced by their softmin-weighted average, w_b ~ exp(-(cost_b - min cost) / lam).  Around the rollout launch an
iteration is five small HIP launches (`torch.ops.monoforce.mppi_perturb`, `path_costs`, `mppi_update`: monoforce_amd/csrc/mppi.hip)
plus the noise draw; nothing is read back to the host, so `step` and `plan` can be captured into a hipGraph (monoforce_amd.capture).
Where the robot goes is scored too, when `step` / `plan` are given a 2-D `cost_map` on the terrain grid and / or a `path` to follow: one more
launch (`torch.ops.monoforce.pose_costs`, monoforce_amd/csrc/pose_costs.hip) adds

    w_map mean_p max_n bilinear(cost_map, footprint point n of kept pose p) + w_path mean_p distance(x_p[0:2], path)

to the cost above, +inf for a rollout with any footprint sample not below `lethal`.  Both are device tensors the launch reads.
The nominal lives in ONE device buffer that every step updates in place: replaying a captured step iterates, like calling it does.
"""
import torch

from . import ops

__all__ = ['MPPIPlanner']


class MPPIPlanner:
    def __init__(self, dphysics, n_trajs=None, n_iters=4, lam=0.05, sigma=(0.3, 0.6), weights=None, keep_nominal=True, pose_stride=None,
                 lethal=float('inf'), off_map=float('inf'), footprint=None):
        """`weights`: dict(inclination, force, goal, map, path), default (1, 0, 1, 0, 0); `sigma`: noise scale of (v, w); `keep_nominal`:
        sequence 0 is the unperturbed nominal (the update can then never do worse than keeping it); limits are +-cfg.vel_max /
        +-cfg.omega_max.  Cost map: a footprint sample that is not < `lethal` makes its rollout's cost +inf (inf: no such rule), a footprint
        point off the map samples `off_map`; `footprint` [N,3]: body-frame points the map is sampled under (default: the DPhysics robot points).
        `pose_stride`: None = 0.5 s between kept poses, or, with a cost map or a path, one kept pose per map cell at full speed."""
        if dphysics.precise:
            raise ValueError('MPPIPlanner uses the float32 fast-math path-cost kernels: construct DPhysics(precise=False)')
        w = dict(inclination=1.0, force=0.0, goal=1.0, map=0.0, path=0.0)
        if weights is not None:
            unknown = set(weights) - set(w)
            if unknown:
                raise ValueError(f'unknown cost weights {sorted(unknown)}: inclination, force, goal, map, path')
            w.update(weights)
        if not lam > 0:
            raise ValueError('lam must be positive')
        self.dp = dphysics
        self.cfg = dphysics.dphys_cfg
        self.device = torch.device(dphysics.device)
        self.n_trajs = int(n_trajs or self.cfg.n_sim_trajs)
        self.n_iters = int(n_iters)
        self.lam = float(lam)
        self.sigma = (float(sigma[0]), float(sigma[1]))
        self.weights = (float(w['inclination']), float(w['force']), float(w['goal']))      # path_costs' three
        self.pose_weights = (float(w['map']), float(w['path']))
        self.lethal, self.off_map = float(lethal), float(off_map)
        self.footprint = (ops.footprint_points(dphysics) if footprint is None else
                          torch.as_tensor(footprint).detach().to(device=self.device, dtype=torch.float32).reshape(-1, 3).contiguous())
        self.keep_nominal = bool(keep_nominal)
        self.pose_stride = pose_stride
        self.T = int(self.cfg.traj_sim_time / self.cfg.dt)
        self.lo = (-float(self.cfg.vel_max), -float(self.cfg.omega_max))
        self.hi = (float(self.cfg.vel_max), float(self.cfg.omega_max))
        self.nominal = torch.zeros(self.T, 2, device=self.device)

    def reset(self, nominal=None):
        """Set the nominal sequence ([T,2]; zeros by default) -- in place: a captured step keeps reading the same buffer."""
        if nominal is None:
            self.nominal.zero_()
        else:
            assert tuple(nominal.shape) == (self.T, 2), f'nominal must be [{self.T}, 2], got {tuple(nominal.shape)}'
            self.nominal.copy_(nominal)
        return self.nominal

    def shift(self, steps=1):
        """Warm start for the next frame: drop the first `steps` controls, repeat the last one."""
        k = min(max(int(steps), 0), self.T)
        if k:
            self.nominal.copy_(torch.cat([self.nominal[k:], self.nominal[-1:].expand(k, 2)]))
        return self.nominal

    @torch.no_grad()
    def step(self, z_grid, goal, friction=None, pose0=None, noise=None, generator=None, cost_map=None, path=None):
        """One MPPI iteration.  z_grid [H,W] (or [1,H,W]) float32; goal: DEVICE tensor [2] (x, y), read by the launch -- a captured step
        follows `goal.copy_(...)`; pose0: optional 4x4 start pose shared by all samples; noise: optional [B,T,2] standard-normal draw;
        cost_map: optional DEVICE tensor [H,W] on the nodes of z_grid, path: optional DEVICE tensor [P,2] -- read by the launch too
        (`cost_map.copy_(...)`, `path.copy_(...)`).  Returns dict(controls, cost_rows, Xs, Rs, pose_steps, force_cost, terms, costs, weights,
        best, n_valid, nominal), all on the device (`best`, `n_valid`: int32 [1]); `nominal` is the planner's own buffer, which the next
        step overwrites.  With a cost map or a path the dict gains `pose_terms` [B,2] = (map, cross-track) and `costs` is the sum."""
        dev = self.device
        if self.dp.precise:
            raise ValueError('MPPIPlanner uses the float32 fast-math path-cost kernels: construct DPhysics(precise=False)')
        if z_grid.dtype != torch.float32:
            raise TypeError('MPPIPlanner.step: float32 only')
        if not (torch.is_tensor(goal) and goal.is_cuda and goal.numel() == 2):
            raise TypeError('MPPIPlanner.step: goal must be a device tensor [2]')
        w_map, w_path = self.pose_weights
        for name, t, wt in (('cost_map', cost_map, w_map), ('path', path, w_path)):
            if t is None and wt != 0:
                raise ValueError(f'MPPIPlanner.step: the {name.split("_")[-1]} weight is {wt} but no {name} was given')
            if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
                raise TypeError(f'MPPIPlanner.step: {name} must be a float32 device tensor')
        scored = cost_map is not None or path is not None
        pose_stride = self.pose_stride
        if scored and pose_stride is None:      # one kept pose per map cell at full speed
            pose_stride = max(int(float(self.cfg.grid_res) / (float(self.cfg.vel_max) * float(self.cfg.dt)) + 1e-9), 1)
        B, T = self.n_trajs, self.T
        if noise is None:
            noise = torch.randn(B, T, 2, device=dev, generator=generator)
        assert tuple(noise.shape) == (B, T, 2), f'noise must be [{B}, {T}, 2], got {tuple(noise.shape)}'
        controls = torch.ops.monoforce.mppi_perturb(self.nominal, noise, self.sigma, self.lo, self.hi, self.keep_nominal)
        z = z_grid if z_grid.dim() == 3 else z_grid.unsqueeze(0)
        mu = None if friction is None else (friction if friction.dim() == 3 else friction.unsqueeze(0))
        state = None
        if pose0 is not None:       # as TrajectoryShooter.shoot (monoforce_node.py:67-72)
            x = pose0[:3, 3].to(dev).repeat(B, 1)
            state = (x, torch.zeros_like(x), pose0[:3, :3].to(dev).repeat(B, 1, 1).contiguous(), torch.zeros_like(x))
        w_incl, w_force, w_goal = self.weights
        out = self.dp.rollout_costs(z, controls, state=state, friction=mu, pose_stride=pose_stride, project=w_incl != 0)
        costs, terms = torch.ops.monoforce.path_costs(out['cost_rows'], out['force_cost'] if w_force != 0 else None, out['Xs'][:, -1],
                                                      goal, self.weights)
        pose_terms = None
        if scored:      # in place over path_costs' result: `costs` is the sum
            costs, pose_terms = ops.pose_costs_into(out['Xs'], out['Rs'], self.footprint, cost_map, path, costs, self.cfg.grid_res, self.cfg.d_max,
                                                    self.lethal, self.off_map, self.pose_weights, costs)
        nominal, weights, best, n_valid = ops.mppi_update_into(costs, controls, self.nominal, self.lam, self.nominal)
        res = dict(controls=controls, cost_rows=out['cost_rows'], Xs=out['Xs'], Rs=out['Rs'], pose_steps=out['pose_steps'],
                   force_cost=out['force_cost'], terms=terms, costs=costs, weights=weights, best=best, n_valid=n_valid, nominal=nominal)
        if scored:
            res['pose_terms'] = pose_terms
        return res

    @torch.no_grad()
    def plan(self, z_grid, goal, friction=None, pose0=None, noise=None, generator=None, cost_map=None, path=None):
        """`n_iters` steps from the current nominal; returns the last step's dict.  `noise`: optional [n_iters,B,T,2]; `cost_map`, `path`: as `step`."""
        out = None
        for i in range(self.n_iters):
            out = self.step(z_grid, goal, friction=friction, pose0=pose0, noise=None if noise is None else noise[i], generator=generator,
                            cost_map=cost_map, path=path)
        return out
