"""The optimisation loop of `scripts/fit_terrain.py:46-69` with nothing left on the host: `TerrainFitter`.

The reference's loop is `torch.optim.Adam` over two parameter groups, a `loss.item()` per iteration and `if loss < loss_min: z_grid_best =
z_grid.clone()`.  Here one kernel launch behind the fit step (`mf_terrain_fit_update_*`, csrc/terrain_fit.hip) does the Adam update of both
maps and the best-so-far bookkeeping, with the iteration count, the smallest loss, its iteration and the loss history in device memory;
in graph mode the step's launches and that one replay as ONE hipGraph per iteration and the host never waits for the device.

`mf_terrain_fit_update_*` and `mf_terrain_fit_grid_cap` are marshalled here and nowhere else (`update`, `grid_cap`).
"""
import math
import warnings

import torch

from . import _lib
from . import dist as mfdist
from .capture import capture

__all__ = ['TerrainFitter', 'parse_bounds', 'update', 'grid_cap', 'new_state']


def parse_bounds(bounds):
    """`bounds` of `TerrainFitter` -> (flags, z_lo, z_hi, mu_lo, mu_hi) as `MfFitDesc` takes them.  None: no projection (the reference);
    else a dict with the keys 'z' and / or 'mu', each None or a pair (lo, hi) with lo <= hi (either may be infinite)."""
    out = [0, -math.inf, math.inf, -math.inf, math.inf]
    if bounds is None:
        return tuple(out)
    if not isinstance(bounds, dict) or set(bounds) - {'z', 'mu'}:
        raise ValueError(f"bounds must be None or a dict with the keys 'z' and 'mu', got {bounds!r}")
    for k, (name, flag) in enumerate((('z', _lib.MF_FIT_CLAMP_Z), ('mu', _lib.MF_FIT_CLAMP_MU))):
        box = bounds.get(name)
        if box is None:
            continue
        try:
            lo, hi = (float(v) for v in box)
        except (TypeError, ValueError):
            raise ValueError(f'bounds[{name!r}] must be None or a pair (lo, hi), got {box!r}') from None
        if not lo <= hi:
            raise ValueError(f'bounds[{name!r}] needs lo <= hi, got ({lo}, {hi})')
        out[0] |= flag
        out[1 + 2 * k], out[2 + 2 * k] = lo, hi
    return tuple(out)


def grid_cap():
    """The most workgroups (of 256 threads) one update launch uses; more cells than `256 * grid_cap()` take further trips of its loop."""
    return int(_lib.lib().mf_terrain_fit_grid_cap())


def new_state(dtype, device, max_iters):
    """Fresh device state of a fit: (state int32 [4] = step, best_step, ticket, reserved; loss_min [1]; history [max_iters])."""
    state = torch.tensor([0, -1, 0, 0], dtype=torch.int32, device=device)
    return state, torch.full((1,), math.inf, dtype=dtype, device=device), torch.full((max_iters,), math.nan, dtype=dtype, device=device)


def update(desc, z, mu, g_z, g_mu, m_z, v_z, m_mu, v_mu, loss, z_best, mu_best, state, loss_min, history):
    """One `mf_terrain_fit_update_*` launch on z's device and current stream (include/monoforce_hip.h): Adam on both maps from the
    gradients `g_z`, `g_mu`, then best-so-far and history from `loss` (a device scalar).  Contiguous tensors of z's dtype; `state` int32 [4].
    `mu` and its companions may be None when `desc.n_mu == 0`.  Writes through raw pointers: tensor versions are the caller's business."""
    _lib.require_hip_tensor(z, 'z')
    _lib.launch('mf_terrain_fit_update', z.device, desc, z, mu, g_z, g_mu, m_z, v_z, m_mu, v_mu, loss, z_best, mu_best, state, loss_min,
                history if history.numel() else None, dtype=z.dtype)


class TerrainFitter:
    """`scripts/fit_terrain.py:46-69` on the GPU: `step()` = one iteration of (`problem`'s forward + loss + backward, Adam on the height and
    the friction map, best-so-far), `run(n)` = n of them, neither with a host synchronisation.

        fit = TerrainFitter(problem, z0, mu0, lr=(0.02, 0.01))     # the reference's two parameter groups
        out = fit.run(100)                                         # out['z_best'], out['loss'] (the 100 losses), out['best_iter'] ...

    `problem` is a `TerrainFitProblem` (its `tv_weight` gives the regularised fit).  The fitter owns `z` and `mu` ([H,W] leaves cloned
    from `z0`, `mu0`; float32 or float64), Adam's moments, the snapshots `z_best`, `mu_best` and the device state: `history[max_iters]`,
    `loss_min`, `best_iter` (-1 before any improvement) and the device's own step count.

    Semantics, as the reference has them: the loss of iteration i is the loss at the parameters BEFORE update i; it improves iff
    `loss < loss_min` (strict; a NaN never does); the snapshot then taken holds the parameters AFTER update i -- the reference clones
    `z_grid` behind `optimizer.step()`.  `mu_best` (the reference keeps the height map only) and `bounds` (a box projection behind each
    update, e.g. `dict(mu=(0, inf))`; None: off, the reference) are extensions.  Adam is `torch.optim.Adam`'s default single-tensor step
    (no amsgrad, no weight decay) with `lr = (lr_z, lr_mu)`.

    `graph=True`: the problem's launches and the update are captured once into one hipGraph; a capture the runtime refuses falls back to
    launch by launch with a warning.  `graph=False`: `problem.step(eager=True)`, then the update.  With several ranks active
    (`dist.active()`) the fitter runs ungraphed -- `problem.step` (which exchanges the gradients), then the update; that route has been
    run on one rank only.  The kernel writes `z` and `mu` through raw pointers; their version counters are bumped after every `step()`
    and once after every `run()`, so autograd and the version checks of the rollout caches see the write."""

    def __init__(self, problem, z0, mu0, lr=(0.02, 0.01), betas=(0.9, 0.999), eps=1e-8, bounds=None, max_iters=1000, graph=True):
        if z0.dim() != 2 or mu0.dim() != 2:
            raise ValueError(f'z0 and mu0 must be [H,W] maps, got {tuple(z0.shape)} and {tuple(mu0.shape)}')
        if z0.dtype != mu0.dtype or z0.device != mu0.device:
            raise ValueError('z0 and mu0 must share dtype and device')
        _lib.scalar_suffix(z0.dtype)
        lr_z, lr_mu = (float(v) for v in lr)
        beta1, beta2 = (float(v) for v in betas)
        max_iters = int(max_iters)
        if lr_z < 0 or lr_mu < 0 or not (0 <= beta1 < 1 and 0 <= beta2 < 1) or not eps > 0 or max_iters < 0:
            raise ValueError(f'need lr >= 0, betas in [0, 1), eps > 0, max_iters >= 0; got lr={lr}, betas={betas}, eps={eps}, max_iters={max_iters}')
        flags, z_lo, z_hi, mu_lo, mu_hi = parse_bounds(bounds)
        self.problem = problem
        self.max_iters = max_iters
        self.graph = bool(graph)
        self.iteration = 0          # iterations launched so far (host side; the device keeps its own count)
        self.z = z0.detach().clone().contiguous().requires_grad_(True)
        self.mu = mu0.detach().clone().contiguous().requires_grad_(True)
        self.desc = _lib.MfFitDesc(n_z=self.z.numel(), n_mu=self.mu.numel(), max_iters=max_iters, flags=flags, lr_z=lr_z, lr_mu=lr_mu,
                                   beta1=beta1, beta2=beta2, eps=float(eps), z_lo=z_lo, z_hi=z_hi, mu_lo=mu_lo, mu_hi=mu_hi)
        self.m_z, self.v_z, self.m_mu, self.v_mu = (torch.zeros_like(t) for t in (self.z.detach(), self.z.detach(), self.mu.detach(), self.mu.detach()))
        self.z_best, self.mu_best = self.z.detach().clone(), self.mu.detach().clone()
        self.state, self.loss_min, self.history = new_state(self.z.dtype, self.z.device, max_iters)
        self._state0 = self.state.clone()
        self._captured = None

    # -- state ---------------------------------------------------------------------------------------------------------------------
    @property
    def best_iter(self):
        """0-d int32 device view: the iteration whose loss is `loss_min` (-1: none yet)."""
        return self.state[1]

    @property
    def device_step(self):
        """0-d int32 device view of the device's own iteration count."""
        return self.state[0]

    def reset(self, z0=None, mu0=None):
        """Back to the start: moments, step, `loss_min`, `best_iter` and the history; the parameters to `z0` / `mu0` where given, else
        kept (the snapshots follow the parameters).  In place: a captured graph stays valid.  No host synchronisation."""
        with torch.no_grad():
            if z0 is not None:
                self.z.copy_(z0)
            if mu0 is not None:
                self.mu.copy_(mu0)
            for t in (self.m_z, self.v_z, self.m_mu, self.v_mu):
                t.zero_()
            self.z_best.copy_(self.z)
            self.mu_best.copy_(self.mu)
            self.state.copy_(self._state0)
            self.loss_min.fill_(math.inf)
            self.history.fill_(math.nan)
        self.iteration = 0

    # -- one iteration ---------------------------------------------------------------------------------------------------------------
    def _update(self, loss, g_z, g_mu):
        if g_z is None or g_mu is None:
            raise RuntimeError('TerrainFitter: the step left no gradient for z or mu')
        dt = self.z.dtype
        update(self.desc, self.z.detach(), self.mu.detach(), g_z.detach().to(dt).contiguous(), g_mu.detach().to(dt).contiguous(),
               self.m_z, self.v_z, self.m_mu, self.v_mu, loss.detach().to(dt), self.z_best, self.mu_best, self.state, self.loss_min, self.history)

    def _iterate_eager(self):
        eager = not mfdist.active()        # several ranks: the problem's own step (graph or not), which exchanges gradients and loss
        loss = self.problem.step(self.z, self.mu, eager=True) if eager else self.problem.step(self.z, self.mu)
        self._update(loss, self.z.grad, self.mu.grad)

    def _everything(self):
        return (self.z.detach(), self.mu.detach(), self.z_best, self.mu_best, self.state, self.loss_min, self.history, self.m_z, self.v_z,
                self.m_mu, self.v_mu)

    def _restore(self, snap):
        with torch.no_grad():
            for t, old in zip(self._everything(), snap):
                t.copy_(old)

    def _capture(self):
        dev = self.z.device
        snap = [t.clone() for t in self._everything()]

        def iterate():
            loss, gz, gmu = self.problem._fwd_bwd(self.z, self.mu)
            self._update(loss, gz, gmu)
            return gz, gmu

        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        try:
            with torch.cuda.stream(s):      # warm-up on the capture stream (per-stream workspaces exist, the update's code object is loaded) ...
                for _ in range(2):
                    iterate()
                self._restore(snap)         # ... which leaves no trace: parameters, moments, snapshots and state as they were
            torch.cuda.current_stream(dev).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with capture(g, stream=s, capture_error_mode='thread_local'):
                gz, gmu = iterate()
        except RuntimeError:
            torch.cuda.synchronize(dev)
            self._restore(snap)
            raise
        return dict(graph=g, gz=gz, gmu=gmu)

    def _iterate(self):
        if self.graph and not mfdist.active():
            if self._captured is None:
                try:
                    self._captured = self._capture()
                except RuntimeError as e:       # a capture the runtime refuses: launch by launch, from the state the capture found
                    warnings.warn(f'TerrainFitter: hipGraph capture failed ({str(e).splitlines()[0][:120]}); running launch by launch')
                    self.graph = False
                    return self._iterate_eager()
            self._captured['graph'].replay()
            self.z.grad, self.mu.grad = self._captured['gz'], self._captured['gmu']
            return
        self._iterate_eager()

    def _bump(self):
        torch.autograd.graph.increment_version(self.z)
        torch.autograd.graph.increment_version(self.mu)

    def _room(self, n):
        if n < 0 or self.iteration + n > self.max_iters:
            raise ValueError(f'{n} more iterations after {self.iteration} do not fit the history of max_iters={self.max_iters}')

    def step(self):
        """One iteration.  Returns the 0-d device tensor of this iteration's loss (a view of the history); no host synchronisation."""
        self._room(1)
        self._iterate()
        self._bump()
        self.iteration += 1
        return self.history[self.iteration - 1]

    def run(self, n):
        """`n` iterations without a host synchronisation.  Returns device tensors only: `loss` (this call's slice of the history),
        `loss_min`, `best_iter` (0-d), the snapshots `z_best`, `mu_best` and the live parameters `z`, `mu`."""
        n = int(n)
        self._room(n)
        start = self.iteration
        try:
            for _ in range(n):
                self._iterate()
                self.iteration += 1
        finally:
            self._bump()
        return dict(loss=self.history[start:start + n], loss_min=self.loss_min[0], best_iter=self.state[1], z_best=self.z_best,
                    mu_best=self.mu_best, z=self.z, mu=self.mu)
