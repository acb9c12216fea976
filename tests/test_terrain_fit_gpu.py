"""The terrain-fit loop on the GPU (monoforce_amd/fit.py, csrc/terrain_fit.hip).

Kernel level: `fit.update` alone, fed synthetic gradients and losses, against `torch.optim.Adam` itself on the CPU in float64 plus the
reference's best-tracking (scripts/fit_terrain.py:61-69).  Bars on the parameters (of order 1, lr <= 0.02, K = 8 steps): float64 1e-12
absolute; float32 the rule of the project's side kernels, max(1e-6, 2 x the error of torch.optim.Adam in float32 on the CPU against the same
referee).  Counts, best step, smallest loss, history and snapshots are exact.  Loop level: `TerrainFitter` around a `TerrainFitProblem`.

Every measured error is printed on a line starting with `terrain-fit-error` (`pytest -s`); profiles/terrain_fit_errors.txt keeps them.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K = 8
LR, BETAS, EPS = (0.02, 0.01), (0.9, 0.999), 1e-8

SEQUENCES = {
    'decreasing': [8, 7, 6, 5, 4, 3, 2, 1],
    'increasing': [1, 2, 3, 4, 5, 6, 7, 8],
    'alternating': [5, 6, 4, 7, 3, 8, 2, 9],
    'tie': [3, 3, 2, 2, 2, 5, 1, 1],
    'nan': [5, 4, 3, math.nan, 2, 6, math.nan, 1.5],
}


def _cap_cells():
    from monoforce_amd import fit
    return fit.grid_cap() * 256


def _sizes():
    return [(1, 1), (63, 65), (64, 64), (255, 257), (256, 1), (1600, 400), ('cap+300', 1000)]


def _resolve(size):
    n_z, n_mu = size
    return (_cap_cells() + 300 if n_z == 'cap+300' else n_z), n_mu


def make_inputs(n_z, n_mu, seed):
    """Parameters of order 1 and K gradients per map, all float32-representable (both dtypes and the referee see the same numbers).
    By cell index modulo 8: 0 -> a gradient that is exactly zero in every step, 1 / 2 -> +-1e-12, 3 / 4 -> +-1e4, the rest ordinary
    values, a fifth of them exact zeros in single steps.  (The friction map's pattern starts at 5: a one-cell map is an ordinary cell.)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, n, off in (('z', n_z, 0), ('mu', n_mu, 5)):
        p0 = (torch.rand(n, generator=g) * 2 - 1).float()
        gr = torch.randn(K, n, generator=g).float()
        gr[torch.rand(K, n, generator=g) < 0.2] = 0.0
        kind = (torch.arange(n) + off) % 8
        for k, v in ((0, 0.0), (1, 1e-12), (2, -1e-12), (3, 1e4), (4, -1e4)):
            gr[:, kind == k] = v
        out[name] = (p0, gr, kind == 0)
    return out


def referee(inp, losses, dtype, bounds=None, lr=LR, betas=BETAS, eps=EPS, grads=None):
    """torch.optim.Adam (two parameter groups) on the CPU in `dtype` + the reference's loop: the loss of step i belongs to the parameters
    before it; `if loss < loss_min` the maps are cloned AFTER optimizer.step().  A box is applied behind the step, outside Adam."""
    z = inp['z'][0].to(dtype).clone().requires_grad_(True)
    mu = inp['mu'][0].to(dtype).clone().requires_grad_(True)
    gz, gmu = (inp['z'][1], inp['mu'][1]) if grads is None else grads
    opt = torch.optim.Adam([{'params': z, 'lr': lr[0]}, {'params': mu, 'lr': lr[1]}], betas=betas, eps=eps)
    loss_min, best_step, z_best, mu_best, after = math.inf, -1, z.detach().clone(), mu.detach().clone(), []
    for i, loss in enumerate(losses):
        z.grad, mu.grad = gz[i].to(dtype).reshape(z.shape), gmu[i].to(dtype).reshape(mu.shape)
        opt.step()
        with torch.no_grad():
            for p, name in ((z, 'z'), (mu, 'mu')):
                if bounds and bounds.get(name) is not None:
                    p.clamp_(*bounds[name])
        if loss < loss_min:
            loss_min, best_step, z_best, mu_best = loss, i, z.detach().clone(), mu.detach().clone()
        after.append((z.detach().clone(), mu.detach().clone()))
    st = opt.state
    return dict(z=z.detach(), mu=mu.detach(), z_best=z_best, mu_best=mu_best, loss_min=loss_min, best_step=best_step, after=after,
                m_z=st[z]['exp_avg'], v_z=st[z]['exp_avg_sq'], m_mu=st[mu]['exp_avg'], v_mu=st[mu]['exp_avg_sq'])


class KernelRun:
    """The buffers of one fit driven through `fit.update` alone."""

    def __init__(self, inp, losses, dtype, flags=0, box=(-math.inf, math.inf, -math.inf, math.inf), max_iters=K, lr=LR):
        from monoforce_amd import _lib, fit
        self.fit = fit
        self.p = {n: inp[n][0].to(dtype).to(DEV) for n in ('z', 'mu')}
        self.g = {n: inp[n][1].to(dtype).to(DEV) for n in ('z', 'mu')}
        self.m = {n: torch.zeros_like(self.p[n]) for n in ('z', 'mu')}
        self.v = {n: torch.zeros_like(self.p[n]) for n in ('z', 'mu')}
        self.best = {n: self.p[n].clone() for n in ('z', 'mu')}
        self.losses = torch.tensor(losses, dtype=dtype, device=DEV)
        self.state, self.loss_min, _ = fit.new_state(dtype, DEV, 0)
        self.guarded = torch.full((max_iters + 1,), -777.0, dtype=dtype, device=DEV)      # the history and one guard element behind it
        self.history = self.guarded[:max_iters]
        self.desc = _lib.MfFitDesc(n_z=self.p['z'].numel(), n_mu=self.p['mu'].numel(), max_iters=max_iters, flags=flags, lr_z=lr[0], lr_mu=lr[1],
                                   beta1=BETAS[0], beta2=BETAS[1], eps=EPS, z_lo=box[0], z_hi=box[1], mu_lo=box[2], mu_hi=box[3])

    def launch(self, i):
        self.fit.update(self.desc, self.p['z'], self.p['mu'], self.g['z'][i], self.g['mu'][i], self.m['z'], self.v['z'], self.m['mu'], self.v['mu'],
                        self.losses[i], self.best['z'], self.best['mu'], self.state, self.loss_min, self.history)

    def back_to_back(self):
        """Steps 1..K with no synchronisation in between: a commit that could overtake another workgroup's reads would show here."""
        for i in range(len(self.losses)):
            self.launch(i)
        torch.cuda.synchronize()
        return self

    def one_by_one(self):
        """The same steps, synchronised: the parameters after every step."""
        after = []
        for i in range(len(self.losses)):
            self.launch(i)
            torch.cuda.synchronize()
            after.append((self.p['z'].clone(), self.p['mu'].clone()))
        return after


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def max_err(a, b):
    return float((a.double().cpu() - b.double()).abs().max()) if a.numel() else 0.0


def param_bar(dtype, aten_err):
    return 1e-12 if dtype == torch.float64 else max(1e-6, 2.0 * aten_err)


def check_against_referee(tag, run, ref, ref32, dtype):
    """Parameters and snapshots by the bars of the module docstring; moments by the same figure relative to each cell's own gradient scale
    (g up to 1e4, g^2 up to 1e8)."""
    for name in ('z', 'mu'):
        e_hip = max(max_err(run.p[name], ref[name]), max_err(run.best[name], ref[name + '_best']))
        e_aten = 0.0 if ref32 is None else max(max_err(ref32[name], ref[name]), max_err(ref32[name + '_best'], ref[name + '_best']))
        bar = param_bar(dtype, e_aten)
        print(f'terrain-fit-error {tag} {name:2s} parameters hip {e_hip:.3g} aten_f32 {e_aten:.3g} bar {bar:.3g}')
        assert e_hip <= bar, (tag, name, e_hip, bar)
        scale = run.g[name].double().abs().amax(0).cpu()
        for mom, power in (('m', 1), ('v', 2)):
            got, want = getattr(run, mom)[name].double().cpu(), ref[f'{mom}_{name}'].double()
            s = scale ** power
            assert bool((got[s == 0] == 0).all())
            rel = float(((got - want).abs()[s > 0] / s[s > 0]).max()) if bool((s > 0).any()) else 0.0
            rel_aten = 0.0
            if ref32 is not None and bool((s > 0).any()):
                rel_aten = float(((ref32[f'{mom}_{name}'].double() - want).abs()[s > 0] / s[s > 0]).max())
            assert rel <= param_bar(dtype, rel_aten), (tag, name, mom, rel, rel_aten)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('size', _sizes(), ids=lambda s: f'{s[0]}x{s[1]}')
def test_update_kernel_against_torch_adam(size, dtype):
    n_z, n_mu = _resolve(size)
    if size[0] == 'cap+300':
        assert n_z + n_mu > _cap_cells()          # the grid-stride loop takes a second trip
    inp = make_inputs(n_z, n_mu, seed=n_z + 7 * n_mu)
    for seq, losses in SEQUENCES.items():
        tag = f'kernel {n_z}x{n_mu} {str(dtype)[6:]} {seq}'
        ref = referee(inp, losses, torch.float64)
        ref32 = referee(inp, losses, torch.float32) if dtype == torch.float32 else None
        run = KernelRun(inp, losses, dtype).back_to_back()
        # exact: counts, best step, smallest loss, history, a ticket back at zero
        assert run.state.tolist() == [K, ref['best_step'], 0, 0], (tag, run.state.tolist())
        assert float(run.loss_min) == ref['loss_min'], tag
        assert same_bits(run.history, run.losses), tag
        assert float(run.guarded[K]) == -777.0, tag
        # the snapshots are the parameters after the best step, to the bit: a second, synchronised pass of the same inputs
        again = KernelRun(inp, losses, dtype)
        after = again.one_by_one()
        assert same_bits(run.p['z'], again.p['z']) and same_bits(run.p['mu'], again.p['mu']), tag
        assert torch.equal(run.best['z'], after[ref['best_step']][0]) and torch.equal(run.best['mu'], after[ref['best_step']][1]), tag
        # a cell whose gradient is zero in every step has not moved, to the bit
        for name in ('z', 'mu'):
            still = inp[name][2].to(DEV)
            assert same_bits(run.p[name][still], inp[name][0].to(dtype).to(DEV)[still]), (tag, name)
        check_against_referee(tag, run, ref, ref32, dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_update_kernel_box_projection(dtype):
    """mu in [0, 1] with gradients that push out of the box: the referee's clamped parameters; the moments do not see the clamp; and
    without a box the result is, to the bit, that of a box of +-inf."""
    n_z, n_mu = 255, 257
    inp = make_inputs(n_z, n_mu, seed=11)
    g = torch.Generator().manual_seed(12)
    edge = torch.rand(n_mu, generator=g) < 0.5
    mu0 = torch.where(edge, 0.02 * torch.rand(n_mu, generator=g), 1 - 0.02 * torch.rand(n_mu, generator=g)).float()
    inp['mu'] = (mu0, inp['mu'][1], inp['mu'][2])
    losses = SEQUENCES['alternating']
    bounds, lr = dict(mu=(0.0, 1.0)), (0.02, 0.02)
    ref = referee(inp, losses, torch.float64, bounds=bounds, lr=lr)
    ref32 = referee(inp, losses, torch.float32, bounds=bounds, lr=lr) if dtype == torch.float32 else None
    assert int((ref['mu'] == 0).sum()) > 10 and int((ref['mu'] == 1).sum()) > 10       # the box binds on both sides
    from monoforce_amd import _lib
    boxed = KernelRun(inp, losses, dtype, flags=_lib.MF_FIT_CLAMP_MU, box=(0.0, 0.0, 0.0, 1.0), lr=lr).back_to_back()      # (z's box is not read)
    assert boxed.state.tolist() == [K, ref['best_step'], 0, 0]
    assert float(boxed.p['mu'].min()) == 0.0 and float(boxed.p['mu'].max()) == 1.0
    check_against_referee(f'kernel-box {n_z}x{n_mu} {str(dtype)[6:]}', boxed, ref, ref32, dtype)
    free = KernelRun(inp, losses, dtype, lr=lr).back_to_back()
    assert float(free.p['mu'].min()) < 0.0 and float(free.p['mu'].max()) > 1.0
    for name in ('z', 'mu'):
        assert same_bits(boxed.m[name], free.m[name]) and same_bits(boxed.v[name], free.v[name])
    assert same_bits(boxed.p['z'], free.p['z'])
    inf = math.inf
    wide = KernelRun(inp, losses, dtype, flags=_lib.MF_FIT_CLAMP_Z | _lib.MF_FIT_CLAMP_MU, box=(-inf, inf, -inf, inf), lr=lr).back_to_back()
    for name in ('z', 'mu'):
        assert same_bits(wide.p[name], free.p[name]) and same_bits(wide.best[name], free.best[name])
    assert wide.state.tolist() == free.state.tolist()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_update_kernel_history_stops_at_max_iters(dtype):
    """K launches into a history of K - 2: the first K - 2 losses are kept, nothing is written behind the buffer, the step keeps counting
    and the best-tracking goes on."""
    inp = make_inputs(1600, 400, seed=3)
    losses = SEQUENCES['decreasing']
    run = KernelRun(inp, losses, dtype, max_iters=K - 2).back_to_back()
    assert run.history.shape == (K - 2,) and same_bits(run.history, run.losses[:K - 2])
    assert float(run.guarded[K - 2]) == -777.0
    assert run.state.tolist() == [K, K - 1, 0, 0] and float(run.loss_min) == 1.0
    full = KernelRun(inp, losses, dtype).back_to_back()
    assert same_bits(run.p['z'], full.p['z']) and same_bits(run.best['mu'], full.best['mu'])


# ---- loop level ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 100), (1, 50)]
ITERS = 6
_problems = {}


def problem(B, T, tv_weight=0.0):
    """(TerrainFitProblem, z0, mu0) at 128 x 128 cells: rollouts of bench.py's synthetic controls, ground truth from another terrain.  Built
    once per shape and shared: the tests give it parameters of their own and leave it as it is."""
    key = (B, T, tv_weight)
    if key not in _problems:
        from bench import build_problem
        from monoforce_amd import synthetic as syn
        from monoforce_amd.train import TerrainFitProblem
        _, dp, _, _, z, mu, ctrl = build_problem(B, T, 4, DEV, 1, seed=0, grid_res=0.1)
        z_true = syn.bump_terrain(syn.bump_params(100), 6.4, 0.1).to(DEV)
        _problems[key] = (TerrainFitProblem(dp, z_true, mu.to(DEV), ctrl.to(DEV), tv_weight=tv_weight), z.to(DEV), mu.to(DEV))
    return _problems[key]


def eager_step(prob, z, mu):
    """Loss and gradients of the problem at (z, mu), launch by launch, on leaves of their own."""
    zc, mc = z.detach().clone().requires_grad_(True), mu.detach().clone().requires_grad_(True)
    loss = prob.step(zc, mc, eager=True)
    return float(loss), zc.grad.clone(), mc.grad.clone()


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize('B, T', SHAPES)
def test_fitter_eager_route_against_torch_adam(B, T):
    """`step()` six times launch by launch; the gradients and losses it used, recorded, drive the CPU float64 Adam: parameters, snapshot,
    best iteration and smallest loss agree by the kernel-level bars (recording takes the rollout's float-atomic noise out)."""
    from monoforce_amd import TerrainFitter
    prob, z0, mu0 = problem(B, T)
    fit = TerrainFitter(prob, z0, mu0, lr=LR, betas=BETAS, eps=EPS, max_iters=ITERS, graph=False)
    gz, gmu, losses, versions = [], [], [], []
    for i in range(ITERS):
        loss = fit.step()
        gz.append(fit.z.grad.detach().clone().cpu().flatten())
        gmu.append(fit.mu.grad.detach().clone().cpu().flatten())
        losses.append(float(loss))
        versions.append(fit.z._version)
    assert fit.iteration == ITERS and versions == sorted(set(versions))        # every step bumps the version counter
    assert int(fit.device_step) == ITERS and fit.history.tolist() == losses
    inp = dict(z=(z0.cpu().flatten(), None, None), mu=(mu0.cpu().flatten(), None, None))
    ref = referee(inp, losses, torch.float64, grads=(gz, gmu))
    ref32 = referee(inp, losses, torch.float32, grads=(gz, gmu))
    assert int(fit.best_iter) == ref['best_step'] and float(fit.loss_min) == ref['loss_min']
    for name, got, best in (('z', fit.z, fit.z_best), ('mu', fit.mu, fit.mu_best)):
        e_hip = max(max_err(got.detach().flatten(), ref[name]), max_err(best.flatten(), ref[name + '_best']))
        e_aten = max(max_err(ref32[name], ref[name]), max_err(ref32[name + '_best'], ref[name + '_best']))
        bar = param_bar(torch.float32, e_aten)
        print(f'terrain-fit-error loop-eager B={B} T={T} {name:2s} parameters hip {e_hip:.3g} aten_f32 {e_aten:.3g} bar {bar:.3g}')
        assert e_hip <= bar, (name, e_hip, bar)


def first_step_checks(name, p0, p, g, lr):
    """After ONE Adam step from zero moments a cell has moved against its gradient by lr |g| / (|g| + eps)."""
    g, moved = g.double(), (p0.double() - p.detach().double())
    big = g.abs() > 1e-6 * g.abs().max()
    assert int(big.sum()) > 0
    assert bool((torch.sign(moved[big]) == torch.sign(g[big])).all()), name
    dev = (moved[big].abs() - lr).abs()
    tol = lr * (EPS / g[big].abs() + 1e-5)
    assert bool((dev <= tol).all()), (name, float((dev - tol).max()))
    assert same_bits(p.detach()[g == 0], p0[g == 0]), name


@pytest.mark.parametrize('B, T', SHAPES)
def test_fitter_graph_route(B, T):
    """Properties of the replayed loop that do not need bitwise-repeatable gradients: the first step's size and direction, the history
    against eager losses at the live parameters, the counts, and a warm-up that left no trace."""
    from monoforce_amd import TerrainFitter
    prob, z0, mu0 = problem(B, T)
    loss0, g_z, g_mu = eager_step(prob, z0, mu0)
    fit = TerrainFitter(prob, z0, mu0, lr=LR, betas=BETAS, eps=EPS, max_iters=ITERS, graph=True)
    out = fit.run(1)
    assert fit.graph and fit._captured is not None and fit.iteration == 1 and int(fit.device_step) == 1
    first_step_checks('z', z0, fit.z, g_z, LR[0])
    first_step_checks('mu', mu0, fit.mu, g_mu, LR[1])
    h0 = float(out['loss'][0])
    print(f'terrain-fit-error loop-graph B={B} T={T} history[0] against the eager loss: {rel(h0, loss0):.3g} bar 1e-05')
    assert rel(h0, loss0) <= 1e-5
    assert int(out['best_iter']) == 0 and float(out['loss_min']) == h0 and same_bits(out['z_best'], fit.z.detach())
    # the moments are ONE step's (two warm-up steps would leave 1 - 0.9^3 = 0.271 g instead of 0.1 g)
    for m, v, g in ((fit.m_z, fit.v_z, fit.z.grad), (fit.m_mu, fit.v_mu, fit.mu.grad)):
        assert float((m.double() - (1 - BETAS[0]) * g.double()).abs().max()) <= 1e-6 * (1 - BETAS[0]) * float(g.abs().max())
        assert float((v.double() - (1 - BETAS[1]) * g.double() ** 2).abs().max()) <= 1e-6 * (1 - BETAS[1]) * float(g.abs().max()) ** 2
    # the replay reads the live maps: back to the start, five iterations, a clone, one more
    fit.reset(z0, mu0)
    fit.run(5)
    z5, mu5 = fit.z.detach().clone(), fit.mu.detach().clone()
    out = fit.run(1)
    loss5 = eager_step(prob, z5, mu5)[0]
    print(f'terrain-fit-error loop-graph B={B} T={T} history[5] against the eager loss: {rel(float(fit.history[5]), loss5):.3g} bar 1e-05')
    assert rel(float(fit.history[5]), loss5) <= 1e-5 and rel(float(fit.history[0]), loss0) <= 1e-5
    assert out['loss'].shape == (1,) and float(out['loss'][0]) == float(fit.history[5])
    assert fit.iteration == ITERS and int(fit.device_step) == ITERS
    assert float(out['loss_min']) == float(fit.history.min()) and int(out['best_iter']) == int(fit.history.argmin())
    with pytest.raises(ValueError, match='max_iters'):
        fit.run(1)


def parent_loop(prob, z0, mu0):
    """The loop as its callers wrote it before: problem.step + torch.optim.Adam over two groups + loss.item()."""
    z, mu = z0.clone().requires_grad_(True), mu0.clone().requires_grad_(True)
    opt = torch.optim.Adam([{'params': z, 'lr': LR[0]}, {'params': mu, 'lr': LR[1]}], betas=BETAS, eps=EPS)
    losses = []
    for _ in range(ITERS):
        losses.append(prob.step(z, mu).item())
        opt.step()
    return torch.tensor(losses, dtype=torch.float64)


@pytest.mark.parametrize('B, T', SHAPES)
def test_fitter_graph_against_eager_histories(B, T):
    """Six iterations replayed against six launch by launch: the loss histories differ by no more than ten times what two runs of the
    parent-form loop differ by (the run-to-run noise of the rollout's float atomics), floor 1e-5.  Measured on an MI355X: 64 x 100 graph
    against eager 0.029 and 0.038 with a noise of 0.0072 and 0.034 in the same runs (2 cm Adam steps make the 64 rollouts diverge from
    last-bit differences of the gradient within six iterations); 1 x 50, where one rollout leaves the atomics no choice of order, 0 to 6e-7
    with a noise of 1e-6."""
    from monoforce_amd import TerrainFitter
    prob, z0, mu0 = problem(B, T)
    a, b = parent_loop(prob, z0, mu0), parent_loop(prob, z0, mu0)
    noise = float(((a - b).abs() / b.abs()).max())
    hist = {}
    for graph in (True, False):
        fit = TerrainFitter(prob, z0, mu0, lr=LR, betas=BETAS, eps=EPS, max_iters=ITERS, graph=graph)
        hist[graph] = fit.run(ITERS)['loss'].double().cpu()
    diff = float(((hist[True] - hist[False]).abs() / hist[False].abs()).max())
    against_parent = float(((hist[True] - a).abs() / a.abs()).max())
    bar = max(1e-5, 10 * noise)
    print(f'terrain-fit-error loop-histories B={B} T={T} graph against eager {diff:.3g} (against the parent-form loop {against_parent:.3g}) '
          f'parent-form run-to-run noise {noise:.3g} bar {bar:.3g}')
    assert diff <= bar


@pytest.mark.parametrize('B, T', SHAPES)
def test_fitter_run_never_synchronises(B, T):
    from monoforce_amd import TerrainFitter
    prob, z0, mu0 = problem(B, T)
    fit = TerrainFitter(prob, z0, mu0, max_iters=ITERS + 1, graph=True)
    fit.run(1)                                     # (the capture)
    assert fit._captured is not None
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = fit.run(ITERS)
        loss = out['loss']
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert fit.iteration == ITERS + 1 and int(fit.device_step) == ITERS + 1 and bool(torch.isfinite(loss).all()) and loss.shape == (ITERS,)


TV_LR = (0.002, 0.001)


@pytest.mark.parametrize('B, T', SHAPES)
def test_fitter_tv_regularised(B, T):
    """`TerrainFitProblem(tv_weight=0.1)` under the fitter: history[0] is the eager regularised loss, and the loss after six iterations is
    below the first.  The rates are a tenth of the reference's (0.02, 0.01), for a reason that lies in Adam and the regulariser, not in
    the code under test: Adam's first steps move every cell with a non-zero gradient by +-lr whatever the gradient's size, total variation
    has a kink wherever two neighbours are level, and the neighbouring cells of the start terrain differ by 0.0019 m (median; mean 0.005) --
    a 0.02 m step overshoots those kinks tenfold and roughens the map.  Measured on an MI355X, the loop as its callers wrote it before
    (`problem.step` + `torch.optim.Adam`) at the reference's rates RISES over these six iterations, and the fitter follows it digit for digit:
    64 x 100: 0.001350 -> 0.001913, 0.002021, 0.002080, 0.002019, 0.001970, then 0.001899 (the fitter: ..., 0.001970, then 0.001900);
    1 x 50: 0.001205 -> 0.001675, 0.001697, 0.002391, 0.001656, 0.001510, then 0.001557.  At (0.002, 0.001), the median neighbour
    difference, both fall: 0.001350 -> 0.001210 and 0.001205 -> 0.001129 (0.1 x TV alone is 0.00107 of either start value)."""
    from monoforce_amd import TerrainFitter
    prob, z0, mu0 = problem(B, T, tv_weight=0.1)
    plain = eager_step(problem(B, T)[0], z0, mu0)[0]
    loss0 = eager_step(prob, z0, mu0)[0]
    assert loss0 > plain                            # the regulariser is in the loss
    fit = TerrainFitter(prob, z0, mu0, lr=TV_LR, max_iters=ITERS, graph=True)
    out = fit.run(ITERS)
    h = out['loss'].double().cpu()
    after = eager_step(prob, fit.z, fit.mu)[0]
    print(f'terrain-fit-error loop-tv B={B} T={T} history[0] against the eager regularised loss: {rel(float(h[0]), loss0):.3g} bar 1e-05; '
          f'losses {[round(float(v), 6) for v in h]} then {after:.6f}')
    assert rel(float(h[0]), loss0) <= 1e-5
    assert after < float(h[0])


@pytest.mark.parametrize('B, T', SHAPES)
def test_fitter_reset(B, T):
    from monoforce_amd import TerrainFitter
    prob, z0, mu0 = problem(B, T)
    fit = TerrainFitter(prob, z0, mu0, lr=LR, max_iters=ITERS, graph=True)
    first = float(fit.run(3)['loss'][0])
    assert not torch.equal(fit.z.detach(), z0) and float(fit.m_z.abs().max()) > 0
    z3 = fit.z.detach().clone()
    fit.reset()                                     # the parameters are kept
    assert same_bits(fit.z.detach(), z3) and same_bits(fit.z_best, z3) and fit.iteration == 0
    fit.reset(z0, mu0)
    assert fit.state.tolist() == [0, -1, 0, 0] and math.isinf(float(fit.loss_min)) and bool(fit.history.isnan().all())
    assert all(float(t.abs().max()) == 0.0 for t in (fit.m_z, fit.v_z, fit.m_mu, fit.v_mu))
    assert same_bits(fit.z.detach(), z0) and same_bits(fit.mu.detach(), mu0) and same_bits(fit.mu_best, mu0)
    again = float(fit.run(1)['loss'][0])
    assert rel(again, first) <= 1e-5 and int(fit.device_step) == 1 and int(fit.best_iter) == 0
