"""The fit loop of scripts/fit_terrain.py:46-69 in two forms, timed over whole loops of 100 iterations:

    fitter   `TerrainFitter.run(100)`: the step's launches and ONE update launch (Adam on both maps + best-so-far, state on the device)
             replayed as one hipGraph per iteration; the host never waits
    parent   the loop as it was written before the fitter existed: `TerrainFitProblem(graph=True).step` + `torch.optim.Adam` over two
             parameter groups + `loss.item()` + `if loss < loss_min: z_best = z.clone()`

    python tools/bench_terrain_fit.py [--loops 7] [--iters 100] [--out profiles/terrain_fit.txt]

Shapes: BASELINE configs[0] (1 rollout x 200 steps on 128 x 128 cells) and configs[2] (1024 rollouts x 500 steps x 4 points on 256 x 256).
Method: both forms in one process, alternating loop by loop after one warm-up loop each (captures included); every loop starts from the
same parameters with fresh optimiser state (the reset is outside the timed window); HIP events around each whole loop and the host's wall
clock beside them (the loop ends in a synchronise); per-iteration figures are loop time / iterations; median, min and max over the loops.
The update launch's own time: HIP events around 200 back-to-back launches on the fitter's buffers, per launch."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_problem  # noqa: E402
from monoforce_amd import fit as mffit  # noqa: E402
from monoforce_amd import synthetic as syn  # noqa: E402
from monoforce_amd.train import TerrainFitProblem  # noqa: E402

DEV = 'cuda'
LR, BETAS, EPS = (0.02, 0.01), (0.9, 0.999), 1e-8
SHAPES = [dict(name='configs[0]', B=1, T=200, grid_res=0.1), dict(name='configs[2]', B=1024, T=500, grid_res=0.05)]


class ParentLoop:
    def __init__(self, prob, z0, mu0):
        self.prob, self.z0, self.mu0 = prob, z0, mu0
        self.z, self.mu = z0.clone().requires_grad_(True), mu0.clone().requires_grad_(True)
        self.reset()

    def reset(self):
        with torch.no_grad():
            self.z.copy_(self.z0)
            self.mu.copy_(self.mu0)
        self.opt = torch.optim.Adam([{'params': self.z, 'lr': LR[0]}, {'params': self.mu, 'lr': LR[1]}], betas=BETAS, eps=EPS)
        self.loss_min, self.z_best, self.losses = float('inf'), None, []

    def run(self, n):
        for _ in range(n):
            loss = self.prob.step(self.z, self.mu)
            self.opt.step()
            value = loss.item()
            self.losses.append(value)
            if value < self.loss_min:
                self.loss_min = value
                self.z_best = self.z.detach().clone()


def timed_loop(run, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    run(n)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n, (time.perf_counter() - t0) * 1e3 / n


def stats(ms):
    ms = np.asarray(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4), max_ms=round(float(ms.max()), 4))


def update_launch_ms(fit, n=200):
    """The update launch alone, on the fitter's own buffers and its last gradients; parameters and state are put back afterwards."""
    snap = [t.clone() for t in fit._everything()]
    loss = fit.history[0].clone()

    def go():
        for _ in range(n):
            fit._update(loss, fit.z.grad, fit.mu.grad)
    go()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    go()
    b.record()
    torch.cuda.synchronize()
    fit._restore(snap)
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loops', type=int, default=7)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'terrain_fit.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_terrain_fit needs the MI355X'
    lines = ['# tools/bench_terrain_fit.py: the fit loop of scripts/fit_terrain.py:46-69, TerrainFitter.run against the loop form it replaces',
             '# (TerrainFitProblem(graph=True).step + torch.optim.Adam over two groups + loss.item() + conditional clone), same process, alternating',
             f'# loops of {args.iters} iterations, {args.loops} timed loops per form after one warm-up loop; ms per ITERATION; events = HIP events around',
             '# the whole loop, wall = host clock around the loop and its final synchronise',
             f'# device: {torch.cuda.get_device_name(0)}']
    verdicts = []
    for shape in SHAPES:
        B, T, res = shape['B'], shape['T'], shape['grid_res']
        _, dp, _, _, z, mu, ctrl = build_problem(B, T, 4, DEV, 1, seed=0, grid_res=res)
        z_true = syn.bump_terrain(syn.bump_params(100), 6.4, res).to(DEV)
        z0, mu0, ctrl = z.to(DEV), mu.to(DEV), ctrl.to(DEV)
        parent = ParentLoop(TerrainFitProblem(dp, z_true, mu0, ctrl, graph=True), z0, mu0)
        fitter = mffit.TerrainFitter(TerrainFitProblem(dp, z_true, mu0, ctrl), z0, mu0, lr=LR, betas=BETAS, eps=EPS, max_iters=args.iters, graph=True)
        forms = dict(fitter=(lambda: fitter.reset(z0, mu0), fitter.run), parent=(parent.reset, parent.run))
        for reset, run in forms.values():      # warm-up: captures, code objects, Adam's state kernels
            reset()
            run(args.iters)
        assert fitter.graph and fitter._captured is not None and parent.prob.graph
        torch.cuda.synchronize()
        first = dict(fitter=float(fitter.history[0]), parent=parent.losses[0])
        ms = {k: ([], []) for k in forms}
        for _ in range(args.loops):
            for k, (reset, run) in forms.items():
                reset()
                ev, wall = timed_loop(run, args.iters)
                ms[k][0].append(ev)
                ms[k][1].append(wall)
        upd = update_launch_ms(fitter)
        for k in forms:
            row = dict(shape=shape['name'], B=B, T=T, cells=int(z0.numel()), form=k, iters_per_loop=args.iters, loops=args.loops,
                       events=stats(ms[k][0]), wall=stats(ms[k][1]), first_loss=float('%.6g' % first[k]))
            if k == 'fitter':
                row['update_launch_ms'] = round(upd, 4)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        ratio = float(np.median(ms['parent'][0]) / np.median(ms['fitter'][0]))
        ratio_wall = float(np.median(ms['parent'][1]) / np.median(ms['fitter'][1]))
        verdicts.append(ratio >= 1 and ratio_wall >= 1)
        lines.append(f'# {shape["name"]}: parent / fitter = {ratio:.2f} (events), {ratio_wall:.2f} (wall), medians; TerrainFitter.run is '
                     f'{"not above" if verdicts[-1] else "ABOVE"} the parent form; the update launch alone: {upd * 1e3:.1f} us')
        print(lines[-1], flush=True)
        del parent, fitter, forms
    lines.append('# TerrainFitter.run is not above the parent form at either shape' if all(verdicts) else
                 '# TerrainFitter.run is ABOVE the parent form somewhere: see the lines marked ABOVE')
    lines.append('# the update is the one-launch ticket form (the last workgroup commits the scalars); a two-launch form was not built')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
