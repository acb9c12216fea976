"""One iteration of gradient descent on K control sequences: `ControlRefiner` (HIP objective + update kernels around the autograd rollout)
against the same loop written with ATen ops.

    python tools/bench_refine.py [--sizes 16,64,256] [--iters 60] [--warmup 10] [--out profiles/control_refine.txt]

All forms run the same differentiable rollout (`DPhysics.forward` through autograd, T = 500, one shared 256 x 256 map pair, the 4-point body)
and its backward, and differ in everything around it:
    graph   ControlRefiner(graph=True): rollout | traj_objective (value + gradient) | rollout backward | control_refine_update, ONE hipGraph replay
    eager   ControlRefiner(graph=False): the same launches, one by one
    aten    rollout | trajectory_objective_aten | autograd through it and the rollout | torch.optim.Adam | clamp_ | torch.where copies of the best
The objective weighs all four terms (cost map, path, goal, inclination) at one kept pose per map cell at full speed (pose_stride = 5: 101 poses).
The aten form's Adam has ONE rate for both channels (a rate per channel needs two parameter tensors and a stack per iteration); its
best-so-far bookkeeping is per sequence and reads nothing on the host, like the kernel's.
Method: HIP events around every iteration, the three forms alternating in one process after a warm-up of all; median, minimum and 90th
percentile over the iterations (`median_ms` ...: device time); then loops of ten iterations of one form between two synchronisations by the
wall clock, seven loops per form, alternating (`loop_wall_ms`: what a caller waits per iteration, the host's launch work included).  Every
form goes back to the same start controls every ten iterations, so that the rollouts stay comparable."""
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
from monoforce_amd import ControlRefiner, ops  # noqa: E402
from monoforce_amd.refine import trajectory_objective_aten  # noqa: E402

DEV = 'cuda'
T = 500
WEIGHTS = dict(goal=1.0, map=0.5, path=0.5, inclination=0.2)
LR = (0.05, 0.1)


def smooth_cost_map(n=256):
    i, j = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32), indexing='ij')
    m = 0.002 * i + 0.001 * j
    for ci, cj, s in ((150.0, 140.0, 12.0), (170.0, 110.0, 20.0), (120.0, 160.0, 8.0)):
        m = m + torch.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (2 * s * s))
    return m


class AtenRefiner:
    """The iteration `ControlRefiner` replaces, written with ATen ops around the same rollout."""

    def __init__(self, ref, ctrl0):
        self.ref = ref
        self.controls = ctrl0.detach().clone().to(DEV).requires_grad_(True)
        self.opt = torch.optim.Adam([self.controls], lr=LR[0])
        self.lo, self.hi = torch.tensor(ref.lo, device=DEV), torch.tensor(ref.hi, device=DEV)
        self.best_controls = self.controls.detach().clone()
        self.best_cost = torch.full((ctrl0.shape[0],), float('inf'), device=DEV)
        self.start = ctrl0.detach().clone().to(DEV)

    def reset(self):
        with torch.no_grad():
            self.controls.copy_(self.start)
        self.opt = torch.optim.Adam([self.controls], lr=LR[0])
        self.best_cost.fill_(float('inf'))

    def step(self, z, goal, mu, cost_map, path):
        r = self.ref
        states, _ = r.dp(z, self.controls, friction=mu, _want_forces=False)
        costs, _ = trajectory_objective_aten(states[0], states[2], goal, points=r.footprint, cost_map=cost_map, path=path, weights=r.weights,
                                             pose_stride=r._stride(True), grid_res=r.cfg.grid_res, d_max=r.cfg.d_max, lethal=r.lethal, off_map=r.off_map)
        self.opt.zero_grad(set_to_none=True)
        costs.sum().backward()
        with torch.no_grad():
            improved = costs.detach() < self.best_cost
            self.best_controls = torch.where(improved[:, None, None], self.controls, self.best_controls)
            self.best_cost = torch.where(improved, costs.detach(), self.best_cost)
        self.opt.step()
        with torch.no_grad():
            self.controls.copy_(torch.minimum(torch.maximum(self.controls, self.lo), self.hi))
        return costs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='16,64,256')
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'control_refine.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_refine needs the MI355X'
    assert args.iters >= 50, 'at least 50 iterations'
    lines = ['# tools/bench_refine.py: one refiner iteration, ControlRefiner replayed (graph) and launch by launch (eager) vs its ATen composition (aten);',
             '# T = 500, shared 256 x 256 maps, 4-point body, weights ' + json.dumps(WEIGHTS) + ', 101 kept poses',
             f'# HIP events per iteration, forms alternating in one process, {args.warmup} warm-up + {args.iters} timed iterations each (median_ms, min_ms, p90_ms);',
             '# loop_wall_ms: wall clock per iteration over loops of ten iterations of one form between two synchronisations, median and minimum of seven; ms',
             f'# device: {torch.cuda.get_device_name(0)}']
    cm = smooth_cost_map().to(DEV)
    path = torch.tensor([[0.0, 0.3], [0.8, 0.5], [1.6, 1.2], [2.4, 1.4]], device=DEV)
    goal = torch.tensor([2.0, 1.0], device=DEV)
    for K in [int(v) for v in args.sizes.split(',')]:
        cfg, dp, pts, masks, z, mu, ctrl0 = build_problem(K, T, 4, DEV, 1)
        zd, md = z.to(DEV).unsqueeze(0), mu.to(DEV).unsqueeze(0)
        total = max(args.warmup, 10)
        refs = {k: ControlRefiner(dp, ctrl0, weights=WEIGHTS, lr=LR, footprint=ops.footprint_points(dp), max_iters=total, graph=(k == 'graph'))
                for k in ('graph', 'eager')}
        at = AtenRefiner(refs['eager'], ctrl0)
        forms = dict(graph=lambda r=refs['graph']: r.step(zd, goal, friction=md, cost_map=cm, path=path),
                     eager=lambda r=refs['eager']: r.step(zd, goal, friction=md, cost_map=cm, path=path),
                     aten=lambda: at.step(zd, goal, md, cm, path))

        def restart():
            for r in refs.values():
                r.reset(ctrl0)
            at.reset()

        for _ in range(args.warmup):
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        assert refs['graph'].graph, 'the capture was refused: the graph row would time the eager route'
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)] for k in forms}
        for i in range(args.iters):
            if i % 10 == 0:
                restart()
            for k, fn in forms.items():
                a, b = ev[k][i]
                a.record()
                fn()
                b.record()
        torch.cuda.synchronize()
        ms = {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
        # ... and the host's share: loops of ten iterations of ONE form between two synchronisations, by the wall clock (the events above see the
        # device alone: while another form's kernels run, the host enqueues ahead)
        loops = {k: [] for k in forms}
        for _ in range(7):
            for k, fn in forms.items():
                restart()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                loops[k].append((time.perf_counter() - t0) * 100.0)      # ms per iteration
                if k == 'graph':
                    best_graph = float(refs['graph'].best_cost.min())
        for k in forms:
            row = dict(K=K, form=k, median_ms=round(float(np.median(ms[k])), 4), min_ms=round(float(ms[k].min()), 4),
                       p90_ms=round(float(np.percentile(ms[k], 90)), 4), loop_wall_ms=round(float(np.median(loops[k])), 4),
                       loop_wall_min_ms=round(float(min(loops[k])), 4))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        med = {k: float(np.median(ms[k])) for k in forms}
        wall = {k: float(np.median(loops[k])) for k in forms}
        lines.append(f'# K = {K}: device time aten / graph = {med["aten"] / med["graph"]:.2f}, aten / eager = {med["aten"] / med["eager"]:.2f}; wall clock aten / graph = '
                     f'{wall["aten"] / wall["graph"]:.2f}, eager / graph = {wall["eager"] / wall["graph"]:.2f} (medians); best cost of a ten-iteration loop: graph {best_graph:.4f} '
                     f'aten {float(at.best_cost.min()):.4f}')
        print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
