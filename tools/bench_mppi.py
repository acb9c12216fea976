"""One MPPI iteration: `MPPIPlanner.step` (HIP kernels around the rollout) against the ATen composition of the same iteration.

    python tools/bench_mppi.py [--sizes 4096,16384] [--iters 60] [--warmup 10] [--out profiles/mppi_iteration.txt]

Both forms draw their own noise (`torch.randn`), run the same path-cost rollout (`DPhysics.rollout_costs`, T = 500, one shared 256 x 256
map pair, the 4-point body) and differ in everything around it:
    hip    mppi_perturb | rollout | path_costs | mppi_update (statistics, partial sums, finish)
    aten   sigma * noise, + nominal, clamp, row 0 | rollout | costs_from_rows + the goal distance | softmax | einsum
Method: HIP events around every iteration, the two forms alternating in one process after a warm-up of both; median and minimum over the
iterations.  Launches per iteration are counted by the profiler in one extra iteration of each form (outside the timed ones); model bytes
are what each form's passes must move, computed from the shapes below (caches may hold some of it)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_problem  # noqa: E402
from monoforce_amd import MPPIPlanner  # noqa: E402
from monoforce_amd.planner import costs_from_rows  # noqa: E402

DEV = 'cuda'
T = 500


class AtenMPPI:
    """The iteration `MPPIPlanner.step` replaces, written with ATen ops (inclination + goal cost, keep_nominal)."""

    def __init__(self, mp):
        self.mp, self.nominal = mp, torch.zeros(mp.T, 2, device=DEV)
        f = lambda v: torch.tensor(v, device=DEV)  # noqa: E731
        self.sigma, self.lo, self.hi = f(mp.sigma), f(mp.lo), f(mp.hi)

    @torch.no_grad()
    def step(self, z, goal, friction=None):
        mp = self.mp
        noise = torch.randn(mp.n_trajs, mp.T, 2, device=DEV)
        controls = torch.clamp(self.nominal + self.sigma * noise, self.lo, self.hi)
        controls[0] = torch.clamp(self.nominal, self.lo, self.hi)
        out = mp.dp.rollout_costs(z, controls, friction=friction, pose_stride=mp.pose_stride, project=True)
        costs = mp.weights[0] * costs_from_rows(out['cost_rows'], 'inclination') + mp.weights[2] * (out['Xs'][:, -1, :2] - goal).norm(dim=-1)
        w = torch.softmax(-costs / mp.lam, dim=0)
        self.nominal = torch.einsum('b,btk->tk', w, controls)
        return costs, w


def model_bytes(B, H, W):
    """Bytes each form's passes move per iteration, from the shapes (float32).  Shared: the noise draw, the rollout's reads of the controls
    and the map pair, its 16-byte rows and decimated poses."""
    bt = B * T
    shared = 8 * bt + 8 * bt + 2 * 4 * H * W + 16 * bt + 11 * (48 * B)      # randn write, rollout: controls, maps, rows, 11 pose rows
    hip = (8 * bt + 8 * bt          # perturb: noise in, controls out
           + 16 * bt                # path costs: one pass over the rows
           + 8 * bt)                # update: one pass over the controls (the [B] vectors and the chunk sums are < 1 % of it)
    aten = (8 * bt * 2              # sigma * noise
            + 8 * bt * 2            # + nominal
            + 8 * bt * 2            # clamp
            + 4 * bt * 2            # -r0
            + 4 * bt * 2 * 2        # clamp, asin
            + 4 * bt * 3            # atan2(r1, r2)
            + 4 * bt * 2 * 2        # two abs
            + 4 * bt * 2            # two means
            + 8 * bt)               # einsum: one pass over the controls
    return shared + hip, shared + aten


def count_launches(fn):
    """Device kernels of one call of `fn` as the profiler sees them; None where no device activity is reported."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n or None
    except Exception as exc:      # the count is a side figure: the timings below do not depend on it
        print(f'# launch count not available: {exc}', file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='4096,16384')
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mppi_iteration.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mppi needs the MI355X'
    assert args.iters >= 50, 'at least 50 iterations'
    lines = ['# tools/bench_mppi.py: one MPPI iteration, MPPIPlanner.step (hip) vs its ATen composition (aten); T = 500, shared 256 x 256 maps, 4-point body',
             f'# HIP events per iteration, forms alternating in one process, {args.warmup} warm-up + {args.iters} timed iterations each; ms',
             f'# device: {torch.cuda.get_device_name(0)}']
    def write(rows):
        text = list(lines)
        for r in rows:
            text.append(json.dumps({k: v for k, v in r.items() if k != 'fn'}))
            if r['form'] == 'aten':
                ratio = r['median_ms'] / text_hip[r['B']]
                text.append(f'# B = {r["B"]}: aten / hip = {ratio:.3f} (median); the hip form is {"not slower" if ratio >= 1 else "SLOWER"}')
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(text) + '\n')

    rows, text_hip = [], {}
    for B in [int(v) for v in args.sizes.split(',')]:
        cfg, dp, pts, masks, z, mu, _ = build_problem(B, T, 4, DEV, 1)
        zd, md = z.to(DEV).unsqueeze(0), mu.to(DEV).unsqueeze(0)
        goal = torch.tensor([2.0, 1.0], device=DEV)
        mp = MPPIPlanner(dp, n_trajs=B)
        at = AtenMPPI(mp)
        forms = dict(hip=lambda mp=mp, zd=zd, md=md, goal=goal: mp.step(zd, goal, friction=md),
                     aten=lambda at=at, zd=zd, md=md, goal=goal: at.step(zd, goal, friction=md))
        for _ in range(args.warmup):
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)] for k in forms}
        for i in range(args.iters):
            for k, fn in forms.items():
                if i % 10 == 0:      # both forms start from the same nominal now and then: their rollouts stay comparable
                    mp.reset()
                    at.nominal.zero_()
                a, b = ev[k][i]
                a.record()
                fn()
                b.record()
        torch.cuda.synchronize()
        ms = {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
        nbytes = dict(zip(('hip', 'aten'), model_bytes(B, zd.shape[-2], zd.shape[-1])))
        for k in forms:
            rows.append(dict(B=B, form=k, median_ms=round(float(np.median(ms[k])), 4), min_ms=round(float(ms[k].min()), 4),
                             p90_ms=round(float(np.percentile(ms[k], 90)), 4), launches=None, model_MB=round(nbytes[k] / 1e6, 1), fn=forms[k]))
            print(json.dumps({k2: v for k2, v in rows[-1].items() if k2 != 'fn'}), flush=True)
        text_hip[B] = rows[-2]['median_ms']
    write(rows)            # the timings are on disk before the profiler is started
    for r in rows:
        r['launches'] = count_launches(r['fn'])
        print(f'# B = {r["B"]} {r["form"]}: {r["launches"]} launches per iteration', flush=True)
    write(rows)


if __name__ == '__main__':
    main()
