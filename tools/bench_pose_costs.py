"""Planner costs from poses: `torch.ops.monoforce.pose_costs` (one HIP launch) against an ATen composition of the same formulas, and one
`MPPIPlanner.step` with and without the two terms.

    python tools/bench_pose_costs.py [--sizes 4096,16384] [--iters 60] [--warmup 10] [--out profiles/pose_costs.txt]

Inputs: the kept poses of a real path-cost rollout (`DPhysics.rollout_costs`, T = 500, pose_stride 10: Tp = 51, the 4-point body on the shared
256 x 256 bump terrain), a 256 x 256 cost map, an 8-vertex path, and two footprints: the body's 4 points and 223 points in a tradr-sized box.
    hip    pose_costs: footprint, bilinear samples, max over the points, means over the poses, segment distances, the sum -- one launch
    aten   einsum (footprint) | divide, floor, clamp, four indexed reads, the blend | max, mean | segment distances (min over segments) | sum
Method: HIP events around every call, the two forms alternating in one process after a warm-up of both; median and minimum over the calls.
The achieved rate is bilinear samples per second of the hip form (B x Tp x N samples, four gathers each): the bytes are tiny (48 B per pose and a
map that stays in L2), so the kernel is expected to be bound by gathers and instruction issue, not by memory bandwidth."""
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
from monoforce_amd import ops as mf_ops  # noqa: E402
from monoforce_amd import synthetic as syn  # noqa: E402

DEV = 'cuda'
T, POSE_STRIDE = 500, 10
LETHAL, OFF_MAP, WEIGHTS = 2.0, 1.5, (0.7, 1.3)


@torch.no_grad()
def aten_pose_costs(Xs, Rs, points, cost_map, path, base, grid_res, d_max, lethal, off_map, weights):
    """The formulas of include/monoforce_hip.h (MfPoseCostDesc) as ATen ops on the device."""
    H, W = cost_map.shape
    Tp = Xs.shape[1]
    q = Xs[..., None, :2] + torch.einsum('btij,nj->btni', Rs[..., :2, :], points)
    u, v = (q[..., 0] + d_max) / grid_res, (q[..., 1] + d_max) / grid_res
    on = (u >= 0) & (u <= H - 1) & (v >= 0) & (v <= W - 1)
    u, v = torch.where(on, u, 0.0), torch.where(on, v, 0.0)
    ix, iy = torch.clamp(torch.floor(u).long(), max=H - 2), torch.clamp(torch.floor(v).long(), max=W - 2)
    fx, fy = u - ix, v - iy
    s = (1 - fx) * (1 - fy) * cost_map[ix, iy] + fx * (1 - fy) * cost_map[ix + 1, iy] + (1 - fx) * fy * cost_map[ix, iy + 1] + fx * fy * cost_map[ix + 1, iy + 1]
    s = torch.where(on, s, off_map)
    is_lethal = (~(s < lethal)).flatten(1).any(dim=1)
    mp = torch.where(is_lethal, float('inf'), s.max(dim=-1).values.sum(dim=-1) / Tp)
    a, b = path[:-1], path[1:]
    ab, ap = b - a, Xs[..., None, :2] - a
    len2 = (ab * ab).sum(-1)
    t = torch.where(len2 > 0, torch.clamp((ap * ab).sum(-1) / torch.where(len2 > 0, len2, 1.0), 0.0, 1.0), 0.0)
    d = ap - t[..., None] * ab
    xt = torch.sqrt((d * d).sum(-1).min(dim=-1).values).sum(dim=-1) / Tp
    costs = base + torch.where(is_lethal, float('inf'), weights[0] * mp) + weights[1] * xt
    return costs, torch.stack([mp, xt], dim=-1)


def alternate(forms, iters, warmup):
    """forms: dict name -> callable.  HIP events around every call, the forms alternating; returns dict name -> ms array."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in forms}
    for i in range(iters):
        for k, fn in forms.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4), p90_ms=round(float(np.percentile(ms, 90)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='4096,16384')
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pose_costs.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pose_costs needs the MI355X'
    lines = ['# tools/bench_pose_costs.py: pose_costs (hip, one launch) vs its ATen composition (aten); kept poses of a T = 500 rollout at pose_stride 10',
             '# (Tp = 51), 256 x 256 cost map, 8-vertex path; and one MPPIPlanner.step without / with the map and path terms (4-point footprint)',
             f'# HIP events per call, forms alternating in one process, {args.warmup} warm-up + {args.iters} timed calls each; ms',
             f'# device: {torch.cuda.get_device_name(0)}']
    g = torch.Generator().manual_seed(0)
    path = torch.tensor([[0.0, 0.0], [0.5, 0.1], [1.0, 0.4], [1.4, 0.9], [1.6, 1.5], [1.6, 2.2], [1.3, 2.8], [0.8, 3.2]], device=DEV)
    bodies = {4: None, 223: torch.as_tensor(syn.robot_points_box(223, seed=1, n_tracks=2)[0], dtype=torch.float32).to(DEV)}
    verdicts = []
    for B in [int(v) for v in args.sizes.split(',')]:
        cfg, dp, pts, masks, z, mu, _ = build_problem(B, T, 4, DEV, 1)
        zd, md = z.to(DEV).unsqueeze(0), mu.to(DEV).unsqueeze(0)
        cm = torch.rand(zd.shape[-2], zd.shape[-1], generator=g).to(DEV)
        cm[150:170, 120:140] = 5.0
        goal = torch.tensor([2.0, 1.0], device=DEV)
        plain = MPPIPlanner(dp, n_trajs=B, pose_stride=POSE_STRIDE)
        out = plain.step(zd, goal, friction=md)
        Xs, Rs, base = out['Xs'], out['Rs'], out['costs'].clone()
        Tp = Xs.shape[1]
        bodies[4] = mf_ops.footprint_points(dp)
        scal = (float(cfg.grid_res), float(cfg.d_max), LETHAL, OFF_MAP)
        for N, points in bodies.items():
            forms = dict(hip=lambda p=points: torch.ops.monoforce.pose_costs(Xs, Rs, p, cm, path, base, *scal, list(WEIGHTS)),
                         aten=lambda p=points: aten_pose_costs(Xs, Rs, p, cm, path, base, *scal, WEIGHTS))
            (ch, th), (ca, ta) = forms['hip'](), forms['aten']()
            fin = torch.isfinite(ca)
            same_set = bool(torch.equal(torch.isfinite(ch), fin))
            dev = float((ch[fin] - ca[fin]).abs().max() / ca[fin].abs().max()) if bool(fin.any()) and same_set else float('nan')
            ms = alternate(forms, args.iters, args.warmup)
            samples = B * Tp * N
            for k in forms:
                row = dict(what='pose_costs', B=B, Tp=Tp, N=N, form=k, **stats(ms[k]))
                if k == 'hip':
                    row.update(gsamples_per_s=round(samples / (np.median(ms[k]) * 1e-3) / 1e9, 2), lethal=int((~fin).sum()), same_lethal_set=same_set,
                               max_rel_dev_from_aten=dev)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
            ratio = float(np.median(ms['aten']) / np.median(ms['hip']))
            verdicts.append(ratio >= 1)
            lines.append(f'# B = {B}, N = {N}: aten / hip = {ratio:.2f} (median); the hip kernel is {"below" if ratio >= 1 else "NOT BELOW"} the ATen composition')
            print(lines[-1], flush=True)
        scored = MPPIPlanner(dp, n_trajs=B, pose_stride=POSE_STRIDE, weights=dict(map=WEIGHTS[0], path=WEIGHTS[1]), lethal=LETHAL, off_map=OFF_MAP)
        forms = dict(step=lambda: plain.step(zd, goal, friction=md), step_map_path=lambda: scored.step(zd, goal, friction=md, cost_map=cm, path=path))
        ms = alternate(forms, args.iters, args.warmup)
        for k in forms:
            lines.append(json.dumps(dict(what='MPPIPlanner.step', B=B, Tp=Tp, N=4, form=k, **stats(ms[k]))))
            print(lines[-1], flush=True)
        lines.append(f'# B = {B}: the two terms add {float(np.median(ms["step_map_path"]) - np.median(ms["step"])):.4f} ms to a step (median)')
    lines.append('# the hip kernel is below the ATen composition at every size measured' if all(verdicts) else
                 '# the hip kernel is NOT below the ATen composition at every size measured: see the lines marked NOT BELOW')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
