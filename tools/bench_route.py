"""`cost_to_go` / `extract_route` on the MI355X: the HIP kernels (`mf_cost_to_go_*`: one initialisation launch + n_rounds launches of the
tiled round kernel; `mf_extract_route_*`: one launch, one wave) against the ATen form (`cost_to_go_aten`: Jacobi sweeps of shifted
`torch.minimum`s -- what a user would write on the device without the kernels).

    python tools/bench_route.py [--iters 20] [--warmup 3] [--out profiles/route.txt] [--rounds-ab profiles/route_default_rounds.txt]
    python tools/bench_route.py --rounds-ab-only      (only the A/B behind the default n_rounds: tiles + 2 against 4 * tiles + 2 on every map)

Maps, 256 x 256 float32, grid_res 0.1, d_max 12.8:
    open         no walls
    ridge        `traversability_map` of a synthetic terrain with a ridge across it and one pass through the ridge
    serpentine   walls every 32 rows with one-node gaps on alternating sides
Forms:
    hip_default  default n_rounds (`default_rounds`: 4 * tiles + 2 = 258), into static buffers
    hip_enough   n_rounds = rounds_used + 1, the fewest that still report convergence; (hip_default - hip_enough) / (the rounds saved) is the
                 price of a converged-then-empty round
    aten         exactly the sweeps the map needs (found once, outside the timed region, by sweeping until nothing changes)
    route        the walk and the resampling to 64 vertices, from the node farthest from the goal
each launch by launch and replayed as a hipGraph (the ATen form is captured only up to 600 sweeps).  Method: HIP events around every
call, the forms alternating in one process after a warm-up of all; median, minimum and p90 over the calls.  Before timing, the HIP field is
checked to be bit-equal to the ATen one."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_map_losses import alternate, captured, stats  # noqa: E402
from monoforce_amd import costmap as cm, route  # noqa: E402

DEV = 'cuda'
N, RES, DMAX = 256, 0.1, 12.8


def position(i, j):
    return [i * RES - DMAX, j * RES - DMAX]


def maps():
    """name -> (cost map, lethal, goal node)"""
    gen = torch.Generator().manual_seed(0)
    out = {'open': (torch.zeros(N, N), 1.0, (200, 200))}
    i = torch.arange(float(N)).view(N, 1) * RES
    j = torch.arange(float(N)).view(1, N) * RES
    z = 0.3 * torch.sin(0.5 * i) * torch.cos(0.4 * j) + 0.01 * torch.randn(N, N, generator=gen)
    ridge = 1.5 * torch.exp(-((i - 0.45 * j - 7.0) / 0.5) ** 2)                                 # a ridge across the map ...
    ridge = ridge * (1.0 - torch.exp(-((j - 5.0) / 0.8) ** 2))                                  # ... with one pass through it
    out['ridge'] = (cm.traversability_map((z + ridge).to(DEV), RES, 0.3).cpu(), 0.9, (230, 128))
    s = 0.25 * torch.rand(N, N, generator=gen)
    for n, row in enumerate(range(31, N - 1, 32)):
        s[row, :] = 2.0
        s[row, 0 if n % 2 else N - 1] = 0.0
    out['serpentine'] = (s, 1.0, (0, 0))
    return out


def serpentine_small(H=70, W=45, every=7):
    """The small serpentine of tests/test_route_gpu.py: a wall every `every` rows, one-node gaps on alternating sides."""
    c = torch.from_numpy((0.25 * np.random.default_rng(3).random((H, W), dtype=np.float32)))
    for n, i in enumerate(range(every - 1, H - 1, every)):
        c[i, :] = 2.0
        c[i, 0 if n % 2 else W - 1] = 0.0
    return c


def default_rounds_ab(out):
    """The A/B behind the default n_rounds: every map with tiles + 2 rounds and with 4 * tiles + 2, status and rounds_used of each."""
    lines = ['# default n_rounds, A/B: n_rounds = tiles + 2 against 4 * tiles + 2 (route.default_rounds); status 0 = converged, 2 = NOT_CONVERGED',
             f'# device: {torch.cuda.get_device_name(0)}']
    cases = [('serpentine 70x45, a wall every 7 rows', serpentine_small(), 1.0, (0, 0), 3.2)]
    cases += [(f'{k} {N}x{N}', c, lethal, g, DMAX) for k, (c, lethal, g) in maps().items()]
    for name, cost, lethal, gnode, d_max in cases:
        cost = cost.to(DEV)
        H, W = cost.shape
        goal = [gnode[0] * RES - d_max, gnode[1] * RES - d_max]
        want = route.cost_to_go_aten(cost, goal, RES, d_max, lethal)
        tiles = (-(-H // route.TILE)) * (-(-W // route.TILE))
        for n_rounds in (tiles + 2, route.default_rounds(H, W)):
            field, status, used = route.cost_to_go(cost, goal, RES, d_max, lethal, n_rounds=n_rounds, return_status=True)
            lines.append(json.dumps(dict(map=name, tiles=tiles, n_rounds=n_rounds, status=int(status[0]), rounds_used=int(used[0]),
                                         bit_equal_to_aten=bool(torch.equal(field, want)))))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def metadata_lines():
    try:
        import kernel_metadata
        return ['# ' + json.dumps(dict(kernel=name, **m)) for o, name, m in kernel_metadata.kernels() if o == 'cost_to_go.o']
    except Exception as e:      # (no LLVM tools, or the objects are not next to the library)
        return [f'# kernel metadata not available here: {type(e).__name__}']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'route.txt'))
    ap.add_argument('--rounds-ab', default=os.path.join(REPO, 'profiles', 'route_default_rounds.txt'),
                    help='where the A/B behind the default n_rounds goes')
    ap.add_argument('--rounds-ab-only', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_route needs the MI355X'
    default_rounds_ab(args.rounds_ab)
    if args.rounds_ab_only:
        return
    lines = [f'# cost_to_go / extract_route on {N}x{N} float32 cost maps, grid_res {RES}, alpha 4, tile {route.TILE}: the HIP kernels (static buffers) vs',
             '# cost_to_go_aten given exactly the sweeps each map needs',
             f'# HIP events per call, forms alternating in one process, {args.warmup} warm-up + {args.iters} timed calls each; ms',
             f'# device: {torch.cuda.get_device_name(0)}']
    lines += metadata_lines() or ['# kernel metadata not available here: the objects are not next to the library']
    i32 = dict(dtype=torch.int32, device=DEV)
    for name, (cost, lethal, gnode) in maps().items():
        cost = cost.to(DEV)
        goal = torch.tensor(position(*gnode), device=DEV).view(1, 2)
        want, st, sweeps = route.cost_to_go_aten(cost, goal, RES, DMAX, lethal, return_status=True)
        n_default = route.default_rounds(N, N)
        field, status, rounds = torch.empty_like(cost), torch.zeros(1, **i32), torch.zeros(1, **i32)
        work = torch.empty(route.work_ints(1, N, N, n_default), **i32)

        def hip(n_rounds):
            return route.cost_to_go_into(cost, goal, RES, DMAX, lethal, 4.0, n_rounds, field, status, rounds, work)
        hip(n_default)
        exact = bool(torch.equal(field, want))
        used, st_default = int(rounds[0]), int(status[0])
        enough = used + 1
        hip(enough)
        assert exact and st_default == 0 and int(status[0]) == 0 and torch.equal(field, want), (name, exact, st_default, int(status[0]))
        far = int(torch.where(torch.isfinite(want), want, -1.0).argmax())
        start = torch.tensor(position(far // N, far % N), device=DEV).view(1, 2)
        nodes, n_nodes, rcost = torch.zeros(1, N * N, **i32), torch.zeros(1, **i32), torch.zeros(1, device=DEV)
        path, rstatus = torch.zeros(1, 64, 2, device=DEV), torch.zeros(1, **i32)

        def walk():
            return route.extract_route_into(field, cost, start, goal, RES, DMAX, lethal, 4.0, nodes, n_nodes, rcost, path, rstatus)
        walk()
        L = int(n_nodes[0])
        assert int(rstatus[0]) == 0 and L > 1, (name, int(rstatus[0]), L)
        lines.append(f'# {name}: rounds_used {used} of {n_default} (bit-equal to the ATen field: {exact}); the ATen form needs {sweeps} sweeps; '
                     f'reachable {float(torch.isfinite(want).float().mean()):.3f} of the nodes; route of {L} nodes from node {far}')
        print(lines[-1], flush=True)

        def aten():
            return route.cost_to_go_aten(cost, goal, RES, DMAX, lethal, n_sweeps=sweeps)
        forms = dict(hip_default_launch=lambda: hip(n_default), hip_enough_launch=lambda: hip(enough), route_launch=walk, aten_launch=aten)
        graphs = dict(hip_default=captured(lambda: hip(n_default)), hip_enough=captured(lambda: hip(enough)), route=captured(walk))
        if sweeps <= 600:
            graphs['aten'] = captured(aten)
        forms.update({k + '_graph': g.replay for k, g in graphs.items()})
        ms = alternate(forms, args.iters, args.warmup)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k in forms:
            lines.append(json.dumps(dict(map=name, form=k, **stats(ms[k]))))
            print(lines[-1], flush=True)
        mark = len(lines)
        for mode in ('launch', 'graph'):
            empty = (med[f'hip_default_{mode}'] - med[f'hip_enough_{mode}']) / (n_default - enough) * 1e3
            lines.append(f'# {name}, {mode}: a converged-then-empty round costs {empty:.2f} us; a working round '
                         f'{med[f"hip_enough_{mode}"] / enough * 1e3:.2f} us (hip_enough / {enough} rounds); the walk '
                         f'{med[f"route_{mode}"] / L * 1e3:.3f} us per node over {L} nodes')
            if f'aten_{mode}' in med:
                lines.append(f'# {name}, {mode}: aten / hip_default = {med[f"aten_{mode}"] / med[f"hip_default_{mode}"]:.1f}, aten / hip_enough = '
                             f'{med[f"aten_{mode}"] / med[f"hip_enough_{mode}"]:.1f} (medians)')
        print('\n'.join(lines[mark:]), flush=True)
        del graphs, forms
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
