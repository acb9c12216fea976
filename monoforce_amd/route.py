"""Global routes on a cost map: `cost_to_go` is the cost-to-go field of a `cost_map` towards a goal, `extract_route` the optimal route from
a start as the `[P,2]` polyline `MPPIPlanner`, `TrajectoryShooter` and `ControlRefiner` take as `path=`, and `RoutePlanner` both in static
buffers: terrain -> `TraversabilityMap` -> `RoutePlanner` -> `MPPIPlanner.step(cost_map=tm.cost, path=rp.path)` stays on the device.

The map lives on the nodes of `z_grid` (first axis x, node (i, j) at `i*grid_res - d_max`, `j*grid_res - d_max`).  A node is passable iff
its cost is finite and `< lethal`; its factor is `s = 1 + alpha*max(cost, 0)`; the eight moves (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (-1,1) (1,-1)
(1,1) need both ends passable, a diagonal one also the two nodes it passes between; an edge weighs `len * ((s[u] + s[v]) * 0.5)` with
`len = grid_res` or `grid_res * sqrt(2)`.  The field is 0 at the goal's nearest node and `min_u fl(d[u] + w(u,v))` elsewhere, `+inf` where
nothing leads; the route follows `argmin_u fl(d[u] + w(u,v))`, ties to the earlier move.  Every operation is rounded separately in the
map's dtype (float32 or float64), so the field is bit-equal to a heap Dijkstra in that dtype whatever the order of relaxation.  The full
definition is the comment of `MfCostToGoDesc` in include/monoforce_hip.h.

GPU tensors: `mf_cost_to_go_*` (one initialisation launch and `n_rounds` launches of a tiled round kernel; converged rounds are empty
launches) and `mf_extract_route_*` (one launch, one wave per map) of monoforce_amd/csrc/cost_to_go.hip, marshalled here and nowhere else.
Nothing is allocated by a launch and the host reads nothing back, so the calls sit in a hipGraph.  `status` bits (int32 per map, on the
device): GOAL_BLOCKED, NOT_CONVERGED (raise `n_rounds`: the field is an upper bound), START_UNREACHABLE, TRUNCATED.
`cost_to_go_aten` / `extract_route_host` are the same definition as Jacobi sweeps of shifted `torch.minimum`s and a walk on the host: they
serve CPU tensors and are the yardstick of tools/bench_route.py.  Not differentiable."""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

__all__ = ['TILE', 'MAX_VERTICES', 'GOAL_BLOCKED', 'NOT_CONVERGED', 'START_UNREACHABLE', 'TRUNCATED', 'MOVES', 'DEFAULT_LETHAL', 'default_rounds',
           'cost_to_go', 'cost_to_go_into', 'cost_to_go_aten', 'extract_route', 'extract_route_into', 'extract_route_host', 'RoutePlanner']

TILE = _lib.MF_ROUTE_TILE                    # edge of the tile of nodes one workgroup owns (MF_ROUTE_TILE)
MAX_VERTICES = _lib.MF_ROUTE_MAX_VERTICES    # most vertices of a path (what pose_costs / trajectory_objective read)
GOAL_BLOCKED, NOT_CONVERGED = _lib.MF_ROUTE_GOAL_BLOCKED, _lib.MF_ROUTE_NOT_CONVERGED
START_UNREACHABLE, TRUNCATED = _lib.MF_ROUTE_START_UNREACHABLE, _lib.MF_ROUTE_TRUNCATED
MOVES = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))
DEFAULT_LETHAL = 1.0                         # a traversability cost of 1 (a fully ramped term) and a keep-out map's 1 are walls
SQRT2 = 1.4142135623730951


def default_rounds(H, W):
    """Default `n_rounds` of an H x W map: 4 * tiles + 2.  A round carries the field across one tile border, so an open map needs about
    tiles_h + tiles_w rounds and a serpentine one round per border its route crosses; one more round has to change nothing for the call to
    report convergence.  On small maps tiles + 2 leaves no room for a winding route (a 70 x 45 map has 6 tiles, a serpentine with a wall
    every 7 rows crosses 12 borders and used 17 rounds: profiles/route_default_rounds.txt), hence the factor; rounds after convergence
    are empty launches."""
    return 4 * (-(-int(H) // TILE)) * (-(-int(W) // TILE)) + 2


def _checked(cost_map, grid_res, alpha):
    if cost_map.dim() not in (2, 3):
        raise ValueError(f'route: cost_map must be [H,W] or [S,H,W], got {tuple(cost_map.shape)}')
    if cost_map.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'route: cost_map must be float32 or float64, got {cost_map.dtype}')
    if cost_map.shape[-1] != 1 and cost_map.stride(-1) != 1:
        raise ValueError(f'route: cost_map must have unit stride along W (it is read in place), got stride {cost_map.stride(-1)}')
    if not float(grid_res) > 0:
        raise ValueError(f'route: grid_res must be positive, got {grid_res}')
    if not 0 <= float(alpha) < float('inf'):
        raise ValueError(f'route: alpha must be finite and not negative, got {alpha}')
    if cost_map.shape[-2] * cost_map.shape[-1] >= 2 ** 31:
        raise ValueError('route: H * W must be below 2^31 (nodes are int32 indices)')


def _maps(cost_map):
    return cost_map.shape[0] if cost_map.dim() == 3 else 1


def _strides(t):
    return (t.stride(0) if t.dim() == 3 else 0), t.stride(-2)


def _positions(p, S, like, name):
    """`p` ([2] or [S,2]; a tensor or numbers) as an [S,2] tensor of `like`'s dtype on its device -- itself when it already is one."""
    p = torch.as_tensor(p, dtype=like.dtype, device=like.device) if not isinstance(p, torch.Tensor) else p.detach()
    if p.numel() != 2 * S:
        raise ValueError(f'route: {name} must hold {S} position(s) of 2 coordinates, got {tuple(p.shape)}')
    return p.to(device=like.device, dtype=like.dtype).reshape(S, 2).contiguous()


# ---- the launches --------------------------------------------------------------------------------------------------------------------------
def work_ints(S, H, W, n_rounds):
    """int32 words of scratch `cost_to_go_into` needs (mf_cost_to_go_work_ints)."""
    return _lib.size_query('mf_cost_to_go_work_ints', _lib.MfCostToGoDesc(S=S, H=H, W=W, n_rounds=n_rounds, grid_res=1.0))


def cost_to_go_into(cost_map, goal, grid_res, d_max, lethal, alpha, n_rounds, field, status, rounds_used, work):
    """The launches: `cost_map` [H,W] or [S,H,W] on the GPU (read in place through its strides), `goal` [S,2] of its dtype; writes `field`
    (contiguous, cost_map's shape and dtype), `status` and `rounds_used` (int32 [S]); `work`: int32 scratch of `work_ints(...)` words.
    No allocation, no host read."""
    _checked(cost_map, grid_res, alpha)
    _lib.require_hip_tensor(cost_map, 'cost_map')
    S = _maps(cost_map)
    H, W = cost_map.shape[-2:]
    if int(n_rounds) < 1:
        raise ValueError(f'route: n_rounds must be at least 1, got {n_rounds}')
    for name, t, shape, dtype in (('goal', goal, (S, 2), cost_map.dtype), ('field', field, tuple(cost_map.shape), cost_map.dtype),
                                  ('status', status, (S,), torch.int32), ('rounds_used', rounds_used, (S,), torch.int32)):
        if t.dtype != dtype or t.device != cost_map.device or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f'route: {name} must be a contiguous {dtype} {shape} tensor on {cost_map.device}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    d = _lib.MfCostToGoDesc(S=S, H=H, W=W, n_rounds=int(n_rounds), grid_res=float(grid_res), d_max=float(d_max), lethal=float(lethal),
                            alpha=float(alpha))
    d.c_stride_s, d.c_stride_h = _strides(cost_map)
    need = S * (2 * (-(-H // TILE)) * (-(-W // TILE)) + int(n_rounds))
    if work.dtype != torch.int32 or work.device != cost_map.device or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f'route: work must be a contiguous int32 tensor of at least {need} words on {cost_map.device}')
    _lib.launch('mf_cost_to_go', cost_map.device, d, cost_map, goal, field, status, rounds_used, work, dtype=cost_map.dtype, timer='cost_to_go_kernel')
    return field


def extract_route_into(field, cost_map, start, goal, grid_res, d_max, lethal, alpha, nodes, n_nodes, route_cost, path, status):
    """The launch: `field` as `cost_to_go` made it from `cost_map`; `start`, `goal` [S,2] of their dtype; writes `nodes` (int32
    [S,max_nodes]), `n_nodes` (int32 [S]), `route_cost` ([S], the maps' dtype) and `path` (float32 [S,P,2]); `status` (int32 [S]) keeps its
    field bits and gets the route bits.  No allocation, no host read."""
    _checked(cost_map, grid_res, alpha)
    _lib.require_hip_tensor(cost_map, 'cost_map')
    S = _maps(cost_map)
    H, W = cost_map.shape[-2:]
    if path.dim() != 3 or not 2 <= path.shape[1] <= MAX_VERTICES:
        raise ValueError(f'route: path must be [S,P,2] with P in 2..{MAX_VERTICES}, got {tuple(path.shape)}')
    if nodes.dim() != 2 or nodes.shape[1] < 2:
        raise ValueError(f'route: nodes must be [S,max_nodes] with max_nodes >= 2, got {tuple(nodes.shape)}')
    P, max_nodes = path.shape[1], nodes.shape[1]
    f = cost_map.dtype
    for name, t, shape, dtype in (('field', field, tuple(cost_map.shape), f), ('start', start, (S, 2), f), ('goal', goal, (S, 2), f),
                                  ('nodes', nodes, (S, max_nodes), torch.int32), ('n_nodes', n_nodes, (S,), torch.int32),
                                  ('route_cost', route_cost, (S,), f), ('path', path, (S, P, 2), torch.float32), ('status', status, (S,), torch.int32)):
        if t.dtype != dtype or t.device != cost_map.device or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f'route: {name} must be a contiguous {dtype} {shape} tensor on {cost_map.device}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    d = _lib.MfRouteDesc(S=S, H=H, W=W, P=P, max_nodes=max_nodes, grid_res=float(grid_res), d_max=float(d_max), lethal=float(lethal),
                         alpha=float(alpha))
    d.c_stride_s, d.c_stride_h = _strides(cost_map)
    _lib.launch('mf_extract_route', cost_map.device, d, field, cost_map, start, goal, nodes, n_nodes, route_cost, path, status, dtype=f,
                timer='extract_route_kernel')
    return path


# ---- the ATen / host form ------------------------------------------------------------------------------------------------------------------
def _shift(x, di, dj, fill):
    """y[..., i, j] = x[..., i + di, j + dj], `fill` off the map."""
    H, W = x.shape[-2:]
    return F.pad(x, (1, 1, 1, 1), value=fill)[..., 1 + di:1 + di + H, 1 + dj:1 + dj + W]


def _scalars(grid_res, d_max, lethal, alpha, dtype, device):
    """The descriptor's C floats in the maps' dtype, as 0-dim tensors (fills: no host copy)."""
    return [torch.full((), float(np.float32(v)), dtype=dtype, device=device) for v in (grid_res, d_max, lethal, alpha)]


def _edge_weights(cost, res, lethal, alpha):
    """passable [S,H,W] (bool) and the weights w[m] [S,H,W] of move m INTO each node (+inf for a move that is not permitted)."""
    zero = torch.zeros((), dtype=cost.dtype, device=cost.device)
    inf = torch.full((), float('inf'), dtype=cost.dtype, device=cost.device)
    ok = torch.isfinite(cost) & (cost < lethal)
    s = alpha * torch.maximum(cost, zero) + 1
    okf = ok.to(torch.uint8)
    diag = res * torch.full((), SQRT2, dtype=cost.dtype, device=cost.device)
    w = []
    for di, dj in MOVES:
        allowed = ok & (_shift(okf, di, dj, 0) != 0)
        if di and dj:
            allowed = allowed & (_shift(okf, di, 0, 0) != 0) & (_shift(okf, 0, dj, 0) != 0)
        length = diag if (di and dj) else res
        w.append(torch.where(allowed, length * ((_shift(s, di, dj, 1.0) + s) * 0.5), inf))
    return ok, w


def cost_to_go_aten(cost_map, goal, grid_res, d_max, lethal=DEFAULT_LETHAL, alpha=4.0, n_sweeps=None, return_status=False):
    """`cost_to_go` as an ATen composition on cost_map's device: Jacobi sweeps `d <- min(d, min_m shift_m(d) + w_m)`.  `n_sweeps=None`:
    sweeps until one changes nothing (a host read per sweep); a number: exactly that many and no host read (capturable).  Each op is
    rounded separately, so the converged field is bit-equal to the kernel's.  Returns `field`, or `(field, status, sweeps)` with
    `return_status` (status: GOAL_BLOCKED | NOT_CONVERGED bits, int32 [S]; sweeps: the sweeps run)."""
    _checked(cost_map, grid_res, alpha)
    with torch.no_grad():
        cost = (cost_map if cost_map.dim() == 3 else cost_map[None]).detach()
        S, H, W = cost.shape
        dev, f = cost.device, cost.dtype
        res, dm, leth, alph = _scalars(grid_res, d_max, lethal, alpha, f, dev)
        g = _positions(goal, S, cost, 'goal')
        ok, w = _edge_weights(cost, res, leth, alph)
        node = torch.round((g + dm) / res)                                                  # [S,2], ties to even; NaN matches nothing
        ii = torch.arange(H, device=dev, dtype=f).view(1, H, 1)
        jj = torch.arange(W, device=dev, dtype=f).view(1, 1, W)
        at_goal = (ii == node[:, 0].view(S, 1, 1)) & (jj == node[:, 1].view(S, 1, 1)) & ok
        inf = torch.full((), float('inf'), dtype=f, device=dev)
        d = torch.where(at_goal, torch.zeros((), dtype=f, device=dev), inf)
        if n_sweeps is not None and int(n_sweeps) < 1:
            raise ValueError(f'route: n_sweeps must be at least 1, got {n_sweeps}')
        moved = torch.zeros(S, dtype=torch.bool, device=dev)
        sweeps = 0
        while n_sweeps is None or sweeps < int(n_sweeps):
            new = d
            for (di, dj), wm in zip(MOVES, w):
                new = torch.minimum(new, _shift(d, di, dj, float('inf')) + wm)
            sweeps += 1
            if n_sweeps is None:
                if torch.equal(new, d):
                    break
            elif sweeps == int(n_sweeps):
                moved = (new != d).flatten(1).any(1)
            d = new
        status = (torch.where(at_goal.flatten(1).any(1), 0, GOAL_BLOCKED) | torch.where(moved, NOT_CONVERGED, 0)).to(torch.int32)
        field = d if cost_map.dim() == 3 else d[0]
    return (field, status, sweeps) if return_status else field


def _np_node(p, d_max, res, H, W):
    fi, fj = np.rint((p[0] + d_max) / res), np.rint((p[1] + d_max) / res)
    if not (0 <= fi <= H - 1 and 0 <= fj <= W - 1):
        return None
    return int(fi), int(fj)


def extract_route_host(field, cost_map, start, goal, grid_res, d_max, lethal=DEFAULT_LETHAL, alpha=4.0, n_vertices=64, max_nodes=None):
    """`extract_route` as a walk on the host (numpy scalars of the maps' dtype); tensors come back on field's device."""
    _checked(cost_map, grid_res, alpha)
    if not 2 <= int(n_vertices) <= MAX_VERTICES:
        raise ValueError(f'route: n_vertices must be in 2..{MAX_VERTICES}, got {n_vertices}')
    S = _maps(cost_map)
    H, W = cost_map.shape[-2:]
    max_nodes = H * W if max_nodes is None else int(max_nodes)
    if max_nodes < 2:
        raise ValueError(f'route: max_nodes must be at least 2, got {max_nodes}')
    P = int(n_vertices)
    dev = field.device
    cost = cost_map.detach().reshape(S, H, W).cpu().numpy()
    d = field.detach().reshape(S, H, W).cpu().numpy()
    T = cost.dtype.type
    res, dm, leth, alph = (T(np.float32(v)) for v in (grid_res, d_max, lethal, alpha))
    res32, dm32 = np.float32(grid_res), np.float32(d_max)
    diag = res * T(SQRT2)
    starts = _positions(start, S, cost_map, 'start').cpu().numpy()
    goals = _positions(goal, S, cost_map, 'goal').cpu().numpy()
    nodes = np.zeros((S, max_nodes), np.int32)
    n_nodes, status = np.zeros(S, np.int32), np.zeros(S, np.int32)
    route_cost, path = np.full(S, np.inf, cost.dtype), np.zeros((S, P, 2), np.float32)
    with np.errstate(all='ignore'):
        for s in range(S):
            c = cost[s]
            ok = np.isfinite(c) & (c < leth)
            fac = T(1) + alph * np.maximum(c, T(0))
            v, gnode = _np_node(starts[s], dm, res, H, W), _np_node(goals[s], dm, res, H, W)
            if v is None or not np.isfinite(d[s][v]):
                status[s] |= START_UNREACHABLE
                path[s] = starts[s].astype(np.float32)
                continue
            route_cost[s] = d[s][v]
            L = 0
            while True:
                nodes[s, L] = v[0] * W + v[1]
                L += 1
                if v == gnode:
                    break
                if L == max_nodes:
                    status[s] |= TRUNCATED
                    break
                best, arg = T(np.inf), None
                for di, dj in MOVES:
                    u = (v[0] + di, v[1] + dj)
                    if not (0 <= u[0] < H and 0 <= u[1] < W) or not ok[u]:
                        continue
                    if di and dj and not (ok[u[0], v[1]] and ok[v[0], u[1]]):
                        continue
                    cand = d[s][u] + (diag if (di and dj) else res) * ((fac[u] + fac[v]) * T(0.5))
                    if cand < best:
                        best, arg = cand, u
                if arg is None:
                    status[s] |= TRUNCATED
                    break
                v = arg
            n_nodes[s] = L
            pick = nodes[s, (np.arange(P, dtype=np.int64) * (L - 1)) // (P - 1)]
            path[s, :, 0] = (pick // W).astype(np.float32) * res32 - dm32
            path[s, :, 1] = (pick % W).astype(np.float32) * res32 - dm32
    out = dict(path=torch.from_numpy(path), nodes=torch.from_numpy(nodes), n_nodes=torch.from_numpy(n_nodes),
               route_cost=torch.from_numpy(route_cost), status=torch.from_numpy(status))
    if cost_map.dim() == 2:
        out['path'] = out['path'][0]
    return {k: t.to(dev) for k, t in out.items()}


# ---- the public forms ----------------------------------------------------------------------------------------------------------------------
def cost_to_go(cost_map, goal, grid_res, d_max, lethal=DEFAULT_LETHAL, alpha=4.0, n_rounds=None, out=None, return_status=False):
    """Cost-to-go field of `cost_map` ([H,W] or [S,H,W]; float32 or float64, unit stride along W, read in place) towards `goal` ([2] or
    [S,2], metres): the cost of the cheapest 8-connected route from every node, `+inf` where there is none (definition: module docstring).
    `lethal`: costs not below it (and non-finite ones) are walls; `alpha`: weight of the cost against distance.  `n_rounds`: launches of the
    round kernel, default `default_rounds(H, W)`.  `out`: a contiguous buffer of cost_map's shape.  Returns `field`, or
    `(field, status, rounds_used)` with `return_status` (int32 [S] each, on the device; NOT_CONVERGED: raise n_rounds).

    GPU tensors: the HIP kernels.  CPU tensors: `cost_to_go_aten`, swept until it stops changing.  Not differentiable."""
    cost_map = cost_map.detach()
    if not cost_map.is_cuda:
        field, status, sweeps = cost_to_go_aten(cost_map, goal, grid_res, d_max, lethal, alpha, None, True)
        if out is not None:
            field = out.copy_(field)
        return (field, status, torch.full_like(status, sweeps)) if return_status else field
    _checked(cost_map, grid_res, alpha)
    S = _maps(cost_map)
    H, W = cost_map.shape[-2:]
    n_rounds = default_rounds(H, W) if n_rounds is None else int(n_rounds)
    dev = cost_map.device
    field = torch.empty(cost_map.shape, dtype=cost_map.dtype, device=dev) if out is None else out
    status, rounds_used = torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    work = torch.empty(S * (2 * (-(-H // TILE)) * (-(-W // TILE)) + max(n_rounds, 1)), dtype=torch.int32, device=dev)
    cost_to_go_into(cost_map, _positions(goal, S, cost_map, 'goal'), grid_res, d_max, lethal, alpha, n_rounds, field, status, rounds_used, work)
    return (field, status, rounds_used) if return_status else field


def extract_route(field, cost_map, start, goal, grid_res, d_max, lethal=DEFAULT_LETHAL, alpha=4.0, n_vertices=64, max_nodes=None, status=None):
    """The optimal route from `start` to `goal` ([2] or [S,2], metres) on `field = cost_to_go(cost_map, goal, ...)` (same scalars).
    Returns `dict(path, nodes, n_nodes, route_cost, status)`: `path` float32 [P,2] ([S,P,2] for [S,H,W] maps) with P = `n_vertices` in
    2..256, resampled evenly (by node count) from the `n_nodes` nodes of the route; `nodes` int32 [S,max_nodes] = i*W + j (default
    max_nodes: H*W); `route_cost` [S] = the field at the start node; `status` int32 [S]: START_UNREACHABLE (every vertex is the start
    itself), TRUNCATED (the route is longer than max_nodes), on top of the field bits of a `status=` handed in.

    GPU tensors: one launch.  CPU tensors: `extract_route_host`."""
    cost_map, field = cost_map.detach(), field.detach()
    if not cost_map.is_cuda:
        out = extract_route_host(field, cost_map, start, goal, grid_res, d_max, lethal, alpha, n_vertices, max_nodes)
        if status is not None:
            out['status'] = out['status'] | (status & (GOAL_BLOCKED | NOT_CONVERGED))
        return out
    _checked(cost_map, grid_res, alpha)
    S = _maps(cost_map)
    H, W = cost_map.shape[-2:]
    dev = cost_map.device
    max_nodes = H * W if max_nodes is None else int(max_nodes)
    if not 2 <= int(n_vertices) <= MAX_VERTICES:
        raise ValueError(f'route: n_vertices must be in 2..{MAX_VERTICES}, got {n_vertices}')
    if max_nodes < 2:
        raise ValueError(f'route: max_nodes must be at least 2, got {max_nodes}')
    nodes = torch.zeros(S, max_nodes, dtype=torch.int32, device=dev)
    n_nodes = torch.empty(S, dtype=torch.int32, device=dev)
    route_cost = torch.empty(S, dtype=cost_map.dtype, device=dev)
    path = torch.empty(S, int(n_vertices), 2, dtype=torch.float32, device=dev)
    status = torch.zeros(S, dtype=torch.int32, device=dev) if status is None else status.clone()
    extract_route_into(field.contiguous(), cost_map, _positions(start, S, cost_map, 'start'), _positions(goal, S, cost_map, 'goal'), grid_res, d_max,
                       lethal, alpha, nodes, n_nodes, route_cost, path, status)
    return dict(path=path[0] if cost_map.dim() == 2 else path, nodes=nodes, n_nodes=n_nodes, route_cost=route_cost, status=status)


class RoutePlanner:
    """The global route of a planner loop, in static buffers: `rp = RoutePlanner(dphysics)`, then per frame `rp(cost_map, start, goal)`
    writes `rp.field`, `rp.path`, `rp.status`, `rp.route_cost`, `rp.n_nodes` (and `rp.nodes`, `rp.rounds_used`) in place and returns
    `rp.path` -- `[P,2]` float32 for an [H,W] map, `[S,P,2]` for [S,H,W] -- e.g. `mppi.step(z, goal, cost_map=tm.cost, path=rp(tm(z), start, goal))`.
    The buffers are allocated by the FIRST call (from cost_map's shape, dtype and device); every later call is launches only, no
    allocation and no host read, so it can be captured into a hipGraph behind `TraversabilityMap` and ahead of `MPPIPlanner.step`.

    `start` and `goal` ([2] or [S,2]) are device tensors the launches read: contiguous ones of cost_map's dtype are read in place (refresh
    them with `copy_`), anything else is copied into `rp.start` / `rp.goal` first.  `dphysics_or_cfg`: a `DPhysics` module or a
    `DPhysConfig` (its `grid_res` and `d_max` are read).  `n_vertices`: P, 2..256.  `lethal`, `alpha`, `n_rounds`, `max_nodes`: as
    `cost_to_go` / `extract_route`.  `rp.status` is on the device and never read here: check NOT_CONVERGED / START_UNREACHABLE when
    convenient.  GPU tensors only.  Not differentiable."""

    def __init__(self, dphysics_or_cfg, n_vertices=64, lethal=DEFAULT_LETHAL, alpha=4.0, n_rounds=None, max_nodes=None):
        cfg = getattr(dphysics_or_cfg, 'dphys_cfg', dphysics_or_cfg)
        self.grid_res, self.d_max = float(cfg.grid_res), float(cfg.d_max)
        if not 2 <= int(n_vertices) <= MAX_VERTICES:
            raise ValueError(f'route: n_vertices must be in 2..{MAX_VERTICES}, got {n_vertices}')
        self.n_vertices, self.lethal, self.alpha = int(n_vertices), float(lethal), float(alpha)
        self.n_rounds, self.max_nodes = n_rounds, max_nodes
        self.field = self.path = self.status = self.route_cost = self.n_nodes = self.nodes = self.rounds_used = None
        self.start = self.goal = None

    def _position(self, p, name):
        S = self._path.shape[0]
        if isinstance(p, torch.Tensor) and p.dtype == self.field.dtype and p.device == self.field.device and p.is_contiguous() and p.numel() == 2 * S:
            return p.detach().view(S, 2)
        buf = getattr(self, name)
        p = torch.as_tensor(p)
        if p.numel() != 2 * S:
            raise ValueError(f'route: {name} must hold {S} position(s) of 2 coordinates, got {tuple(p.shape)}')
        return buf.copy_(p.reshape(S, 2))

    def __call__(self, cost_map, start, goal):
        cost_map = cost_map.detach()
        if self.field is None:
            _lib.require_hip_tensor(cost_map, 'cost_map')
            _checked(cost_map, self.grid_res, self.alpha)
            S, dev, f = _maps(cost_map), cost_map.device, cost_map.dtype
            H, W = cost_map.shape[-2:]
            self.n_rounds = default_rounds(H, W) if self.n_rounds is None else int(self.n_rounds)
            self.max_nodes = H * W if self.max_nodes is None else int(self.max_nodes)
            if self.n_rounds < 1 or self.max_nodes < 2:
                raise ValueError(f'route: n_rounds must be at least 1 and max_nodes at least 2, got {self.n_rounds}, {self.max_nodes}')
            self.field = torch.empty(cost_map.shape, dtype=f, device=dev)
            self._path = torch.empty(S, self.n_vertices, 2, dtype=torch.float32, device=dev)
            self.path = self._path[0] if cost_map.dim() == 2 else self._path
            self.status, self.rounds_used, self.n_nodes = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(3))
            self.route_cost = torch.empty(S, dtype=f, device=dev)
            self.nodes = torch.zeros(S, self.max_nodes, dtype=torch.int32, device=dev)
            self.start, self.goal = torch.zeros(S, 2, dtype=f, device=dev), torch.zeros(S, 2, dtype=f, device=dev)
            self._work = torch.empty(S * (2 * (-(-H // TILE)) * (-(-W // TILE)) + self.n_rounds), dtype=torch.int32, device=dev)
        start, goal = self._position(start, 'start'), self._position(goal, 'goal')
        cost_to_go_into(cost_map, goal, self.grid_res, self.d_max, self.lethal, self.alpha, self.n_rounds, self.field, self.status, self.rounds_used,
                        self._work)
        extract_route_into(self.field, cost_map, start, goal, self.grid_res, self.d_max, self.lethal, self.alpha, self.nodes, self.n_nodes,
                           self.route_cost, self._path, self.status)
        return self.path
