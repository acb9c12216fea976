"""Referee of the route feature (monoforce_amd/route.py, mf_cost_to_go_* / mf_extract_route_*): a heap Dijkstra and the route walk in
numpy, restating the definition of include/monoforce_hip.h at MfCostToGoDesc with every operation done on numpy scalars of the case's dtype
(so each is rounded once, in that dtype).  Also the maps the CPU and GPU tests share, cached: a referee result is computed once per case.

Exactness: rounded addition is monotone and the weights are positive, so the field is the unique fixed point of the relaxation and any
implementation that relaxes to convergence reaches these bits; the tests compare with `torch.equal` / `np.array_equal`."""
import functools
import heapq

import numpy as np
import torch

MOVES = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))
GOAL_BLOCKED, NOT_CONVERGED, START_UNREACHABLE, TRUNCATED = 1, 2, 4, 8
GRID_RES, D_MAX = 0.1, 3.2
SIZES = ((5, 7), (33, 40), (70, 45))
DTYPES = {'f32': np.float32, 'f64': np.float64}


def scalars(dtype, grid_res, d_max, lethal, alpha):
    """The descriptor carries C floats; the kernel converts them to its scalar type once."""
    T = np.dtype(dtype).type
    return T, T(np.float32(grid_res)), T(np.float32(d_max)), T(np.float32(lethal)), T(np.float32(alpha))


def node_of(p, d_max, res, H, W):
    """Nearest node of a position (ties to even), None off the map or for NaN."""
    with np.errstate(all='ignore'):
        fi, fj = np.rint((p[0] + d_max) / res), np.rint((p[1] + d_max) / res)
    if not (fi >= 0 and fi <= H - 1 and fj >= 0 and fj <= W - 1):
        return None
    return int(fi), int(fj)


def position_of(node, grid_res=GRID_RES, d_max=D_MAX):
    """World position of a node as python floats (exactly representable inputs of the tests: float32 arithmetic)."""
    return (float(np.float32(node[0]) * np.float32(grid_res) - np.float32(d_max)), float(np.float32(node[1]) * np.float32(grid_res) - np.float32(d_max)))


def graph(cost, grid_res, lethal, alpha):
    T, res, _, leth, alph = scalars(cost.dtype, grid_res, 0.0, lethal, alpha)
    with np.errstate(all='ignore'):
        ok = np.isfinite(cost) & (cost < leth)
        fac = (T(1) + alph * np.maximum(cost, T(0))).astype(cost.dtype)
    return T, res, res * T(1.4142135623730951), ok, fac


def permitted(ok, v, m):
    H, W = ok.shape
    di, dj = MOVES[m]
    u = (v[0] + di, v[1] + dj)
    if not (0 <= u[0] < H and 0 <= u[1] < W) or not ok[u] or not ok[v]:
        return None
    if di and dj and not (ok[u[0], v[1]] and ok[v[0], u[1]]):
        return None
    return u


def weight(T, res, diag, fac, u, v, m):
    with np.errstate(all='ignore'):
        return (diag if m >= 4 else res) * ((fac[u] + fac[v]) * T(0.5))


def cost_to_go(cost, goal, grid_res=GRID_RES, d_max=D_MAX, lethal=1.0, alpha=4.0):
    """cost [H,W] numpy (float32 or float64), goal (x, y).  Returns (field, status)."""
    H, W = cost.shape
    T, res, diag, ok, fac = graph(cost, grid_res, lethal, alpha)
    dm = T(np.float32(d_max))
    d = np.full((H, W), np.inf, cost.dtype)
    g = node_of((T(goal[0]), T(goal[1])), dm, res, H, W)
    if g is None or not ok[g]:
        return d, GOAL_BLOCKED
    d[g] = T(0)
    heap = [(T(0), g)]
    done = np.zeros((H, W), bool)
    with np.errstate(all='ignore'):
        while heap:
            dv, v = heapq.heappop(heap)
            if done[v]:
                continue
            done[v] = True
            for m in range(8):
                u = permitted(ok, v, m)
                if u is None or done[u]:
                    continue
                cand = dv + weight(T, res, diag, fac, u, v, m)
                if cand < d[u]:
                    d[u] = cand
                    heapq.heappush(heap, (cand, u))
    return d, 0


def extract_route(field, cost, start, goal, grid_res=GRID_RES, d_max=D_MAX, lethal=1.0, alpha=4.0, n_vertices=64, max_nodes=None):
    """The walk.  Returns dict(path [P,2] float32, nodes (the n_nodes walked), n_nodes, route_cost, status (route bits only))."""
    H, W = cost.shape
    T, res, diag, ok, fac = graph(cost, grid_res, lethal, alpha)
    dm = T(np.float32(d_max))
    P = int(n_vertices)
    max_nodes = H * W if max_nodes is None else max_nodes
    start = (T(start[0]), T(start[1]))
    v = node_of(start, dm, res, H, W)
    g = node_of((T(goal[0]), T(goal[1])), dm, res, H, W)
    if v is None or not np.isfinite(field[v]):
        path = np.tile(np.array([start[0], start[1]]).astype(np.float32), (P, 1))
        return dict(path=path, nodes=np.zeros(0, np.int32), n_nodes=0, route_cost=T(np.inf), status=START_UNREACHABLE)
    nodes, status = [], 0
    with np.errstate(all='ignore'):
        while True:
            nodes.append(v[0] * W + v[1])
            if v == g:
                break
            if len(nodes) == max_nodes:
                status |= TRUNCATED
                break
            best, arg = T(np.inf), None
            for m in range(8):
                u = permitted(ok, v, m) if ok[v] else None
                if u is None:
                    continue
                cand = field[u] + weight(T, res, diag, fac, u, v, m)
                if cand < best:      # (strict: ties stay with the earlier move)
                    best, arg = cand, u
            if arg is None:
                status |= TRUNCATED
                break
            v = arg
    nodes = np.array(nodes, np.int32)
    L = len(nodes)
    pick = nodes[[(p * (L - 1)) // (P - 1) for p in range(P)]]
    r32, d32 = np.float32(grid_res), np.float32(d_max)
    path = np.stack([(pick // W).astype(np.float32) * r32 - d32, (pick % W).astype(np.float32) * r32 - d32], 1).astype(np.float32)
    return dict(path=path, nodes=nodes, n_nodes=L, route_cost=field[node_of(start, dm, res, H, W)], status=status)


def check_route_is_legal(nodes, cost, lethal=1.0):
    """Property check without the field: every node passable, consecutive nodes one permitted move apart."""
    H, W = cost.shape
    with np.errstate(all='ignore'):
        ok = np.isfinite(cost) & (cost < np.dtype(cost.dtype).type(np.float32(lethal)))
    vs = [(int(n) // W, int(n) % W) for n in nodes]
    assert all(ok[v] for v in vs)
    for a, b in zip(vs[:-1], vs[1:]):
        step = (b[0] - a[0], b[1] - a[1])
        assert step in MOVES, (a, b)
        assert permitted(ok, a, MOVES.index(step)) == b, (a, b)


# ---- maps -----------------------------------------------------------------------------------------------------------------------------------
def random_map(H, W, seed, dtype=np.float64, walls=0.12):
    """Costs uniform in [0,1) (float32 values, so both dtypes see the same map) with `walls` of the nodes lethal (cost 2) or NaN."""
    g = np.random.default_rng(seed)
    c = g.random((H, W), dtype=np.float32)
    r = g.random((H, W))
    c[r < walls] = 2.0
    c[r < walls / 4] = np.nan
    return c.astype(dtype)


def serpentine(H=70, W=45, every=7, dtype=np.float64, seed=3):
    """Walls across the map every `every` rows with a one-node gap alternating between the two sides: the only route from the first row
    to the last runs the full width between every pair of walls, so it crosses every tile border in W once per lane."""
    c = (0.25 * np.random.default_rng(seed).random((H, W), dtype=np.float32)).astype(dtype)
    for n, i in enumerate(range(every - 1, H - 1, every)):
        c[i, :] = 2.0
        c[i, 0 if n % 2 else W - 1] = 0.0
    return c


def border_goal_maps(T, H=70, W=45, dtype=np.float64, seed=5):
    """Maps whose goal node lies on a tile border (tile edge T) and is seen from the tile across the border only through the goal itself:
    name -> (cost, goal node).  `row` / `col`: a wall along row / column T - 1, the last of its tile, whose only gap is the goal;
    `dead_end`: the goal at (T - 1, 10) walled in on three sides, its only exit (T, 10) in the next tile; `corner`: the goal at
    (T - 1, T - 1) walled in to the north and west, its three exits in three other tiles."""
    base = (0.25 * np.random.default_rng(seed).random((H, W), dtype=np.float32)).astype(dtype)
    out = {}
    c = base.copy()
    c[T - 1, :] = 2.0
    c[T - 1, 5] = 0.0
    out['row'] = (c, (T - 1, 5))
    c = base.copy()
    c[:, T - 1] = 2.0
    c[5, T - 1] = 0.0
    out['col'] = (c, (5, T - 1))
    c = base.copy()
    for n in ((T - 1, 9), (T - 1, 11), (T - 2, 9), (T - 2, 10), (T - 2, 11)):
        c[n] = 2.0
    out['dead_end'] = (c, (T - 1, 10))
    c = base.copy()
    for n in ((T - 2, T - 2), (T - 2, T - 1), (T - 2, T), (T - 1, T - 2), (T, T - 2)):
        c[n] = np.nan
    out['corner'] = (c, (T - 1, T - 1))
    return out


def open_map(H, W, dtype=np.float64):
    return np.zeros((H, W), dtype)


def reachable_share(field, cost, lethal=1.0):
    with np.errstate(all='ignore'):
        ok = np.isfinite(cost) & (cost < lethal)
    return float(np.isfinite(field[ok]).mean()) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def case(kind, H, W, dtype_name, goal_node, seed=0, alpha=4.0, lethal=1.0):
    """A cached case: dict(cost, goal, field, status) with numpy arrays that callers must not modify."""
    dtype = DTYPES[dtype_name]
    cost = {'random': lambda: random_map(H, W, seed, dtype), 'serpentine': lambda: serpentine(H, W, 7, dtype), 'open': lambda: open_map(H, W, dtype)}[kind]()
    if kind == 'random' and 0 <= goal_node[0] < H and 0 <= goal_node[1] < W:
        cost[goal_node] = 0.5      # the goal node itself is passable (the blocked-goal case makes its own)
    goal = position_of(goal_node)
    field, status = cost_to_go(cost, goal, lethal=lethal, alpha=alpha)
    cost.setflags(write=False)
    field.setflags(write=False)
    return dict(cost=cost, goal=goal, goal_node=goal_node, field=field, status=status)


def to_torch(a, device='cpu'):
    return torch.from_numpy(np.array(a)).to(device)
