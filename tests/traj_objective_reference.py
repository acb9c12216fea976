"""Referee of the trajectory objective (monoforce_amd/csrc/traj_objective.hip, monoforce_amd/refine.py): the formulas of include/monoforce_hip.h
(MfTrajObjDesc) restated in plain torch in the dtype of `Xs` (float64 in the tests), its gradient by autograd, the cases of the GPU tests
and the rule that takes rows next to a kink out of a gradient comparison.  Test code: the product never imports it.

The scalars of the launch descriptor are C floats: every function rounds them to float32 first (as tests/pose_costs_reference.py does), so
a float64 evaluation differs from the kernel by its arithmetic alone.

Exclusions.  The objective has kinks (the footprint maximum, cell edges of the bilinear blend, the map border, the nearest segment, |.| at 0);
next to one, float32 may legitimately take the other branch and its gradient is then the other one-sided derivative.  `excluded_rows`
decides -- in float64, from the inputs alone, before any result is looked at -- which pose rows (b, p) are too close: any of
    the gap between the two largest footprint samples          (cost units; bodies of at least two points)
    the arg-max sample's distance to a cell edge or the border  (cells)
    the gap between the two nearest segments                    (metres; see below)
    the path distance, or (last kept row) the goal distance     (metres)
    |roll| or |pitch| where it is not exactly 0                 (radians)
below 1e-4.  "The two nearest segments": segments that meet in a vertex tie EXACTLY for every position in that vertex's outer cone (both
clamp onto the vertex), as does a zero-length segment with its neighbours -- a large share of all rows, and a harmless one: the closest
point, and with it the gradient, is the same whichever segment is named.  The gap is therefore taken to the nearest segment whose closest
point lies more than 1e-6 m from the nearest segment's closest point.
"""
import torch

from tests import pose_costs_cases as pc
from tests import pose_costs_reference as ref
from tests.mppi_reference import _f32

F64 = torch.float64
INF = float('inf')
MARGIN = 1e-4
SAME_POINT = 1e-6
WEIGHTS = (0.7, 1.3, 0.9, 1.1)         # map, path, goal, inclination
# (B, T, pose_stride, N, P): B in {1, 3, 65} (a partial second group of 64 rollouts); (T, stride) in {(1, 1), (50, 7), (50, 50)}: Tp = 1, 8, 2 -- at
# (50, 7) the last step, 49, is itself a multiple of the stride; (51, 7): Tp = 9, the last kept step the clamp T - 1 = 50 behind 49; (50, 3) and
# (50, 2): Tp = 18 and 26, the clamp again and a second, ragged trip of the kernel's loop over 16 pose rows; N either side
# of a 16-lane row (16 / 17) and of its fourth trip (65), and the small bodies; P = 0, 1, 2, 18 (no path, a point, one segment, 17 segments: a
# second trip of the 16-lane deal).  tests/test_refine_cpu.py ties the table to the kernel's source.
CASES = [(1, 1, 1, 1, 0), (3, 1, 1, 4, 1), (3, 50, 7, 4, 2), (65, 50, 7, 17, 18), (65, 50, 50, 16, 2), (3, 50, 2, 65, 18), (65, 50, 3, 4, 0),
         (1, 50, 50, 9, 1), (3, 50, 7, 8, 18), (3, 51, 7, 4, 1)]
# seeds of the pose generator, where the default draw leaves more than 5 % of a case's rows next to a kink (tests/test_refine_cpu.py checks the share)
SEEDS = {(3, 50, 2, 65, 18): 1}


def kept_steps(T, pose_stride):
    Tp = 1 + (T - 1 + pose_stride - 1) // pose_stride
    return torch.tensor([min(p * pose_stride, T - 1) for p in range(Tp)])


def smooth_map(map_shape=pc.RECT, seed=0):
    """A few Gaussians plus a ramp, float32 [H,W]: exact ties between footprint samples are measure-zero."""
    g = torch.Generator().manual_seed(900 + seed)
    H, W = map_shape
    i, j = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing='ij')
    m = 0.01 * i + 0.007 * j
    for _ in range(5):
        ci, cj = torch.rand(1, generator=g, dtype=F64) * H, torch.rand(1, generator=g, dtype=F64) * W
        s = 4.0 + 6.0 * torch.rand(1, generator=g, dtype=F64)
        m = m + (0.5 + torch.rand(1, generator=g, dtype=F64)) * torch.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (2 * s * s))
    return m.float()


def make_case(B, T, pose_stride, N, P, seed=None):
    """Inputs of one case, float32 on the CPU: poses and footprint of `pose_costs_cases.constructed` on the rectangular map (footprint points
    kept 1e-3 cells away from the border: one axis runs partly off the map), a smooth cost map, a walk path, a goal."""
    c = pc.constructed(B, T, N, seed=SEEDS.get((B, T, pose_stride, N, P)) if seed is None else seed, map_shape=pc.RECT)
    g = torch.Generator().manual_seed(31 * B + 7 * T + N + 1000 * P)
    return dict(Xs=c['Xs'], Rs=c['Rs'], points=c['points'], cost_map=smooth_map(seed=B + N), path=pc.walk_path(P, map_shape=pc.RECT) if P else None,
                goal=(torch.rand(2, generator=g) * 4 - 2), pose_stride=pose_stride, shape=(B, T, pose_stride, N, P))


def _safe_sqrt(n2):
    pos = n2 > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, n2, torch.ones_like(n2))), n2)


def segment_offsets(xy, path):
    """xy [...,2], path [P,2] -> (offset to the closest point of every segment [...,S,2], S = max(P - 1, 1))."""
    a, b = (path[:-1], path[1:]) if path.shape[0] > 1 else (path, path)
    ab, ap = b - a, xy[..., None, :] - a
    len2 = (ab * ab).sum(-1)
    t = torch.where(len2 > 0, torch.clamp((ap * ab).sum(-1) / torch.where(len2 > 0, len2, torch.ones_like(len2)), 0.0, 1.0), torch.zeros_like(len2))
    return ap - t[..., None] * ab


def evaluate(Xs, Rs, goal, points, cost_map, path, weights, pose_stride, grid_res=pc.GRID_RES, d_max=pc.D_MAX, lethal=INF, off_map=INF):
    """dict(costs [B], terms [B,4], carrier [B], s [B,Tp,N] or None, uv, d_seg [B,Tp,S] or None, off_seg, roll, pitch [B,Tp], goal_dist [B]) in the
    dtype of Xs.  `carrier` is the finite expression whose derivative the gradient is defined as (the map term with non-finite maxima taken
    out, no lethal rule); `costs` the documented value."""
    dt = Xs.dtype
    B, T = Xs.shape[:2]
    steps = kept_steps(T, pose_stride)
    Tp = steps.numel()
    X, R = Xs[:, steps], Rs[:, steps]
    w = _f32(list(weights), dt)
    zero = torch.zeros(B, dtype=dt)
    out = dict(s=None, uv=None, d_seg=None, off_seg=None)
    mp = xt = mp_fin = zero
    is_lethal = torch.zeros(B, dtype=torch.bool)
    if cost_map is not None:
        q = ref.footprint(X, R, points)
        s, _ = ref.sample(cost_map, q, grid_res, d_max, off_map)
        out['s'], out['uv'] = s, (q + _f32(d_max, dt)) / _f32(grid_res, dt)
        is_lethal = (~(s < _f32(lethal, dt))).flatten(1).any(dim=1)
        f = s.max(dim=-1).values
        mp = torch.where(is_lethal, torch.full_like(zero, INF), f.sum(-1) / Tp)
        mp_fin = torch.where(torch.isfinite(f), f, torch.zeros_like(f)).sum(-1) / Tp
    if path is not None:
        off = segment_offsets(X[..., :2], path.to(dt))
        d2 = (off * off).sum(-1)
        out['d_seg'], out['off_seg'] = _safe_sqrt(d2), off
        xt = _safe_sqrt(d2.min(dim=-1).values).sum(-1) / Tp
    e = Xs[:, T - 1, :2] - goal.to(dt)
    gl = _safe_sqrt((e * e).sum(-1))
    r = R[..., 2, :]
    h = r / torch.sqrt((r * r).sum(-1, keepdim=True))
    roll, pitch = torch.atan2(h[..., 1], h[..., 2]), torch.asin(torch.clamp(-h[..., 0], -1.0, 1.0))
    incl = (roll.abs() + pitch.abs()).sum(-1) / Tp
    rest = w[2] * gl + w[3] * incl
    if path is not None:
        rest = w[1] * xt + rest
    costs, carrier = rest, rest
    if cost_map is not None:
        costs = torch.where(is_lethal, torch.full_like(zero, INF), w[0] * mp) + rest
        carrier = w[0] * mp_fin + rest
    out.update(costs=costs, terms=torch.stack([mp, xt, gl, incl], -1), carrier=carrier, roll=roll, pitch=pitch, goal_dist=gl, steps=steps)
    return out


def case_weights(case, weights=WEIGHTS):
    """`weights` with the weight of an absent input (no cost map, no path) set to 0, as the entry point demands."""
    w = list(weights)
    if case['cost_map'] is None:
        w[0] = 0.0
    if case['path'] is None:
        w[1] = 0.0
    return tuple(w)


def gradients(case, weights=WEIGHTS, gcosts=None, dtype=F64, fn=None, **scalars):
    """(costs, terms, gXs [B,T,3], gRs [B,T,3,3]) of one case in `dtype`: the referee's autograd, or with `fn` (trajectory_objective_aten's
    signature) that function's."""
    Xs, Rs = case['Xs'].detach().to(dtype).clone().requires_grad_(True), case['Rs'].detach().to(dtype).clone().requires_grad_(True)      # (leaves of its own: the case stays as it is)
    cm = None if case['cost_map'] is None else case['cost_map'].to(dtype)
    pa = None if case['path'] is None else case['path'].to(dtype)
    weights = case_weights(case, weights)
    if fn is None:
        o = evaluate(Xs, Rs, case['goal'].to(dtype), case['points'].to(dtype), cm, pa, weights, case['pose_stride'], **scalars)
        costs, terms, carrier = o['costs'], o['terms'], o['carrier']
    else:
        sc = dict(grid_res=pc.GRID_RES, d_max=pc.D_MAX, lethal=INF, off_map=INF)
        sc.update(scalars)
        sc = {k: float(torch.tensor(v, dtype=torch.float32)) for k, v in sc.items()}
        costs, terms = fn(Xs, Rs, case['goal'].to(dtype), points=case['points'].to(dtype), cost_map=cm, path=pa,
                          weights=[float(v) for v in _f32(list(weights), F64)], pose_stride=case['pose_stride'], **sc)
        carrier = costs
    gc = torch.ones_like(carrier) if gcosts is None else gcosts.to(dtype)
    gX, gR = torch.autograd.grad((gc * carrier).sum(), [Xs, Rs], allow_unused=True)
    gX = torch.zeros_like(Xs) if gX is None else gX
    gR = torch.zeros_like(Rs) if gR is None else gR
    return costs.detach(), terms.detach(), gX, gR


def excluded_rows(case, off_map=INF):
    """bool [B,Tp]: the kept pose rows too close to a kink (module docstring), decided in float64 from the inputs alone."""
    with torch.no_grad():
        d = lambda t: None if t is None else t.double()  # noqa: E731
        o = evaluate(d(case['Xs']), d(case['Rs']), d(case['goal']), d(case['points']), d(case['cost_map']), d(case['path']), WEIGHTS,
                     case['pose_stride'], off_map=off_map)
        B, Tp = o['roll'].shape
        bad = torch.zeros(B, Tp, dtype=torch.bool)
        if o['s'] is not None:
            s, uv = o['s'], o['uv']
            H, W = case['cost_map'].shape
            last = torch.tensor([H - 1, W - 1], dtype=F64)
            k = s.argmax(dim=-1, keepdim=True)
            uvk = torch.gather(uv, 2, k[..., None].expand(-1, -1, 1, 2)).squeeze(2)
            on = ((uvk >= 0) & (uvk <= last)).all(-1)
            if s.shape[-1] > 1:
                # an on-map maximum: the gap to the runner-up; an off-map one (zero gradient whichever off-map point is named: those tie
                # exactly, harmlessly): the gap to the best ON-map sample
                on_all = ((uv >= 0) & (uv <= last)).all(-1)
                top = torch.topk(s, 2, dim=-1).values
                best_on = torch.where(on_all, s, torch.full_like(s, -INF)).max(dim=-1).values
                gap = torch.where(on, top[..., 0] - top[..., 1], s.max(dim=-1).values - best_on)
                bad |= gap < MARGIN                           # (inf - finite = inf: an infinite off_map is never close)
            frac = uvk - torch.floor(uvk)
            edge = torch.minimum(frac, 1 - frac).min(-1).values
            border = torch.minimum(uvk.abs(), (uvk - last).abs()).min(-1).values
            bad |= on & ((edge < MARGIN) | (border < MARGIN))
            bad |= (torch.minimum(uv.abs(), (uv - last).abs()) < MARGIN).flatten(2).any(-1)      # any point on the border: it may change sides
        if o['d_seg'] is not None:
            ds, off = o['d_seg'], o['off_seg']
            dmin, kmin = ds.min(dim=-1)
            bad |= dmin < MARGIN
            nearest = torch.gather(off, 2, kmin[..., None, None].expand(-1, -1, 1, 2))
            other = ((off - nearest) ** 2).sum(-1).sqrt() > SAME_POINT          # the same position minus another closest point
            rival = torch.where(other, ds, torch.full_like(ds, INF)).min(dim=-1).values
            bad |= rival - dmin < MARGIN
        for a in (o['roll'].abs(), o['pitch'].abs()):
            bad |= (a != 0) & (a < MARGIN)
        bad[:, -1] |= o['goal_dist'] < MARGIN
        return bad


def row_mask(case, bad):
    """bool [B,T]: the steps whose gradient rows are compared -- every step that is not kept (those rows must be zero) and every kept row not excluded."""
    B, T = case['Xs'].shape[:2]
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[:, kept_steps(T, case['pose_stride'])] = ~bad
    return mask


def time_major(t):
    """The layout the rollout hands out: a time-major buffer viewed [B,T,...]."""
    return t.transpose(0, 1).contiguous().transpose(0, 1)


def kink_case():
    """One rollout of three kept poses on a 9 x 9 map of grid_res = 0.25 m, d_max = 1 m, every number dyadic, so that float32 and float64 evaluate
    it exactly and the ties are EXACT.  m[i][j] = i: the sample is u, whatever v.  Pose 0: two footprint points at the same x and different y tie
    exactly for the maximum (the first must take the gradient, which shows in dJ/dR through the point's own coordinates; they are off the map at pose 1), its position sits on
    path vertex 0 (distance exactly 0) and its third row is (0, 0, 1) (roll = pitch = 0 exactly).  Pose 1: the arg-max points are off the map
    (off_map = 100, finite: zero map gradient).  Pose 2, the last: on the goal (distance exactly 0)."""
    X = torch.tensor([[[0.0, 0.0, 0.0], [0.75, 0.0, 0.0], [-0.5, 0.25, 0.0]]])
    R = torch.eye(3).repeat(1, 3, 1, 1).clone()
    R[0, 2, 2] = torch.tensor([0.25, 0.0, 1.0])        # pose 2: a tilted third row, not normalised
    points = torch.tensor([[0.5, -0.125, 0.0], [0.5, 0.25, 0.0], [-0.25, 0.0, 0.0], [0.125, 0.125, 0.0]])
    m = torch.arange(9, dtype=torch.float32)[:, None].expand(9, 9).contiguous()
    path = torch.tensor([[0.0, 0.0], [0.5, 0.5], [0.5, 1.0]])
    return dict(Xs=X, Rs=R, points=points, cost_map=m, path=path, goal=torch.tensor([-0.5, 0.25]), pose_stride=1, shape=(1, 3, 1, 4, 3)), \
        dict(grid_res=0.25, d_max=1.0, off_map=100.0)

