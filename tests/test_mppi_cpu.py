"""MPPI without a GPU: the referee of the kernels (tests/mppi_reference.py) pinned against explicit loops and hand-computed values, the
descriptor mirror, argument validation of the three entry points, and the code-object metadata of mppi.o."""
import ctypes
import math
import os
import sys

import pytest
import torch

from tests import mppi_reference as ref
from tests.conftest import REPO

F64 = torch.float64


# ---- the referee against explicit loops -----------------------------------------------------------------------------------------------
def _loop_perturb(nominal, noise, sigma, lo, hi, keep):
    B, T, _ = noise.shape
    out = torch.empty(B, T, 2, dtype=F64)
    for b in range(B):
        for t in range(T):
            for k in range(2):
                v = float(nominal[t, k])
                if not (keep and b == 0):
                    v = v + sigma[k] * float(noise[b, t, k])
                out[b, t, k] = min(max(v, lo[k]), hi[k])
    return out


def _loop_costs(rows, force, x_last, goal, w):
    B, T, _ = rows.shape
    costs, terms = torch.empty(B, dtype=F64), torch.empty(B, 3, dtype=F64)
    for b in range(B):
        roll = sum(abs(math.atan2(float(rows[b, t, 1]), float(rows[b, t, 2]))) for t in range(T)) / T
        pitch = sum(abs(math.asin(min(max(-float(rows[b, t, 0]), -1.0), 1.0))) for t in range(T)) / T
        f = 0.0 if force is None else float(force[b])
        g = math.hypot(float(x_last[b, 0]) - float(goal[0]), float(x_last[b, 1]) - float(goal[1]))
        terms[b] = torch.tensor([roll + pitch, f, g], dtype=F64)
        costs[b] = w[0] * (roll + pitch) + w[1] * f + w[2] * g
    return costs, terms


def _loop_update(costs, controls, nominal, lam):
    B, T, _ = controls.shape
    finite = [b for b in range(B) if math.isfinite(float(costs[b]))]
    if not finite:
        return nominal.clone(), torch.zeros(B, dtype=F64), -1, 0
    cmin = min(float(costs[b]) for b in finite)
    best = next(b for b in finite if float(costs[b]) == cmin)
    e = [math.exp(-(float(costs[b]) - cmin) / lam) if b in finite else 0.0 for b in range(B)]
    s = sum(e)
    w = torch.tensor([v / s for v in e], dtype=F64)
    out = torch.zeros(T, 2, dtype=F64)
    for b in range(B):
        out += w[b] * controls[b]
    return out, w, best, len(finite)


# (scalars that float32 holds exactly: the referee rounds the descriptor's scalars to float32, the loops take them as they are)
SIGMA, LO, HI = (0.25, 0.5), (-1.0, -2.0), (1.0, 2.0)


@pytest.mark.parametrize('B,T', [(1, 1), (2, 3), (7, 5)])
def test_referee_matches_explicit_loops(B, T):
    g = torch.Generator().manual_seed(B * 100 + T)
    nominal = torch.rand(T, 2, dtype=F64, generator=g) * 2 - 1
    noise = torch.randn(B, T, 2, dtype=F64, generator=g) * 3
    for keep in (False, True):
        assert torch.equal(ref.perturb(nominal, noise, SIGMA, LO, HI, keep), _loop_perturb(nominal, noise, SIGMA, LO, HI, keep))
    rows = torch.randn(B, T, 4, dtype=F64, generator=g)
    rows[0, 0, :3] = 0.0                                     # atan2(0, 0) = 0, asin(0) = 0
    rows[-1, -1, 0] = 1.5                                    # outside the asin domain: clamped
    force, x_last, goal = torch.rand(B, dtype=F64, generator=g), torch.randn(B, 3, dtype=F64, generator=g), torch.tensor([1.0, 0.5], dtype=F64)
    for w, f in (((1.0, 0.5, 2.0), force), ((1.0, 0.0, 1.0), None)):
        c, t = ref.path_costs(rows, f, x_last, goal, w)
        lc, lt = _loop_costs(rows, f, x_last, goal, w)
        assert torch.allclose(c, lc, rtol=1e-14, atol=1e-15) and torch.allclose(t, lt, rtol=1e-14, atol=1e-15)
    costs = torch.rand(B, dtype=F64, generator=g)
    controls = torch.randn(B, T, 2, dtype=F64, generator=g)
    for lam in (0.5, 0.0625):
        n, w, best, nv = ref.update(costs, controls, nominal, lam)
        ln, lw, lbest, lnv = _loop_update(costs, controls, nominal, lam)
        assert torch.allclose(n, ln, rtol=1e-13, atol=1e-15) and torch.allclose(w, lw, rtol=1e-13, atol=1e-300) and (best, nv) == (lbest, lnv)


# ---- hand-computed values at B = 3, T = 2 -------------------------------------------------------------------------------------------
def test_referee_hand_computed_values():
    nominal = torch.tensor([[0.5, 0.0], [0.75, -1.75]], dtype=F64)
    noise = torch.tensor([[[9.0, 9.0], [9.0, 9.0]], [[1.0, -2.0], [2.0, -1.0]], [[-8.0, 8.0], [0.0, 0.0]]], dtype=F64)
    u = ref.perturb(nominal, noise, SIGMA, LO, HI, True)
    #            row 0 = nominal     0.5+0.25, 0-1 | 0.75+0.5 -> 1, -1.75-0.5 -> -2     0.5-2 -> -1, 0+4 -> 2 | nominal
    want = torch.tensor([[[0.5, 0.0], [0.75, -1.75]], [[0.75, -1.0], [1.0, -2.0]], [[-1.0, 2.0], [0.75, -1.75]]], dtype=F64)
    assert torch.equal(u, want)
    assert torch.equal(ref.perturb(nominal, noise, SIGMA, LO, HI, False)[0], torch.tensor([[1.0, 2.0], [1.0, 2.0]], dtype=F64))
    # rows: (r0, r1, r2, s).  level: roll = pitch = 0; nose down a quarter turn: pitch = pi/2; on its side: roll = pi/2
    level, nose, side = [0.0, 0.0, 1.0, 7.0], [-1.0, 0.0, 0.0, 7.0], [0.0, 1.0, 0.0, 7.0]
    rows = torch.tensor([[level, level], [nose, level], [side, [-2.0, -1.0, 0.0, 7.0]]], dtype=F64)
    x_last = torch.tensor([[1.0, 0.5, 9.0], [4.0, 4.5, 9.0], [1.0, -0.5, 9.0]], dtype=F64)
    goal = torch.tensor([1.0, 0.5], dtype=F64)
    force = torch.tensor([2.0, 4.0, 8.0], dtype=F64)
    c, t = ref.path_costs(rows, force, x_last, goal, (1.0, 0.5, 2.0))
    q = math.pi / 4            # a quarter turn in one of two steps: mean = pi / 4
    want_t = torch.tensor([[0.0, 2.0, 0.0], [q, 4.0, 5.0], [2 * q + q, 8.0, 1.0]], dtype=F64)      # rollout 2: roll (pi/2, pi/2), pitch (0, pi/2)
    assert torch.allclose(t, want_t, rtol=1e-15, atol=0)
    assert torch.allclose(c, torch.tensor([1.0, q + 2.0 + 10.0, 3 * q + 4.0 + 2.0], dtype=F64), rtol=1e-15, atol=0)
    assert torch.equal(ref.path_costs(rows, None, x_last, goal, (0.0, 0.0, 1.0))[0], torch.tensor([0.0, 5.0, 1.0], dtype=F64))
    # costs 0, ln 2, ln 4 at lambda = 1: e = (1, 1/2, 1/4), weights (4, 2, 1) / 7
    costs = torch.tensor([math.log(4.0), 0.0, math.log(2.0)], dtype=F64) + 3.0
    n, w, best, nv = ref.update(costs, want, nominal, 1.0)
    assert torch.allclose(w, torch.tensor([1.0, 4.0, 2.0], dtype=F64) / 7, rtol=1e-14, atol=0) and (best, nv) == (1, 3)
    assert torch.allclose(n, (want[0] + 4 * want[1] + 2 * want[2]) / 7, rtol=1e-14, atol=0)


def test_referee_edge_cases():
    g = torch.Generator().manual_seed(3)
    controls, nominal = torch.randn(4, 3, 2, dtype=F64, generator=g), torch.randn(3, 2, dtype=F64, generator=g)
    nan, inf = float('nan'), float('inf')
    # one NaN cost: weight exactly 0, the rest as if it were not there
    n, w, best, nv = ref.update(torch.tensor([nan, 2.0, 1.0, 2.0], dtype=F64), controls, nominal, 0.5)
    n3, w3, _, _ = ref.update(torch.tensor([2.0, 1.0, 2.0], dtype=F64), controls[1:], nominal, 0.5)
    assert w[0] == 0 and torch.equal(w[1:], w3) and torch.allclose(n, n3, rtol=1e-15) and (best, nv) == (2, 3)
    n, w, best, nv = ref.update(torch.tensor([inf, -inf, 1.0, nan], dtype=F64), controls, nominal, 0.5)
    assert w.tolist() == [0.0, 0.0, 1.0, 0.0] and torch.equal(n, controls[2]) and (best, nv) == (2, 1)
    # no finite cost: the nominal comes back, no weights, best = -1
    n, w, best, nv = ref.update(torch.tensor([nan, nan, inf, nan], dtype=F64), controls, nominal, 0.5)
    assert torch.equal(n, nominal) and not w.any() and (best, nv) == (-1, 0)
    # a tie for the minimum: the first index, equal weights
    n, w, best, nv = ref.update(torch.tensor([3.0, 1.0, 1.0, 3.0], dtype=F64), controls, nominal, 0.5)
    assert best == 1 and w[1] == w[2] and w[0] == w[3] and abs(float(w.sum()) - 1) < 1e-15
    # lambda = 1e-6: one-hot, no NaN;  lambda = 1e6: the mean
    for dt in (torch.float32, F64):
        c = torch.tensor([0.7, 0.3, 0.9, 0.31], dtype=dt)
        n, w, best, nv = ref.update(c, controls.to(dt), nominal.to(dt), 1e-6)
        assert w.tolist() == [0.0, 1.0, 0.0, 0.0] and torch.equal(n, controls[1].to(dt)) and best == 1 and torch.isfinite(n).all()
        n, w, best, nv = ref.update(c, controls.to(dt), nominal.to(dt), 1e6)
        assert torch.allclose(w, torch.full((4,), 0.25, dtype=dt), rtol=1e-5) and torch.allclose(n, controls.to(dt).mean(0), rtol=1e-5, atol=1e-6)
    # NaN rows propagate into the cost of their rollout alone
    rows = torch.rand(3, 4, 4, dtype=F64, generator=g)
    rows[1, 2, 1] = nan
    c, _ = ref.path_costs(rows, None, torch.zeros(3, 3, dtype=F64), torch.zeros(2, dtype=F64), (1.0, 0.0, 1.0))
    assert torch.isnan(c[1]) and torch.isfinite(c[[0, 2]]).all()


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def built_lib():
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import _lib
    return _lib.lib()


def test_descriptor_mirror_matches_header(built_lib):
    from monoforce_amd import _lib
    built_lib.mf_sizeof.restype = ctypes.c_int
    built_lib.mf_sizeof.argtypes = [ctypes.c_char_p]
    assert built_lib.mf_sizeof(b'MfMppiDesc') == ctypes.sizeof(_lib.MfMppiDesc) == 80
    for name in ('mf_mppi_perturb_f32', 'mf_path_costs_f32', 'mf_mppi_update_f32', 'mf_mppi_scratch_bytes'):
        assert name in _lib.SYMBOLS and hasattr(built_lib, name)
    from monoforce_amd import MPPIPlanner, TrajectoryShooter  # noqa: F401      (exported side by side)


def test_argument_validation_without_gpu(built_lib):
    """Every rejected argument is reported before any launch: an error code and a message, on a box without a GPU."""
    from monoforce_amd import _lib
    f2 = lambda a, b: (ctypes.c_float * 2)(a, b)  # noqa: E731
    p = ctypes.c_void_p(1 << 20)       # never dereferenced: validation fails first

    def desc(**kw):
        d = dict(B=8, T=5, sigma=f2(0.3, 0.6), lo=f2(-1, -2), hi=f2(1, 2), w_incl=1.0, w_force=0.0, w_goal=1.0, lam=0.05,
                 row_stride_b=4, row_stride_t=32, x_stride_b=3)
        d.update(kw)
        return _lib.MfMppiDesc(**d)

    def calls(d):
        r = ctypes.byref(d) if d is not None else None
        return [built_lib.mf_mppi_perturb_f32(r, p, p, p, None),
                built_lib.mf_path_costs_f32(r, p, None, p, p, p, p, None),
                built_lib.mf_mppi_update_f32(r, p, p, p, p, p, p, p, p, ctypes.c_longlong(1 << 30), None)]

    INVALID, UNSUPPORTED = 1, 2
    for d, code, word in [(None, INVALID, b'null descriptor'), (desc(B=0), INVALID, b'positive'), (desc(T=-3), INVALID, b'positive'),
                          (desc(lam=0.0), INVALID, b'lambda'), (desc(lam=-1.0), INVALID, b'lambda'), (desc(lam=float('nan')), INVALID, b'lambda'),
                          (desc(sigma=f2(0.3, -0.1)), INVALID, b'sigma'), (desc(lo=f2(1.5, -2)), INVALID, b'lo <= hi'),
                          (desc(B=1 << 15, T=1 << 14), UNSUPPORTED, b'2^31')]:
        for rc in calls(d):
            assert rc == code and word in built_lib.mf_last_error(), (rc, built_lib.mf_last_error())
    assert built_lib.mf_mppi_scratch_bytes(ctypes.byref(desc(B=0))) == -1 and built_lib.mf_mppi_scratch_bytes(None) == -1
    assert built_lib.mf_mppi_scratch_bytes(ctypes.byref(desc(B=1 << 13, T=1 << 15))) > 0       # B T 4 = 2^30: still supported
    # null pointers, one argument at a time
    d = ctypes.byref(desc())
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert built_lib.mf_mppi_perturb_f32(d, *a, None) == INVALID and b'null' in built_lib.mf_last_error()
    for k in (0, 2, 3, 4):          # (terms, the last one, may be NULL)
        a = [p, None, p, p, p, p]
        a[k] = None
        assert built_lib.mf_path_costs_f32(d, *a, None) == INVALID and b'null' in built_lib.mf_last_error()
    for k in range(8):
        a = [p] * 8
        a[k] = None
        assert built_lib.mf_mppi_update_f32(d, *a, ctypes.c_longlong(1 << 30), None) == INVALID and b'null' in built_lib.mf_last_error()
    # the force term: a buffer exactly when it has a weight
    assert built_lib.mf_path_costs_f32(d, p, p, p, p, p, p, None) == INVALID and b'force_cost' in built_lib.mf_last_error()
    assert built_lib.mf_path_costs_f32(ctypes.byref(desc(w_force=0.5)), p, None, p, p, p, p, None) == INVALID and b'force_cost' in built_lib.mf_last_error()
    # scratch: one byte short
    need = built_lib.mf_mppi_scratch_bytes(d)
    assert need == 1 * 5 * 8 and built_lib.mf_mppi_scratch_bytes(ctypes.byref(desc(B=65))) == 2 * 5 * 8
    assert built_lib.mf_mppi_update_f32(d, *([p] * 8), ctypes.c_longlong(need - 1), None) == INVALID and b'scratch' in built_lib.mf_last_error()


def test_mppi_kernels_use_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import kernel_metadata
    rows = [(n, m) for o, n, m in kernel_metadata.kernels() if o == 'mppi.o']
    names = ' '.join(n for n, _ in rows)
    for k in ('mppi_perturb_kernel', 'path_costs_kernel<true>', 'path_costs_kernel<false>', 'mppi_stats_kernel', 'mppi_partial_kernel', 'mppi_finish_kernel'):
        assert k in names, (k, names)
    assert all(m['scratch'] == 0 for _, m in rows), rows
