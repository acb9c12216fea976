"""No-GPU checks of the terrain-fit loop (monoforce_amd/fit.py, csrc/terrain_fit.hip): descriptor layout, the refusals the entry point makes
before any launch, the lazy export, and the host-side argument handling of `TerrainFitter`."""
import ctypes
import math
import subprocess
import sys
import types

import pytest

from tests.conftest import REPO


@pytest.fixture(scope='module')
def built_lib():
    import __graft_entry__ as g
    g.build()
    from monoforce_amd import _lib
    return _lib.lib()


def test_fit_desc_layout_matches_header(built_lib):
    from monoforce_amd import _lib
    built_lib.mf_sizeof.restype = ctypes.c_int
    built_lib.mf_sizeof.argtypes = [ctypes.c_char_p]
    assert built_lib.mf_sizeof(b'MfFitDesc') == ctypes.sizeof(_lib.MfFitDesc) == 96


def test_grid_cap_is_readable(built_lib):
    from monoforce_amd import fit
    assert fit.grid_cap() >= 1 and fit.grid_cap() * 256 >= 2 * 256 * 256      # the flagship's two maps are one trip of the loop


GOOD = dict(n_z=16, n_mu=4, max_iters=8, flags=0, lr_z=0.02, lr_mu=0.01, beta1=0.9, beta2=0.999, eps=1e-8, z_lo=-1.0, z_hi=1.0, mu_lo=0.0, mu_hi=1.0)


@pytest.mark.parametrize('change, message', [
    (dict(n_z=0), 'n_z must be positive'),
    (dict(n_z=-3), 'n_z must be positive'),
    (dict(n_mu=-1), 'n_mu must not be negative'),
    (dict(max_iters=-1), 'max_iters must not be negative'),
    (dict(beta1=1.0), 'beta1, beta2 must be in [0, 1)'),
    (dict(beta1=-0.1), 'beta1, beta2 must be in [0, 1)'),
    (dict(beta2=1.5), 'beta1, beta2 must be in [0, 1)'),
    (dict(beta2=math.nan), 'beta1, beta2 must be in [0, 1)'),
    (dict(eps=0.0), 'eps must be positive'),
    (dict(eps=-1e-8), 'eps must be positive'),
    (dict(lr_z=-0.02), 'lr must not be negative'),
    (dict(lr_mu=-0.01), 'lr must not be negative'),
    (dict(flags=1, z_lo=1.0, z_hi=-1.0), 'bounds need lo <= hi'),
    (dict(flags=2, mu_lo=1.0, mu_hi=0.0), 'bounds need lo <= hi'),
    (dict(flags=2, mu_lo=math.nan), 'bounds need lo <= hi'),
])
@pytest.mark.parametrize('suffix', ['f32', 'f64'])
def test_update_refuses_bad_descriptors_before_any_launch(built_lib, suffix, change, message):
    """MF_REQUIRE runs in front of the launch: with pointers that are not NULL (and never followed) each refusal is met on a CPU-only box."""
    from monoforce_amd import _lib
    fn = getattr(built_lib, f'mf_terrain_fit_update_{suffix}')
    p = ctypes.c_void_p(64)
    d = _lib.MfFitDesc(**{**GOOD, **change})
    assert fn(ctypes.byref(d), *([p] * 14), None) == 1
    assert built_lib.mf_last_error().decode() == f'terrain_fit_update: {message}'


def test_update_refuses_null_arguments(built_lib):
    from monoforce_amd import _lib
    fn = built_lib.mf_terrain_fit_update_f32
    p = ctypes.c_void_p(64)
    assert fn(None, *([p] * 14), None) == 1 and built_lib.mf_last_error() == b'terrain_fit_update: null descriptor'
    d = _lib.MfFitDesc(**GOOD)
    # argument order: z, mu, g_z, g_mu, m_z, v_z, m_mu, v_mu, loss, z_best, mu_best, state, loss_min, history
    for k in (0, 2, 4, 5, 8, 9, 11, 12, 13):
        args = [p] * 14
        args[k] = None
        assert fn(ctypes.byref(d), *args, None) == 1 and built_lib.mf_last_error() == b'terrain_fit_update: null argument', k
    for k in (1, 3, 6, 7, 10):
        args = [p] * 14
        args[k] = None
        assert fn(ctypes.byref(d), *args, None) == 1 and built_lib.mf_last_error() == b'terrain_fit_update: null friction argument', k
    # a flag that is not set leaves its bounds unread: lo > hi is no refusal then (the call gets as far as the null check)
    d = _lib.MfFitDesc(**{**GOOD, 'z_lo': 1.0, 'z_hi': -1.0})
    assert fn(ctypes.byref(d), None, *([p] * 13), None) == 1 and built_lib.mf_last_error() == b'terrain_fit_update: null argument'


def test_terrain_fitter_is_a_lazy_export():
    """`from monoforce_amd import TerrainFitter` works, and importing the package alone still pulls in neither torch nor the module."""
    code = ("import sys, monoforce_amd; assert 'torch' not in sys.modules and 'monoforce_amd.fit' not in sys.modules; "
            "from monoforce_amd import TerrainFitter; import monoforce_amd.fit as f; assert TerrainFitter is f.TerrainFitter; print('ok')")
    out = subprocess.run([sys.executable, '-c', code], cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr[-2000:]


def test_bounds_parsing():
    from monoforce_amd import _lib
    from monoforce_amd.fit import parse_bounds
    inf = math.inf
    assert parse_bounds(None) == (0, -inf, inf, -inf, inf)
    assert parse_bounds({}) == (0, -inf, inf, -inf, inf)
    assert parse_bounds(dict(z=None, mu=None)) == (0, -inf, inf, -inf, inf)
    assert parse_bounds(dict(mu=(0, 1))) == (_lib.MF_FIT_CLAMP_MU, -inf, inf, 0.0, 1.0)
    assert parse_bounds(dict(z=(-2.5, 2.5), mu=None)) == (_lib.MF_FIT_CLAMP_Z, -2.5, 2.5, -inf, inf)
    assert parse_bounds(dict(z=[-1, 1], mu=(0.0, inf))) == (_lib.MF_FIT_CLAMP_Z | _lib.MF_FIT_CLAMP_MU, -1.0, 1.0, 0.0, inf)
    assert parse_bounds(dict(z=(0.5, 0.5)))[1:3] == (0.5, 0.5)
    for bad in (dict(z=(1, -1)), dict(mu=(math.nan, 1)), dict(z=(1,)), dict(z=3.0), dict(height=(0, 1)), [(0, 1)], dict(mu=(0, 1, 2)), dict(z=('a', 'b'))):
        with pytest.raises(ValueError, match='bounds'):
            parse_bounds(bad)


def _host_fitter(**kw):
    """A fitter on CPU tensors around a problem that is never stepped: what the constructor and the host-side checks need."""
    import torch
    from monoforce_amd import TerrainFitter
    return TerrainFitter(types.SimpleNamespace(), torch.zeros(4, 6), torch.ones(4, 6), graph=False, **kw)


def test_run_refuses_to_overrun_max_iters():
    """The history holds max_iters losses: a call that would launch more is refused on the host, before anything is launched."""
    fit = _host_fitter(max_iters=5)
    assert fit.iteration == 0 and fit.history.shape == (5,)
    with pytest.raises(ValueError, match='max_iters=5'):
        fit.run(6)
    fit.iteration = 3       # (as after three iterations)
    with pytest.raises(ValueError, match='max_iters=5'):
        fit.run(3)
    fit.iteration = 5
    with pytest.raises(ValueError, match='max_iters=5'):
        fit.step()
    with pytest.raises(ValueError):
        fit.run(-1)
    out = fit.run(0)        # nothing to launch: the (empty) slice of the history
    assert out['loss'].shape == (0,) and fit.iteration == 5


def test_constructor_state_and_refusals():
    import torch
    from monoforce_amd import TerrainFitter, _lib
    fit = _host_fitter(max_iters=7, bounds=dict(mu=(0, 1)), lr=(0.5, 0.25), betas=(0.8, 0.99), eps=1e-6)
    d = fit.desc
    assert (d.n_z, d.n_mu, d.max_iters, d.flags) == (24, 24, 7, _lib.MF_FIT_CLAMP_MU)
    assert (d.lr_z, d.lr_mu, d.beta1, d.beta2, d.eps, d.mu_lo, d.mu_hi) == (0.5, 0.25, 0.8, 0.99, 1e-6, 0.0, 1.0)
    assert fit.state.tolist() == [0, -1, 0, 0] and fit.state.dtype == torch.int32
    assert math.isinf(float(fit.loss_min)) and bool(fit.history.isnan().all())
    assert fit.z.requires_grad and fit.mu.requires_grad and fit.z.is_leaf and torch.equal(fit.mu_best, torch.ones(4, 6))
    assert not any(float(t.abs().max()) for t in (fit.m_z, fit.v_z, fit.m_mu, fit.v_mu))
    z, mu = torch.zeros(4, 6), torch.ones(4, 6)
    for kw in (dict(lr=(-1, 0.1)), dict(betas=(1.0, 0.9)), dict(eps=0.0), dict(max_iters=-1), dict(bounds=dict(z=(1, 0)))):
        with pytest.raises(ValueError):
            TerrainFitter(types.SimpleNamespace(), z, mu, **kw)
    with pytest.raises(ValueError, match='maps'):
        TerrainFitter(types.SimpleNamespace(), z[0], mu[0])
    with pytest.raises(ValueError, match='dtype'):
        TerrainFitter(types.SimpleNamespace(), z, mu.double())
    with pytest.raises(TypeError, match='float32 or float64'):
        TerrainFitter(types.SimpleNamespace(), z.half(), mu.half())
