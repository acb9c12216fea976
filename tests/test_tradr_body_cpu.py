"""The reference's REAL tradr body (config/meshes/tradr.obj): `dphys_config.points_from_obj` + `robot_geometry` against
the fixture `tests/golden/tradr_body.npz` (written by gen_golden.py through the reference's own `robot_geometry`,
dphys_config.py:38-74; open3d's voxel_down_sample restated there -- third-party, unpinned), and the CPU oracle against the
reference's own rollouts of that 175-point body."""
import os

import numpy as np
import pytest
import torch

from oracle import dphysics_oracle as orc
from tests import helpers as hp


@pytest.fixture(scope='module')
def mesh(tmp_path_factory):
    """The reference's tradr.obj as the loader sees it -- its 'v' lines, 8 decimals, rebuilt from tests/golden/tradr_mesh.npz -- in a
    directory of its own."""
    path = tmp_path_factory.mktemp('meshes') / 'tradr.obj'
    with open(path, 'w') as f:
        f.writelines('v %.8f %.8f %.8f\n' % tuple(r) for r in hp.load('tradr_mesh')['vertices'])
    return str(path)


def _sorted_rows(a):
    a = np.asarray(a, np.float64)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def test_fixture_is_the_175_point_body():
    g = hp.load('tradr_body')
    assert g['points'].shape == (175, 3) and g['points'].dtype == np.float32
    assert g['masks'].shape == (2, 175) and [int(m.sum()) for m in g['masks']] == [45, 45]
    assert not (g['masks'][0] & g['masks'][1]).any()
    assert np.allclose(g['robot_size'], [1.152, 0.574], atol=5e-4)


def test_points_from_obj_on_the_reference_mesh(mesh):
    """The mesh loader of the product (no open3d): same point SET, same masks per point, same robot_size as the fixture."""
    from monoforce_amd import dphys_config as dc
    g = hp.load('tradr_body')
    pts = dc.points_from_obj(mesh, voxel_size=0.1)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (175, 3)
    assert np.abs(_sorted_rows(pts.numpy()) - _sorted_rows(g['points'])).max() <= 1e-6
    p, parts, size = dc.robot_geometry('tradr', pts)
    assert [int(m.sum()) for m in parts] == [45, 45]
    assert abs(float(size[0]) - g['robot_size'][0]) <= 1e-6 and abs(float(size[1]) - g['robot_size'][1]) <= 1e-6
    # masks are per point: compare them through the points they select
    for m, mg in zip(parts, g['masks']):
        assert np.abs(_sorted_rows(p[m].numpy()) - _sorted_rows(g['points'][mg])).max() <= 1e-6
    # without down-sampling: every vertex of the file
    assert dc.points_from_obj(mesh, voxel_size=None).shape[0] == int(g['n_vertices'])


def test_dphysconfig_finds_the_mesh_through_the_environment(mesh, monkeypatch):
    from monoforce_amd.dphys_config import DPhysConfig
    monkeypatch.setenv('MONOFORCE_MESH_DIR', os.path.dirname(mesh))
    cfg = DPhysConfig(robot='tradr')
    assert cfg.robot_points.shape == (175, 3) and [int(m.sum()) for m in cfg.driving_parts] == [45, 45]
    assert cfg.robot_mass == 40.0 and abs(float(cfg.robot_size[1]) - 0.5736) < 1e-3


@pytest.mark.parametrize('tag', ['f32', 'f64'])
@pytest.mark.parametrize('integ', [0, 1])
def test_oracle_on_the_real_body_vs_reference(tag, integ):
    """B = 2, T = 48, 175 points, 64 x 64 per-rollout maps: oracle outputs and autograd gradients == the reference's."""
    g = hp.load('tradr_body')
    dt = hp.DT[tag]
    d_max, res, T = (float(v) for v in g['meta'])
    z, mu, ctrl = (torch.as_tensor(g[k]).to(dt) for k in ('z', 'mu', 'ctrl'))
    spec = hp.spec_from(g['points'], g['masks'], integ, res, d_max)
    z.requires_grad_(True); mu.requires_grad_(True); ctrl.requires_grad_(True)
    states, forces = orc.rollout(spec, z, ctrl, friction=mu)
    outs = list(states) + list(forces)
    tol = 1e-11 if tag == 'f64' else 5e-5
    for k, o in zip(hp.OUT_KEYS, outs):
        key = f'{tag}/i{integ}/{k}'
        if key in g.files:
            assert hp.rel_err(o.detach(), g[key]) <= tol, (k, hp.rel_err(o.detach(), g[key]))
    hp.probe_loss(outs, dt).backward()
    gtol = 1e-9 if tag == 'f64' else 5e-3
    assert hp.rel_err(z.grad, g[f'{tag}/i{integ}/g_z']) <= gtol
    assert hp.rel_err(mu.grad, g[f'{tag}/i{integ}/g_mu']) <= gtol
    assert hp.rel_err(ctrl.grad, g[f'{tag}/i{integ}/g_ctrl']) <= gtol
