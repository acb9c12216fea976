"""The referee of the heightmap kernel (tests/heightmap_reference.py) without a GPU: pinned bit for bit on the reference's four stored outputs
(tests/golden/heightmap.npz), and the constructed clouds of tests/heightmap_cases.py shown to hold what their names say."""
import numpy as np
import pytest
import torch

from tests import heightmap_cases as hc
from tests import helpers as hp
from tests.heightmap_reference import estimate_heightmap


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd'])
def test_referee_reproduces_the_stored_outputs(tag):
    g = hp.load('heightmap')
    res, d_max, h_max, r_min, h_min = g[f'{tag}/kw']
    hm = estimate_heightmap(torch.as_tensor(g['points']), grid_res=float(res), d_max=float(d_max), h_max=float(h_max),
                            r_min=None if r_min < 0 else float(r_min), h_min=None if np.isnan(h_min) else float(h_min))
    assert hm.dtype == torch.float32 and np.array_equal(hm.numpy(), g[f'{tag}/hm'])


def _cell(x, y, kw):
    e = hc.edges_of(kw['grid_res'], kw['d_max'])
    return int((e < x).sum()) - 1, int((e < y).sum()) - 1


def test_constructed_clouds_hold_what_they_are_named_for():
    pts, kw = hc.contention()
    hm = estimate_heightmap(pts, **kw)
    i, j = _cell(0.35, -1.15, kw)
    inside = pts[(pts[:, 0] > 0.305) & (pts[:, 0] < 0.395) & (pts[:, 1] > -1.195) & (pts[:, 1] < -1.105) & (pts[:, 2].abs() < 1.0)]
    assert inside.shape[0] > 95000 and float(hm[0, i, j]) == float(inside[:, 2].max()) and float(pts[:, 2].max()) > 1.0
    assert 500 < int(hm[1].sum()) <= 1001

    pts, kw = hc.negative()
    hm = estimate_heightmap(pts, **kw)
    assert float(hm[0].max()) <= 0.0 and float(hm[0].min()) < -0.5 and int(hm[1].sum()) > 1000
    i, j = _cell(2.05, 2.05, kw)
    assert float(hm[1, i, j]) == 1.0 and np.signbit(hm[0, i, j].numpy()) and float(hm[0, i, j]) == 0.0           # -0.0, not +0.0
    i, j = _cell(-2.05, 3.05, kw)
    assert float(hm[0, i, j]) == float(np.float32(-1e-40)) != 0.0

    pts, kw = hc.infinite_and_on_the_box()
    hm = estimate_heightmap(pts, **kw)
    assert bool(torch.isfinite(hm).all()) and 300 < int(hm[1].sum()) <= 460
    assert float(hm[1, 0, :].sum() + hm[1, -1, :].sum()) < 40           # (the points ON the box did not land in the border cells)

    pts, kw = hc.six_columns()
    hm = estimate_heightmap(pts, **kw)
    assert pts.shape[1] == 6 and float(hm[0].max()) < 0.95 and int(hm[1].sum()) > 300
    assert float(estimate_heightmap(pts[:, :3], **kw)[0].max()) == float(np.float32(0.95))      # ... which their x, y, z alone would not tell

    pts, kw = hc.at_r_min()
    assert float(estimate_heightmap(pts, **kw)[1].sum()) == 0.0 and float(estimate_heightmap(pts, **dict(kw, r_min=None))[1].sum()) == 8.0
    pts, kw = hc.one_ulp_beyond_r_min()
    hm = estimate_heightmap(pts[:8], **kw)
    assert float(hm[1].sum()) == 8.0                                        # the larger coordinate one ulp out: kept, all eight
    assert float(estimate_heightmap(pts[:8], **dict(kw, r_min=float(np.nextafter(np.float32(1.25), np.float32(2.0)))))[1].sum()) == 0.0


@pytest.mark.parametrize('grid_res,d_max', hc.ODD_GRIDS)
def test_edge_clouds_sit_on_every_edge_and_the_formula_guess_is_wrong_there(grid_res, d_max):
    pts, kw = hc.on_and_around_every_edge(grid_res, d_max)
    e = hc.edges_of(grid_res, d_max)
    n = e.numel()
    assert (2 * d_max / grid_res) % 1 > 0.1 and n == int(np.ceil(2 * d_max / grid_res))
    assert all(bool((pts[:, k].unsqueeze(1) == e).any(0).all()) for k in (0, 1))           # every edge occurs as an x and as a y
    assert bool(((pts[:, 0] > e[-1]) & (pts[:, 0] < d_max)).sum() >= 4)
    # the kernel's first guess, restated: floor((v - edges[0]) * float32(1 / grid_res)) in float32, against bucketize - 1
    v = pts[:, 0][(pts[:, 0] > -d_max) & (pts[:, 0] < d_max)]
    guess = torch.clamp(torch.floor((v - e[0]) * torch.tensor(1.0 / grid_res, dtype=torch.float32)).long(), 0, n - 1)
    want = torch.bucketize(v, e) - 1
    print(f'{grid_res} / {d_max}: the guess is one too high at {int((guess > want).sum())} and one too low at {int((guess < want).sum())} of {v.numel()} coordinates')
    assert int((guess > want).sum()) > 10 and int((guess - want).abs().max()) == 1
    hm = estimate_heightmap(pts, **kw)
    assert tuple(hm.shape) == (2, n, n) and float(hm[1, -1, :].sum()) > 0 and float(hm[1, :, -1].sum()) > 0 and float(hm[1, 0, :].sum()) > 0
