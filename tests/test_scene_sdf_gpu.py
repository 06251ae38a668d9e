"""Scene mesh -> signed-distance volume on an MI355X: the cases of tests/scene_sdf_common.py on the product library, a captured build,
and a level-5 sphere at 128^3 (grid against brute force) and 256^3 against the analytic sphere.  That module's docstring derives
every tolerance."""
import numpy as np
import pytest
import torch

import scene_sdf_common as K
from lemo_amd import _hip
from lemo_amd.scene import build_scene_sdf, prepare_scene_mesh

pytestmark = pytest.mark.gpu

SPHERE_R = 0.9
SPHERE_C = np.array([0.113, -0.047, 1.021])
SPHERE_MIN, SPHERE_MAX = np.array([-1.2, -1.3, -0.3], np.float32), np.array([1.4, 1.3, 2.4], np.float32)


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.fixture(scope='module')
def sphere(gpu):
    """icosphere(5): 20480 faces -> (prepared mesh, sagitta of the polyhedron from its largest circumradius)"""
    lib, device = gpu
    v, f = K.icosphere(5)
    v = (v * SPHERE_R + SPHERE_C).astype(np.float32)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    la, lb, lc = np.linalg.norm(b - c, axis=1), np.linalg.norm(c - a, axis=1), np.linalg.norm(a - b, axis=1)
    rc = float(np.max(la * lb * lc / (2 * np.linalg.norm(np.cross(b - a, c - a), axis=1))))
    radius = np.linalg.norm(v.astype(np.float64) - SPHERE_C, axis=1)
    # the surface lies between the spheres of radius min|v| - sagitta and max|v| (the corners are rounded to fp32)
    sag = float(radius.min() - np.sqrt(radius.min() ** 2 - rc ** 2))
    return prepare_scene_mesh(K.dev(v, device), f, _lib=lib), sag + float(radius.max() - radius.min())


def _against_sphere(S, bound, what):
    c = S.centres().double()
    exact = torch.linalg.norm(c - torch.tensor(SPHERE_C, device=c.device), dim=-1) - SPHERE_R
    err = float((S.sdf.double() - exact).abs().max())
    print(f'{what}: max |sdf - sphere| = {err:.3g}, bound {bound:.3g} (sagitta) + {K.DIST_TOL:.3g}')
    assert err <= bound + K.DIST_TOL + 4e-7                  # 4e-7: the centres in float32 (1 ulp of 2.4 m per axis)
    assert float((S.sdf < 0).float().mean()) > 0.05


@pytest.mark.parametrize('name', K.CASES)
def test_modes_identical_and_float64(gpu, name):
    K.check_case(*gpu, name)


def test_edge_rules(gpu):
    K.check_edge_rules(*gpu)


def test_sampler_returns_the_volume_at_its_centres(gpu):
    K.check_sampler(*gpu)


def test_prox_files_round_trip(gpu, tmp_path):
    K.check_files(*gpu, tmp_path)


def test_captured_build_equals_eager(gpu):
    K.check_graph(*gpu)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    K.check_validation(*gpu, monkeypatch)


def test_sphere_128_grid_equals_brute_and_analytic(gpu, sphere):
    lib, _ = gpu
    mesh, bound = sphere
    kw = dict(dim=128, grid_min=SPHERE_MIN, grid_max=SPHERE_MAX, return_nearest=True, _lib=lib)
    brute, grid = build_scene_sdf(mesh, mode='brute', **kw), build_scene_sdf(mesh, mode='grid', **kw)
    assert torch.equal(grid.sdf.view(torch.int32), brute.sdf.view(torch.int32)) and torch.equal(grid.nearest, brute.nearest)
    _against_sphere(grid, bound, 'icosphere(5) at 128^3')


def test_sphere_256_grid_analytic(gpu, sphere):
    lib, _ = gpu
    mesh, bound = sphere
    S = build_scene_sdf(mesh, dim=256, grid_min=SPHERE_MIN, grid_max=SPHERE_MAX, mode='grid', _lib=lib)
    _against_sphere(S, bound, 'icosphere(5) at 256^3')
