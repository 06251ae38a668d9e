"""Body overlays on an MI355X: the cases of tests/render_common.py on the product library, plus the full-size ones.  The yardstick
is that module's numpy restatement of the documented rule, in float64 and float32; no pyrender fixture exists."""
import pytest
import torch

import render_common as R
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('cull', [False, True])
@pytest.mark.parametrize('name', R.SOUPS)
@pytest.mark.parametrize('W,H', R.SIZES)
def test_triangle_soups_against_the_restatement(gpu, W, H, name, cull):
    R.check_render(*gpu, name, W, H, cull)


@pytest.mark.parametrize('rings,segs,W,H', R.SPHERES)
def test_smooth_spheres_against_the_restatement(gpu, rings, segs, W, H):
    R.check_render(*gpu, f'S{rings}x{segs}', W, H, True)


@pytest.mark.parametrize('rings,segs,W,H', R.SPHERES)
def test_vertex_normals(gpu, rings, segs, W, H):
    R.check_normals(*gpu, rings, segs, W, H)


@pytest.mark.parametrize('name', ['F300', 'full', 'near', 'S24x32'])
def test_result_does_not_depend_on_face_order(gpu, name):
    R.check_permuted_faces(*gpu, name, 67, 45)


@pytest.mark.parametrize('W,H', R.SIZES)
def test_background(gpu, W, H):
    R.check_background(*gpu, W, H)


@pytest.mark.parametrize('radius', [0, 2, 3])
@pytest.mark.parametrize('W,H', R.SIZES)
def test_points(gpu, W, H, radius):
    R.check_points(*gpu, W, H, radius)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    R.check_validation(*gpu, monkeypatch)


def test_full_size_body_at_1920x1080(gpu):
    R.check_full_size(*gpu)


def test_prox_window_to_overlay_images(gpu):
    R.check_hand_over(*gpu)
