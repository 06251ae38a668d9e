"""Scene views on an MI355X: the cases of tests/scene_view_common.py on the product library, plus the full-size ones.  The yardstick
is that module's numpy restatement of the documented rules, in float64 and float32; no pyrender or open3d fixture exists."""
import pytest
import torch

import scene_view_common as S
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('cull', [False, True])
@pytest.mark.parametrize('lit,colored', [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize('W,H', S.SIZES)
def test_layers_against_the_restatement(gpu, W, H, lit, colored, cull):
    S.check_layers(*gpu, W, H, cull, lit, colored)


@pytest.mark.parametrize('P', [1, 5, 130])
@pytest.mark.parametrize('W,H', S.SIZES)
def test_spheres_against_the_restatement(gpu, W, H, P):
    S.check_spheres(*gpu, W, H, P)


@pytest.mark.parametrize('W,H', S.SIZES)
def test_body_alone_is_the_body_renderer(gpu, W, H):
    S.check_body_only(*gpu, W, H)


@pytest.mark.parametrize('W,H', S.SIZES)
def test_depth_owner_and_chunk_anchors(gpu, W, H):
    S.check_anchors(*gpu, W, H)


def test_result_does_not_depend_on_scene_face_or_sphere_order(gpu):
    S.check_permutations(*gpu, 67, 45)


@pytest.mark.parametrize('W,H', S.SIZES)
def test_set_view_and_scene_transform(gpu, W, H):
    S.check_set_view(*gpu, W, H)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    S.check_validation(*gpu, monkeypatch)


def test_full_size_scene_body_and_spheres_at_1920x1080(gpu):
    S.check_full_size(*gpu)


def test_prox_window_to_scene_view_images(gpu):
    S.check_hand_over(*gpu)
