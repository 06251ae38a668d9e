"""Occlusion masks on an MI355X: the cases of tests/occlusion_common.py on the product library, plus the full-size ones.  The
yardstick is that module's float64 restatement; no pyrender fixture exists (see its docstring)."""
import pytest
import torch

import occlusion_common as O
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('moved', [False, True])
@pytest.mark.parametrize('cull', [False, True])
@pytest.mark.parametrize('name', O.RASTER_MESHES)
@pytest.mark.parametrize('W,H', O.RASTER_SIZES)
def test_raster_against_the_restatement(gpu, W, H, name, cull, moved):
    O.check_raster(*gpu, name, W, H, cull, moved)


def test_raster_at_1920x1080(gpu):
    O.check_raster(*gpu, 'hd', 0, 0, True, False, full=True)


@pytest.mark.parametrize('name', ['F300', 'full', 'near'])
def test_raster_is_independent_of_run_and_face_order(gpu, name):
    O.check_raster_independence(*gpu, name, 67, 45)


@pytest.mark.parametrize('F', [1, 65, 300])
@pytest.mark.parametrize('P', [1, 25, 67, 92])
@pytest.mark.parametrize('T', [1, 3, 70])
def test_query_against_the_restatement(gpu, T, P, F):
    O.check_query(*gpu, T, P, F)


def test_query_on_designed_geometry(gpu):
    O.check_query_designed(*gpu)


def test_query_depth_is_the_rendered_body_depth(gpu):
    O.check_query_equals_raster(*gpu)


def test_full_size_joints_and_markers(gpu):
    O.check_full_size(*gpu)


def test_mask_drives_a_prox_window_and_the_trainer_loader(gpu, tmp_path):
    O.check_hand_over(*gpu, tmp_path, full=True)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    O.check_validation(*gpu, monkeypatch)
