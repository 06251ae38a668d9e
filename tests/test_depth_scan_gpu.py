"""Depth frames to body scans on an MI355X: the cases of tests/depth_scan_common.py on the product library.  That module's docstring
derives every tolerance."""
import pytest
import torch

import depth_scan_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('name', list(K.SHAPES))
def test_ray_table_and_rotation_against_the_restatement(gpu, name):
    K.check_host_constants(*gpu, name)


@pytest.mark.parametrize('coord', ['color', None])
@pytest.mark.parametrize('mask_on_color', [True, False])
@pytest.mark.parametrize('name', K.SMALL)
def test_create_scan_against_float64_and_own_pixels(gpu, name, mask_on_color, coord):
    K.check_case(*gpu, name, mask_on_color, coord)


def test_create_scan_at_the_prox_size(gpu):
    K.check_case(*gpu, 'full', True, 'color')


@pytest.mark.parametrize('flip', [False, True])
def test_raw_uint16_depth(gpu, flip):
    K.check_raw(*gpu, flip)


def test_scan_feeds_scan_terms(gpu):
    K.check_round_trip(*gpu)


def test_projection_drop_in(gpu):
    K.check_drop_in(*gpu)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    K.check_refusals(*gpu, monkeypatch)
