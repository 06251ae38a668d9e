"""The self-penetration term on an MI355X: the cases of tests/selfpen_common.py on the product library, plus the body model's mesh at
full size once and the fitter's captured iteration.  That module's docstring derives every tolerance."""
import pytest
import torch

import selfpen_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('name,B', K.MESH_CASES)
def test_search_modes_identical_and_float64(gpu, name, B):
    K.check_search(*gpu, name, B)


def test_search_closed_form_pairs(gpu):
    K.check_closed_form(*gpu)


def test_search_capacity_keeps_the_first_pairs(gpu):
    K.check_capacity(*gpu)


def test_search_part_filter(gpu):
    K.check_filter(*gpu)


def test_search_at_full_size(gpu):
    K.check_full_size(*gpu)


@pytest.mark.parametrize('outside', [True, False])
@pytest.mark.parametrize('sigma', K.SIGMAS)
@pytest.mark.parametrize('name,B', K.LOSS_CASES)
def test_loss_against_float64(gpu, name, B, sigma, outside):
    K.check_loss(*gpu, name, B, sigma, outside)


def test_loss_edge_rules(gpu):
    K.check_loss_edges(*gpu)


def test_self_penetration_term(gpu):
    K.check_term(*gpu)


def test_prox_fitter_selfpen_and_smooth_terms(gpu, monkeypatch):
    K.check_prox_fitter(*gpu, monkeypatch)


def test_prox_fitter_graph_equals_eager(gpu, monkeypatch):
    K.check_fitter_graph(*gpu, monkeypatch)


def test_compat_mesh_intersection(gpu, monkeypatch):
    K.check_compat(*gpu, monkeypatch)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    K.check_validation(*gpu, monkeypatch)
