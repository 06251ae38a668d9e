"""The smoothness prior's own training set on an MI355X: the cases of tests/dataset_global_checks.py on the product library."""
import pytest
import torch

import dataset_global_checks as G
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('M', G.MS)
@pytest.mark.parametrize('T', [30, 120])
def test_kernel_on_reference_markers_gives_the_reference_images(gpu, T, M):
    G.check_kernel_vs_fixture(*gpu, T, M)


@pytest.mark.parametrize('M', G.MS)
def test_end_to_end_from_amass_parameters(gpu, tmp_path, M):
    G.check_end_to_end(*gpu, tmp_path, M)


@pytest.mark.parametrize('M', G.MS)
@pytest.mark.parametrize('T', [30, 120])
def test_statistics_against_float64_and_the_saved_ones(gpu, T, M):
    G.check_statistics(*gpu, T, M)


@pytest.mark.parametrize('T,M,N,chunk', G.SHAPES)
def test_indexing_sweep_against_the_restatement(gpu, T, M, N, chunk):
    G.check_shape(*gpu, T, M, N, chunk)


def test_built_image_is_what_the_fit_loop_feeds_the_encoder(gpu):
    G.check_fit_side_image(*gpu)


def test_trainer_takes_the_built_set_without_a_copy_and_steps(gpu):
    G.check_trainer_takes_it(*gpu)


def test_fitter_is_constructed_from_the_statistics(gpu):
    G.check_fitter_takes_the_statistics(*gpu)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    G.check_validation(*gpu, monkeypatch)
