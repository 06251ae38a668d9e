"""Chamfer nearest neighbours and the PROX scene-contact term on an MI355X: the cases of tests/chamfer_common.py on the product
library, plus the contact shape at full size once.  That module's docstring derives every tolerance."""
import pytest
import torch

import chamfer_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


def test_sizes_are_the_librarys(gpu):
    K.check_sizes(gpu[0])


@pytest.mark.parametrize('B,N,M', K.LATTICE_SHAPES)
def test_lattice_is_exact_with_lowest_index_ties(gpu, B, N, M):
    K.check_lattice(*gpu, B, N, M)


@pytest.mark.parametrize('kind', K.RANDOM_KINDS)
@pytest.mark.parametrize('B,N,M', K.RANDOM_SHAPES)
def test_random_points_against_float64(gpu, B, N, M, kind):
    K.check_random(*gpu, B, N, M, kind)


def test_results_do_not_depend_on_split_run_or_sharing(gpu):
    K.check_independence(*gpu)


@pytest.mark.parametrize('kind', K.RANDOM_KINDS)
def test_backward_against_float64(gpu, monkeypatch, kind):
    K.check_backward(*gpu, monkeypatch, 2, 70, 130, kind)


def test_backward_one_sided(gpu, monkeypatch):
    K.check_backward(*gpu, monkeypatch, 2, 70, 130, 'prox', bidirectional=False)


def test_backward_sums_a_shared_target_over_the_batch(gpu, monkeypatch):
    K.check_backward(*gpu, monkeypatch, 3, 33, 2 * K.CH.SPLIT_LENGTH + 7, 'normal', bidirectional=False, shared=True)


def test_module_through_autograd_backward(gpu):
    K.check_module_backward(*gpu)


def test_compat_fills_the_wrappers_buffers(gpu, monkeypatch):
    K.check_compat(*gpu, monkeypatch)


@pytest.mark.parametrize('B', [1, 3])
def test_contact_term_against_float64(gpu, B):
    K.check_contact_term(*gpu, B)


def test_prox_fitter_contact_loss(gpu, monkeypatch):
    K.check_prox_fitter(*gpu, monkeypatch)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    K.check_validation(*gpu, monkeypatch)


def test_contact_shape_at_full_size(gpu):
    K.check_full_size(*gpu)
