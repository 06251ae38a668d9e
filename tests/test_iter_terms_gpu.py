"""The iteration kernels without a C entry point of their own (prox_frame_dense, prox_sparse, prox_adam / prox_tail; fit_losses,
dverts_assemble / the fused dverts_vertex, fit_tail), one loss term at a time against the float64 oracles, on an MI355X: the cases of
tests/iter_terms_common.py on the product library (eager closure / step calls only).  That module's docstring derives every bound
and margin."""
import pytest
import torch

import iter_terms_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('case', list(K.PROX_TERMS))
def test_prox_one_term_against_float64(gpu, case):
    K.check_prox_term(*gpu, case)


@pytest.mark.parametrize('B', K.PROX_B_SWEEP)
def test_prox_later_window_frozen_frames(gpu, B):
    K.check_prox_window(*gpu, B)


def test_prox_create_refusals(gpu):
    K.check_prox_refusals(*gpu)


@pytest.mark.parametrize('case', K.PROX_EMPTY)
def test_prox_empty_selection(gpu, case):
    K.check_prox_empty(*gpu, case)


def test_prox_sparse_second_block_row(gpu):
    K.check_prox_many_friction_vertices(*gpu)


@pytest.mark.parametrize('full', [False, True])
@pytest.mark.parametrize('term', K.AMASS_TERMS)
def test_amass_one_term_against_float64(gpu, term, full):
    K.check_amass_term(*gpu, term, full)


def test_amass_dverts_assemble_fallback(gpu):
    K.check_amass_term(*gpu, 'all', True, large=True)


@pytest.mark.parametrize('prior', K.AMASS_PRIORS)
def test_amass_prior_gradient_of_the_tail_kernel(gpu, prior):
    K.check_amass_prior(*gpu, prior)


def test_amass_prior_gradient_per_frame(gpu):
    K.check_amass_prior_per_frame(*gpu)


def test_zz_error_ratios(gpu):
    """prints the worst kernel / float32-oracle error ratio of every case above (pytest -s; DESIGN.md quotes them)"""
    K.report_ratios()
