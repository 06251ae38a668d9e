"""The iteration kernels without a C entry point of their own (prox_frame_dense, prox_sparse, prox_adam / prox_tail; fit_losses,
dverts_assemble / the fused dverts_vertex, fit_tail), one loss term at a time against the float64 oracles, on the host emulator: the
cases of tests/iter_terms_common.py, whose docstring derives every bound and margin."""
import pytest
import torch

import iter_terms_common as K

CPU = torch.device('cpu')


@pytest.mark.parametrize('case', list(K.PROX_TERMS))
def test_prox_one_term_against_float64(emu_lib, case):
    K.check_prox_term(emu_lib, CPU, case)


@pytest.mark.parametrize('B', K.PROX_B_SWEEP)
def test_prox_later_window_frozen_frames(emu_lib, B):
    K.check_prox_window(emu_lib, CPU, B)


def test_prox_create_refusals(emu_lib):
    K.check_prox_refusals(emu_lib, CPU)


@pytest.mark.parametrize('case', K.PROX_EMPTY)
def test_prox_empty_selection(emu_lib, case):
    K.check_prox_empty(emu_lib, CPU, case)


def test_prox_sparse_second_block_row(emu_lib):
    K.check_prox_many_friction_vertices(emu_lib, CPU)


@pytest.mark.parametrize('full', [False, True])
@pytest.mark.parametrize('term', K.AMASS_TERMS)
def test_amass_one_term_against_float64(emu_lib, term, full):
    K.check_amass_term(emu_lib, CPU, term, full)


def test_amass_dverts_assemble_fallback(emu_lib):
    K.check_amass_term(emu_lib, CPU, 'all', True, large=True)


@pytest.mark.parametrize('prior', K.AMASS_PRIORS)
def test_amass_prior_gradient_of_the_tail_kernel(emu_lib, prior):
    K.check_amass_prior(emu_lib, CPU, prior)


def test_amass_prior_gradient_per_frame(emu_lib):
    K.check_amass_prior_per_frame(emu_lib, CPU)


def test_zz_error_ratios(emu_lib):
    """prints the worst kernel / float32-oracle error ratio of every case above (pytest -s; DESIGN.md quotes them)"""
    K.report_ratios()
