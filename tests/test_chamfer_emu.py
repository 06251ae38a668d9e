"""Chamfer nearest neighbours and the PROX scene-contact term (lemo_amd.chamfer, csrc/chamfer_kernels.hip) on the host emulator:
the cases of tests/chamfer_common.py, whose docstring derives every tolerance."""
import pytest
import torch

import chamfer_common as K

CPU = torch.device('cpu')


def test_sizes_are_the_librarys(emu_lib):
    K.check_sizes(emu_lib)


@pytest.mark.parametrize('B,N,M', K.LATTICE_SHAPES)
def test_lattice_is_exact_with_lowest_index_ties(emu_lib, B, N, M):
    K.check_lattice(emu_lib, CPU, B, N, M)


@pytest.mark.parametrize('kind', K.RANDOM_KINDS)
@pytest.mark.parametrize('B,N,M', K.RANDOM_SHAPES)
def test_random_points_against_float64(emu_lib, B, N, M, kind):
    K.check_random(emu_lib, CPU, B, N, M, kind)


def test_results_do_not_depend_on_split_run_or_sharing(emu_lib):
    K.check_independence(emu_lib, CPU)


@pytest.mark.parametrize('kind', K.RANDOM_KINDS)
def test_backward_against_float64(emu_lib, monkeypatch, kind):
    K.check_backward(emu_lib, CPU, monkeypatch, 2, 70, 130, kind)


def test_backward_one_sided(emu_lib, monkeypatch):
    K.check_backward(emu_lib, CPU, monkeypatch, 2, 70, 130, 'prox', bidirectional=False)


def test_backward_sums_a_shared_target_over_the_batch(emu_lib, monkeypatch):
    K.check_backward(emu_lib, CPU, monkeypatch, 3, 33, 2 * K.CH.SPLIT_LENGTH + 7, 'normal', bidirectional=False, shared=True)


def test_module_through_autograd_backward(emu_lib):
    K.check_module_backward(emu_lib, CPU)


def test_compat_fills_the_wrappers_buffers(emu_lib, monkeypatch):
    K.check_compat(emu_lib, CPU, monkeypatch)


def test_compat_has_no_cpu_path():
    K.check_compat_without_a_library()


@pytest.mark.parametrize('B', [1, 3])
def test_contact_term_against_float64(emu_lib, B):
    K.check_contact_term(emu_lib, CPU, B)


def test_prox_fitter_contact_loss(emu_lib, monkeypatch):
    K.check_prox_fitter(emu_lib, CPU, monkeypatch)


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    K.check_validation(emu_lib, CPU, monkeypatch)
