"""The smoothness prior's own training set (lemo_amd.dataset.SmoothClipImageBuilder, mode LEMO_CLIP_GLOBAL of
csrc/dataset_kernels.hip) on the host emulator: the cases of tests/dataset_global_checks.py."""
import pytest
import torch

import dataset_global_checks as G

CPU = torch.device('cpu')


def test_restatement_is_held_to_the_reference_fixture():
    G.check_restatement_is_the_reference()


@pytest.mark.parametrize('M', G.MS)
@pytest.mark.parametrize('T', [30, 120])
def test_kernel_on_reference_markers_gives_the_reference_images(emu_lib, T, M):
    G.check_kernel_vs_fixture(emu_lib, CPU, T, M)


@pytest.mark.parametrize('M', G.MS)
def test_end_to_end_from_amass_parameters(emu_lib, tmp_path, M):
    G.check_end_to_end(emu_lib, CPU, tmp_path, M)


@pytest.mark.parametrize('M', G.MS)
@pytest.mark.parametrize('T', [30, 120])
def test_statistics_against_float64_and_the_saved_ones(emu_lib, T, M):
    G.check_statistics(emu_lib, CPU, T, M)


@pytest.mark.parametrize('T,M,N,chunk', G.SHAPES)
def test_indexing_sweep_against_the_restatement(emu_lib, T, M, N, chunk):
    G.check_shape(emu_lib, CPU, T, M, N, chunk)


def test_built_image_is_what_the_fit_loop_feeds_the_encoder(emu_lib):
    G.check_fit_side_image(emu_lib, CPU)


def test_trainer_takes_the_built_set_without_a_copy_and_steps(emu_lib):
    G.check_trainer_takes_it(emu_lib, CPU)


def test_fitter_is_constructed_from_the_statistics(emu_lib):
    G.check_fitter_takes_the_statistics(emu_lib, CPU)


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    G.check_validation(emu_lib, CPU, monkeypatch)
