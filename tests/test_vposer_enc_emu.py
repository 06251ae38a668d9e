"""The VPoser encoder (lemo_vposer_encode_fwd / _bwd) and the methods built on it (VPoser.encode / forward / sample_poses, embed_body_pose,
with_pose_embedding) on the host emulator: the cases of tests/vposer_enc_common.py, whose docstring derives every tolerance."""
import pytest
import torch

import vposer_enc_common as K

CPU = torch.device('cpu')


@pytest.mark.parametrize('B,variant', K.FWD_CASES)
def test_encode_forward_against_float64(emu_lib, B, variant):
    K.check_fwd(emu_lib, CPU, B, variant)


def test_encode_forward_refusals_write_nothing(emu_lib):
    K.check_fwd_refusals(emu_lib, CPU)


@pytest.mark.parametrize('B,which,variant', K.BWD_CASES)
def test_encode_backward_against_float64(emu_lib, B, which, variant):
    K.check_bwd(emu_lib, CPU, B, which, variant)


def test_encode_backward_refusals_write_nothing(emu_lib):
    K.check_bwd_refusals(emu_lib, CPU)


def test_encode_method_shapes_bits_and_autograd(emu_lib):
    K.check_encode_shapes_and_autograd(emu_lib, CPU)


def test_loading_another_state_repacks(emu_lib):
    K.check_repack(emu_lib, CPU)


def test_forward_with_eps_and_sample_poses(emu_lib):
    K.check_forward_and_samples(emu_lib, CPU)


def test_matrot2aa_and_aa2matrot_round_trip(emu_lib):
    K.check_rotation_helpers(emu_lib, CPU)


def test_embed_body_pose(emu_lib):
    K.check_embed(emu_lib, CPU)


def test_with_pose_embedding_starts_a_window(emu_lib):
    K.check_with_pose_embedding(emu_lib)


def test_against_the_recorded_reference_run(emu_lib):
    K.check_reference_run(emu_lib, CPU)


def test_zz_error_ratios(emu_lib):
    """prints the worst kernel error / bound ratios of the cases above (pytest -s; DESIGN.md quotes them) and checks that the forward and
    the backward kernel were both launched"""
    K.report_ratios()
