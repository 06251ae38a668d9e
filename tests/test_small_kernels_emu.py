"""The marker encode / decode kernels, lemo_smooth_loss, lemo_adam_flat(_ctr) and lemo_dec_end_fwd through their own C entry points on
the host emulator: the cases of tests/small_kernels_common.py, whose docstring derives every bound."""
import pytest
import torch

import small_kernels_common as K

CPU = torch.device('cpu')


@pytest.mark.parametrize('M1', K.MARKER_M1)
@pytest.mark.parametrize('T', K.ENC_T)
def test_marker_encode_against_long_double(emu_lib, T, M1):
    K.check_encode(emu_lib, CPU, T, M1)


def test_marker_encode_heading_beyond_half_pi(emu_lib):
    K.check_encode(emu_lib, CPU, 161, 68, wide=True)


def test_marker_encode_refusals_write_nothing(emu_lib):
    K.check_encode_refusals(emu_lib, CPU)


@pytest.mark.parametrize('J', K.REC_J)
@pytest.mark.parametrize('T', K.DEC_T)
def test_reconstruct_global_body_against_long_double(emu_lib, T, J):
    K.check_reconstruct(emu_lib, CPU, T, J)


def test_reconstruct_global_body_refusals_write_nothing(emu_lib):
    K.check_reconstruct_refusals(emu_lib, CPU)


@pytest.mark.parametrize('J', K.DECODE_J)
@pytest.mark.parametrize('T', K.DEC_T)
def test_decode_clip_labels_markers_and_post(emu_lib, T, J):
    K.check_decode(emu_lib, CPU, T, J)


def test_decode_clip_refusals_write_nothing(emu_lib):
    K.check_decode_refusals(emu_lib, CPU)


@pytest.mark.parametrize('H,W,Cn', K.SMOOTH_SHAPES)
def test_smooth_loss_against_float64(emu_lib, H, W, Cn):
    K.check_smooth(emu_lib, CPU, H, W, Cn)


def test_smooth_loss_refusals_write_nothing(emu_lib):
    K.check_smooth_refusals(emu_lib, CPU)


@pytest.mark.parametrize('lr', K.ADAM_LR)
@pytest.mark.parametrize('t', K.ADAM_T)
def test_adam_flat_against_torch(emu_lib, t, lr):
    K.check_adam(emu_lib, CPU, t, lr)


@pytest.mark.parametrize('t', (1, 999))
def test_adam_flat_ctr_is_adam_flat_at_the_counter(emu_lib, t):
    K.check_adam_ctr(emu_lib, CPU, t)


def test_adam_flat_refusals_write_nothing(emu_lib):
    K.check_adam_refusals(emu_lib, CPU)


@pytest.mark.parametrize('bs,H,W,gap', K.DEC_END_SHAPES)
def test_dec_end_fwd_against_float64(emu_lib, bs, H, W, gap):
    K.check_dec_end(emu_lib, CPU, bs, H, W, gap)


def test_dec_end_fwd_refusals_write_nothing(emu_lib):
    K.check_dec_end_refusals(emu_lib, CPU)


def test_zz_error_ratios(emu_lib):
    """prints the worst measured / bound ratios of the cases above (pytest -s; DESIGN.md quotes them)"""
    K.report_ratios()
