"""The marker encode / decode kernels, lemo_smooth_loss, lemo_adam_flat(_ctr) and lemo_dec_end_fwd through their own C entry points on
an MI355X: the cases of tests/small_kernels_common.py on the product library.  That module's docstring derives every bound."""
import pytest
import torch

import small_kernels_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('M1', K.MARKER_M1)
@pytest.mark.parametrize('T', K.ENC_T)
def test_marker_encode_against_long_double(gpu, T, M1):
    K.check_encode(*gpu, T, M1)


def test_marker_encode_heading_beyond_half_pi(gpu):
    K.check_encode(*gpu, 161, 68, wide=True)


def test_marker_encode_refusals_write_nothing(gpu):
    K.check_encode_refusals(*gpu)


@pytest.mark.parametrize('J', K.REC_J)
@pytest.mark.parametrize('T', K.DEC_T)
def test_reconstruct_global_body_against_long_double(gpu, T, J):
    K.check_reconstruct(*gpu, T, J)


def test_reconstruct_global_body_refusals_write_nothing(gpu):
    K.check_reconstruct_refusals(*gpu)


@pytest.mark.parametrize('J', K.DECODE_J)
@pytest.mark.parametrize('T', K.DEC_T)
def test_decode_clip_labels_markers_and_post(gpu, T, J):
    K.check_decode(*gpu, T, J)


def test_decode_clip_refusals_write_nothing(gpu):
    K.check_decode_refusals(*gpu)


@pytest.mark.parametrize('H,W,Cn', K.SMOOTH_SHAPES)
def test_smooth_loss_against_float64(gpu, H, W, Cn):
    K.check_smooth(*gpu, H, W, Cn)


def test_smooth_loss_refusals_write_nothing(gpu):
    K.check_smooth_refusals(*gpu)


@pytest.mark.parametrize('lr', K.ADAM_LR)
@pytest.mark.parametrize('t', K.ADAM_T)
def test_adam_flat_against_torch(gpu, t, lr):
    K.check_adam(*gpu, t, lr)


@pytest.mark.parametrize('t', (1, 999))
def test_adam_flat_ctr_is_adam_flat_at_the_counter(gpu, t):
    K.check_adam_ctr(*gpu, t)


def test_adam_flat_refusals_write_nothing(gpu):
    K.check_adam_refusals(*gpu)


@pytest.mark.parametrize('bs,H,W,gap', K.DEC_END_SHAPES)
def test_dec_end_fwd_against_float64(gpu, bs, H, W, gap):
    K.check_dec_end(*gpu, bs, H, W, gap)


def test_dec_end_fwd_refusals_write_nothing(gpu):
    K.check_dec_end_refusals(*gpu)


def test_zz_error_ratios(gpu):
    """prints the worst measured / bound ratios of the cases above (pytest -s; DESIGN.md quotes them)"""
    K.report_ratios()
