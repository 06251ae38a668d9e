"""The VPoser encoder (lemo_vposer_encode_fwd / _bwd) and the methods built on it (VPoser.encode / forward / sample_poses, embed_body_pose,
with_pose_embedding) on an MI355X: the cases of tests/vposer_enc_common.py, whose docstring derives every tolerance."""
import pytest
import torch

import vposer_enc_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('B,variant', K.FWD_CASES)
def test_encode_forward_against_float64(gpu, B, variant):
    K.check_fwd(*gpu, B, variant)


def test_encode_forward_refusals_write_nothing(gpu):
    K.check_fwd_refusals(*gpu)


@pytest.mark.parametrize('B,which,variant', K.BWD_CASES)
def test_encode_backward_against_float64(gpu, B, which, variant):
    K.check_bwd(*gpu, B, which, variant)


def test_encode_backward_refusals_write_nothing(gpu):
    K.check_bwd_refusals(*gpu)


def test_encode_forward_rows_past_65535(gpu):
    K.check_large(*gpu)


def test_encode_method_shapes_bits_and_autograd(gpu):
    K.check_encode_shapes_and_autograd(*gpu)


def test_encode_refuses_a_cpu_tensor(gpu):
    vp = K.make_vp(*gpu)
    with pytest.raises(_hip.LemoHipError):
        vp.encode(K.poses(3, 1))


def test_loading_another_state_repacks(gpu):
    K.check_repack(*gpu)


def test_forward_with_eps_and_sample_poses(gpu):
    K.check_forward_and_samples(*gpu)


def test_matrot2aa_and_aa2matrot_round_trip(gpu):
    K.check_rotation_helpers(*gpu)


def test_embed_body_pose(gpu):
    K.check_embed(*gpu)


def test_with_pose_embedding_starts_a_window(gpu):
    K.check_with_pose_embedding(gpu[0])


def test_against_the_recorded_reference_run(gpu):
    K.check_reference_run(*gpu)


def test_zz_error_ratios(gpu):
    """prints the worst kernel error / bound ratios of the cases above (pytest -s; DESIGN.md quotes them) and checks that the forward and
    the backward kernel were both launched"""
    K.report_ratios()
