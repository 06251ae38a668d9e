"""The body-model kernels (lbs_verts_fwd in its four forms, lbs_verts_fwd_active, every route of lbs_verts_bwd, smplx_pose_fwd / _bwd,
joints_assemble, the 6-D -> axis-angle head, the rotation part of vposer_decode) through their own C entry points on an MI355X: the cases of tests/lbs_common.py, whose docstring
derives every tolerance."""
import pytest
import torch

import lbs_common as L
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('form,V,n,nj,KW,B,transl,vp', L.FWD_CASES)
def test_lbs_forward_against_float64(gpu, form, V, n, nj, KW, B, transl, vp):
    L.check_fwd(*gpu, form, V, n, nj, KW, B, transl, vp)


@pytest.mark.parametrize('V,nj,KW,B', L.BITS_CASES)
def test_lbs_forward_presplit_and_subset_bits(gpu, V, nj, KW, B):
    L.check_fwd_bits(*gpu, V, nj, KW, B)


def test_lbs_forward_refusals_write_nothing(gpu):
    L.check_fwd_refusals(*gpu)


@pytest.mark.parametrize('n,B,KW', L.ACTIVE_CASES)
def test_lbs_forward_over_a_set_against_float64(gpu, n, B, KW):
    L.check_active(*gpu, n, B, KW, with_transl=B != 17, want_vp=B != 1)


def test_lbs_forward_over_a_set_refusals_write_nothing(gpu):
    L.check_active_refusals(*gpu)


@pytest.mark.parametrize('name', sorted(L.BWD_CASES))
def test_lbs_backward_route_against_float64(gpu, name):
    L.check_bwd(*gpu, name)


def test_lbs_backward_refusals_write_nothing(gpu):
    L.check_bwd_refusals(*gpu)


@pytest.mark.parametrize('nj,n_extra,n_lmk,transl', L.JOINT_CASES)
def test_joints_assemble(gpu, nj, n_extra, n_lmk, transl):
    L.check_joints(*gpu, nj, n_extra, n_lmk, transl)


@pytest.mark.parametrize('N', L.ROT_N)
def test_rot6d_to_axis_angle_against_float64(gpu, N):
    L.check_rot6d(*gpu, N)


@pytest.mark.parametrize('B,ncomp,expr,form', L.POSE_CASES)
def test_pose_stage_forward_against_float64(gpu, B, ncomp, expr, form):
    L.check_pose_fwd(*gpu, B, ncomp, expr, form)


@pytest.mark.parametrize('B', (1, 33))
def test_pose_stage_fused_producers_give_the_same_bits(gpu, B):
    L.check_pose_fused_producers(*gpu, B)


@pytest.mark.parametrize('B,ncomp,expr,dfp', L.POSE_BWD_CASES)
def test_pose_stage_backward_against_float64(gpu, B, ncomp, expr, dfp):
    L.check_pose_bwd(*gpu, B, ncomp, expr, dfp)


@pytest.mark.parametrize('B', L.VPOSER_B)
def test_vposer_decode_rotation_part_against_float64(gpu, B):
    L.check_vposer_rot(*gpu, B)


def test_presplit_blend_operand_is_bit_identical(gpu):
    L.check_presplit_blend_bits(*gpu)


def test_f16_presplit_blend_is_fp32_sized(gpu):
    L.check_f16_presplit_blend(*gpu)


def test_zz_error_ratios(gpu):
    """prints the worst kernel / restatement error ratios of the cases above (pytest -s; DESIGN.md quotes them) and checks that every
    forward form and every backward route was launched"""
    L.report_lbs_ratios()
