"""The body-model kernels (lbs_verts_fwd in its four forms, lbs_verts_fwd_active, every route of lbs_verts_bwd, smplx_pose_fwd / _bwd,
joints_assemble, the 6-D -> axis-angle head, the rotation part of vposer_decode) through their own C entry points on the host emulator: the cases of tests/lbs_common.py, whose docstring
derives every tolerance."""
import pytest
import torch

import lbs_common as L

CPU = torch.device('cpu')


def test_presplit_layouts_resum_to_the_features():
    L.check_xgs_layouts()


@pytest.mark.parametrize('form,V,n,nj,KW,B,transl,vp', L.FWD_CASES)
def test_lbs_forward_against_float64(emu_lib, form, V, n, nj, KW, B, transl, vp):
    L.check_fwd(emu_lib, CPU, form, V, n, nj, KW, B, transl, vp)


@pytest.mark.parametrize('V,nj,KW,B', L.BITS_CASES)
def test_lbs_forward_presplit_and_subset_bits(emu_lib, V, nj, KW, B):
    L.check_fwd_bits(emu_lib, CPU, V, nj, KW, B)


def test_lbs_forward_refusals_write_nothing(emu_lib):
    L.check_fwd_refusals(emu_lib, CPU)


@pytest.mark.parametrize('n,B,KW', L.ACTIVE_CASES)
def test_lbs_forward_over_a_set_against_float64(emu_lib, n, B, KW):
    L.check_active(emu_lib, CPU, n, B, KW, with_transl=B != 17, want_vp=B != 1)


def test_lbs_forward_over_a_set_refusals_write_nothing(emu_lib):
    L.check_active_refusals(emu_lib, CPU)


@pytest.mark.parametrize('name', sorted(L.BWD_CASES))
def test_lbs_backward_route_against_float64(emu_lib, name):
    L.check_bwd(emu_lib, CPU, name)


def test_lbs_backward_refusals_write_nothing(emu_lib):
    L.check_bwd_refusals(emu_lib, CPU)


@pytest.mark.parametrize('nj,n_extra,n_lmk,transl', L.JOINT_CASES)
def test_joints_assemble(emu_lib, nj, n_extra, n_lmk, transl):
    L.check_joints(emu_lib, CPU, nj, n_extra, n_lmk, transl)


@pytest.mark.parametrize('N', L.ROT_N)
def test_rot6d_to_axis_angle_against_float64(emu_lib, N):
    L.check_rot6d(emu_lib, CPU, N)


@pytest.mark.parametrize('B,ncomp,expr,form', L.POSE_CASES)
def test_pose_stage_forward_against_float64(emu_lib, B, ncomp, expr, form):
    L.check_pose_fwd(emu_lib, CPU, B, ncomp, expr, form)


@pytest.mark.parametrize('B', (1, 33))
def test_pose_stage_fused_producers_give_the_same_bits(emu_lib, B):
    L.check_pose_fused_producers(emu_lib, CPU, B)


@pytest.mark.parametrize('B,ncomp,expr,dfp', L.POSE_BWD_CASES)
def test_pose_stage_backward_against_float64(emu_lib, B, ncomp, expr, dfp):
    L.check_pose_bwd(emu_lib, CPU, B, ncomp, expr, dfp)


@pytest.mark.parametrize('B', L.VPOSER_B)
def test_vposer_decode_rotation_part_against_float64(emu_lib, B):
    L.check_vposer_rot(emu_lib, CPU, B)


def test_presplit_blend_operand_is_bit_identical(emu_lib):
    L.check_presplit_blend_bits(emu_lib, CPU)


def test_f16_presplit_blend_is_fp32_sized(emu_lib):
    L.check_f16_presplit_blend(emu_lib, CPU)


def test_zz_error_ratios(emu_lib):
    """prints the worst kernel / restatement error ratios of the cases above (pytest -s; DESIGN.md quotes them) and checks that every
    forward form and every backward route was launched"""
    L.report_lbs_ratios()
