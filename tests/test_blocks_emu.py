"""The GEMM and autoencoder block kernels (gemm_nt16, gemm_nt16_splitk, maxpool3s2, stuff2, conv3x3_wgrad and its two-stage form,
sdf_sample) through their own C entry points on the host emulator: the cases of tests/blocks_common.py, whose docstring derives
every tolerance."""
import pytest
import torch

import blocks_common as K

CPU = torch.device('cpu')


@pytest.mark.parametrize('epi', K.GEMM_EPIS)
@pytest.mark.parametrize('M,N,Kd', K.GEMM_SHAPES)
def test_gemm_nt16_against_float64(emu_lib, M, N, Kd, epi):
    K.check_gemm(emu_lib, CPU, M, N, Kd, epi)


@pytest.mark.parametrize('epi', K.GEMM_EPIS)
def test_gemm_nt16_tight_strides(emu_lib, epi):
    K.check_gemm(emu_lib, CPU, 48, 33, 80, epi, tight=True)


def test_gemm_nt16_refusals_write_nothing(emu_lib):
    K.check_gemm_refusals(emu_lib, CPU)


@pytest.mark.parametrize('k16,S', K.SPLITK_KS)
@pytest.mark.parametrize('N', K.SPLITK_N)
@pytest.mark.parametrize('M', K.SPLITK_M)
def test_gemm_splitk_against_float64(emu_lib, M, N, k16, S):
    K.check_splitk(emu_lib, CPU, M, N, k16, S)


def test_gemm_splitk_refusals_write_nothing(emu_lib):
    K.check_splitk_refusals(emu_lib, CPU)


@pytest.mark.parametrize('kind', K.POOL_KINDS)
@pytest.mark.parametrize('H,W', K.POOL_HW)
@pytest.mark.parametrize('Cn', K.POOL_C)
def test_maxpool_forward_and_backward(emu_lib, Cn, H, W, kind):
    K.check_pool(emu_lib, CPU, Cn, H, W, kind)


def test_maxpool_refuses_ragged_channels(emu_lib):
    K.check_pool_refusals(emu_lib, CPU)


@pytest.mark.parametrize('hw,HW', K.STUFF_CASES)
def test_stuffing_forward_and_backward(emu_lib, hw, HW):
    K.check_stuff(emu_lib, CPU, *hw, *HW)


def test_stuffing_refusals_write_nothing(emu_lib):
    K.check_stuff_refusals(emu_lib, CPU)


@pytest.mark.parametrize('H,W', K.WGRAD_HW)
@pytest.mark.parametrize('cin,cout,cin_real,cout_real', K.WGRAD_CH)
def test_wgrad_against_float64_and_two_stage_bits(emu_lib, cin, cout, cin_real, cout_real, H, W):
    K.check_wgrad(emu_lib, CPU, cin, cout, cin_real, cout_real, H, W)


def test_wgrad_reduce_multi_two_jobs_one_without_bias(emu_lib):
    K.check_wgrad_multi(emu_lib, CPU)


def test_wgrad_refusals_write_nothing(emu_lib):
    K.check_wgrad_refusals(emu_lib, CPU)


@pytest.mark.parametrize('N', K.SDF_N)
@pytest.mark.parametrize('name', sorted(K.SDF_VOLUMES))
def test_sdf_sample_value_and_gradient(emu_lib, name, N):
    K.check_sdf(emu_lib, CPU, name, N)


def test_zz_error_ratios(emu_lib):
    """prints the worst kernel / restatement error ratios of the cases above (pytest -s; DESIGN.md quotes them)"""
    K.report_ratios()
