"""The GEMM and autoencoder block kernels (gemm_nt16, gemm_nt16_splitk, maxpool3s2, stuff2, conv3x3_wgrad and its two-stage form,
sdf_sample) through their own C entry points on an MI355X: the cases of tests/blocks_common.py on the product library.  That
module's docstring derives every tolerance."""
import pytest
import torch

import blocks_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('epi', K.GEMM_EPIS)
@pytest.mark.parametrize('M,N,Kd', K.GEMM_SHAPES)
def test_gemm_nt16_against_float64(gpu, M, N, Kd, epi):
    K.check_gemm(*gpu, M, N, Kd, epi)


@pytest.mark.parametrize('epi', K.GEMM_EPIS)
def test_gemm_nt16_tight_strides(gpu, epi):
    K.check_gemm(*gpu, 48, 33, 80, epi, tight=True)


def test_gemm_nt16_refusals_write_nothing(gpu):
    K.check_gemm_refusals(*gpu)


@pytest.mark.parametrize('k16,S', K.SPLITK_KS)
@pytest.mark.parametrize('N', K.SPLITK_N)
@pytest.mark.parametrize('M', K.SPLITK_M)
def test_gemm_splitk_against_float64(gpu, M, N, k16, S):
    K.check_splitk(*gpu, M, N, k16, S)


def test_gemm_splitk_refusals_write_nothing(gpu):
    K.check_splitk_refusals(*gpu)


@pytest.mark.parametrize('kind', K.POOL_KINDS)
@pytest.mark.parametrize('H,W', K.POOL_HW)
@pytest.mark.parametrize('Cn', K.POOL_C)
def test_maxpool_forward_and_backward(gpu, Cn, H, W, kind):
    K.check_pool(*gpu, Cn, H, W, kind)


def test_maxpool_refuses_ragged_channels(gpu):
    K.check_pool_refusals(*gpu)


@pytest.mark.parametrize('hw,HW', K.STUFF_CASES)
def test_stuffing_forward_and_backward(gpu, hw, HW):
    K.check_stuff(*gpu, *hw, *HW)


def test_stuffing_refusals_write_nothing(gpu):
    K.check_stuff_refusals(*gpu)


@pytest.mark.parametrize('H,W', K.WGRAD_HW)
@pytest.mark.parametrize('cin,cout,cin_real,cout_real', K.WGRAD_CH)
def test_wgrad_against_float64_and_two_stage_bits(gpu, cin, cout, cin_real, cout_real, H, W):
    K.check_wgrad(*gpu, cin, cout, cin_real, cout_real, H, W)


def test_wgrad_reduce_multi_two_jobs_one_without_bias(gpu):
    K.check_wgrad_multi(*gpu)


def test_wgrad_refusals_write_nothing(gpu):
    K.check_wgrad_refusals(*gpu)


@pytest.mark.parametrize('N', K.SDF_N)
@pytest.mark.parametrize('name', sorted(K.SDF_VOLUMES))
def test_sdf_sample_value_and_gradient(gpu, name, N):
    K.check_sdf(*gpu, name, N)


def test_zz_error_ratios(gpu):
    """prints the worst kernel / restatement error ratios of the cases above (pytest -s; DESIGN.md quotes them)"""
    K.report_ratios()
