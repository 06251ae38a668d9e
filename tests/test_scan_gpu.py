"""The PROX depth terms on an MI355X: the cases of tests/scan_common.py on the product library, plus the body model's mesh at full
size once.  That module's docstring derives every tolerance."""
import pytest
import torch

import scan_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('name,B', K.VIS_CASES)
def test_visibility_brute_equals_binned_and_float64(gpu, name, B):
    K.check_visibility(*gpu, name, B)


def test_visibility_fallback_and_edge_rules(gpu):
    K.check_fallback(*gpu)


def test_visibility_at_full_size(gpu):
    K.check_full_size(*gpu)


@pytest.mark.parametrize('lattice', [True, False])
@pytest.mark.parametrize('B,N,M', K.MASKED_SHAPES)
def test_masked_nearest(gpu, B, N, M, lattice):
    K.check_masked(*gpu, B, N, M, lattice)


@pytest.mark.parametrize('B,N,M', [(3, 7, 5), (3, 70, 2 * K._L + 7)])
def test_masked_nearest_backward(gpu, B, N, M):
    K.check_masked_backward(*gpu, B, N, M)


@pytest.mark.parametrize('coincide', [False, True])
def test_scan_terms_against_float64(gpu, monkeypatch, coincide):
    K.check_terms(*gpu, monkeypatch, coincide)


def test_prox_fitter_scan_terms(gpu, monkeypatch):
    K.check_prox_fitter(*gpu, monkeypatch)


def test_compat_psbody_visibility(gpu, monkeypatch):
    K.check_compat(*gpu, monkeypatch)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    K.check_validation(*gpu, monkeypatch)
