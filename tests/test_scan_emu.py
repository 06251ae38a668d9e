"""The PROX depth terms (lemo_amd.scan: csrc/visibility_kernels.hip, lemo_chamfer_masked_forward) on the host emulator: the cases of
tests/scan_common.py, whose docstring derives every tolerance."""
import pytest
import torch

import scan_common as K

CPU = torch.device('cpu')


def test_body_mask_fixture():
    m = K.body_mask_golden()
    assert m.shape == (10475,) and int(m.sum()) == 10475 - 5023


@pytest.mark.parametrize('name,B', K.VIS_CASES)
def test_visibility_brute_equals_binned_and_float64(emu_lib, name, B):
    K.check_visibility(emu_lib, CPU, name, B)


def test_visibility_fallback_and_edge_rules(emu_lib):
    K.check_fallback(emu_lib, CPU)


@pytest.mark.parametrize('lattice', [True, False])
@pytest.mark.parametrize('B,N,M', K.MASKED_SHAPES)
def test_masked_nearest(emu_lib, B, N, M, lattice):
    K.check_masked(emu_lib, CPU, B, N, M, lattice)


@pytest.mark.parametrize('B,N,M', [(3, 7, 5), (3, 70, 2 * K._L + 7)])
def test_masked_nearest_backward(emu_lib, B, N, M):
    K.check_masked_backward(emu_lib, CPU, B, N, M)


@pytest.mark.parametrize('coincide', [False, True])
def test_scan_terms_against_float64(emu_lib, monkeypatch, coincide):
    K.check_terms(emu_lib, CPU, monkeypatch, coincide)


def test_prox_fitter_scan_terms(emu_lib, monkeypatch):
    K.check_prox_fitter(emu_lib, CPU, monkeypatch)


def test_compat_psbody_visibility(emu_lib, monkeypatch):
    K.check_compat(emu_lib, CPU, monkeypatch)


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    K.check_validation(emu_lib, CPU, monkeypatch)
