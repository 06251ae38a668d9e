"""The optional terms of the PROX window engine (lemo_prox_set_terms: contact, s2m / m2s, self-penetration, marker velocity) on the
host emulator: the cases of tests/prox_terms_common.py, whose docstring derives every tolerance."""
import pytest
import torch

import prox_terms_common as K

CPU = torch.device('cpu')
pytestmark = pytest.mark.timeout(1800)


@pytest.mark.parametrize('which,first', K.PARITY_CASES)
def test_engine_matches_fitter_with_the_term_live(emu_lib, which, first):
    K.check_parity(emu_lib, CPU, which, first)


@pytest.mark.parametrize('which', K.SINGLE)
def test_values_and_gradient_share_against_float64(emu_lib, which):
    K.check_float64(emu_lib, CPU, which)


def test_engine_without_the_arguments_is_untouched(emu_lib, monkeypatch):
    K.check_default_untouched(emu_lib, CPU, monkeypatch)


def test_validation(emu_lib):
    K.check_validation(emu_lib, CPU)


def test_terms_struct_layout_matches_the_header():
    K.check_layout()


def test_nonfinite_scan_point_latches(emu_lib):
    K.check_nonfinite(emu_lib, CPU)
