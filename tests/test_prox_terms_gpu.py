"""The optional terms of the PROX window engine (lemo_prox_set_terms) on an MI355X: the cases of tests/prox_terms_common.py on the
product library, plus what only the device shows -- graph replay against eager launches and engine against engine, bit for bit.  That
module's docstring derives every tolerance."""
import pytest
import torch

import prox_terms_common as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('which,first', K.PARITY_CASES)
def test_engine_matches_fitter_with_the_term_live(gpu, which, first):
    K.check_parity(*gpu, which, first)


@pytest.mark.parametrize('which', K.SINGLE)
def test_values_and_gradient_share_against_float64(gpu, which):
    K.check_float64(*gpu, which)


def test_graph_replay_and_second_engine_bit_for_bit(gpu):
    K.check_reproducible(*gpu)


def test_engine_without_the_arguments_is_untouched(gpu, monkeypatch):
    K.check_default_untouched(*gpu, monkeypatch)


def test_validation(gpu):
    K.check_validation(*gpu)


def test_nonfinite_scan_point_latches(gpu):
    K.check_nonfinite(*gpu)
