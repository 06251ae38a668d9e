"""The self-penetration term (lemo_amd.selfpen: csrc/selfpen_kernels.hip) on the host emulator: the cases of tests/selfpen_common.py,
whose docstring derives every tolerance."""
import pytest
import torch

import selfpen_common as K

CPU = torch.device('cpu')


def test_yardstick_conditions_hold_in_float64():
    """the cases themselves: enough colliding pairs, few excused ones, and the float32 restatement agrees outside the excuse set"""
    for name, B in K.MESH_CASES:
        verts, f = K.sp_case(name, B)
        for b, (strict, loose, plain) in enumerate(K.reference(name, B)):
            assert len(plain) >= K.MIN_PAIRS and len(strict ^ loose) <= K.EXCUSE_CAP * len(plain), (name, b, len(plain), len(strict ^ loose))
            assert not ((K.collide32(verts[b], f) ^ plain) - (strict ^ loose))


@pytest.mark.parametrize('name,B', K.MESH_CASES)
def test_search_modes_identical_and_float64(emu_lib, name, B):
    K.check_search(emu_lib, CPU, name, B)


def test_search_closed_form_pairs(emu_lib):
    K.check_closed_form(emu_lib, CPU)


def test_search_capacity_keeps_the_first_pairs(emu_lib):
    K.check_capacity(emu_lib, CPU)


def test_search_part_filter(emu_lib):
    K.check_filter(emu_lib, CPU)


@pytest.mark.parametrize('outside', [True, False])
@pytest.mark.parametrize('sigma', K.SIGMAS)
@pytest.mark.parametrize('name,B', K.LOSS_CASES)
def test_loss_against_float64(emu_lib, name, B, sigma, outside):
    K.check_loss(emu_lib, CPU, name, B, sigma, outside)


def test_loss_edge_rules(emu_lib):
    K.check_loss_edges(emu_lib, CPU)


def test_self_penetration_term(emu_lib):
    K.check_term(emu_lib, CPU)


def test_prox_fitter_selfpen_and_smooth_terms(emu_lib, monkeypatch):
    K.check_prox_fitter(emu_lib, CPU, monkeypatch)


def test_compat_mesh_intersection(emu_lib, monkeypatch):
    K.check_compat(emu_lib, CPU, monkeypatch)


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    K.check_validation(emu_lib, CPU, monkeypatch)
