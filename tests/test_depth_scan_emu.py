"""Depth frames to body scans (lemo_amd.depth: csrc/depth_scan_kernels.hip) on the host emulator: the cases of
tests/depth_scan_common.py, whose docstring derives every tolerance."""
import pytest
import torch

import depth_scan_common as K

CPU = torch.device('cpu')


@pytest.mark.parametrize('name', list(K.SHAPES))
def test_ray_table_and_rotation_against_the_restatement(emu_lib, name):
    K.check_host_constants(emu_lib, CPU, name)


@pytest.mark.parametrize('coord', ['color', None])
@pytest.mark.parametrize('mask_on_color', [True, False])
@pytest.mark.parametrize('name', K.SMALL)
def test_create_scan_against_float64_and_own_pixels(emu_lib, name, mask_on_color, coord):
    K.check_case(emu_lib, CPU, name, mask_on_color, coord)


def test_create_scan_at_the_prox_size(emu_lib):
    K.check_case(emu_lib, CPU, 'full', True, 'color')


@pytest.mark.parametrize('flip', [False, True])
def test_raw_uint16_depth(emu_lib, flip):
    K.check_raw(emu_lib, CPU, flip)


def test_scan_feeds_scan_terms(emu_lib):
    K.check_round_trip(emu_lib, CPU)


def test_projection_drop_in(emu_lib):
    K.check_drop_in(emu_lib, CPU)


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    K.check_refusals(emu_lib, CPU, monkeypatch)
