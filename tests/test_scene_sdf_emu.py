"""Scene mesh -> signed-distance volume (lemo_amd.scene.build_scene_sdf: csrc/scene_sdf_kernels.hip) on the host emulator: the cases of
tests/scene_sdf_common.py, whose docstring derives every tolerance."""
import pytest
import torch

import scene_sdf_common as K

CPU = torch.device('cpu')


def test_yardstick_conditions_hold_in_float64():
    """the cases themselves: few excused voxels, enough negative ones, and the box agrees with its closed form"""
    K.check_yardstick_conditions()


@pytest.mark.parametrize('name', K.CASES)
def test_modes_identical_and_float64(emu_lib, name):
    K.check_case(emu_lib, CPU, name)


def test_edge_rules(emu_lib):
    K.check_edge_rules(emu_lib, CPU)


def test_sampler_returns_the_volume_at_its_centres(emu_lib):
    K.check_sampler(emu_lib, CPU)


def test_prox_files_round_trip(emu_lib, tmp_path):
    K.check_files(emu_lib, CPU, tmp_path)


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    K.check_validation(emu_lib, CPU, monkeypatch)
