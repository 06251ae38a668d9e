"""Occlusion masks (lemo_amd.occlusion, csrc/occlusion_kernels.hip) on the host emulator: the small cases of
tests/occlusion_common.py.  The yardstick is that module's float64 restatement; no pyrender fixture exists (see its docstring)."""
import pytest
import torch

import occlusion_common as O

CPU = torch.device('cpu')


@pytest.mark.parametrize('moved', [False, True])
@pytest.mark.parametrize('cull', [False, True])
@pytest.mark.parametrize('name', O.RASTER_MESHES)
@pytest.mark.parametrize('W,H', O.RASTER_SIZES)
def test_raster_against_the_restatement(emu_lib, W, H, name, cull, moved):
    O.check_raster(emu_lib, CPU, name, W, H, cull, moved)


@pytest.mark.parametrize('name', ['F300', 'full', 'near'])
def test_raster_is_independent_of_run_and_face_order(emu_lib, name):
    O.check_raster_independence(emu_lib, CPU, name, 67, 45)


@pytest.mark.parametrize('F', [1, 65, 300])
@pytest.mark.parametrize('P', [1, 25, 67, 92])
@pytest.mark.parametrize('T', [1, 3, 70])
def test_query_against_the_restatement(emu_lib, T, P, F):
    O.check_query(emu_lib, CPU, T, P, F)


def test_query_on_designed_geometry(emu_lib):
    O.check_query_designed(emu_lib, CPU)


def test_query_depth_is_the_rendered_body_depth(emu_lib):
    O.check_query_equals_raster(emu_lib, CPU)


def test_mask_drives_a_prox_window_and_the_trainer_loader(emu_lib, tmp_path):
    O.check_hand_over(emu_lib, CPU, tmp_path, full=False, B=16)           # the GPU suite runs the [100, 67] window


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    O.check_validation(emu_lib, CPU, monkeypatch)
