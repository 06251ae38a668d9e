"""Body overlays (lemo_amd.render, csrc/render_kernels.hip) on the host emulator: the small cases of tests/render_common.py.  The
yardstick is that module's numpy restatement of the documented rule, in float64 and float32; no pyrender fixture exists."""
import pytest
import torch

import render_common as R

CPU = torch.device('cpu')


@pytest.mark.parametrize('cull', [False, True])
@pytest.mark.parametrize('name', R.SOUPS)
@pytest.mark.parametrize('W,H', R.SIZES)
def test_triangle_soups_against_the_restatement(emu_lib, W, H, name, cull):
    R.check_render(emu_lib, CPU, name, W, H, cull)


@pytest.mark.parametrize('rings,segs,W,H', R.SPHERES)
def test_smooth_spheres_against_the_restatement(emu_lib, rings, segs, W, H):
    R.check_render(emu_lib, CPU, f'S{rings}x{segs}', W, H, True)


@pytest.mark.parametrize('rings,segs,W,H', R.SPHERES)
def test_vertex_normals(emu_lib, rings, segs, W, H):
    R.check_normals(emu_lib, CPU, rings, segs, W, H)


@pytest.mark.parametrize('name', ['F300', 'full', 'near', 'S24x32'])
def test_result_does_not_depend_on_face_order(emu_lib, name):
    R.check_permuted_faces(emu_lib, CPU, name, 67, 45)


@pytest.mark.parametrize('W,H', R.SIZES)
def test_background(emu_lib, W, H):
    R.check_background(emu_lib, CPU, W, H)


@pytest.mark.parametrize('radius', [0, 2, 3])
@pytest.mark.parametrize('W,H', R.SIZES)
def test_points(emu_lib, W, H, radius):
    R.check_points(emu_lib, CPU, W, H, radius)


def test_prox_window_to_one_overlay_image(emu_lib):
    R.check_hand_over(emu_lib, CPU, n=1)                      # one 1920 x 1080 frame of the window; the GPU suite renders all 14


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    R.check_validation(emu_lib, CPU, monkeypatch)
