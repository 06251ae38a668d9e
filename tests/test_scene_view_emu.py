"""Scene views (lemo_amd.scene_view, csrc/view_kernels.hip) on the host emulator: the small cases of tests/scene_view_common.py.  The
yardstick is that module's numpy restatement of the documented rules, in float64 and float32; no pyrender or open3d fixture exists."""
import pytest
import torch

import scene_view_common as S

CPU = torch.device('cpu')


@pytest.mark.parametrize('cull', [False, True])
@pytest.mark.parametrize('lit,colored', [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize('W,H', S.SIZES)
def test_layers_against_the_restatement(emu_lib, W, H, lit, colored, cull):
    S.check_layers(emu_lib, CPU, W, H, cull, lit, colored)


@pytest.mark.parametrize('P', [1, 5, 130])
@pytest.mark.parametrize('W,H', S.SIZES)
def test_spheres_against_the_restatement(emu_lib, W, H, P):
    S.check_spheres(emu_lib, CPU, W, H, P)


@pytest.mark.parametrize('W,H', S.SIZES)
def test_body_alone_is_the_body_renderer(emu_lib, W, H):
    S.check_body_only(emu_lib, CPU, W, H)


@pytest.mark.parametrize('W,H', S.SIZES)
def test_depth_owner_and_chunk_anchors(emu_lib, W, H):
    S.check_anchors(emu_lib, CPU, W, H)


def test_result_does_not_depend_on_scene_face_or_sphere_order(emu_lib):
    S.check_permutations(emu_lib, CPU, 67, 45)


def test_look_at():
    S.check_look_at()


@pytest.mark.parametrize('W,H', S.SIZES)
def test_set_view_and_scene_transform(emu_lib, W, H):
    S.check_set_view(emu_lib, CPU, W, H)


def test_load_ply(tmp_path):
    S.check_load_ply(tmp_path)


def test_prox_window_to_one_scene_view_image(emu_lib):
    S.check_hand_over(emu_lib, CPU, n=1)                      # one 1920 x 1080 frame of the window; the GPU suite renders all 14


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    S.check_validation(emu_lib, CPU, monkeypatch)
