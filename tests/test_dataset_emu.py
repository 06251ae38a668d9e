"""Dataset builder (lemo_amd/dataset.py, csrc/dataset_kernels.hip) on the host emulator: the cases of tests/dataset_checks.py."""
import pytest
import torch

import dataset_checks as K

CPU = torch.device('cpu')


def test_restatement_is_held_to_the_reference_fixture():
    K.check_restatement_is_the_reference()


@pytest.mark.parametrize('T', [30, 120])
def test_kernel_on_reference_markers_gives_the_reference_images(emu_lib, T):
    K.check_kernel_vs_fixture(emu_lib, CPU, T)


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('T,M,N,chunk', K.SHAPES)
def test_kernel_and_statistics_against_the_restatement(emu_lib, mode, T, M, N, chunk):
    K.check_shape(emu_lib, CPU, mode, T, M, N, chunk)


def test_layout_is_the_permuted_get_local_markers_4chan(emu_lib):
    K.check_layout(emu_lib, CPU)


def test_decode_clip_recovers_the_canonicalised_markers(emu_lib):
    K.check_round_trip(emu_lib, CPU)


def test_end_to_end_from_amass_parameters(emu_lib, tmp_path):
    K.check_end_to_end(emu_lib, CPU, tmp_path)


def test_divide_clips_is_the_reference_rule(tmp_path):
    K.check_divide_clips(tmp_path)


def test_bad_arguments_raise_before_any_launch(emu_lib, monkeypatch):
    K.check_validation(emu_lib, CPU, monkeypatch)


def test_trainers_take_the_built_tensor_without_a_copy(emu_lib):
    from lemo_amd.infill_train import InfillPriorTrainer
    from train_epoch_common import default_ae_state
    img = torch.zeros(3, 4, 208, 29)
    tr = InfillPriorTrainer(default_ae_state(1), batch=2, H=210, W=45, use_graph=False, device=CPU, _lib=emu_lib)
    tr.upload_dataset(img)
    assert tr._data.data_ptr() == img.data_ptr()
    tr.close()
    from train_epoch_common import sp_trainer
    img = torch.zeros(3, 1, 204, 30)
    tr = sp_trainer(emu_lib, CPU, False, bs=2, d=204, t=30)
    tr.upload_dataset(img)
    assert tr._data.data_ptr() == img.data_ptr()
    tr.close()
