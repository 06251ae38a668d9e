"""Dataset builder on an MI355X: the cases of tests/dataset_checks.py on the product library, and the built tensor handed
to the infilling-prior trainer without leaving the device."""
import pytest
import torch

import dataset_checks as K
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.mark.parametrize('T', [30, 120])
def test_kernel_on_reference_markers_gives_the_reference_images(gpu, T):
    K.check_kernel_vs_fixture(*gpu, T)


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('T,M,N,chunk', K.SHAPES)
def test_kernel_and_statistics_against_the_restatement(gpu, mode, T, M, N, chunk):
    K.check_shape(*gpu, mode, T, M, N, chunk)


def test_layout_is_the_permuted_get_local_markers_4chan(gpu):
    K.check_layout(*gpu)


def test_decode_clip_recovers_the_canonicalised_markers(gpu):
    K.check_round_trip(*gpu)


def test_bad_arguments_raise_before_any_launch(gpu, monkeypatch):
    K.check_validation(*gpu, monkeypatch)


def test_end_to_end_and_two_epoch_steps_from_the_device_tensor(gpu, tmp_path):
    """upload_dataset(images) followed by two fit_epoch steps gives the same log, bit for bit, as the same images uploaded from
    the host; the device tensor is taken as it is"""
    from lemo_amd.infill_train import InfillPriorTrainer
    from train_epoch_common import default_ae_state, same_bits
    lib, dev = gpu
    img = K.check_end_to_end(lib, dev, tmp_path)
    idx = torch.tensor([[0, 3], [2, 1]])
    logs = []
    for data in (img, img.cpu().numpy()):
        tr = InfillPriorTrainer(default_ae_state(41), batch=2, H=img.shape[2] + 2, W=img.shape[3] + 16, lr=1e-3, use_graph=False, device=dev, _lib=lib)
        tr.upload_dataset(data)
        if data is img:
            assert tr._data.data_ptr() == img.data_ptr()
        logs.append(tr.fit_epoch(idx))
        tr.close()
    assert same_bits(logs[0], logs[1])
