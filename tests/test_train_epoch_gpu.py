"""GPU suite: the loop level of the training engines on an MI355X (tests/train_epoch_common.py has the cases, shared with the
emulator suite): assembly bit for bit against the torch recipes, an epoch (eager and as a replayed graph) against the eager loop
of step() calls it replaces, the checkpoint, and one case of each engine at the shipped image shape."""
import gc
import weakref

import pytest
import torch

import train_epoch_common as E
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    return _hip.get_lib(), torch.device('cuda', 0)


@pytest.fixture(scope='module')
def ae_data():
    return E.ae_clips(), E.prox_masks()


@pytest.mark.parametrize('recipe', ['random', 'prox', 'none'])
def test_ae_assembly_is_the_torch_recipe_bit_for_bit(gpu, ae_data, recipe):
    E.check_ae_assembly(*gpu, recipe, *ae_data)


def test_smoothness_assembly_is_network_input_bit_for_bit(gpu):
    E.check_sp_assembly(*gpu, E.sp_clips())


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('recipe', ['random', 'prox'])
def test_ae_epoch_is_the_loop_it_replaces_and_evaluate_epoch_changes_nothing(gpu, ae_data, recipe, use_graph):
    E.check_ae_epoch_is_the_loop(*gpu, use_graph, recipe, *ae_data)


@pytest.mark.parametrize('use_graph', [False, True])
def test_smoothness_epoch_is_the_loop_it_replaces_and_evaluate_epoch_changes_nothing(gpu, use_graph):
    E.check_sp_epoch_is_the_loop(*gpu, use_graph, E.sp_clips())


@pytest.mark.parametrize('use_graph', [False, True])
def test_ae_checkpoint_resumes_bit_identically(gpu, ae_data, use_graph):
    E.check_ae_checkpoint(*gpu, use_graph, *ae_data)


def test_smoothness_checkpoint_resumes_bit_identically(gpu):
    E.check_sp_checkpoint(*gpu, True, E.sp_clips())


def test_bad_indices_are_refused_on_the_host(gpu):
    E.check_bad_indices_are_refused(*gpu)


def test_close_during_a_capture_parks_the_destroy(gpu, monkeypatch):
    """close() while some stream is being captured (pretended here: no capture is started) must not destroy the engine under it:
    the destroy is parked with the workspace, h is None at once, a second close() does nothing, and the first flush after the
    capture runs the destroy exactly once"""
    lib, dev = gpu
    tr = E.sp_trainer(lib, dev, False)
    torch.cuda.synchronize(dev)
    _hip.flush_deferred()
    destroyed, real = [], lib.sptrain_destroy
    monkeypatch.setattr(lib, 'sptrain_destroy', lambda h: destroyed.append(h) or real(h))
    n0, ws = len(_hip._DEFERRED), weakref.ref(tr.ws)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        tr.close()
        assert destroyed == [] and len(_hip._DEFERRED) == n0 + 1 and tr.h is None
        tr.close()
        assert destroyed == [] and len(_hip._DEFERRED) == n0 + 1
        del tr                                                                   # the trainer goes: the parked destroy holds the workspace
        gc.collect()
        _hip.flush_deferred()                                                    # still "capturing": stays parked
        assert destroyed == [] and len(_hip._DEFERRED) == n0 + 1 and ws() is not None
    _hip.flush_deferred()
    assert len(destroyed) == 1 and len(_hip._DEFERRED) == n0 and ws() is None
    _hip.flush_deferred()
    assert len(destroyed) == 1


def test_a_second_epoch_replays_the_captured_step_with_new_tables(gpu, ae_data):
    """the captured chain carries none of the caller's pointers: a second fit_epoch with another index table, another recipe
    and a fresh log equals an eager trainer's"""
    clips, masks = ae_data
    a = E.ae_trainer(*gpu, True, clips=clips, masks=masks)
    b = E.ae_trainer(*gpu, False, clips=clips, masks=masks)
    for tr in (a, b):
        tr.first = tr.fit_epoch(E.AE_IDX[:2], marker_ids=E.AE_IDS[:2])
        tr.second = tr.fit_epoch(E.AE_IDX[2:4], mask_idx=E.AE_MASK_IDX[2:4])
    assert E.same_bits(a.first, b.first) and E.same_bits(a.second, b.second) and E.same_bits(a.flat_params(), b.flat_params())
    a.close()
    b.close()


def test_ae_at_the_shipped_shape(gpu):
    """bs = 4, 208 x 119 clips (network 210 x 135): the assembly for both recipes and a 2-step fit_epoch == loop"""
    clips, masks = E.ae_clips(n=6, t=119, seed=61), E.prox_masks(L=120, seed=62)
    g = torch.Generator().manual_seed(63)
    idx = torch.tensor([[5, 0, 3, 2], [1, 5, 0, 4]])
    ids = (torch.rand(2, 4, 6, generator=g) * 68).long() - 1            # -1 .. 66
    ids[0, 0, 0], ids[1, 2, 3] = 16, 47
    mi = torch.tensor([[2, 0, 1, 1], [0, 2, 2, 1]])
    kw = dict(bs=4, idx=idx, ids=ids, mask_idx=mi, steps=(0, 1))
    E.check_ae_assembly(*gpu, 'random', clips, masks, **kw)
    E.check_ae_assembly(*gpu, 'prox', clips, masks, **kw)
    E.check_ae_epoch_is_the_loop(*gpu, True, 'random', clips, masks, with_eval=False, **kw)


def test_smoothness_at_the_shipped_shape(gpu):
    """bs = 2, 243 x 120 clips (network 245 x 135)"""
    clips = E.sp_clips(n=4, d=243, t=120, seed=64)
    idx = torch.tensor([[3, 0], [1, 3]])
    E.check_sp_assembly(*gpu, clips, steps=(0, 1), idx=idx)
    E.check_sp_epoch_is_the_loop(*gpu, True, clips, steps=(0, 1), with_eval=False, idx=idx)
