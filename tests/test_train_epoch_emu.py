"""CPU suite: the loop level of the training engines on the host emulator (tests/train_epoch_common.py has the cases): the batch
assembly against the torch recipes bit for bit, an epoch against the loop of step() calls it replaces, the training-state
checkpoint, and the argument rules of the new C entries."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

import train_epoch_common as E
from lemo_amd import _hip
from lemo_amd._hip import ptr

CPU = torch.device('cpu')
ERR_SHAPE, ERR_ARG, ERR_STATE = 10001, 10002, 10003


@pytest.fixture(scope='module')
def ae_data():
    return E.ae_clips(), E.prox_masks()


@pytest.mark.parametrize('recipe', ['random', 'prox', 'none'])
def test_ae_assembly_is_the_torch_recipe_bit_for_bit(emu_lib, ae_data, recipe):
    E.check_ae_assembly(emu_lib, CPU, recipe, *ae_data)


def test_smoothness_assembly_is_network_input_bit_for_bit(emu_lib):
    E.check_sp_assembly(emu_lib, CPU, E.sp_clips())


@pytest.mark.parametrize('recipe', ['random', 'prox'])
def test_ae_epoch_is_the_loop_it_replaces_and_evaluate_epoch_changes_nothing(emu_lib, ae_data, recipe):
    E.check_ae_epoch_is_the_loop(emu_lib, CPU, False, recipe, *ae_data, with_eval=recipe == 'random')


def test_smoothness_epoch_is_the_loop_it_replaces_and_evaluate_epoch_changes_nothing(emu_lib):
    E.check_sp_epoch_is_the_loop(emu_lib, CPU, False, E.sp_clips())


def test_ae_checkpoint_resumes_bit_identically(emu_lib, ae_data):
    E.check_ae_checkpoint(emu_lib, CPU, False, *ae_data)


def test_smoothness_checkpoint_resumes_bit_identically(emu_lib):
    E.check_sp_checkpoint(emu_lib, CPU, False, E.sp_clips())


def test_bad_indices_are_refused_on_the_host(emu_lib):
    E.check_bad_indices_are_refused(emu_lib, CPU)


def test_smoothness_trainer_refuses_bad_index_tables_before_any_launch(emu_lib, monkeypatch):
    """float, bool, wrong-rank, wrong-width, empty and out-of-range idx raise ValueError from the trainers' shared _index_table, with
    its messages, and neither lemo_sptrain_epoch nor lemo_sptrain_batch has been called by then"""
    from lemo_amd._engine import PriorTrainer
    from lemo_amd.infill_train import InfillPriorTrainer
    from lemo_amd.smooth_train import SmoothPriorTrainer
    assert SmoothPriorTrainer._index_table is PriorTrainer._index_table is InfillPriorTrainer._index_table
    st = E.sp_trainer(emu_lib, CPU, False, clips=E.sp_clips())
    calls = []
    for name in ('sptrain_epoch', 'sptrain_batch'):
        monkeypatch.setattr(emu_lib, name, lambda *a, _n=name: calls.append(_n) or 0)
    ok = E.SP_IDX[:2]
    high, low = ok.clone(), ok.clone()
    high[1, 0], low[0, 1] = E.SP_N, -1
    cases = ((ok.float(), 'idx must be an integer tensor'), (ok.double().numpy(), 'idx must be an integer tensor'),
             (ok > 0, 'idx must be an integer tensor'), (ok[0], f'idx: expected [n_steps, {E.SP_BS}], got (2,)'),
             (ok[:, :, None], f'idx: expected [n_steps, {E.SP_BS}], got (2, 2, 1)'), (ok[:, :1], f'idx: expected [n_steps, {E.SP_BS}], got (2, 1)'),
             (ok[:0], f'idx: expected [n_steps, {E.SP_BS}], got (0, 2)'), (high, f'idx holds values outside [0, {E.SP_N})'),
             (low, f'idx holds values outside [0, {E.SP_N})'))
    for fn in (st.fit_epoch, st.evaluate_epoch, lambda i: st.assemble(0, i)):
        for arg, msg in cases:
            with pytest.raises(ValueError) as err:
                fn(arg)
            assert str(err.value) == msg
    with pytest.raises(ValueError):
        st.assemble(2, ok)                                                       # a good table, a step past its end
    assert calls == []
    monkeypatch.undo()
    assert st.fit_epoch(ok.int().numpy()).shape == (2, 3)                        # a good table in another integer type still runs
    st.close()


def test_upload_prox_masks_takes_both_layouts(emu_lib, ae_data):
    clips, masks = ae_data
    tr = E.ae_trainer(emu_lib, CPU, False, clips=clips)
    tr.upload_prox_masks(masks)
    a = tr._masks.clone()
    tr.upload_prox_masks(masks[:, :, ::3])
    assert a.shape == (3, 67, E.MASK_L) and torch.equal(a, tr._masks)
    tr.close()


def test_engine_argument_and_state_errors(emu_lib):
    lib = emu_lib
    H, W, bs = E.AE_D + 2, E.AE_T + 16, 1
    n = int(lib.aetrain_ws_floats(H, W, bs))
    ws = torch.zeros(n)
    d = _hip.AetrainDesc(H=H, W=W, bs=bs, lr=1e-4, w_body=10., w_v=10., w_c=1., ws=ptr(ws), ws_floats=n, use_graph=0)
    h = lib.aetrain_create(C.byref(d))
    data, idx, log = torch.zeros(2, 4, E.AE_D, E.AE_T), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 4)
    ids, masks = torch.full((1, 1, 6), -1, dtype=torch.int32), torch.ones(1, 67, E.AE_T)
    x, y = torch.zeros(1, 4, H, W), torch.zeros(1, H, W)
    blob = torch.zeros(int(lib.aetrain_state_floats()))

    def desc(**kw):
        base = dict(data=ptr(data), n_clips=2, idx=ptr(idx), n_steps=1, recipe=_hip.MASK_NONE, log=ptr(log), train=1)
        base.update(kw)
        return C.byref(_hip.AetrainEpochDesc(**base))
    try:
        assert lib.aetrain_epoch(h, desc(), None) == ERR_STATE
        assert lib.aetrain_state_save(h, ptr(blob), None) == ERR_STATE
        assert lib.aetrain_epoch(h, None, None) == ERR_ARG
        assert lib.aetrain_epoch(None, desc(), None) == ERR_ARG
        for bad in (dict(data=None), dict(idx=None), dict(log=None), dict(n_clips=0), dict(n_steps=0), dict(recipe=3),
                    dict(recipe=_hip.MASK_RANDOM), dict(recipe=_hip.MASK_PROX, masks=ptr(masks), n_masks=1, mask_len=E.AE_T),
                    dict(recipe=_hip.MASK_PROX, masks=ptr(masks), n_masks=1, mask_len=E.AE_T - 1, mask_idx=ptr(idx)),
                    dict(recipe=_hip.MASK_PROX, masks=ptr(masks), n_masks=0, mask_len=E.AE_T, mask_idx=ptr(idx))):
            assert lib.aetrain_epoch(h, desc(**bad), None) == ERR_ARG, bad
        assert lib.aetrain_batch(h, desc(), 1, ptr(x), ptr(y), None) == ERR_ARG          # step outside the table
        assert lib.aetrain_batch(h, desc(), -1, ptr(x), ptr(y), None) == ERR_ARG
        assert lib.aetrain_batch(h, desc(), 0, None, ptr(y), None) == ERR_ARG
        assert lib.aetrain_batch(h, desc(recipe=_hip.MASK_RANDOM, marker_ids=ptr(ids)), 0, ptr(x), ptr(y), None) == 0
        assert lib.aetrain_state_save(h, None, None) == ERR_ARG and lib.aetrain_state_load(h, None, None) == ERR_ARG
        assert lib.aetrain_state_load(h, ptr(blob), None) == 0                           # a state load is a load
        assert lib.aetrain_state_save(h, ptr(blob), None) == 0
    finally:
        lib.aetrain_destroy(h)
    # the masking recipes are defined for d = 208 only; clips too short to reflect-pad by 8 are a shape error
    for hh, ww, recipe, want in ((20, 28, _hip.MASK_RANDOM, ERR_ARG), (20, 24, _hip.MASK_NONE, ERR_SHAPE)):
        n = int(lib.aetrain_ws_floats(hh, ww, 1))
        ws2 = torch.zeros(n)
        d2 = _hip.AetrainDesc(H=hh, W=ww, bs=1, lr=1e-4, w_body=10., w_v=10., w_c=1., ws=ptr(ws2), ws_floats=n, use_graph=0)
        h2 = lib.aetrain_create(C.byref(d2))
        try:
            assert lib.aetrain_batch(h2, desc(recipe=recipe, marker_ids=ptr(ids)), 0, ptr(x), ptr(y), None) == want
        finally:
            lib.aetrain_destroy(h2)
    # smoothness engine
    Hs, Wsp = E.SP_D + 2, E.SP_T + 15
    n = int(lib.sptrain_ws_floats(Hs, Wsp, 1))
    ws3 = torch.zeros(n)
    d3 = _hip.SptrainDesc(H=Hs, W=Wsp, bs=1, lr=1e-4, weight_rec=1., weight_smooth=1000., ws=ptr(ws3), ws_floats=n, use_graph=0)
    h3 = lib.sptrain_create(C.byref(d3))
    sdata, slog, sx = torch.zeros(2, 1, E.SP_D, E.SP_T), torch.zeros(1, 3), torch.zeros(1, Hs, Wsp)
    sblob = torch.zeros(int(lib.sptrain_state_floats()))

    def sdesc(**kw):
        base = dict(data=ptr(sdata), n_clips=2, idx=ptr(idx), n_steps=1, log=ptr(slog), train=1)
        base.update(kw)
        return C.byref(_hip.SptrainEpochDesc(**base))
    try:
        assert lib.sptrain_epoch(h3, sdesc(), None) == ERR_STATE
        assert lib.sptrain_state_save(h3, ptr(sblob), None) == ERR_STATE
        for bad in (dict(data=None), dict(idx=None), dict(log=None), dict(n_clips=0), dict(n_steps=0)):
            assert lib.sptrain_epoch(h3, sdesc(**bad), None) == ERR_ARG, bad
        assert lib.sptrain_batch(h3, sdesc(), 1, ptr(sx), None) == ERR_ARG
        assert lib.sptrain_batch(h3, sdesc(), 0, None, None) == ERR_ARG
        assert lib.sptrain_batch(h3, sdesc(), 0, ptr(sx), None) == 0
        assert lib.sptrain_state_load(h3, None, None) == ERR_ARG
        assert lib.sptrain_state_floats() == 3 * lib.sptrain_n_param() + 2
        assert lib.aetrain_state_floats() == 3 * lib.ae_n_param() + 2
    finally:
        lib.sptrain_destroy(h3)


def test_epoch_descriptor_layouts_match_the_header():
    """the ctypes mirrors of lemo_aetrain_epoch_desc / lemo_sptrain_epoch_desc have the C structs' size and field offsets"""
    fields = {'lemo_aetrain_epoch_desc': (_hip.AetrainEpochDesc, [f for f, _ in _hip.AetrainEpochDesc._fields_]),
              'lemo_sptrain_epoch_desc': (_hip.SptrainEpochDesc, [f for f, _ in _hip.SptrainEpochDesc._fields_])}
    src = '#include <cstdio>\n#include <cstddef>\n#include "lemo_hip.h"\nint main(){\n'
    for name, (_, fl) in fields.items():
        src += f'printf("%zu", sizeof({name}));' + ''.join(f'printf(" %zu", offsetof({name}, {f}));' for f in fl) + 'printf("\\n");\n'
    src += f'printf("%d %d %d\\n", LEMO_MASK_NONE, LEMO_MASK_RANDOM, LEMO_MASK_PROX); return 0;}}\n'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, 'o.cpp'), 'w').write(src)
        subprocess.run(['g++', '-I', os.path.join(root, 'include'), os.path.join(td, 'o.cpp'), '-o', os.path.join(td, 'o')], check=True)
        lines = subprocess.run([os.path.join(td, 'o')], check=True, capture_output=True, text=True).stdout.strip().split('\n')
    for line, (name, (cls, fl)) in zip(lines, fields.items()):
        assert [C.sizeof(cls)] + [getattr(cls, f).offset for f in fl] == [int(v) for v in line.split()], name
    assert [int(v) for v in lines[2].split()] == [_hip.MASK_NONE, _hip.MASK_RANDOM, _hip.MASK_PROX]


def test_assembly_kernels_use_no_scratch_and_no_lds():
    from test_resource_usage import HIPCC, _usage
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    res = _usage('train_epoch_kernels.hip')
    names = [k for k in res if 'assemble_kernel' in k or 'ep_' in k or 'train_step_counter' in k]
    assert len(names) >= 6, sorted(res)
    for k in names:
        assert res[k].get('ScratchSize [bytes/lane]', 0) == 0 and res[k].get('VGPRs Spill', 0) == 0, k
        assert res[k].get('LDS Size [bytes/block]', 0) == 0, k
