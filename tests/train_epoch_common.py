"""Shared by test_train_epoch_emu.py (host emulator) and test_train_epoch_gpu.py (MI355X): the loop level of the two training
engines (lemo_*train_epoch / _batch / _state_*) against the torch recipes it replaces.  Every comparison is on the raw bits
(float32 viewed as int32, so a -0 / +0 mismatch shows): the assembly kernels move data, and an epoch runs the step's own kernels.

Shapes (the smallest the recipes allow): the masking recipes fix d = 208 rows; T = 12 frames is the shortest clip that
reflect-pads by 8 with room to spare -> network 210 x 28, N = 7 clips, bs = 3.  Smoothness: N = 5, bs = 2, d = 9, T = 13 -> 12
velocity frames -> network 11 x 28 (d + 2, T + 15)."""
import numpy as np
import torch

import sptrain_common as SR
from lemo_amd.infill_train import InfillPriorTrainer, default_ae_state, mask_prox, mask_random_markers, network_tensors
from lemo_amd.smooth_train import SmoothPriorTrainer, network_input

AE_N, AE_BS, AE_D, AE_T = 7, 3, 208, 12
SP_N, SP_BS, SP_D, SP_T = 5, 2, 9, 13
MASK_L = 16
# rows are non-contiguous, repeat a clip across steps (0, 3 and 6; 4 and 0) and include clips 0 and N - 1
AE_IDX = torch.tensor([[0, 6, 3], [5, 0, 2], [6, 1, 3], [2, 6, 0]])
SP_IDX = torch.tensor([[4, 0], [2, 4], [0, 3], [1, 4]])
# 16 and 47 (foot rows), a repeated id, ids 0 and 66, unused slots, an image with no id at all
AE_IDS = torch.tensor([[[16, 5, 5, -1, -1, -1], [47, -1, -1, -1, -1, -1], [0, 66, 30, 60, 12, 3]],
                       [[-1, -1, -1, -1, -1, -1], [60, 1, 2, 2, -1, -1], [66, -1, -1, -1, -1, -1]],
                       [[0, -1, -1, -1, -1, -1], [-1, 30, -1, -1, -1, -1], [47, 16, 33, -1, -1, -1]],
                       [[8, 9, -1, -1, -1, -1], [16, -1, -1, -1, -1, -1], [65, 64, 63, 62, 61, 60]]])
AE_MASK_IDX = torch.tensor([[0, 1, 2], [2, 2, 1], [1, 0, 0], [2, 1, 0]])


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ae_clips(n=AE_N, d=AE_D, t=AE_T, seed=31):
    """clip images with negative values, exact zeros and 0 / 1 contact labels in channel 0's last 4 rows"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(n, 4, d, t, generator=g) * 0.5
    img[:, 0, -4:] = (torch.rand(n, 4, t, generator=g) > 0.5).float()
    img[:, 0, 5, ::3] = 0.
    img[:, 0, 6, 1::3] = -0.
    return img


def prox_masks(L=MASK_L, seed=32):
    """[3, L, 201] as load_prox_mask_clips returns them: mask 0 all ones, mask 1 hides marker 30 in frames 2 .. 6 only (and marker 5
    from frame 10 on, partly past the clip's end), mask 2 random"""
    m = np.ones((3, L, 67), np.float32)
    m[1, 2:7, 30] = 0
    m[1, 10:, 5] = 0
    m[2] = (np.random.default_rng(seed).random((L, 67)) > 0.3).astype(np.float32)
    return np.repeat(m, 3, axis=2)


def ae_reference_batch(clips, masks, recipe, s, idx=AE_IDX, ids=AE_IDS, mask_idx=AE_MASK_IDX):
    """(x, y) of step s from the torch recipes on the gathered clips (CPU)"""
    cl = clips[idx[s]]
    if recipe == 'random':
        rows = []
        for i in range(cl.shape[0]):                     # unused (-1) slots are not part of the reference helper: valid ids only
            v = ids[s, i][ids[s, i] >= 0]
            rows.append(mask_random_markers(cl[i:i + 1], v[None])[0] if len(v) else cl[i])
        inp = torch.stack(rows)
    elif recipe == 'prox':
        inp = mask_prox(cl, masks[mask_idx[s].numpy()])
    else:
        inp = cl
    return network_tensors(inp, cl)


def recipe_args(recipe, steps, ids=AE_IDS, mask_idx=AE_MASK_IDX):
    return {'random': dict(marker_ids=ids[steps]), 'prox': dict(mask_idx=mask_idx[steps]), 'none': {}}[recipe]


def ae_trainer(lib, device, use_graph, seed=41, bs=AE_BS, d=AE_D, t=AE_T, clips=None, masks=None):
    tr = InfillPriorTrainer(default_ae_state(seed), batch=bs, H=d + 2, W=t + 16, lr=1e-3, use_graph=use_graph, device=device, _lib=lib)
    if clips is not None:
        tr.upload_dataset(clips)
    if masks is not None:
        tr.upload_prox_masks(masks)
    return tr


def ae_loop(tr, batches):
    """the loop an epoch replaces: one step(x, y, prepared=True) per torch-built batch -> the loss rows"""
    rows = []
    for x, y in batches:
        tr.step(x.to(tr.device), y.to(tr.device), prepared=True)
        rows.append(tr._losses.cpu().clone())
    return torch.stack(rows)


def ae_eval_rows(tr, batches):
    rows = []
    for x, y in batches:
        tr.evaluate(x.to(tr.device), y.to(tr.device), prepared=True)
        rows.append(tr._losses.cpu().clone())
    return torch.stack(rows)


def check_ae_assembly(lib, device, recipe, clips, masks, steps=(0, 1, 2), bs=AE_BS, idx=AE_IDX, ids=AE_IDS, mask_idx=AE_MASK_IDX):
    d, t = clips.shape[2], clips.shape[3]
    tr = ae_trainer(lib, device, False, bs=bs, d=d, t=t, clips=clips, masks=masks)
    sel = list(steps)
    kw = recipe_args(recipe, sel, ids, mask_idx)
    for k, s in enumerate(sel):
        x, y = tr.assemble(k, idx[sel], **kw)
        wx, wy = ae_reference_batch(clips, masks, recipe, s, idx, ids, mask_idx)
        assert same_bits(x, wx), (recipe, s, int((bits(x) != bits(wx)).sum()))
        assert same_bits(y, wy), (recipe, s)
    tr.close()


def check_ae_epoch_is_the_loop(lib, device, use_graph, recipe, clips, masks, steps=(0, 1, 2), with_eval=True, bs=AE_BS, idx=AE_IDX,
                               ids=AE_IDS, mask_idx=AE_MASK_IDX):
    """fit_epoch == the loop of step() calls on the torch-built batches, rows and parameters; before it, evaluate_epoch == evaluate
    per batch and changes nothing (the fit_epoch that follows still equals the loop)"""
    d, t = clips.shape[2], clips.shape[3]
    sel = list(steps)
    batches = [ae_reference_batch(clips, masks, recipe, s, idx, ids, mask_idx) for s in sel]
    kw = recipe_args(recipe, sel, ids, mask_idx)
    a = ae_trainer(lib, device, use_graph, bs=bs, d=d, t=t, clips=clips, masks=masks)
    b = ae_trainer(lib, device, False, bs=bs, d=d, t=t)
    if with_eval:
        p0 = a.flat_params()
        ev = a.evaluate_epoch(idx[sel], **kw)
        assert ev.shape == (len(sel), 4)
        assert same_bits(ev, ae_eval_rows(b, batches))
        assert same_bits(a.flat_params(), p0)
    log = a.fit_epoch(idx[sel], **kw)
    want = ae_loop(b, batches)
    assert log.shape == (len(sel), 4) and log.device.type == 'cpu'
    assert same_bits(log, want), (log, want)
    assert same_bits(a.flat_params(), b.flat_params())
    assert not same_bits(log[0], log[1])                 # different batches
    a.close()
    b.close()


def check_ae_checkpoint(lib, device, use_graph, clips, masks, recipe='random'):
    """2 steps, save, 2 more = A; a fresh trainer (other weights) loads the blob and takes the same 2 steps: bit-identical"""
    a = ae_trainer(lib, device, use_graph, clips=clips, masks=masks)
    a.fit_epoch(AE_IDX[:2], **recipe_args(recipe, [0, 1]))
    blob = a.save_state()
    assert blob.dtype == torch.float32 and blob.device.type == 'cpu' and blob.numel() == 3 * a.flat_params().numel() + 2
    assert same_bits(blob[:a.flat_params().numel()], a.flat_params()) and blob[-2:].tolist() == [2.0, 0.0]
    log_a = a.fit_epoch(AE_IDX[2:4], **recipe_args(recipe, [2, 3]))
    c = ae_trainer(lib, device, use_graph, seed=43, clips=clips, masks=masks)
    assert not same_bits(c.flat_params(), a.flat_params())
    c.load_state(blob)
    assert same_bits(c.save_state(), blob)
    log_c = c.fit_epoch(AE_IDX[2:4], **recipe_args(recipe, [2, 3]))
    assert same_bits(log_c, log_a)
    assert same_bits(c.flat_params(), a.flat_params())
    assert same_bits(c.save_state(), a.save_state()) and a.save_state()[-2:].tolist() == [4.0, 0.0]
    for bad in (blob[:-1], torch.cat([blob, blob[:1]]), blob.double()):
        try:
            c.load_state(bad)
        except ValueError:
            continue
        raise AssertionError('a blob of the wrong length or type was accepted')
    a.close()
    c.close()


# ---- smoothness prior
def sp_clips(n=SP_N, d=SP_D, t=SP_T, seed=51):
    return torch.randn(n, 1, d, t, generator=torch.Generator().manual_seed(seed)) * 0.5


def sp_trainer(lib, device, use_graph, seed=3, bs=SP_BS, d=SP_D, t=SP_T, clips=None):
    enc, dec = SR.random_state(seed)
    tr = SmoothPriorTrainer(enc, dec, batch=bs, H=d + 2, W=t + 15, lr=1e-3, use_graph=use_graph, device=device, _lib=lib)
    if clips is not None:
        tr.upload_dataset(clips)
    return tr


def sp_rows(tr, xs, train):
    rows = []
    for x in xs:
        (tr.step if train else tr.evaluate)(x.to(tr.device), prepared=True)
        rows.append(tr._losses.cpu().clone())
    return torch.stack(rows)


def check_sp_assembly(lib, device, clips, steps=(0, 1, 2), bs=SP_BS, idx=SP_IDX):
    tr = sp_trainer(lib, device, False, bs=bs, d=clips.shape[2], t=clips.shape[3], clips=clips)
    sel = list(steps)
    for k, s in enumerate(sel):
        assert same_bits(tr.assemble(k, idx[sel]), network_input(clips[idx[s]])), s
    tr.close()


def check_sp_epoch_is_the_loop(lib, device, use_graph, clips, steps=(0, 1, 2), with_eval=True, bs=SP_BS, idx=SP_IDX):
    d, t = clips.shape[2], clips.shape[3]
    sel = list(steps)
    xs = [network_input(clips[idx[s]]) for s in sel]
    a = sp_trainer(lib, device, use_graph, bs=bs, d=d, t=t, clips=clips)
    b = sp_trainer(lib, device, False, bs=bs, d=d, t=t)
    if with_eval:
        p0 = a.flat_params()
        ev = a.evaluate_epoch(idx[sel])
        assert ev.shape == (len(sel), 3) and same_bits(ev, sp_rows(b, xs, False))
        assert same_bits(a.flat_params(), p0)
    log = a.fit_epoch(idx[sel])
    want = sp_rows(b, xs, True)
    assert log.shape == (len(sel), 3) and log.device.type == 'cpu'
    assert same_bits(log, want), (log, want)
    assert same_bits(a.flat_params(), b.flat_params())
    assert not same_bits(log[0], log[1])
    a.close()
    b.close()


def check_sp_checkpoint(lib, device, use_graph, clips):
    a = sp_trainer(lib, device, use_graph, clips=clips)
    a.fit_epoch(SP_IDX[:2])
    blob = a.save_state()
    n = a.flat_params().numel()
    assert blob.numel() == 3 * n + 2 and same_bits(blob[:n], a.flat_params()) and blob[-2:].tolist() == [2.0, 0.0]
    log_a = a.fit_epoch(SP_IDX[2:4])
    c = sp_trainer(lib, device, use_graph, seed=4, clips=clips)
    assert not same_bits(c.flat_params(), a.flat_params())
    c.load_state(blob)
    assert same_bits(c.save_state(), blob)
    log_c = c.fit_epoch(SP_IDX[2:4])
    assert same_bits(log_c, log_a) and same_bits(c.flat_params(), a.flat_params()) and same_bits(c.save_state(), a.save_state())
    for bad in (blob[:-1], torch.cat([blob, blob[:1]])):
        try:
            c.load_state(bad)
        except ValueError:
            continue
        raise AssertionError('a blob of the wrong length was accepted')
    a.close()
    c.close()


def check_bad_indices_are_refused(lib, device):
    """every out-of-range index raises ValueError on the host; nothing is launched"""
    import pytest
    clips, masks = ae_clips(), prox_masks()
    tr = ae_trainer(lib, device, False, clips=clips, masks=masks)
    ok = AE_IDX[:1]
    bad_idx = ok.clone(); bad_idx[0, 1] = AE_N
    bad_ids = AE_IDS[:1].clone(); bad_ids[0, 2, 1] = 67
    bad_mi = AE_MASK_IDX[:1].clone(); bad_mi[0, 0] = 3
    for fn in (tr.fit_epoch, tr.evaluate_epoch, lambda *a, **k: tr.assemble(0, *a, **k)):
        for args, kw in ((bad_idx, {}), (-bad_idx, {}), (ok, dict(marker_ids=bad_ids)), (ok, dict(marker_ids=AE_IDS[:1] - 1)),
                         (ok, dict(mask_idx=bad_mi)), (ok, dict(mask_idx=-bad_mi)), (ok.float(), {}), (ok[:, :2], {}),
                         (ok, dict(marker_ids=AE_IDS[:2])), (ok, dict(marker_ids=AE_IDS[:1], mask_idx=AE_MASK_IDX[:1]))):
            with pytest.raises(ValueError):
                fn(args, **kw)
    with pytest.raises(ValueError):
        tr.upload_prox_masks(prox_masks(L=AE_T - 1))                              # L < T
    with pytest.raises(ValueError):
        tr.upload_dataset(clips[:, :, :-1])
    with pytest.raises(ValueError):
        tr.assemble(1, ok)
    uneven = prox_masks(); uneven[1, 8, 91] = 0                                 # one of marker 30's three columns only
    with pytest.raises(ValueError):
        tr.upload_prox_masks(uneven)
    tr.close()
    st = sp_trainer(lib, device, False, clips=sp_clips())
    bad = SP_IDX[:1].clone(); bad[0, 0] = SP_N
    for fn in (st.fit_epoch, st.evaluate_epoch, lambda i: st.assemble(0, i)):
        for arg in (bad, -bad, SP_IDX[:1, :1]):
            with pytest.raises(ValueError):
                fn(arg)
    st.close()
    fresh = sp_trainer(lib, device, False)
    with pytest.raises(ValueError):
        fresh.fit_epoch(SP_IDX[:1])                                              # no dataset yet
    fresh.close()
