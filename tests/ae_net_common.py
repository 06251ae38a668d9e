"""The infilling autoencoder's two native engines -- the finetune engine (lemo_ae_*: K clips, K parameter sets) and the batch trainer
(lemo_aetrain_*: one parameter set over bs images) -- walk one network description (csrc/ae_engine.hpp).  Helpers of the tests that
hold them to it: the same parameters and images through both engines' forwards, and the layout sizes both report."""
import ctypes as C

import numpy as np
import torch

from lemo_amd import _hip
from lemo_amd._hip import ptr
from lemo_amd.infill_train import default_ae_state, flatten_state

# (H, W, K): 22 x 19 has odd sizes at several of the five levels and ends at 1 x 1; 6 x 2 is the smallest the trainer accepts
SHAPES = [(22, 19, 1), (22, 19, 3), (6, 2, 2)]

N_PARAM = 4114219
STATE_FLOATS = 12342659
AE_WS_FLOATS = {(6, 2): 20773952, (14, 9): 20870848, (22, 19): 21074176, (210, 135): 39951232}
AETRAIN_WS_FLOATS = {                     # bs = 1, 3, 8, 9
    (6, 2): (24909120, 33386816, 54581120, 54683904),
    (14, 9): (25006016, 33677632, 55356672, 55556416),
    (22, 19): (25209344, 34287552, 56983104, 57386112),
    (210, 135): (44086720, 90919744, 208002368, 223805056),
}
AETRAIN_BS = (1, 3, 8, 9)

_FLAT = None


def _flat_params():
    global _FLAT
    if _FLAT is None:
        _FLAT = torch.from_numpy(flatten_state(default_ae_state(17)).astype(np.float32))
    return _FLAT


def both_forwards(lib, H, W, K, dev='cpu'):
    """the same flat parameter vector in every clip of a K-clip finetune engine and in a trainer with bs = K, the same K images
    -> (rec [K][H][W] of lemo_ae_forward_clip, rec [K][H][W] of lemo_aetrain_eval)"""
    sync = torch.cuda.synchronize if dev != 'cpu' else (lambda: None)
    g = torch.Generator().manual_seed(1000 * H + 10 * W + K)
    x = (torch.randn(K, 4, H, W, generator=g) * 0.5).to(dev)
    y = torch.randn(K, H, W, generator=g).to(dev)
    flat = _flat_params().to(dev)
    assert flat.numel() == lib.ae_n_param()

    n = int(lib.ae_ws_floats(H, W))
    ws = torch.zeros(K * n, device=dev)
    h = lib.ae_create(C.byref(_hip.AeDesc(H, W, 3e-6, ptr(ws), K * n, K)))
    assert h
    moc = torch.full((H, W), 1.0 / (H * W), device=dev)
    rec_ft = torch.zeros(K, H, W, device=dev)
    try:
        for c in range(K):
            assert lib.ae_load_clip(h, c, ptr(flat), ptr(x[c]), ptr(moc), None) == 0
        for c in range(K):
            assert lib.ae_forward_clip(h, c, ptr(rec_ft[c]), None, None) == 0
        sync()
    finally:
        lib.ae_destroy(h)

    n = int(lib.aetrain_ws_floats(H, W, K))
    ws = torch.zeros(n, device=dev)
    d = _hip.AetrainDesc(H=H, W=W, bs=K, lr=1e-4, w_body=10., w_v=10., w_c=1., ws=ptr(ws), ws_floats=n, use_graph=0)
    h = lib.aetrain_create(C.byref(d))
    assert h
    rec_tr, losses = torch.zeros(K, H, W, device=dev), torch.zeros(4, device=dev)
    try:
        assert lib.aetrain_load(h, ptr(flat), None) == 0
        assert lib.aetrain_eval(h, ptr(x), ptr(y), ptr(losses), ptr(rec_tr), None) == 0
        sync()
    finally:
        lib.aetrain_destroy(h)
    return rec_ft.cpu(), rec_tr.cpu()


def assert_same_network(lib, H, W, K, dev='cpu'):
    rec_ft, rec_tr = both_forwards(lib, H, W, K, dev)
    assert torch.isfinite(rec_ft).all() and float(rec_ft.abs().max()) > 0
    for c in range(K):
        assert torch.equal(rec_ft[c], rec_tr[c]), (H, W, K, c, float((rec_ft[c] - rec_tr[c]).abs().max()))
