"""Native training of the motion smoothness prior: ``models/AE_sep.py::Enc`` + ``Dec`` (downsample=False, z_channel=64) as
``train_smooth_prior.py:96-136`` trains them, on the ``lemo_sptrain_*`` engine (include/lemo_hip.h).

Per step, for ``clip_img [bs, 1, d, T]``: ``x = reflect_pad(clip_img[..., 1:] - clip_img[..., :-1], (8, 8, 1, 1))``,
``z = Enc(x)``, ``rec = Dec(z)``, ``loss = w_rec * l1(x, rec) + w_smooth * mean((z[..., 1:] - z[..., :-1]) ** 2)``, one
``torch.optim.Adam(lr)`` step over all Enc and Dec parameters.  Data loading stays the caller's (the reference's
``TrainLoader`` yields exactly ``clip_img``).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip
from ._hip import ptr
from .priors import DEC_IN, DEC_OUT, ENC_CHANNELS, dec_layer_keys, enc_layer_keys


def param_layout() -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of the 40 tensors in the engine's flat order: Enc then Dec, each in state_dict order"""
    out = []
    for l, k in enumerate(enc_layer_keys()):
        ci, co = ENC_CHANNELS[l], ENC_CHANNELS[l + 1]
        out += [(k + '.weight', (co, ci, 3, 3)), (k + '.bias', (co,))]
    for j, k in enumerate(dec_layer_keys()):
        out += [(k + '.weight', (DEC_IN[j], DEC_OUT[j], 3, 3)), (k + '.bias', (DEC_OUT[j],))]
    return out


def n_param() -> int:
    return sum(int(np.prod(s)) for _, s in param_layout())


def flatten_state(enc_sd: Dict, dec_sd: Dict) -> np.ndarray:
    parts = []
    for k, shp in param_layout():
        sd = enc_sd if k.startswith('enc_') else dec_sd
        v = sd[k]
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        if tuple(v.shape) != shp:
            raise ValueError(f'{k}: shape {tuple(v.shape)}, expected {shp}')
        parts.append(np.ascontiguousarray(v, np.float32).ravel())
    return np.concatenate(parts)


def unflatten_state(flat: np.ndarray) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    enc, dec, o = {}, {}, 0
    for k, shp in param_layout():
        n = int(np.prod(shp))
        t = torch.from_numpy(np.array(flat[o:o + n], np.float32).reshape(shp))
        (enc if k.startswith('enc_') else dec)[k] = t
        o += n
    return enc, dec


def default_dec_state(seed: int = 0) -> Dict[str, torch.Tensor]:
    """torch's default ConvTranspose2d initialisation of the decoder's 10 layers, in construction order, from `seed`"""
    g = torch.random.fork_rng(devices=[])
    with g:
        torch.manual_seed(seed)
        sd = {}
        for j, k in enumerate(dec_layer_keys()):
            m = torch.nn.ConvTranspose2d(DEC_IN[j], DEC_OUT[j], 3, stride=1, padding=1)
            sd[k + '.weight'] = m.weight.detach().clone()
            sd[k + '.bias'] = m.bias.detach().clone()
    return sd


def network_input(clip_img: torch.Tensor) -> torch.Tensor:
    """clip_img [bs, 1, d, T] -> the network input [bs, d + 2, T + 15]: velocity, reflect padding (8, 8, 1, 1)"""
    v = clip_img[:, :, :, 1:] - clip_img[:, :, :, :-1]
    return F.pad(v, (8, 8, 1, 1), 'reflect')[:, 0].contiguous().float()


class SmoothPriorTrainer:
    """Enc + Dec training steps on the native engine.  ``batch``, ``H``, ``W``: the batch size and the NETWORK input size
    (245 x 135 for 81 markers with hands and T = 120).  ``dec_state=None`` starts the decoder from torch's default init."""

    def __init__(self, enc_state: Dict, dec_state: Optional[Dict] = None, batch: int = 60, H: int = 245, W: int = 135,
                 lr: float = 1e-4, weight_loss_rec_v: float = 1.0, weight_loss_z_smooth: float = 1000.0, device=None,
                 use_graph: bool = True, seed: int = 0, _lib=None):
        self.lib = _lib or _hip.get_lib()
        if device is None:
            device = torch.device('cpu') if self.lib.is_emu else torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        self.bs, self.H, self.W = int(batch), int(H), int(W)
        # the engine runs on a stream of its own (a graph cannot be captured on the legacy default stream); every call orders it
        # after the caller's current stream and the caller's stream after it
        self.stream = None if self.lib.is_emu else torch.cuda.Stream(self.device)
        nws = self.lib.sptrain_ws_floats(self.H, self.W, self.bs)
        if nws <= 0:
            raise ValueError(f'smoothness-prior training does not take batch {batch} at {H} x {W} (2 <= H, 2 <= W <= 139)')
        self.ws = torch.zeros(int(nws), dtype=torch.float32, device=self.device)
        d = _hip.SptrainDesc(H=self.H, W=self.W, bs=self.bs, lr=float(lr), weight_rec=float(weight_loss_rec_v),
                             weight_smooth=float(weight_loss_z_smooth), ws=ptr(self.ws), ws_floats=int(nws),
                             use_graph=int(bool(use_graph) and not self.lib.is_emu))
        self.h = self.lib.sptrain_create(ctypes.byref(d))
        if not self.h:
            raise _hip.LemoHipError('lemo_sptrain_create failed')
        if dec_state is None:
            dec_state = default_dec_state(seed)
        flat = torch.from_numpy(flatten_state(enc_state, dec_state)).to(self.device)
        self._losses = torch.zeros(3, dtype=torch.float32, device=self.device)
        self._call(lambda s: self.lib.check(self.lib.sptrain_load(self.h, ptr(flat), s), 'sptrain_load'))

    def _s(self):
        return None if self.stream is None else self.stream.cuda_stream

    def _call(self, fn):
        if self.stream is None:
            return fn(None)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        try:
            return fn(self.stream.cuda_stream)
        finally:
            cur.wait_stream(self.stream)

    def _x(self, clip_img: torch.Tensor, prepared: bool) -> torch.Tensor:
        x = clip_img.to(self.device).float().contiguous() if prepared else network_input(clip_img.to(self.device).float())
        if tuple(x.shape) != (self.bs, self.H, self.W):
            raise ValueError(f'network input {tuple(x.shape)}, the trainer was built for {(self.bs, self.H, self.W)}')
        return x

    def step(self, clip_img: torch.Tensor, n: int = 1, prepared: bool = False) -> Tuple[float, float]:
        """n training steps on clip_img [bs, 1, d, T] (prepared=True: already the network input [bs, H, W]) ->
        (loss_rec_v, loss_z_smooth) of the last step"""
        x = self._x(clip_img, prepared)
        self._call(lambda s: self.lib.check(self.lib.sptrain_step(self.h, ptr(x), int(n), ptr(self._losses), s), 'sptrain_step'))
        l = self._losses.cpu()
        return float(l[0]), float(l[1])

    def evaluate(self, clip_img: torch.Tensor, prepared: bool = False) -> Tuple[float, float]:
        x = self._x(clip_img, prepared)
        self._call(lambda s: self.lib.check(self.lib.sptrain_eval(self.h, ptr(x), ptr(self._losses), None, s), 'sptrain_eval'))
        l = self._losses.cpu()
        return float(l[0]), float(l[1])

    def flat_params(self) -> torch.Tensor:
        out = torch.empty(n_param(), dtype=torch.float32, device=self.device)
        self._call(lambda s: self.lib.check(self.lib.sptrain_params(self.h, ptr(out), s), 'sptrain_params'))
        return out.cpu()

    def flat_grads(self) -> torch.Tensor:
        """the gradient of the last training step, in the flat order"""
        out = torch.empty(n_param(), dtype=torch.float32, device=self.device)
        self._call(lambda s: self.lib.check(self.lib.sptrain_grads(self.h, ptr(out), s), 'sptrain_grads'))
        return out.cpu()

    def state_dicts(self) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
        """(enc_sd, dec_sd) as CPU tensors under the reference's keys"""
        return unflatten_state(self.flat_params().numpy())

    # ---- the loop level: the dataset on the device, one call per epoch (lemo_sptrain_epoch)
    def upload_dataset(self, clips) -> None:
        """clips [N, 1, d, T] (d + 2 = H, T + 15 = W): the clip images the epochs gather their batches from"""
        t = torch.as_tensor(np.asarray(clips) if not torch.is_tensor(clips) else clips)
        if t.dim() != 4 or tuple(t.shape[1:]) != (1, self.H - 2, self.W - 15) or t.shape[0] < 1:
            raise ValueError(f'expected clips [N, 1, {self.H - 2}, {self.W - 15}], got {tuple(t.shape)}')
        if self.W - 16 < 9 or self.H < 4:
            raise ValueError('reflect padding by (8, 1) needs more than 8 velocity frames and 2 rows')
        self._data = t.to(self.device, torch.float32).contiguous()

    def _epoch_desc(self, idx):
        """validates the indices on the host (nothing has been launched when it raises) -> (descriptor, the tensor it points into)"""
        if getattr(self, '_data', None) is None:
            raise ValueError('upload_dataset first')
        t = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError('idx must be an integer tensor')
        t = t.cpu().long()
        if t.dim() != 2 or t.shape[1] != self.bs or t.shape[0] < 1:
            raise ValueError(f'idx: expected [n_steps, {self.bs}], got {tuple(t.shape)}')
        if int(t.min()) < 0 or int(t.max()) >= self._data.shape[0]:
            raise ValueError(f'idx holds values outside [0, {self._data.shape[0]})')
        dev_idx = t.to(torch.int32).contiguous().to(self.device)
        d = _hip.SptrainEpochDesc(data=ptr(self._data), n_clips=int(self._data.shape[0]), idx=ptr(dev_idx), n_steps=int(t.shape[0]))
        return d, dev_idx

    def _epoch(self, idx, train):
        d, keep = self._epoch_desc(idx)
        log = torch.zeros(d.n_steps, 3, dtype=torch.float32, device=self.device)
        d.log, d.train = ptr(log), int(train)
        self._call(lambda s: self.lib.check(self.lib.sptrain_epoch(self.h, ctypes.byref(d), s), 'sptrain_epoch'))
        out = log.cpu()                                                        # the epoch's one host wait (keeps `keep` alive until then)
        del keep
        return out

    def fit_epoch(self, idx) -> torch.Tensor:
        """one training step per row of idx [n_steps, bs] (clips of the uploaded dataset): the batches are assembled on the device
        and the host does not wait between steps.  -> the loss log [n_steps, 3] on the CPU, rows (loss_rec_v, loss_z_smooth,
        weighted total).  The RNG (the permutation) stays the caller's."""
        return self._epoch(idx, True)

    def evaluate_epoch(self, idx) -> torch.Tensor:
        """the same batches and log under the current parameters, no update"""
        return self._epoch(idx, False)

    def assemble(self, step: int, idx) -> torch.Tensor:
        """the network input [bs, H, W] of row `step` as the epoch kernel builds it, on the trainer's device"""
        d, keep = self._epoch_desc(idx)
        if not 0 <= int(step) < d.n_steps:
            raise ValueError(f'step {step} outside [0, {d.n_steps})')
        x = torch.empty(self.bs, self.H, self.W, dtype=torch.float32, device=self.device)
        self._call(lambda s: self.lib.check(self.lib.sptrain_batch(self.h, ctypes.byref(d), int(step), ptr(x), s), 'sptrain_batch'))
        _hip.quiesce(self.device, self.lib)                                    # the index table is released on return
        return x

    def save_state(self) -> torch.Tensor:
        """parameters, both Adam moments and the step counter as one flat CPU tensor (include/lemo_hip.h has the layout)"""
        out = torch.empty(int(self.lib.sptrain_state_floats()), dtype=torch.float32, device=self.device)
        self._call(lambda s: self.lib.check(self.lib.sptrain_state_save(self.h, ptr(out), s), 'sptrain_state_save'))
        return out.cpu()

    def load_state(self, blob: torch.Tensor) -> None:
        """restore what save_state returned: training continues bit-identically"""
        n = int(self.lib.sptrain_state_floats())
        if not torch.is_tensor(blob) or blob.dtype != torch.float32 or blob.dim() != 1 or blob.numel() != n:
            raise ValueError(f'a training state is a flat float32 tensor of {n} values')
        t = blob.to(self.device).contiguous()
        self._call(lambda s: self.lib.check(self.lib.sptrain_state_load(self.h, ptr(t), s), 'sptrain_state_load'))
        _hip.quiesce(self.device, self.lib)

    def close(self):
        if getattr(self, 'h', None):
            _hip.quiesce(self.device, self.lib)
            self.lib.sptrain_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
