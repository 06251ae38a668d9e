"""Native training of the motion smoothness prior: ``models/AE_sep.py::Enc`` + ``Dec`` (downsample=False, z_channel=64) as
``train_smooth_prior.py:96-136`` trains them, on the ``lemo_sptrain_*`` engine (include/lemo_hip.h).

Per step, for ``clip_img [bs, 1, d, T]``: ``x = reflect_pad(clip_img[..., 1:] - clip_img[..., :-1], (8, 8, 1, 1))``,
``z = Enc(x)``, ``rec = Dec(z)``, ``loss = w_rec * l1(x, rec) + w_smooth * mean((z[..., 1:] - z[..., :-1]) ** 2)``, one
``torch.optim.Adam(lr)`` step over all Enc and Dec parameters.  Data loading stays the caller's (the reference's
``TrainLoader`` yields exactly ``clip_img``).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip
from ._engine import PriorTrainer
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


class SmoothPriorTrainer(PriorTrainer):
    """Enc + Dec training steps on the native engine.  ``batch``, ``H``, ``W``: the batch size and the NETWORK input size
    (245 x 135 for 81 markers with hands and T = 120).  ``dec_state=None`` starts the decoder from torch's default init."""
    _prefix, _nloss, _n_param = 'sptrain', 3, staticmethod(n_param)

    def __init__(self, enc_state: Dict, dec_state: Optional[Dict] = None, batch: int = 60, H: int = 245, W: int = 135,
                 lr: float = 1e-4, weight_loss_rec_v: float = 1.0, weight_loss_z_smooth: float = 1000.0, device=None,
                 use_graph: bool = True, seed: int = 0, _lib=None):
        super().__init__(_hip.SptrainDesc, batch, H, W, device, use_graph, _lib,
                         f'smoothness-prior training does not take batch {batch} at {H} x {W} (2 <= H, 2 <= W <= 139)',
                         lr=float(lr), weight_rec=float(weight_loss_rec_v), weight_smooth=float(weight_loss_z_smooth))
        self._load(flatten_state(enc_state, default_dec_state(seed) if dec_state is None else dec_state))

    def _x(self, clip_img: torch.Tensor, prepared: bool) -> torch.Tensor:
        x = clip_img.to(self.device).float().contiguous() if prepared else network_input(clip_img.to(self.device).float())
        if tuple(x.shape) != (self.bs, self.H, self.W):
            raise ValueError(f'network input {tuple(x.shape)}, the trainer was built for {(self.bs, self.H, self.W)}')
        return x

    def step(self, clip_img: torch.Tensor, n: int = 1, prepared: bool = False) -> Tuple[float, float]:
        """n training steps on clip_img [bs, 1, d, T] (prepared=True: already the network input [bs, H, W]) ->
        (loss_rec_v, loss_z_smooth) of the last step"""
        x = self._x(clip_img, prepared)
        self._run('step', ptr(x), int(n), ptr(self._losses))
        l = self._losses.cpu()
        return float(l[0]), float(l[1])

    def evaluate(self, clip_img: torch.Tensor, prepared: bool = False) -> Tuple[float, float]:
        x = self._x(clip_img, prepared)
        self._run('eval', ptr(x), ptr(self._losses), None)
        l = self._losses.cpu()
        return float(l[0]), float(l[1])

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
        data = self._dataset()
        dev_idx = self._index_table(idx, 'idx', 0, data.shape[0]).to(self.device)
        d = _hip.SptrainEpochDesc(data=ptr(data), n_clips=int(data.shape[0]), idx=ptr(dev_idx), n_steps=int(dev_idx.shape[0]))
        return d, dev_idx

    def fit_epoch(self, idx) -> torch.Tensor:
        """one training step per row of idx [n_steps, bs] (clips of the uploaded dataset): the batches are assembled on the device
        and the host does not wait between steps.  -> the loss log [n_steps, 3] on the CPU, rows (loss_rec_v, loss_z_smooth,
        weighted total).  The RNG (the permutation) stays the caller's."""
        return self._epoch(*self._epoch_desc(idx), True)

    def evaluate_epoch(self, idx) -> torch.Tensor:
        """the same batches and log under the current parameters, no update"""
        return self._epoch(*self._epoch_desc(idx), False)

    def assemble(self, step: int, idx) -> torch.Tensor:
        """the network input [bs, H, W] of row `step` as the epoch kernel builds it, on the trainer's device"""
        return self._assemble(*self._epoch_desc(idx), step, (self.bs, self.H, self.W))[0]
