"""Native training of the motion infilling prior: ``models/AE.py::AE(downsample=True, in_channel=4, kernel=3)`` as
``train_infill_prior.py:185-203`` trains it (``body_mode='local_markers_4chan'``), on the ``lemo_aetrain_*`` engine
(include/lemo_hip.h).

Per step, for the masked input ``clip_img_input`` and the target ``clip_img`` (both ``[bs, 4, d, T]``):
``x = reflect_pad(clip_img_input, (8, 8, 1, 1))``, ``y = reflect_pad(clip_img, (8, 8, 1, 1))[:, 0]``, ``rec = AE(x)``,
``loss = w_body * l1(y[:, :-5], rec[:, :-5]) + w_v * l1(dy[:, :-5], drec[:, :-5]) + w_c * bce_with_logits(rec[:, -5:], y[:, -5:])``
(``d``: differences of neighbouring frames), one ``torch.optim.Adam(lr)`` step over all 40 tensors.  Data loading and the RNG
stay the caller's: the two masking recipes of the reference are the pure torch helpers below.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip
from ._engine import PriorTrainer
from ._hip import ptr
from .infill import _layers

PAD = (8, 8, 1, 1)
LEFT_FOOT, RIGHT_FOOT = (16, 30), (47, 60)
"""marker ids whose masking also masks the left / right foot-contact rows (train_infill_prior.py:154-159)"""


def param_layout() -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of the 40 tensors in the engine's flat order (state_dict order, lemo_ae_load's order)"""
    out = []
    for l in _layers():
        out += [(l.name + '.weight', (l.cin, l.cout, 3, 3) if l.deconv else (l.cout, l.cin, 3, 3)), (l.name + '.bias', (l.cout,))]
    return out


def n_param() -> int:
    return sum(int(np.prod(s)) for _, s in param_layout())


def flatten_state(sd: Dict) -> np.ndarray:
    parts = []
    for k, shp in param_layout():
        v = sd[k]
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        if tuple(v.shape) != shp:
            raise ValueError(f'{k}: shape {tuple(v.shape)}, expected {shp}')
        parts.append(np.ascontiguousarray(v, np.float32).ravel())
    return np.concatenate(parts)


def unflatten_state(flat) -> Dict[str, torch.Tensor]:
    flat = flat.numpy() if torch.is_tensor(flat) else np.asarray(flat)
    sd, o = {}, 0
    for k, shp in param_layout():
        n = int(np.prod(shp))
        sd[k] = torch.from_numpy(np.array(flat[o:o + n], np.float32).reshape(shp))
        o += n
    return sd


def default_ae_state(seed: int = 0) -> Dict[str, torch.Tensor]:
    """torch's default Conv2d / ConvTranspose2d initialisation bounds (kaiming-uniform a = sqrt(5): 1 / sqrt(fan_in) for weights
    and biases; fan_in = weight.shape[1] * 9, which for ConvTranspose2d is its OUTPUT channel count), drawn from
    numpy.random.default_rng(seed) in state_dict order, so a seed gives the same weights on every torch version"""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shp in param_layout():
        if k.endswith('.weight'):
            bound = 1.0 / np.sqrt(shp[1] * 9)
        else:
            wshape = sd[k[:-len('bias')] + 'weight'].shape
            bound = 1.0 / np.sqrt(wshape[1] * 9)
        sd[k] = torch.from_numpy(rng.uniform(-bound, bound, size=shp).astype(np.float32))
    return sd


def network_tensors(clip_img_input: torch.Tensor, clip_img: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """([bs, 4, d, T] masked input, [bs, 4, d, T] target) -> (x [bs, 4, d + 2, T + 16], y [bs, d + 2, T + 16])"""
    x = F.pad(clip_img_input.float(), PAD, 'reflect').contiguous()
    y = F.pad(clip_img.float(), PAD, 'reflect')[:, 0].contiguous()
    return x, y


def mask_random_markers(clip_img: torch.Tensor, marker_ids: torch.Tensor) -> torch.Tensor:
    """train_infill_prior.py:135-160: a masked copy of clip_img [bs, 4, d, T]; marker_ids [bs, n] long (the caller draws them:
    ``(torch.rand(bs, n) * 67).long()``).  Zeroes channel 0's 3 rows of each marker (after the 3 pelvis rows) and the foot-contact
    rows -4 / -2 (ids 16, 30) and -3 / -1 (ids 47, 60)."""
    out = clip_img.clone()
    rows = marker_ids.long() * 3 + 3
    for i in range(clip_img.shape[0]):
        for r in (rows[i], rows[i] + 1, rows[i] + 2):
            out[i, 0, r, :] = 0.
        ids = marker_ids[i].tolist()
        if LEFT_FOOT[0] in ids or LEFT_FOOT[1] in ids:
            out[i, 0, -4, :] = 0.
            out[i, 0, -2, :] = 0.
        if RIGHT_FOOT[0] in ids or RIGHT_FOOT[1] in ids:
            out[i, 0, -3, :] = 0.
            out[i, 0, -1, :] = 0.
    return out


def load_prox_mask_clips(mask_dir: str, clip_len: int = 120, min_ratio: float = 0.05) -> np.ndarray:
    """train_infill_prior.py:116-127: every ``<mask_dir>/<seq>/mask_markers.npy`` ([T, 67], 0 = masked) cut into clip_len-frame
    clips; a clip is kept when at least min_ratio of its entries are masked.  -> [n, clip_len, 67 * 3] (each marker's column
    repeated for its 3 rows)"""
    out = []
    for d in sorted(os.listdir(mask_dir)):
        mask = np.load(os.path.join(mask_dir, d, 'mask_markers.npy'))
        for i in range(len(mask) // clip_len):
            mc = mask[i * clip_len:(i + 1) * clip_len]
            n_all = mc.shape[0] * mc.shape[1]
            if (n_all - mc.sum()) / n_all >= min_ratio:
                out.append(np.repeat(mc, 3, axis=1))
    return np.asarray(out)


def mask_prox(clip_img: torch.Tensor, mask_clips) -> torch.Tensor:
    """train_infill_prior.py:162-178: clip_img [bs, 4, d, T] with channel 0 multiplied by the PROX masks mask_clips [bs, L, 67 * 3]
    (L >= T; the caller shuffles and picks them), the pelvis rows kept and the foot-contact rows masked where either marker of that
    foot is"""
    bs, T = clip_img.shape[0], clip_img.shape[-1]
    m = torch.as_tensor(np.asarray(mask_clips)).float().permute(0, 2, 1).unsqueeze(1).to(clip_img.device)     # [bs, 1, 201, L]
    left = (m[:, :, 16 * 3:16 * 3 + 1] == 1) * (m[:, :, 30 * 3:30 * 3 + 1] == 1)
    right = (m[:, :, 47 * 3:47 * 3 + 1] == 1) * (m[:, :, 60 * 3:60 * 3 + 1] == 1)
    contact = torch.cat([left, right, left, right], dim=-2).float()
    full = torch.cat([torch.ones(bs, 1, 3, T, device=clip_img.device), m[..., 0:T], contact[..., 0:T]], dim=-2)
    out = clip_img.clone()
    out[:, 0:1] = out[:, 0:1] * full
    return out


class InfillPriorTrainer(PriorTrainer):
    """AE training steps on the native engine.  ``batch``, ``H``, ``W``: the batch size and the NETWORK input size (d + 2, T + 16:
    210 x 135 for 67 markers and 119 frames).  ``state_dict=None`` starts from ``default_ae_state(seed)``."""
    _prefix, _nloss, _n_param = 'aetrain', 4, staticmethod(n_param)
    _masks = None                    # the uploaded PROX masks (upload_prox_masks)

    def __init__(self, state_dict: Optional[Dict] = None, batch: int = 60, H: int = 210, W: int = 135, lr: float = 1e-4,
                 weight_loss_rec_body: float = 10., weight_loss_rec_body_v: float = 10., weight_loss_rec_contact_lbl: float = 1.,
                 seed: int = 0, device=None, use_graph: bool = True, _lib=None):
        super().__init__(_hip.AetrainDesc, batch, H, W, device, use_graph, _lib,
                         f'infilling-prior training does not take batch {batch} at {H} x {W} '
                         f'(1 <= batch <= 128, H >= 6, W >= 2, H * W <= 2^22)',
                         lr=float(lr), w_body=float(weight_loss_rec_body), w_v=float(weight_loss_rec_body_v),
                         w_c=float(weight_loss_rec_contact_lbl))
        self._load(flatten_state(default_ae_state(seed) if state_dict is None else state_dict))

    def _xy(self, clip_img_input, clip_img, prepared):
        for t in (clip_img_input, clip_img):
            if not torch.is_tensor(t):
                raise TypeError('clip images must be torch tensors')
            if t.device != self.device:
                raise ValueError(f'clip images must live on {self.device}, got {t.device}')
        if prepared:
            x, y = clip_img_input.float().contiguous(), clip_img.float().contiguous()
        else:
            if clip_img_input.dim() != 4 or clip_img_input.shape[1] != 4 or clip_img.shape != clip_img_input.shape:
                raise ValueError(f'expected two [bs, 4, d, T] clip images, got {tuple(clip_img_input.shape)} and {tuple(clip_img.shape)}')
            x, y = network_tensors(clip_img_input, clip_img)
        if tuple(x.shape) != (self.bs, 4, self.H, self.W) or tuple(y.shape) != (self.bs, self.H, self.W):
            raise ValueError(f'network input {tuple(x.shape)} / target {tuple(y.shape)}, the trainer was built for '
                             f'{(self.bs, 4, self.H, self.W)} / {(self.bs, self.H, self.W)}')
        return x, y

    def step(self, clip_img_input: torch.Tensor, clip_img: torch.Tensor, n: int = 1, prepared: bool = False) -> Tuple[float, float, float]:
        """n training steps -> (loss_rec_body, loss_rec_body_v, loss_rec_contact_lbl) of the last step.  prepared=True: the inputs
        are already the padded network input x [bs, 4, H, W] and target y [bs, H, W]"""
        x, y = self._xy(clip_img_input, clip_img, prepared)
        self._run('step', ptr(x), ptr(y), int(n), ptr(self._losses))
        l = self._losses.cpu()
        return float(l[0]), float(l[1]), float(l[2])

    def evaluate(self, clip_img_input: torch.Tensor, clip_img: torch.Tensor, return_rec: bool = False, prepared: bool = False):
        """the same losses under the current parameters, no update; return_rec: also the reconstruction [bs, 1, H, W]"""
        x, y = self._xy(clip_img_input, clip_img, prepared)
        rec = torch.empty(self.bs, self.H, self.W, dtype=torch.float32, device=self.device) if return_rec else None
        self._run('eval', ptr(x), ptr(y), ptr(self._losses), ptr(rec))
        l = self._losses.cpu()
        out = (float(l[0]), float(l[1]), float(l[2]))
        return (out + (rec[:, None],)) if return_rec else out

    def last_total(self) -> float:
        return float(self._losses[3].cpu())

    def pool_winners(self) -> List[torch.Tensor]:
        """the max-pool winners of the five encoder blocks in the last forward: [bs, C, Ho, Wo] uint8 taps ky * 3 + kx each"""
        out, h, w = [], self.H, self.W
        for b, c in enumerate((32, 64, 128, 256, 256)):
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            t = torch.empty(self.bs * c * h * w, dtype=torch.uint8, device=self.device)
            self._run('pool_winners', b, ptr(t))
            out.append(t.view(self.bs, c // 8, h, w, 8).permute(0, 1, 4, 2, 3).reshape(self.bs, c, h, w).cpu())
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """the parameters as CPU tensors under the reference's keys (enc_blc1.main.0.weight ... dec_blc5.deconv2.bias)"""
        return unflatten_state(self.flat_params())

    # ---- the loop level: the dataset on the device, one call per epoch (lemo_aetrain_epoch)
    def upload_dataset(self, clips) -> None:
        """clips [N, 4, d, T] (d + 2 = H, T + 16 = W): the unpadded clip images the epochs gather their batches from"""
        t = torch.as_tensor(np.asarray(clips) if not torch.is_tensor(clips) else clips)
        if t.dim() != 4 or tuple(t.shape[1:]) != (4, self.H - 2, self.W - 16) or t.shape[0] < 1:
            raise ValueError(f'expected clips [N, 4, {self.H - 2}, {self.W - 16}], got {tuple(t.shape)}')
        if self.W - 16 < 9:
            raise ValueError('reflect padding by 8 needs clips of more than 8 frames')
        self._data = t.to(self.device, torch.float32).contiguous()

    def upload_prox_masks(self, masks) -> None:
        """the PROX marker masks (1 = visible): what ``load_prox_mask_clips`` returns, [M, L, 67 * 3] with each marker's column
        repeated for its 3 rows, or [M, L, 67]; L >= T.  Kept on the device as [M, 67, L]."""
        m = torch.as_tensor(np.asarray(masks) if not torch.is_tensor(masks) else masks).float()
        if m.dim() != 3 or m.shape[0] < 1 or m.shape[2] not in (67, 201):
            raise ValueError(f'expected masks [M, L, 201] or [M, L, 67], got {tuple(m.shape)}')
        if m.shape[2] == 201:
            m3 = m.reshape(m.shape[0], m.shape[1], 67, 3)
            if not (torch.equal(m3[..., 0], m3[..., 1]) and torch.equal(m3[..., 0], m3[..., 2])):
                raise ValueError("a marker's three mask columns differ: one mask per marker and frame is expected")
            m = m3[..., 0]
        if m.shape[1] < self.W - 16:
            raise ValueError(f'mask clips of {m.shape[1]} frames are shorter than the clips ({self.W - 16} frames)')
        self._masks = m.permute(0, 2, 1).contiguous().to(self.device)

    def _epoch_desc(self, idx, marker_ids=None, mask_idx=None):
        """validates every index on the host (nothing has been launched when it raises) -> (descriptor, the tensors it points into)"""
        data = self._dataset()
        if marker_ids is not None and mask_idx is not None:
            raise ValueError('one masking recipe per call: marker_ids (random markers) or mask_idx (PROX masks)')
        idx = self._index_table(idx, 'idx', 0, data.shape[0])
        n_steps = idx.shape[0]
        keep = [idx.to(self.device)]
        d = _hip.AetrainEpochDesc(data=ptr(data), n_clips=int(data.shape[0]), idx=ptr(keep[0]), n_steps=n_steps, recipe=_hip.MASK_NONE)
        if marker_ids is not None or mask_idx is not None:
            if self.H - 2 != 208:
                raise ValueError(f'the masking recipes are defined for 67 markers (d = 208), the trainer has d = {self.H - 2}')
        if marker_ids is not None:
            ids = torch.as_tensor(np.asarray(marker_ids) if not torch.is_tensor(marker_ids) else marker_ids)
            if ids.dim() == 3 and 1 <= ids.shape[2] < 6:                       # the reference draws 1 - 6 ids per step
                ids = torch.cat([ids, ids.new_full(tuple(ids.shape[:2]) + (6 - ids.shape[2],), -1)], dim=2)
            ids = self._index_table(ids, 'marker_ids', -1, 67, tail=(6,))
            if ids.shape[0] != n_steps:
                raise ValueError(f'marker_ids has {ids.shape[0]} steps, idx {n_steps}')
            keep.append(ids.to(self.device))
            d.recipe, d.marker_ids = _hip.MASK_RANDOM, ptr(keep[-1])
        if mask_idx is not None:
            if self._masks is None:
                raise ValueError('upload_prox_masks first')
            mi = self._index_table(mask_idx, 'mask_idx', 0, self._masks.shape[0])
            if mi.shape[0] != n_steps:
                raise ValueError(f'mask_idx has {mi.shape[0]} steps, idx {n_steps}')
            keep.append(mi.to(self.device))
            d.recipe, d.masks, d.n_masks, d.mask_len, d.mask_idx = (_hip.MASK_PROX, ptr(self._masks), int(self._masks.shape[0]),
                                                                    int(self._masks.shape[2]), ptr(keep[-1]))
        return d, keep

    def fit_epoch(self, idx, marker_ids=None, mask_idx=None) -> torch.Tensor:
        """one training step per row of idx [n_steps, bs] (clips of the uploaded dataset), masked by marker_ids [n_steps, bs, <= 6]
        (random markers, -1 = unused slot) or mask_idx [n_steps, bs] (uploaded PROX masks) or not at all; the batches are
        assembled on the device and the host does not wait between steps.  -> the loss log [n_steps, 4] on the CPU, rows
        (loss_rec_body, loss_rec_body_v, loss_rec_contact_lbl, weighted total).  The RNG stays the caller's."""
        return self._epoch(*self._epoch_desc(idx, marker_ids, mask_idx), True)

    def evaluate_epoch(self, idx, marker_ids=None, mask_idx=None) -> torch.Tensor:
        """the same batches and log under the current parameters, no update (the reference's test-loss loop; average the rows)"""
        return self._epoch(*self._epoch_desc(idx, marker_ids, mask_idx), False)

    def assemble(self, step: int, idx, marker_ids=None, mask_idx=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """the batch of row `step` as the epoch kernels build it: (x [bs, 4, H, W], y [bs, H, W]) on the trainer's device"""
        x, y = self._assemble(*self._epoch_desc(idx, marker_ids, mask_idx), step, (self.bs, 4, self.H, self.W), (self.bs, self.H, self.W))
        return x, y
