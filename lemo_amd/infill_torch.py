"""The infilling prior's training step in plain torch, on the reference's state_dict keys and in any dtype: models/AE.py
AE(downsample=True, in_channel=4, kernel=3) and the loss of train_infill_prior.py:185-203.  The yardstick the native trainer
(infill_train.InfillPriorTrainer) is measured against: its tests in float64, tools/infill_train_rate.py as torch fp32 autograd.

``winners`` (optional): per encoder block the max-pool winners to route through, [bs, C, Ho, Wo] taps ky * 3 + kx (what
InfillPriorTrainer.pool_winners returns) instead of the maxima this computation finds itself.  Max pooling is discontinuous
where two window entries are within rounding of each other; forcing one computation's winners on another compares the two on
the same branch of the function.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from .infill_train import param_layout


def _pool(h: torch.Tensor, taps: Optional[torch.Tensor]) -> torch.Tensor:
    pooled = F.max_pool2d(h, 3, 2, 1)
    if taps is None:
        return pooled
    H, W = h.shape[-2:]
    Ho, Wo = pooled.shape[-2:]
    t = taps.to(h.device).long()
    yo = torch.arange(Ho, device=h.device).view(Ho, 1)
    xo = torch.arange(Wo, device=h.device).view(1, Wo)
    flat = (2 * yo - 1 + t // 3) * W + (2 * xo - 1 + t % 3)
    return h.flatten(2).gather(2, flat.flatten(2)).reshape(pooled.shape)


def ae_forward(sd: Dict[str, torch.Tensor], x: torch.Tensor, winners: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
    """x [bs, 4, H, W] -> rec [bs, 1, H, W]"""
    h, sizes = x, [x.shape]
    for b in range(1, 6):
        k = f'enc_blc{b}.main.'
        h = F.leaky_relu(F.conv2d(h, sd[k + '0.weight'], sd[k + '0.bias'], padding=1), 0.2)
        h = F.leaky_relu(F.conv2d(h, sd[k + '2.weight'], sd[k + '2.bias'], padding=1), 0.2)
        h = _pool(h, None if winners is None else winners[b - 1])
        sizes.append(h.shape)
    for b in range(1, 6):
        k = f'dec_blc{b}.'
        out = sizes[5 - b]
        op = (out[-2] - ((h.shape[-2] - 1) * 2 + 1), out[-1] - ((h.shape[-1] - 1) * 2 + 1))    # ConvTranspose2d(output_size=out)
        h = F.leaky_relu(F.conv_transpose2d(h, sd[k + 'deconv1.weight'], sd[k + 'deconv1.bias'], stride=2, padding=1, output_padding=op), 0.2)
        h = F.conv_transpose2d(h, sd[k + 'deconv2.weight'], sd[k + 'deconv2.bias'], stride=1, padding=1)
        if b < 5:
            h = F.leaky_relu(h, 0.2)
    return h


def losses(rec: torch.Tensor, y: torch.Tensor):
    """rec [bs, 1, H, W], y [bs, H, W] -> (L_body, L_v, L_c) as train_infill_prior.py:192-198 computes them"""
    y = y[:, None]
    yv = y[..., 1:] - y[..., :-1]
    rv = rec[..., 1:] - rec[..., :-1]
    lb = F.l1_loss(y[:, 0, 0:-5], rec[:, 0, 0:-5])
    lv = F.l1_loss(yv[:, 0, 0:-5], rv[:, 0, 0:-5])
    lc = F.binary_cross_entropy_with_logits(rec[:, 0, -5:], y[:, 0, -5:])
    return lb, lv, lc


def total(rec, y, weights=(10., 10., 1.)):
    lb, lv, lc = losses(rec, y)
    return lb, lv, lc, weights[0] * lb + weights[1] * lv + weights[2] * lc
