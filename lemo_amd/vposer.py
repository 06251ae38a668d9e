"""``VPoser`` on the HIP kernels, with the reference's call surface.

Reference: human_body_prior/train/vposer_smpl.py:65-171 (``VPoser``; ``encode`` :91-105, ``decode`` :107-121,
``forward`` :123-141, ``sample_poses`` :143-150, ``matrot2aa`` / ``aa2matrot`` :152-171) and
human_body_prior/tools/model_loader.py:43-72 (``load_vposer``).
LEMO's fitting loops call ``vposer.decode(Z, output_type='aa')`` (utils/utils.py:148; temp_prox/fitting_temp_slide.py:243);
``encode`` is the way from a body pose to the 32-D latent a fit starts from (:func:`embed_body_pose`).  Both run in
``liblemo_hip.so`` in eval mode only; the parameters stay ``nn`` modules so that reference ``state_dict``s load with all keys
matched, and are packed for the kernels on first use.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _hip
from ._hip import ptr


class _DecodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, lib, Z, want_aa: bool):
        Z = Z.contiguous().float()
        _hip.check_device(lib, Z)
        B, dev = Z.shape[0], Z.device
        w = owner._packed(dev)
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        h1, h2, o = e(B, 512), e(B, 512), e(B, 128)
        matrot, aa = e(B, 21, 9), e(B, 63)
        lib.check(lib.vposer_decode_fwd(C.byref(w['struct']), ptr(Z), Z.shape[1], B, ptr(h1), ptr(h2), ptr(o),
                                        ptr(matrot), ptr(aa), lib.stream(dev)), 'vposer_decode_fwd')
        ctx.owner, ctx.lib, ctx.saved, ctx.want_aa = owner, lib, (h1, h2, o), want_aa
        return aa.view(B, 1, 21, 3) if want_aa else matrot.view(B, 1, 21, 9)

    @staticmethod
    def backward(ctx, g):
        h1, h2, o = ctx.saved
        B, dev = h1.shape[0], h1.device
        w = ctx.owner._packed(dev)
        g = g.contiguous().float()
        dz = torch.empty(B, 32, dtype=torch.float32, device=dev)
        d_aa, d_m = (ptr(g), None) if ctx.want_aa else (None, ptr(g))
        scratch = torch.empty(B, 1152, dtype=torch.float32, device=dev)
        ctx.lib.check(ctx.lib.vposer_decode_bwd(C.byref(w['struct']), ptr(h1), ptr(h2), ptr(o), d_aa, d_m, B, ptr(dz),
                                                32, ptr(scratch), ctx.lib.stream(dev)), 'vposer_decode_bwd')
        return None, None, dz, None


BN_EPS = 1e-5
ENC_KEYS = tuple(f'bodyprior_enc_{n}' for n in ('bn1.weight', 'bn1.bias', 'bn1.running_mean', 'bn1.running_var', 'fc1.weight', 'fc1.bias',
                                                'bn2.weight', 'bn2.bias', 'bn2.running_mean', 'bn2.running_var', 'fc2.weight', 'fc2.bias',
                                                'mu.weight', 'mu.bias', 'logvar.weight', 'logvar.bias'))
"""the encoder's entries of a VPoser ``state_dict`` that the eval-mode forward reads"""


def _fragment_order(W: np.ndarray) -> np.ndarray:
    """row-major [M][K] (both multiples of 16) -> P[K/16][M/16][64][4]: lane 16 q + i of (chunk c, tile mt) holds
    W[16 mt + i][16 c + 4 q .. + 3], the A operand of four v_mfma_f32_16x16x4_f32 (csrc/vposer_enc_kernels.hip)"""
    M, K = W.shape
    assert M % 16 == 0 and K % 16 == 0
    return np.ascontiguousarray(W.reshape(M // 16, 16, K // 16, 4, 4).transpose(2, 0, 3, 1, 4)).reshape(-1)


def fold_vposer_enc(sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """the eval-mode encoder as three plain layers: BatchNorm (running statistics, eps 1e-5) folded into the layer behind it in
    float64 and rounded to float32 ONCE.  bn(x) = x s + t with s = gain / sqrt(var + eps), t = shift - mean s, so
    fc(bn(x)) = (W diag(s)) x + (b + W t).  Returns w1 [512][64] (column 63 zero), b1, w2 [512][512], b2, wh [64][512] (mu rows
    0..31, logvar rows 32..63), bh -- float32."""
    g = lambda k: np.asarray(sd['bodyprior_enc_' + k], np.float64)
    out = {}
    for i, n_in in ((1, 64), (2, 512)):
        s = g(f'bn{i}.weight') / np.sqrt(g(f'bn{i}.running_var') + BN_EPS)
        t = g(f'bn{i}.bias') - g(f'bn{i}.running_mean') * s
        W = g(f'fc{i}.weight')
        Wf = np.zeros((512, n_in))
        Wf[:, :W.shape[1]] = W * s[None, :]
        out[f'w{i}'], out[f'b{i}'] = Wf.astype(np.float32), (g(f'fc{i}.bias') + W @ t).astype(np.float32)
    out['wh'] = np.concatenate([g('mu.weight'), g('logvar.weight')]).astype(np.float32)
    out['bh'] = np.concatenate([g('mu.bias'), g('logvar.bias')]).astype(np.float32)
    return out


def pack_vposer_enc(sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """``lemo_vposer_enc_w`` as float32 arrays, keyed by its field names: the folded layers (:func:`fold_vposer_enc`) and their
    transposes in fragment order, and the three bias vectors"""
    f = fold_vposer_enc(sd)
    out = {}
    for a, b in (('w1', 'w1'), ('w2', 'w2'), ('wh', 'wh')):
        out[a + 'p'], out[a + 'tp'] = _fragment_order(f[b]), _fragment_order(np.ascontiguousarray(f[b].T))
    out.update(b1=f['b1'], b2=f['b2'], bh=f['bh'])
    return out


def vposer_enc_weight_struct(sd: Dict[str, np.ndarray], device):
    """Pack ``bodyprior_enc_*`` arrays -> (ctypes struct, tensors that own its memory)."""
    tt = {k: torch.from_numpy(v).to(device) for k, v in pack_vposer_enc(sd).items()}
    return _hip.VPoserEncW(**{k: ptr(v) for k, v in tt.items()}), tt


class _EncodeFn(torch.autograd.Function):
    """(mean, std) of the eval-mode encoder: lemo_vposer_encode_fwd / _bwd, one launch each"""

    @staticmethod
    def forward(ctx, owner, lib, X):
        X = X.contiguous().float()
        _hip.check_device(lib, X)
        assert X.dim() == 2 and X.shape[1] == 63, f'VPoser.encode takes 21 x 3 axis-angle values per pose, got {tuple(X.shape)}'
        B, dev = X.shape[0], X.device
        w = owner._packed_enc(dev)
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        mean, std, h1, h2, lv = e(B, 32), e(B, 32), e(B, 512), e(B, 512), e(B, 32)
        lib.check(lib.vposer_encode_fwd(C.byref(w['struct']), ptr(X), 63, B, ptr(mean), ptr(std), 32, ptr(h1), ptr(h2), ptr(lv),
                                        lib.stream(dev)), 'vposer_encode_fwd')
        ctx.owner, ctx.lib, ctx.saved = owner, lib, (h1, h2, lv)
        return mean, std

    @staticmethod
    def backward(ctx, g_mean, g_std):
        h1, h2, lv = ctx.saved
        B, dev = h1.shape[0], h1.device
        w = ctx.owner._packed_enc(dev)
        g = [None if t is None else t.contiguous().float() for t in (g_mean, g_std)]
        dx = torch.empty(B, 63, dtype=torch.float32, device=dev)
        ctx.lib.check(ctx.lib.vposer_encode_bwd(C.byref(w['struct']), ptr(h1), ptr(h2), ptr(lv), ptr(g[0]), ptr(g[1]), 32, B, ptr(dx), 63,
                                                ctx.lib.stream(dev)), 'vposer_encode_bwd')
        return None, None, dx


class VPoser(nn.Module):
    """state_dict-compatible with vposer_smpl.py:75-89; ``encode`` and ``decode`` run in liblemo_hip.so (eval mode)."""

    def __init__(self, num_neurons=512, latentD=32, data_shape=(1, 21, 3), use_cont_repr=True,
                 _lib: Optional[_hip.HipLib] = None):
        super().__init__()
        assert num_neurons == 512 and latentD == 32 and tuple(data_shape)[1] == 21 and use_cont_repr, \
            'kernels are specialised to VPoser v1.0 (512 neurons, 32-D latent, 21 joints)'
        self.latentD, self.num_joints, self.use_cont_repr = latentD, 21, True
        n_features = int(np.prod(data_shape))
        self.bodyprior_enc_bn1 = nn.BatchNorm1d(n_features)
        self.bodyprior_enc_fc1 = nn.Linear(n_features, num_neurons)
        self.bodyprior_enc_bn2 = nn.BatchNorm1d(num_neurons)
        self.bodyprior_enc_fc2 = nn.Linear(num_neurons, num_neurons)
        self.bodyprior_enc_mu = nn.Linear(num_neurons, latentD)
        self.bodyprior_enc_logvar = nn.Linear(num_neurons, latentD)
        self.bodyprior_dec_fc1 = nn.Linear(latentD, num_neurons)
        self.bodyprior_dec_fc2 = nn.Linear(num_neurons, num_neurons)
        self.bodyprior_dec_out = nn.Linear(num_neurons, self.num_joints * 6)
        self._lib_override = _lib
        self._pack_cache = {}
        self._pack_cache_enc = {}

    def _packed(self, device):
        """decoder weights in the kernels' layouts (both orientations), cached per (device, version)."""
        ps = [self.bodyprior_dec_fc1.weight, self.bodyprior_dec_fc1.bias, self.bodyprior_dec_fc2.weight,
              self.bodyprior_dec_fc2.bias, self.bodyprior_dec_out.weight, self.bodyprior_dec_out.bias]
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in ps)
        if self._pack_cache.get('key') != key:
            t = [p.detach().to(device=device, dtype=torch.float32).contiguous() for p in ps]
            w3 = torch.zeros(128, 512, dtype=torch.float32, device=device); w3[:126] = t[4]
            b3 = torch.zeros(128, dtype=torch.float32, device=device); b3[:126] = t[5]
            tt = dict(w1=t[0], w1t=t[0].t().contiguous(), b1=t[1], w2=t[2], w2t=t[2].t().contiguous(), b2=t[3],
                      w3=w3, w3t=w3.t().contiguous(), b3=b3)
            st = _hip.VPoserW(*[ptr(tt[k]) for k in ('w1', 'w1t', 'b1', 'w2', 'w2t', 'b2', 'w3', 'w3t', 'b3')])
            self._pack_cache = dict(key=key, tensors=tt, struct=st)
        return self._pack_cache

    def _packed_enc(self, device):
        """encoder parameters folded and packed for lemo_vposer_encode_* (:func:`pack_vposer_enc`), cached per (device, versions of
        the parameters AND of the BatchNorm running statistics): loading another state_dict repacks"""
        ts = [getattr(getattr(self, k[:k.index('.')]), k[k.index('.') + 1:]) for k in ENC_KEYS]
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in ts)
        if self._pack_cache_enc.get('key') != key:
            st, tt = vposer_enc_weight_struct({k: t.detach().cpu().numpy() for k, t in zip(ENC_KEYS, ts)}, device)
            self._pack_cache_enc = dict(key=key, tensors=tt, struct=st)
        return self._pack_cache_enc

    def _eval_only(self, what):
        if self.training:
            raise RuntimeError(f'{what} on the HIP path is the eval() forward (dropout = identity, '
                               'model_loader.py:70); call .eval() first')

    def encode(self, Pin):
        """vposer_smpl.py:91-105 in eval mode: Pin [N, 1, 21, 3], [N, 21, 3] or [N, 63] (axis-angle) -> Normal(mean, std), [N, 32]
        each; differentiable with respect to Pin"""
        self._eval_only('encode')
        lib = self._lib_override or _hip.get_lib()
        mean, std = _EncodeFn.apply(self, lib, Pin.reshape(Pin.shape[0], -1))
        return torch.distributions.normal.Normal(mean, std)

    def forward(self, Pin, input_type='matrot', output_type='matrot', eps=None):
        """vposer_smpl.py:123-141: encode -> sample -> decode.  ``eps`` [N, 32] (not in the reference) fixes the sample to
        ``mean + std * eps``; without it the sample is ``q_z.rsample()``."""
        assert output_type in ['matrot', 'aa']
        q_z = self.encode(Pin)
        q_z_sample = q_z.rsample() if eps is None else q_z.mean + q_z.scale * eps
        results = {'mean': q_z.mean, 'std': q_z.scale}
        results['pose_aa' if output_type == 'aa' else 'pose_matrot'] = self.decode(q_z_sample, output_type=output_type)
        return results

    def sample_poses(self, num_poses, output_type='aa', seed=None):
        """vposer_smpl.py:143-150: decode ``num_poses`` draws of N(0, I) from numpy's generator seeded with ``seed``"""
        np.random.seed(seed)
        w = self.bodyprior_dec_fc1.weight
        self.eval()
        with torch.no_grad():
            Zgen = torch.tensor(np.random.normal(0., 1., size=(num_poses, self.latentD)), dtype=w.dtype).to(w.device)
        return self.decode(Zgen, output_type=output_type)

    @staticmethod
    def matrot2aa(pose_matrot, _lib=None):
        """vposer_smpl.py:152-161: [N, 1, num_joints, 9] -> [N, 1, num_joints, 3].  The first two columns of a rotation matrix are
        its 6-D form, so this is the 6-D -> axis-angle kernel of lemo_amd.rotation."""
        from .rotation import convert_to_3D_all
        N = pose_matrot.shape[0]
        return convert_to_3D_all(pose_matrot.reshape(-1, 3, 3)[:, :, :2].reshape(-1, 6), _lib).view(N, 1, -1, 3)

    @staticmethod
    def aa2matrot(pose):
        """vposer_smpl.py:163-171: [N, 1, num_joints, 3] -> [N, 1, num_joints, 9]"""
        from .rotation import angle_axis_to_rotation_matrix
        N = pose.shape[0]
        return angle_axis_to_rotation_matrix(pose.reshape(-1, 3))[:, :3, :3].contiguous().view(N, 1, -1, 9)

    def decode(self, Zin, output_type='matrot'):
        assert output_type in ['matrot', 'aa']
        self._eval_only('decode')
        lib = self._lib_override or _hip.get_lib()
        return _DecodeFn.apply(self, lib, Zin, output_type == 'aa')


def vposer_weight_struct(weights: Dict[str, np.ndarray], device):
    """Pack ``bodyprior_dec_*`` arrays for the fitting engine -> (ctypes struct, tensors)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    w1, w2, w3 = (np.asarray(weights[f'bodyprior_dec_{n}.weight'], np.float32) for n in ('fc1', 'fc2', 'out'))
    w3p = np.zeros((128, 512), np.float32); w3p[:126] = w3            # out layer padded 126 -> 128 rows
    b3p = np.zeros(128, np.float32); b3p[:126] = np.asarray(weights['bodyprior_dec_out.bias'], np.float32)
    tt = dict(w1=t(w1), w1t=t(w1.T), b1=t(weights['bodyprior_dec_fc1.bias']),
              w2=t(w2), w2t=t(w2.T), b2=t(weights['bodyprior_dec_fc2.bias']),
              w3=t(w3p), w3t=t(w3p.T), b3=t(b3p))
    st = _hip.VPoserW(*[ptr(tt[k]) for k in ('w1', 'w1t', 'b1', 'w2', 'w2t', 'b2', 'w3', 'w3t', 'b3')])
    return st, tt


def make_vposer_weights(seed: int = 2) -> Dict[str, np.ndarray]:
    """Seeded ``nn.Linear``-style init of the decoder (no VPoser checkpoint ships with the
    reference -- SURVEY 8(d)); identical stream to ``oracle.lemo_oracle.make_vposer_weights``."""
    import math
    g = torch.Generator().manual_seed(seed)
    w = {}
    for name, (fin, fout) in (('bodyprior_dec_fc1', (32, 512)), ('bodyprior_dec_fc2', (512, 512)),
                              ('bodyprior_dec_out', (512, 126))):
        bound = 1.0 / math.sqrt(fin)
        w[name + '.weight'] = ((torch.rand(fout, fin, generator=g) * 2 - 1) * bound).numpy()
        w[name + '.bias'] = ((torch.rand(fout, generator=g) * 2 - 1) * bound).numpy()
    return w


def make_vposer_enc_weights(seed: int = 2) -> Dict[str, np.ndarray]:
    """Seeded encoder parameters (:data:`ENC_KEYS`), next to :func:`make_vposer_weights`: ``nn.Linear``-style layers and BatchNorm
    terms that are far from the identity, so that a dropped term or a wrong eps changes the output at once -- running means of
    order 0.3, running variances log-uniform over 0.05 .. 4, gains 1 +- 0.3, shifts of order 0.2."""
    import math
    g = torch.Generator().manual_seed(1000 + seed)
    w = {}
    for name, (fin, fout) in (('fc1', (63, 512)), ('fc2', (512, 512)), ('mu', (512, 32)), ('logvar', (512, 32))):
        bound = 1.0 / math.sqrt(fin)
        w[f'bodyprior_enc_{name}.weight'] = ((torch.rand(fout, fin, generator=g) * 2 - 1) * bound).numpy()
        w[f'bodyprior_enc_{name}.bias'] = ((torch.rand(fout, generator=g) * 2 - 1) * bound).numpy()
    for name, n in (('bn1', 63), ('bn2', 512)):
        w[f'bodyprior_enc_{name}.running_mean'] = (torch.randn(n, generator=g) * 0.3).numpy()
        w[f'bodyprior_enc_{name}.running_var'] = torch.exp(torch.rand(n, generator=g) * math.log(80.0) + math.log(0.05)).numpy()
        w[f'bodyprior_enc_{name}.weight'] = (1.0 + (torch.rand(n, generator=g) * 2 - 1) * 0.3).numpy()
        w[f'bodyprior_enc_{name}.bias'] = (torch.randn(n, generator=g) * 0.2).numpy()
    return w


def embed_body_pose(vposer: 'VPoser', body_pose: torch.Tensor):
    """``body_pose`` [B, 63] (or [B, 21, 3]) axis-angle -> ``(pose_embedding [B, 32], reproj_err [B])``: the encoder mean -- what a
    fit that optimises the latent starts from when only a pose is known -- and, per frame, the largest absolute difference in
    radians between ``body_pose`` and ``decode(pose_embedding, 'aa')``: how far from the prior's manifold the pose lies."""
    bp = body_pose.reshape(body_pose.shape[0], -1)
    mean = vposer.encode(bp).mean
    with torch.no_grad():
        err = (vposer.decode(mean.detach(), output_type='aa').reshape(bp.shape[0], -1) - bp.detach().float()).abs().amax(1)
    return mean, err


def _read_vposer_settings(expr_dir):
    """the experiment's ``*.ini`` (what ``configer.Configer`` reads at model_loader.py:36-39): returns a namespace with at
    least num_neurons / latentD / data_shape; the released vposer_v1_0 values when the file or a key is missing"""
    import ast
    import configparser
    vals = dict(num_neurons=512, latentD=32, data_shape=[1, 21, 3])
    inis = sorted(glob.glob(os.path.join(expr_dir, '*.ini')))
    if inis:
        cp = configparser.ConfigParser()
        cp.read(inis[0])
        for sec in cp.sections():
            for k, v in cp.items(sec):
                try:
                    val = ast.literal_eval(v)
                except Exception:
                    val = v
                for name in ('num_neurons', 'latentD', 'data_shape'):
                    if k.lower() == name.lower():
                        vals[name] = list(val) if name == 'data_shape' else int(val)
                    elif k not in vals:
                        vals.setdefault(k, val)
    ps = type('ps', (), vals)()
    ps.best_model_fname = None
    return ps


def load_vposer(expr_dir, vp_model='snapshot'):
    """``human_body_prior.tools.model_loader.load_vposer`` (model_loader.py:43-72): returns ``(vposer, ps)`` with the
    newest ``snapshots/*.pt`` of ``expr_dir`` loaded, in eval mode.  ``ps`` carries the settings of the experiment's
    ``*.ini`` (``num_neurons``, ``latentD``, ``data_shape``, ...), like the reference's ``Configer``.  ``vp_model``:
    ``'snapshot'`` (default) -- the reference would exec the directory's ``vposer_*.py`` to get the class that was trained;
    here the HIP-backed :class:`VPoser` is that class (same ``state_dict`` keys), after checking that the settings match
    what it implements -- or a class to instantiate instead (model_loader.py:66-67)."""
    if not os.path.exists(expr_dir):
        raise ValueError('Could not find the experiment directory: %s' % expr_dir)
    snaps = sorted(glob.glob(os.path.join(expr_dir, 'snapshots', '*.pt')), key=os.path.getmtime)
    if not snaps:
        raise FileNotFoundError(f'no VPoser snapshot under {expr_dir}/snapshots')
    ps = _read_vposer_settings(expr_dir)
    ps.best_model_fname = snaps[-1]
    cls = VPoser if isinstance(vp_model, str) else vp_model
    if cls is VPoser and (ps.num_neurons != 512 or ps.latentD != 32 or list(ps.data_shape)[-2:] != [21, 3]):
        raise NotImplementedError(f'lemo_amd.VPoser implements vposer_v1_0 (512 / 32 / [1,21,3]); {expr_dir} says '
                                  f'{ps.num_neurons} / {ps.latentD} / {ps.data_shape}')
    vp = cls(num_neurons=ps.num_neurons, latentD=ps.latentD, data_shape=tuple(ps.data_shape))
    vp.load_state_dict(torch.load(snaps[-1], map_location='cpu'))
    vp.eval()
    return vp, ps
