"""Training sets of the two motion priors, built on the device from AMASS clips.

The reference builds them on the host, clip by clip (``loader/train_loader_infill.py:87-330``,
``loader/train_loader_smooth.py:83-204``): SMPL-X forward, first-frame canonicalisation, foot-contact labels, the
heading-normalised local representation, a Gaussian filter, then dataset-wide statistics and normalisation.  Here

    clips = read_amass(amass_dir, ['HumanEva', 'CMU'])                       # numpy, the reference's clip division
    builder = ClipImageBuilder({'male': m, 'female': f}, mode='local_markers_4chan')
    images, info = builder.build(clips)                                       # [N, 4, d, T-1] on the device
    trainer.upload_dataset(images)

replaces ``TrainLoader.read_data`` / ``create_body_repr``.  The SMPL-X forward runs on the marker vertices and three joints
only (the active-vertex path of the fitting engine), ``chunk`` clips per call; everything after it is
``csrc/dataset_kernels.hip``, one workgroup per clip.  ``images`` has the layout ``InfillPriorTrainer.upload_dataset``
(``'local_markers_4chan'``) / ``SmoothPriorTrainer.upload_dataset`` (``'local_markers'``: [N, 1, d, T]) take, and stays on
the device; ``info['rot_0_pivot']`` and ``info['contact']`` are what ``loader/optimize_loader_amass_new.py`` hands the
fitting side.

The smoothness prior every fit uses was trained on a third representation, the smoothness loader's default
``global_markers`` (``train_loader_smooth.py:164-167, 184-194``): the markers alone, relative to marker 0 of frame 0 in the
first frame's heading, d = 3 M rows (243 with hands), every row normalised with the set's own mean and one scalar standard
deviation -- the image the fit loop feeds ``Enc`` (``opt_amass_temp.py:366-380``).  ``local_markers`` is NOT that image.

    builder = SmoothClipImageBuilder({'male': m, 'female': f}, with_hand=True)   # body_mode='global_markers'
    images, info = builder.build(clips)                                       # [N, 1, 3 M, T] on the device
    SmoothPriorTrainer(enc, dec, H=3 * 81 + 2, W=T - 1 + 16).upload_dataset(images)
    save_stats(path, info['stats'])                                           # Xmean (1, 1, d) float32, Xstd (d,) float64

``info['stats']`` is what ``AmassTemporalFitter(enc_state, Xmean, Xstd, ...)`` takes, so a prior retrained on someone's own
AMASS split runs in the fit loop with that split's statistics.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _hip
from ._hip import ptr
from .assets import load_vertex_ids
from .body_model import alloc_pose_ws

MODES = {'local_markers_4chan': _hip.CLIP_4CHAN, 'local_markers': _hip.CLIP_SMOOTH}
SAMPLE_RATE = {150: 5, 120: 4, 60: 2}            # train_loader_infill.py:43-50: every other framerate is skipped
T_MAX = 256
STATS_KEYS_4CHAN = ('Xmean_local', 'Xstd_local', 'Xmean_global_xy', 'Xstd_global_xy', 'Xmean_global_r', 'Xstd_global_r')


def divide_clips(sequences: Sequence[Dict], clip_seconds: int = 4) -> List[Dict]:
    """``TrainLoader.divide_clip`` (train_loader_infill.py:31-74) on sequences already read: dicts with ``poses`` [N, 156],
    ``trans`` [N, 3], ``betas``, ``gender`` and ``mocap_framerate``.  ``int(N / clip_len)`` clips of ``clip_seconds`` seconds per
    sequence, sampled down to 30 fps; sequences of another framerate than 150 / 120 / 60 or shorter than one clip give none."""
    out = []
    for seq in sequences:
        fps = int(seq['mocap_framerate'])
        if fps not in SAMPLE_RATE:
            continue
        clip_len, rate = clip_seconds * fps, SAMPLE_RATE[fps]
        poses, trans = np.asarray(seq['poses']), np.asarray(seq['trans'])
        n = len(poses)
        if n < clip_len:
            continue
        for i in range(int(n / clip_len)):
            out.append(dict(trans=trans[clip_len * i:clip_len * (i + 1)][::rate], poses=poses[clip_len * i:clip_len * (i + 1)][::rate],
                            betas=np.asarray(seq['betas'])[:10], gender=str(seq['gender']), mocap_framerate=fps))
    return out


def read_amass(amass_dir: str, dataset_names: Sequence[str], clip_seconds: int = 4) -> List[Dict]:
    """``TrainLoader.read_data``: the ``*/*_poses.npz`` files of every named dataset under ``amass_dir``, divided into clips."""
    clips = []
    for name in dataset_names:
        seqs = []
        for fname in glob.glob(os.path.join(amass_dir, name, '*/*_poses.npz')):
            with np.load(fname) as z:
                seqs.append({k: z[k] for k in ('poses', 'trans', 'betas', 'gender', 'mocap_framerate')})
        clips += divide_clips(seqs, clip_seconds)
    return clips


def save_stats(path: str, stats: Dict[str, np.ndarray]) -> None:
    """npz with the reference's key names (``preprocess_stats/*.npz``): read by the reference and by ``lemo_amd.assets``"""
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in stats.items()})


def load_stats(path: str) -> Dict[str, np.ndarray]:
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


class ClipImageBuilder:
    """``models``: ``lemo_amd`` SMPL-X modules per gender, created with ``use_pca=False, flat_hand_mean=True`` like the
    reference's loaders do."""

    _MODES = MODES

    def __init__(self, models: Dict[str, object], mode: str = 'local_markers_4chan', with_hand: bool = False, clip_fps: int = 30,
                 chunk: int = 256, device=None, _lib: Optional[_hip.HipLib] = None):
        if mode not in self._MODES:
            raise ValueError(f'mode must be one of {sorted(self._MODES)}, got {mode!r}')
        if not models or any(g not in ('male', 'female', 'neutral') for g in models):
            raise ValueError("models: {'male': ..., 'female': ...}")
        if int(chunk) < 1:
            raise ValueError('chunk must be at least 1 clip')
        for g, m in models.items():
            if m.use_pca:
                raise ValueError(f'the {g} model was created with use_pca=True: AMASS poses carry 45 values per hand')
        self.models, self.mode, self.with_hand, self.clip_fps, self.chunk = dict(models), mode, bool(with_hand), float(clip_fps), int(chunk)
        self.lib = _lib or _hip.get_lib()
        self.device = torch.device('cpu') if self.lib.is_emu else torch.device(device if device is not None else 'cuda:0')
        self.marker_ids = np.asarray(load_vertex_ids()['markers81' if with_hand else 'markers67'], np.int64)
        for g, m in models.items():
            if int(self.marker_ids.max()) >= m.data.V:
                raise ValueError(f'the {g} model has {m.data.V} vertices, the marker set reaches vertex {int(self.marker_ids.max())}')
        self.M = len(self.marker_ids)
        self._mode_id = self._MODES[mode]
        self.d = self._rows()

    def _rows(self) -> int:
        return 3 * (self.M + 1) + (4 if self.mode == 'local_markers_4chan' else 0)

    # ---- host-side validation: nothing is launched before it has passed -------------------------------------------------------
    def _validate(self, clips) -> int:
        if len(clips) < 1:
            raise ValueError('no clips')
        T = None
        for i, c in enumerate(clips):
            poses, trans = np.asarray(c['poses']), np.asarray(c['trans'])
            if poses.ndim != 2 or poses.shape[1] != 156:
                raise ValueError(f'clip {i}: poses must be [T, 156] (3 + 63 + 45 + 45), got {poses.shape}')
            if trans.shape != (poses.shape[0], 3):
                raise ValueError(f'clip {i}: trans must be [{poses.shape[0]}, 3], got {trans.shape}')
            if T is None:
                T = poses.shape[0]
            if poses.shape[0] != T:
                raise ValueError(f'clip {i} has {poses.shape[0]} frames, clip 0 has {T}: clips of one set have one length')
            if not 2 <= T <= T_MAX:
                raise ValueError(f'clips of {T} frames: the builder takes 2 to {T_MAX}')
            if str(c['gender']) not in self.models:
                raise ValueError(f'clip {i}: gender {str(c["gender"])!r} has no model (have {sorted(self.models)})')
            if np.asarray(c['betas']).reshape(-1).shape[0] < 10:
                raise ValueError(f'clip {i}: fewer than 10 betas')
        return T

    def _stats_vector(self, stats) -> torch.Tensor:
        d = self.d
        v = np.zeros(2 * d + 4, np.float64)
        try:
            if self.mode == 'local_markers_4chan':
                v[:d], v[d:2 * d] = np.asarray(stats['Xmean_local'], np.float64).reshape(-1), np.asarray(stats['Xstd_local'], np.float64).reshape(-1)
                v[2 * d:] = [float(stats[k]) for k in STATS_KEYS_4CHAN[2:]]
            else:
                v[:d], v[d:2 * d] = np.asarray(stats['Xmean'], np.float64).reshape(-1), np.asarray(stats['Xstd'], np.float64).reshape(-1)
                v[2 * d], v[2 * d + 1] = v[d + 3], v[d]
        except (KeyError, ValueError) as e:
            raise ValueError(f'statistics do not fit mode {self.mode!r} with d = {d}: {e}') from None
        return torch.from_numpy(v).to(self.device)

    def _stats_dict(self, vec: torch.Tensor) -> Dict[str, np.ndarray]:
        v, d = vec.cpu().numpy(), self.d
        if self.mode == 'local_markers_4chan':
            return dict(Xmean_local=v[:d].copy(), Xstd_local=v[d:2 * d].copy(), Xmean_global_xy=np.float64(v[2 * d]),
                        Xstd_global_xy=np.float64(v[2 * d + 1]), Xmean_global_r=np.float64(v[2 * d + 2]), Xstd_global_r=np.float64(v[2 * d + 3]))
        return dict(Xmean=v[:d].reshape(1, 1, d).copy(), Xstd=v[d:2 * d].copy())

    # ---- SMPL-X on the marker vertices and joints 0-2 only ----------------------------------------------------------------
    def _forward(self, model, poses: torch.Tensor, trans: torch.Tensor, betas: torch.Tensor):
        """poses [B, 156], trans [B, 3], betas [B, 10] on the device -> (markers [B, M, 3], joints 0-2 [B, 3, 3])"""
        lib, dev = self.lib, model._device_body(self.device)
        d, B = dev.data, poses.shape[0]
        s = lib.stream(self.device)
        ws, tt, Bp = alloc_pose_ws(B, d.nj, self.device, dev.blend_f16)
        z = lambda n: torch.zeros(B, n, dtype=torch.float32, device=self.device)
        go, body = poses[:, 0:3].contiguous(), poses[:, 3:66].contiguous()
        lh, rh = poses[:, 66:111].contiguous(), poses[:, 111:156].contiguous()
        jaw, leye, reye, expr = z(3), z(3), z(3), z(10)
        pin = _hip.PoseIn(ptr(go), ptr(body), ptr(jaw), ptr(leye), ptr(reye), ptr(lh), ptr(rh), 45, ptr(betas), betas.shape[1], ptr(expr))
        lib.check(lib.smplx_pose_fwd(C.byref(dev.body), C.byref(pin), C.byref(ws), B, s), 'smplx_pose_fwd')
        uset, keep = dev.vertex_set(('dataset', self.M), self.marker_ids)
        blend = torch.empty(B, uset.NCs, dtype=torch.float32, device=self.device)
        verts = torch.empty(B, self.M, 3, dtype=torch.float32, device=self.device)
        lib.check(lib.lbs_verts_fwd_active(C.byref(dev.skin), C.byref(uset), ptr(tt['Xg']), Bp, ptr(tt['A']), d.nj, ptr(trans), B,
                                           ptr(blend), ptr(verts), None, s), 'lbs_verts_fwd_active')
        joints = tt['Jtr'][:, 0:3] + trans[:, None]
        del keep
        return verts, joints

    def _markers(self, clips, T):
        """world-frame markers [N, T, M, 3], pelvis [N, T, 3] and first-frame hips [N, 2, 3] of all clips, ``chunk`` clips per
        forward and gender"""
        N, dev = len(clips), self.device
        markers = torch.empty(N, T, self.M, 3, dtype=torch.float32, device=dev)
        pelvis = torch.empty(N, T, 3, dtype=torch.float32, device=dev)
        hips0 = torch.empty(N, 2, 3, dtype=torch.float32, device=dev)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        for lo in range(0, N, self.chunk):
            part = list(range(lo, min(N, lo + self.chunk)))
            for g, model in self.models.items():
                idx = [i for i in part if str(clips[i]['gender']) == g]
                if not idx:
                    continue
                poses = f32(np.concatenate([np.asarray(clips[i]['poses']) for i in idx]))
                trans = f32(np.concatenate([np.asarray(clips[i]['trans']) for i in idx]))
                betas = f32(np.concatenate([np.tile(np.asarray(clips[i]['betas']).reshape(-1)[:10], (T, 1)) for i in idx]))
                v, j = self._forward(model, poses, trans, betas)
                sel = torch.as_tensor(idx, device=dev)
                markers[sel] = v.view(len(idx), T, self.M, 3)
                j = j.reshape(len(idx), T, 3, 3)
                pelvis[sel] = j[:, :, 0]
                hips0[sel] = j[:, 0, 1:3]
        return markers, pelvis, hips0

    # ---- the native chain on markers that are already there (also the tests' way in) ----------------------------------------
    def _desc(self, markers, pelvis, hips0, lo, hi, **kw):
        return _hip.ClipReprDesc(markers=ptr(markers[lo:hi]), pelvis=ptr(pelvis[lo:hi]), hips0=ptr(hips0[lo:hi]), n_clips=hi - lo,
                                 T=markers.shape[1], M=self.M, mode=self._mode_id, fps=self.clip_fps, **kw)

    def _check_markers(self, markers, pelvis, hips0):
        if markers.dim() != 4 or markers.shape[2:] != (self.M, 3) or markers.shape[0] < 1:
            raise ValueError(f'markers must be [N, T, {self.M}, 3], got {tuple(markers.shape)}')
        N, T = markers.shape[:2]
        if not 2 <= T <= T_MAX:
            raise ValueError(f'clips of {T} frames: the builder takes 2 to {T_MAX}')
        if tuple(pelvis.shape) != (N, T, 3) or tuple(hips0.shape) != (N, 2, 3):
            raise ValueError(f'pelvis must be [{N}, {T}, 3] and hips0 [{N}, 2, 3], got {tuple(pelvis.shape)} and {tuple(hips0.shape)}')
        dev = lambda a: a.detach().to(self.device, torch.float32).contiguous()
        return dev(markers), dev(pelvis), dev(hips0)

    def stats_from_markers(self, markers, pelvis, hips0) -> torch.Tensor:
        """statistics vector [2 d + 4] (float64, device) of the clips' unnormalised images"""
        markers, pelvis, hips0 = self._check_markers(markers, pelvis, hips0)
        lib, N, T = self.lib, markers.shape[0], markers.shape[1]
        s = lib.stream(self.device)
        K = lib.clip_repr_stats_k(self.M, self._mode_id)
        part = torch.empty(N, K, dtype=torch.float64, device=self.device)
        for lo in range(0, N, self.chunk):
            hi = min(N, lo + self.chunk)
            d = self._desc(markers, pelvis, hips0, lo, hi, stats_part=ptr(part[lo:hi]))
            lib.check(lib.clip_repr_stats(C.byref(d), s), 'clip_repr_stats')
        out = torch.empty(2 * self.d + 4, dtype=torch.float64, device=self.device)
        lib.check(lib.clip_repr_stats_reduce(ptr(part), N, T, self.M, self._mode_id, ptr(out), s), 'clip_repr_stats_reduce')
        return out

    def images_from_markers(self, markers, pelvis, hips0, stats_vec: Optional[torch.Tensor] = None, api_layout: bool = False):
        """(images, rot_0_pivot [N] float64 or None, contact [N, T, 4] or None); ``stats_vec`` None: unnormalised"""
        markers, pelvis, hips0 = self._check_markers(markers, pelvis, hips0)
        lib, N, T = self.lib, markers.shape[0], markers.shape[1]
        s = lib.stream(self.device)
        four = self.mode == 'local_markers_4chan'
        F, Cn = (T - 1, 4) if four else (T, 1)
        img = torch.empty((N, Cn, F, self.d) if api_layout else (N, Cn, self.d, F), dtype=torch.float32, device=self.device)
        piv = torch.empty(N, dtype=torch.float64, device=self.device) if four else None
        con = torch.empty(N, T, 4, dtype=torch.float32, device=self.device) if four else None
        if stats_vec is not None:
            stats_vec = stats_vec.to(self.device, torch.float64).contiguous()
            if stats_vec.shape != (2 * self.d + 4,):
                raise ValueError(f'statistics vector must have {2 * self.d + 4} entries')
        for lo in range(0, N, self.chunk):
            hi = min(N, lo + self.chunk)
            d = self._desc(markers, pelvis, hips0, lo, hi, stats=ptr(stats_vec), image=ptr(img[lo:hi]), api_layout=int(api_layout),
                           rot_0_pivot=ptr(piv[lo:hi]) if four else None, contact=ptr(con[lo:hi]) if four else None)
            lib.check(lib.clip_repr_write(C.byref(d), s), 'clip_repr_write')
        return img, piv, con

    # ---- public ---------------------------------------------------------------------------------------------------------
    def compute_stats(self, clips) -> Dict[str, np.ndarray]:
        T = self._validate(clips)
        return self._stats_dict(self.stats_from_markers(*self._markers(clips, T)))

    def _saved(self, vec: torch.Tensor) -> torch.Tensor:
        """the statistics vector as the images are normalised with it: what ``_stats_dict`` hands out"""
        return vec

    def build(self, clips, stats: Optional[Dict] = None, normalize: bool = True, api_layout: bool = False):
        """-> (images, info).  ``stats=None`` is the reference's train split (statistics of these clips, then normalisation);
        passing statistics is its test split; ``normalize=False`` gives the unnormalised images; ``api_layout=True`` gives
        [N, C, F, d] (frame-major rows) instead of the trainers' [N, C, d, F]."""
        T = self._validate(clips)
        vec = self._stats_vector(stats) if (stats is not None and normalize) else None
        markers, pelvis, hips0 = self._markers(clips, T)
        if normalize and vec is None:
            vec = self._saved(self.stats_from_markers(markers, pelvis, hips0))
        img, piv, con = self.images_from_markers(markers, pelvis, hips0, vec if normalize else None, api_layout=api_layout)
        info = dict(stats=self._stats_dict(vec) if vec is not None else None, rot_0_pivot=piv, contact=con)
        return img, info

    save_stats = staticmethod(save_stats)
    load_stats = staticmethod(load_stats)


SMOOTH_BODY_MODES = {'global_markers': _hip.CLIP_GLOBAL}


class SmoothClipImageBuilder(ClipImageBuilder):
    """The smoothness prior's own training set, ``train_loader_smooth.py``'s default ``--body_mode global_markers``: images
    [N, 1, 3 M, T] (M = 67, or 81 ``with_hand``), every row ``(p - marker 0 of frame 0) . R0`` of a marker coordinate,
    normalised with the per-row mean and ONE standard deviation of the whole set.  Chunking, gender mixing, the active-vertex
    forward and the validation are ``ClipImageBuilder``'s; statistics carry the reference's keys, shapes and dtypes
    (``Xmean`` (1, 1, d) float32, ``Xstd`` (d,) float64), and the images are normalised with exactly those (the float32
    ``Xmean``), so that ``build(clips, stats=info['stats'])`` repeats ``build(clips)`` bit for bit."""

    _MODES = SMOOTH_BODY_MODES

    def __init__(self, models: Dict[str, object], with_hand: bool = True, body_mode: str = 'global_markers', clip_fps: int = 30,
                 chunk: int = 256, device=None, _lib: Optional[_hip.HipLib] = None):
        if body_mode in ('global_joints', 'local_joints'):
            raise ValueError(f'body_mode {body_mode!r} is not built here: the joint representations need all 55 regressed joints of '
                             f'every frame, i.e. the all-vertex SMPL-X forward, and no shipped prior was trained on them')
        if body_mode in MODES:
            raise ValueError(f'body_mode {body_mode!r} is ClipImageBuilder(mode={body_mode!r})')
        super().__init__(models, mode=body_mode, with_hand=with_hand, clip_fps=clip_fps, chunk=chunk, device=device, _lib=_lib)

    def _rows(self) -> int:
        return 3 * self.M

    def _stats_vector(self, stats) -> torch.Tensor:
        d = self.d
        try:
            mean, std = np.asarray(stats['Xmean'], np.float64).reshape(-1), np.asarray(stats['Xstd'], np.float64).reshape(-1)
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f'statistics do not fit mode {self.mode!r}: {e!r}') from None
        if mean.shape != (d,) or std.shape != (d,):
            raise ValueError(f'statistics do not fit mode {self.mode!r} with d = {d}: Xmean has {mean.size} entries, Xstd {std.size}')
        v = np.zeros(2 * d + 4, np.float64)
        v[:d], v[d:2 * d], v[2 * d], v[2 * d + 1] = mean, std, std[0], std[0]
        return torch.from_numpy(v).to(self.device)

    def _stats_dict(self, vec: torch.Tensor) -> Dict[str, np.ndarray]:
        v, d = vec.cpu().numpy(), self.d
        return dict(Xmean=v[:d].reshape(1, 1, d).astype(np.float32), Xstd=v[d:2 * d].copy())

    def _saved(self, vec: torch.Tensor) -> torch.Tensor:
        return self._stats_vector(self._stats_dict(vec))

    def build(self, clips, stats: Optional[Dict] = None, normalize: bool = True, api_layout: bool = False):
        """-> (images [N, 1, 3 M, T], info); ``api_layout=True``: [N, T, 3 M], the frame-major rows the fit loop feeds the
        encoder.  ``info['rot_0_pivot']`` and ``info['contact']`` are None: this representation has neither."""
        img, info = super().build(clips, stats=stats, normalize=normalize, api_layout=api_layout)
        return (img[:, 0] if api_layout else img), info
