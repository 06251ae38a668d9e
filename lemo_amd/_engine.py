"""What the Python owners of the native engines share: the one owner of a native handle and its guarded release, the base class of
the two fitting engines, the tensor conversion of their ``load_state``, and the base class of the two prior trainers."""
from __future__ import annotations

import ctypes
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import ptr


def release_on_del(device, lib, destroy, event=None) -> None:
    """``_hip.release`` from a ``__del__``.  An engine's buffers are torch tensors allocated on the default stream but written by
    graph replays on whatever stream its steps ran on.  When the last reference goes, the caching allocator may hand those
    blocks to the next default-stream allocation at once -- while a replay is still in flight they would be written from two
    places -- so the handle is destroyed (and the buffers let go) only after the engine's last launch."""
    rel = getattr(_hip, 'release', None) if _hip is not None else None
    if rel is None:                  # interpreter shutdown: module globals are gone, the process is about to exit
        return
    rel(device, lib, destroy, event)


class NativeHandle:
    """The owner of one native handle: ``self.handle`` (``self.h`` is the same attribute, the name the trainers and the finetune
    session use), made by the subclass's constructor next to ``self.lib`` and ``self.device``.  It is released once, from ``__del__``
    or earlier by whoever calls that: after the owner's last launch (its ``_run_ev`` where it tracks one, the whole device otherwise),
    or parked while a stream capture is going on (``_hip.release``)."""
    _destroy = ''                    # name of the library call that frees the handle ('fit_destroy', ...)
    _held: Tuple[str, ...] = ()      # attributes (the buffers the native side writes) a parked release holds until it has run
    handle = None
    h = property(lambda self: self.handle, lambda self, v: setattr(self, 'handle', v))

    def _s(self):
        return self.lib.stream(self.device)

    def __del__(self, _release=release_on_del):      # (bound here: a default outlives the module's globals)
        h, self.handle = self.handle, None
        if h:
            def destroy(h=h, fn=getattr(self.lib, self._destroy), keep=tuple(getattr(self, k, None) for k in self._held)):
                fn(h)
            _release(self.device, self.lib, destroy, getattr(self, '_run_ev', None))


class NativeEngine(NativeHandle, _hip.StreamOrdered):
    """An engine object that launches on the current stream (the two fitters)."""


def state_tensors(state: Dict, spec: Sequence[Tuple[str, int]], B: int, device) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """``state[k]`` (numpy array or tensor) of every ``(k, width)`` of ``spec`` as a contiguous float32 [B, width] tensor on
    ``device``, and ``state['step']`` (an int or a tensor) as an int32 [1] tensor: what ``lemo_*_load_state`` reads."""
    t = {k: (state[k].detach() if isinstance(state[k], torch.Tensor) else torch.as_tensor(np.asarray(state[k], np.float32))
             ).to(device, torch.float32).reshape(B, w).contiguous() for k, w in spec}
    sv = state['step']
    step = (sv.detach().to(device, torch.int32).reshape(1) if isinstance(sv, torch.Tensor)
            else torch.full((1,), int(sv), dtype=torch.int32, device=device))
    return t, step


class PriorTrainer(NativeHandle):
    """What the two prior trainers share (smooth_train.SmoothPriorTrainer on ``lemo_sptrain_*``, infill_train.InfillPriorTrainer on
    ``lemo_aetrain_*``): the construction plumbing, the stream hand-over, parameters and gradients out, the epoch call and its one
    read-back, batch assembly, checkpoints and the release.  A subclass names its ABI prefix and says how a batch is made."""
    _prefix = ''                     # 'sptrain' / 'aetrain': every native call is lemo_<prefix>_<name>(handle, ..., stream)
    _nloss = 0                       # floats of the loss block (the terms, then the weighted total)
    _n_param = None                  # () -> length of the flat parameter vector
    _destroy = property(lambda self: self._prefix + '_destroy')
    _held = ('ws',)
    _data = None                     # the uploaded dataset (upload_dataset)

    def __init__(self, desc_type, batch, H, W, device, use_graph, lib, refused, **hyper):
        self.lib = lib or _hip.get_lib()
        if device is None:
            device = torch.device('cpu') if self.lib.is_emu else torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        self.bs, self.H, self.W = int(batch), int(H), int(W)
        # the engine runs on a stream of its own (a graph cannot be captured on the legacy default stream); every call orders it
        # after the caller's current stream and the caller's stream after it
        self.stream = None if self.lib.is_emu else torch.cuda.Stream(self.device)
        nws = getattr(self.lib, self._prefix + '_ws_floats')(self.H, self.W, self.bs)
        if nws <= 0:
            raise ValueError(refused)
        self.ws = torch.zeros(int(nws), dtype=torch.float32, device=self.device)
        d = desc_type(H=self.H, W=self.W, bs=self.bs, ws=ptr(self.ws), ws_floats=int(nws),
                      use_graph=int(bool(use_graph) and not self.lib.is_emu), **hyper)
        self.handle = getattr(self.lib, self._prefix + '_create')(ctypes.byref(d))
        if not self.handle:
            raise _hip.LemoHipError(f'lemo_{self._prefix}_create failed')
        self._losses = torch.zeros(self._nloss, dtype=torch.float32, device=self.device)

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

    def _run(self, name, *args):
        """lemo_<prefix>_<name>(handle, *args, stream) on the trainer's stream, checked"""
        name = f'{self._prefix}_{name}'
        return self._call(lambda s: self.lib.check(getattr(self.lib, name)(self.handle, *args, s), name))

    def _load(self, flat: np.ndarray) -> None:
        """the parameters (flat order) into the engine, with a fresh optimiser"""
        t = torch.from_numpy(flat).to(self.device)
        self._run('load', ptr(t))

    def _flat_out(self, name, n) -> torch.Tensor:
        out = torch.empty(int(n), dtype=torch.float32, device=self.device)
        self._run(name, ptr(out))
        return out.cpu()

    def flat_params(self) -> torch.Tensor:
        return self._flat_out('params', self._n_param())

    def flat_grads(self) -> torch.Tensor:
        """the gradient of the last training step (the infilling prior's: summed over the batch), in the flat order"""
        return self._flat_out('grads', self._n_param())

    # ---- the loop level: the dataset on the device, one call per epoch (lemo_*train_epoch)
    def _dataset(self) -> torch.Tensor:
        if self._data is None:
            raise ValueError('upload_dataset first')
        return self._data

    def _index_table(self, t, name, lo, hi, tail=()):
        """[n_steps, bs, *tail] integers in [lo, hi) -> int32 on the CPU; ValueError otherwise (nothing has been launched)"""
        t = torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f'{name} must be an integer tensor')
        t = t.cpu().long()
        if t.dim() != 2 + len(tail) or t.shape[1] != self.bs or tuple(t.shape[2:]) != tuple(tail) or t.shape[0] < 1:
            raise ValueError(f'{name}: expected [n_steps, {self.bs}{"".join(", %d" % v for v in tail)}], got {tuple(t.shape)}')
        if int(t.min()) < lo or int(t.max()) >= hi:
            raise ValueError(f'{name} holds values outside [{lo}, {hi})')
        return t.to(torch.int32).contiguous()

    def _epoch(self, d, keep, train):
        """(descriptor, the tensors it points into) of the subclass's _epoch_desc -> the loss log [n_steps, _nloss] on the CPU"""
        log = torch.zeros(d.n_steps, self._nloss, dtype=torch.float32, device=self.device)
        d.log, d.train = ptr(log), int(train)
        self._run('epoch', ctypes.byref(d))
        out = log.cpu()                                                        # the epoch's one host wait (keeps `keep` alive until then)
        del keep
        return out

    def _assemble(self, d, keep, step, *shapes):
        """the batch of row `step` as the epoch kernels build it: one tensor per shape, on the trainer's device"""
        if not 0 <= int(step) < d.n_steps:
            raise ValueError(f'step {step} outside [0, {d.n_steps})')
        out = [torch.empty(*shp, dtype=torch.float32, device=self.device) for shp in shapes]
        self._run('batch', ctypes.byref(d), int(step), *(ptr(t) for t in out))
        _hip.quiesce(self.device, self.lib)                                    # the index tables (`keep`) are released on return
        return out

    def _state_floats(self) -> int:
        return int(getattr(self.lib, self._prefix + '_state_floats')())

    def save_state(self) -> torch.Tensor:
        """parameters, both Adam moments and the step counter as one flat CPU tensor (include/lemo_hip.h has the layout)"""
        return self._flat_out('state_save', self._state_floats())

    def load_state(self, blob: torch.Tensor) -> None:
        """restore what save_state returned: training continues bit-identically"""
        n = self._state_floats()
        if not torch.is_tensor(blob) or blob.dtype != torch.float32 or blob.dim() != 1 or blob.numel() != n:
            raise ValueError(f'a training state is a flat float32 tensor of {n} values')
        t = blob.to(self.device).contiguous()
        self._run('state_load', ptr(t))
        _hip.quiesce(self.device, self.lib)

    def close(self):
        """release the engine now (idempotent): after everything queued on the device, or -- while a stream is being captured --
        parked with the workspace until the capture is over"""
        NativeHandle.__del__(self)
