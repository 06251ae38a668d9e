"""What the Python owners of the native engines share: the guarded release of a native handle from ``__del__``, the base
class of the two fitting engines and the tensor conversion of their ``load_state``."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _hip


def release_on_del(device, lib, destroy, event=None) -> None:
    """``_hip.release`` from a ``__del__``.  An engine's buffers are torch tensors allocated on the default stream but written by
    graph replays on whatever stream its steps ran on.  When the last reference goes, the caching allocator may hand those
    blocks to the next default-stream allocation at once -- while a replay is still in flight they would be written from two
    places -- so the handle is destroyed (and the buffers let go) only after the engine's last launch."""
    rel = getattr(_hip, 'release', None) if _hip is not None else None
    if rel is None:                  # interpreter shutdown: module globals are gone, the process is about to exit
        return
    rel(device, lib, destroy, event)


class NativeEngine(_hip.StreamOrdered):
    """An engine object that owns one native handle (``self.handle``, made by the subclass's constructor next to ``self.lib``
    and ``self.device``) and launches on the current stream."""
    _destroy = ''                    # name of the library call that frees the handle ('fit_destroy', ...)

    def _s(self):
        return self.lib.stream(self.device)

    def __del__(self, _release=release_on_del):      # (bound here: a default outlives the module's globals)
        h, self.handle = getattr(self, 'handle', None), None
        if h:
            destroy = getattr(self.lib, self._destroy)
            _release(self.device, self.lib, lambda: destroy(h), getattr(self, '_run_ev', None))


def state_tensors(state: Dict, spec: Sequence[Tuple[str, int]], B: int, device) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """``state[k]`` (numpy array or tensor) of every ``(k, width)`` of ``spec`` as a contiguous float32 [B, width] tensor on
    ``device``, and ``state['step']`` (an int or a tensor) as an int32 [1] tensor: what ``lemo_*_load_state`` reads."""
    t = {k: (state[k].detach() if isinstance(state[k], torch.Tensor) else torch.as_tensor(np.asarray(state[k], np.float32))
             ).to(device, torch.float32).reshape(B, w).contiguous() for k, w in spec}
    sv = state['step']
    step = (sv.detach().to(device, torch.int32).reshape(1) if isinstance(sv, torch.Tensor)
            else torch.full((1,), int(sv), dtype=torch.int32, device=device))
    return t, step
