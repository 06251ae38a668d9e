"""Stand-in for ``psbody.mesh.visibility``: ``visibility_compute(v=, f=, cams=)`` with the reference's call shape
(fitting_temp_slide.py:648-649) -- numpy in, numpy out, one mesh per call.  It uploads the mesh, runs
``lemo_amd.scan.vertex_visibility`` (``csrc/visibility_kernels.hip``) once per camera and downloads the answer; new code should call
``vertex_visibility`` on the whole batch instead.  There is no CPU path: without the HIP library the call raises.

``n_dot`` is NOT computed: the reference ignores it, and without normals psbody's own value is not used either; zeros are returned
in its place.  The definition of visibility is the one ``lemo_amd.scan`` states: recalled from psbody's source, not confirmed by a
run."""
import numpy as np
import torch

_lib = None          # tests only: the host-emulated library (it takes CPU tensors and nothing else)


def visibility_compute(v=None, f=None, cams=None, min_dist=1e-3, **unsupported):
    """-> ``(vis uint32 [n_cams, V], n_dot float64 [n_cams, V] of zeros)``"""
    if unsupported:
        raise NotImplementedError(f'visibility_compute: {sorted(unsupported)} are not supported (no normals, sensors or extra meshes)')
    from .... import _hip
    from ....scan import vertex_visibility
    lib = _lib if _lib is not None else _hip.get_lib()
    v, f, cams = np.asarray(v, np.float64), np.asarray(f), np.asarray(cams, np.float64).reshape(-1, 3)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f'visibility_compute: v must be [V, 3] and f [F, 3], got {v.shape} and {f.shape}')
    dev = torch.device('cpu') if lib.is_emu else torch.device('cuda', torch.cuda.current_device())
    n = cams.shape[0]
    verts = torch.from_numpy(np.broadcast_to(v.astype(np.float32), (n,) + v.shape).copy()).to(dev)
    vis = vertex_visibility(verts, f.astype(np.int64), cam=cams.astype(np.float32), min_dist=min_dist, _lib=lib)
    return vis.cpu().numpy().astype(np.uint32), np.zeros((n, v.shape[0]), np.float64)
