"""Stand-in for the ``mesh_intersection`` package (torch-mesh-isect) with the call shapes of fit_temp_loadprox_slide.py:326-344 and
fitting_temp_slide.py:625-635, served from ``lemo_amd.selfpen`` (``csrc/selfpen_kernels.hip``).  The behaviour is the one that module
states; conformance to the package itself is not verified."""
from . import bvh_search_tree, filter_faces, loss  # noqa: F401

_lib = None          # tests only: the host-emulated library (it takes CPU tensors and nothing else)


def _get_lib():
    from ... import _hip
    return _lib if _lib is not None else _hip.get_lib()
