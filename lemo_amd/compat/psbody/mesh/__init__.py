"""Stand-in for ``psbody.mesh``: a ``Mesh`` that holds ``v`` / ``f`` and the ``visibility`` module, served by
``csrc/visibility_kernels.hip``.  Nothing else of the package exists here."""
import numpy as np

from . import visibility  # noqa: F401


class Mesh:
    """``Mesh(v=, f=)`` with ``.v`` (float64 [V, 3]) and ``.f`` (uint32 [F, 3]), as fitting_temp_slide.py:645-646 builds it"""

    def __init__(self, v=None, f=None, **_ignored):
        self.v = None if v is None else np.array(v, dtype=np.float64)
        self.f = None if f is None else np.array(f, dtype=np.uint32)
