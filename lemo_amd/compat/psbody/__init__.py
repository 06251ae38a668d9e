"""Stand-in for the ``psbody`` package: only ``psbody.mesh`` (``Mesh``, ``visibility.visibility_compute``), which is all that
fitting_temp_slide.py:642-652 imports."""
from . import mesh  # noqa: F401
