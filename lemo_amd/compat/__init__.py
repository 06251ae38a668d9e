"""Import-compatible stand-ins for the third-party modules LEMO's hot path imports.

    import lemo_amd.compat.smplx as smplx         # smplx.create / smplx.lbs.lbs / smplx.lbs.transform_mat
    import lemo_amd.compat.chamfer as chamfer     # chamfer.forward / backward on device tensors (csrc/chamfer_kernels.hip)
    import lemo_amd.compat.psbody.mesh            # Mesh, visibility.visibility_compute (csrc/visibility_kernels.hip)
    import lemo_amd.compat.mesh_intersection      # bvh_search_tree.BVH, filter_faces.FilterFaces, loss.DistanceFieldPenetrationLoss (csrc/selfpen_kernels.hip)

``install()`` registers them under the reference's own import names so that ``import smplx`` /
``from smplx.lbs import lbs`` / ``import chamfer`` / ``from psbody.mesh.visibility import visibility_compute`` inside LEMO resolve here.
"""
import sys


def install(force: bool = False) -> None:
    """``sys.modules['smplx']``, ``['smplx.lbs']``, ``['chamfer']``, ``['psbody']``, ``['psbody.mesh']`` and
    ``['psbody.mesh.visibility']``, ``['mesh_intersection']`` and its ``bvh_search_tree`` / ``loss`` / ``filter_faces`` -> this package (existing entries are kept unless ``force``)."""
    from . import chamfer, mesh_intersection, psbody, smplx
    from .psbody import mesh
    from .psbody.mesh import visibility
    from .smplx import lbs
    for name, mod in (('smplx', smplx), ('smplx.lbs', lbs), ('chamfer', chamfer), ('psbody', psbody), ('psbody.mesh', mesh),
                      ('psbody.mesh.visibility', visibility), ('mesh_intersection', mesh_intersection),
                      ('mesh_intersection.bvh_search_tree', mesh_intersection.bvh_search_tree), ('mesh_intersection.loss', mesh_intersection.loss),
                      ('mesh_intersection.filter_faces', mesh_intersection.filter_faces)):
        if force or name not in sys.modules:
            sys.modules[name] = mod
