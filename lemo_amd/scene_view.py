"""3-D views of fitted bodies on the device (``csrc/view_kernels.hip``): the body standing inside the coloured scene mesh, seen
from the PROX camera or from anywhere else, and the body with its markers as coloured spheres -- what the reference shows with
pyrender in ``temp_prox/renderer.py`` (``--rendering_mode 3d``), with open3d in ``temp_prox/viz/viz_fitting.py`` and in
``vis_opt_amass.py``, one frame at a time on the host.

    v, f, c = load_ply(scene_ply)                                   # float32 [Vs, 3], int32 [Fs, 3], uint8 [Vs, 3] or None
    view = SceneView(body_model.faces, scene_vertices=v, scene_faces=f, scene_colors=c,
                     scene_transform=np.linalg.inv(cam2world))      # the PROX camera, the scene brought into camera space
    img = view(out.vertices)                                        # uint8 [B, 1080, 1920, 3] on the device
    view.set_view(look_at(eye, target, up))                         # another viewpoint; rasters the static layer again
    img, depth, owner = view(verts, spheres=markers, sphere_radius=0.02, sphere_colors=cols, return_depth=True, return_owner=True)

Everything per frame takes and returns device tensors.  ``chunk`` frames go into one set of launches and the workspace is sized by
``chunk``, not by the number of frames; the result does not depend on it, bit for bit.

THE RULES BELOW ARE THIS PROJECT'S OWN.  pyrender's metallic-roughness material, open3d's lighting and its tessellated spheres are
not restated; neither library is part of this project's environment.  "Rule 3 / rule 4 of render.py" are the shading and the
quantisation rules of ``lemo_amd/render.py``'s docstring.

1. Transforms.  A point goes through [R | t] as the raster applies a transform on load: ((m0 x + m1 y) + m2 z) + m3 per row, in
   float32, no contraction.  The scene goes through ``view . scene_transform``, composed on the host in float64 and rounded once to
   float32; bodies and sphere centres go through ``view``.  A ``None`` is the identity and moves nothing.
2. Scene layer (static: rastered at construction and at ``set_view``).  Coverage, depth and face id are ``render.py``'s rule 2 for
   the transformed scene as one frame; normals are ``vertex_normals`` of the transformed scene; with the barycentrics b_i of
   render.py's rule 3, colour_k = ((b0 C0k + b1 C1k) + b2 C2k) shade, C the vertex colour as float32 uint8 / 255,
   shade = min(1, ambient + diffuse lambert) from the interpolated normals, two-sided (rule 3), or 1 with ``scene_lit=False``;
   quantised by rule 4.  Kept per view: the depth key [H, W] and rgb [H, W, 3].
3. Body layer (per frame).  ``BodyRenderer``'s: the same normals, the same walk, the same shade (one device function).  With no
   scene, no spheres and ``view=None`` the image is bit for bit ``BodyRenderer(..., cull_backface=False)``'s over a constant
   background of ``bg_color``, and the depth its ``return_depth``.
4. Spheres (per frame, analytic).  Centre c after rule 1, radius r, ray d = (dx, dy, 1) of the pixel's centre as the raster has it.
   A = d . d = (dx dx + dy dy) + 1; q = c x d; disc = A r^2 - ((q0 q0 + q1 q1) + q2 q2) -- the Lagrange form, which does not subtract
   c . c from (d . c)^2 (at c = 3 m and r = 0.02 m that would lose three digits).  A hit iff disc >= 0;
   Z = (((dx c0 + dy c1) + c2) - sqrt(disc)) / A, which counts iff znear <= Z <= zfar.  Normal n = Z d - c, lambert = |n_z| / |n|,
   shade and quantisation as for the body, with the sphere's own colour (uint8 / 255).  Not drawn at all: a sphere whose centre or
   radius is not finite, with r <= 0, or with c_z - r < znear.  Among spheres with the same Z at a pixel the lowest index wins.
5. Composition.  The nearest Z wins, compared through the raster's keys 0xFFFFFFFF - bits(Z).  On equal keys: the body, then the
   spheres, then the scene.  A pixel nothing covers is ``bg_color``.  ``return_depth``: that Z, 0 where nothing is hit;
   ``return_owner``: -1 background, 0 scene, 1 body, 2 + s sphere s.

The kernel finds the spheres that can reach a pixel tile from a conservative screen bound; that is an optimisation, not part of the
rule (the tests try every sphere at every pixel).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _hip
from ._hip import ptr
from .occlusion import MAX_FRAMES, PROX_RENDER, _cam
from .render import _Topology, _normals_into, _unit, _verts

MAX_SPHERES = 256
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


# ---- host helpers ----------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up) -> np.ndarray:
    """world -> camera [4, 4] float64 of a camera at ``eye`` looking at ``target`` in this project's convention (x right, y down,
    z forward): ``target - eye`` maps onto +z, ``up`` into the -y half plane"""
    eye, target, up = (np.asarray(a, np.float64).reshape(-1) for a in (eye, target, up))
    if any(a.shape != (3,) or not np.all(np.isfinite(a)) for a in (eye, target, up)):
        raise ValueError('eye, target and up are three finite values each')
    z = target - eye
    x = np.cross(-up, z)
    if not np.linalg.norm(z) > 0 or not np.linalg.norm(x) > 1e-12 * np.linalg.norm(z) * np.linalg.norm(up):
        raise ValueError('target must differ from eye and up must not be parallel to the viewing direction')
    z = z / np.linalg.norm(z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, :3] = np.stack([x, y, z])
    m[:3, 3] = -m[:3, :3] @ eye
    return m


def load_ply(path):
    """A triangle mesh from an ``ascii`` or ``binary_little_endian`` PLY file -> (vertices float32 [V, 3], faces int32 [F, 3], colours
    uint8 [V, 3] or None).  Reads the vertex properties x y z and, when all three are there as uchar, red green blue; other vertex
    properties are skipped by their declared size; the face element's ``vertex_indices`` / ``vertex_index`` lists must hold three
    indices each.  Anything else raises ValueError."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.find(b'end_header')
    nl = data.find(b'\n', end)
    if not data.startswith(b'ply') or end < 0 or nl < 0:
        raise ValueError(f'{path}: not a PLY file (no "ply" ... "end_header")')
    fmt, elements = None, []
    for line in data[:end].decode('ascii', 'replace').splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ('comment', 'obj_info'):
            continue
        if w[0] == 'format' and len(w) >= 2:
            fmt = w[1]
        elif w[0] == 'element' and len(w) == 3 and w[2].isdigit():
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property' and elements and len(w) == 3 and w[1] in _PLY_TYPES:
            elements[-1][2].append((w[2], _PLY_TYPES[w[1]], None))
        elif w[0] == 'property' and elements and len(w) == 5 and w[1] == 'list' and w[2] in _PLY_TYPES and w[3] in _PLY_TYPES:
            elements[-1][2].append((w[4], _PLY_TYPES[w[3]], _PLY_TYPES[w[2]]))
        else:
            raise ValueError(f'{path}: header line not understood: {line!r}')
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError(f'{path}: format {fmt!r} is not read (ascii and binary_little_endian are)')
    names = [e[0] for e in elements]
    if 'vertex' not in names or 'face' not in names:
        raise ValueError(f'{path}: needs a vertex and a face element, has {names}')
    body = data[nl + 1:]
    tokens = body.split() if fmt == 'ascii' else None
    pos = 0
    verts = faces = colors = None
    for name, count, props in elements:
        has_list = any(p[2] is not None for p in props)
        if name == 'face':
            if len(props) != 1 or props[0][0] not in ('vertex_indices', 'vertex_index') or props[0][2] is None:
                raise ValueError(f'{path}: the face element must hold one list, vertex_indices or vertex_index')
            _, it, ct = props[0]
            if it[0] == 'f' or ct[0] == 'f':
                raise ValueError(f'{path}: the index list must be of integers')
            if fmt == 'ascii':
                rows = np.asarray(tokens[pos:pos + 4 * count])
                if len(rows) != 4 * count:
                    raise ValueError(f'{path}: the face element is cut short or holds a face that is no triangle')
                try:
                    rows = rows.astype(np.int64).reshape(count, 4)
                except ValueError:
                    raise ValueError(f'{path}: the face element holds something that is no integer') from None
                pos += 4 * count
            else:
                rec = np.dtype([('n', '<' + ct), ('i', '<' + it, (3,))])
                if len(body) < pos + count * rec.itemsize:
                    raise ValueError(f'{path}: the face element is cut short or holds a face that is no triangle')
                raw = np.frombuffer(body, rec, count, pos)
                rows = np.concatenate([raw['n'].astype(np.int64)[:, None], raw['i'].astype(np.int64)], 1)
                pos += count * rec.itemsize
            if count and (rows[:, 0] != 3).any():
                raise ValueError(f'{path}: a face that is no triangle (the lists must hold three indices each)')
            faces = rows[:, 1:]
        elif has_list:
            raise ValueError(f'{path}: element {name} holds a list property; only the face element may')
        else:
            if fmt == 'ascii':
                n = count * len(props)
                if len(tokens) < pos + n:
                    raise ValueError(f'{path}: element {name} is cut short')
                try:
                    table = np.asarray(tokens[pos:pos + n]).astype(np.float64).reshape(count, len(props))
                except ValueError:
                    raise ValueError(f'{path}: element {name} holds something that is no number') from None
                cols = {p[0]: table[:, i] for i, p in enumerate(props)}
                pos += n
            else:
                rec = np.dtype([(p[0], '<' + p[1]) for p in props]) if props else np.dtype([])
                if len(body) < pos + count * rec.itemsize:
                    raise ValueError(f'{path}: element {name} is cut short')
                raw = np.frombuffer(body, rec, count, pos)
                cols = {p[0]: raw[p[0]] for p in props}
                pos += count * rec.itemsize
            if name == 'vertex':
                if not all(k in cols for k in 'xyz'):
                    raise ValueError(f'{path}: the vertex element needs x, y and z')
                verts = np.stack([cols[k] for k in 'xyz'], -1).astype(np.float32)
                kinds = {p[0]: p[1] for p in props}
                if all(kinds.get(k) == 'u1' for k in ('red', 'green', 'blue')):
                    colors = np.stack([cols[k] for k in ('red', 'green', 'blue')], -1).astype(np.uint8)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f'{path}: faces name vertices {int(faces.min())} .. {int(faces.max())}, the mesh has {len(verts)}')
    return np.ascontiguousarray(verts), np.ascontiguousarray(faces, np.int32), colors


def _matrix(m, what, rigid):
    """finite [4, 4] with the last row (0, 0, 0, 1) as float64, or None; ``rigid``: a rotation and a translation"""
    if m is None:
        return None
    m = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
    if m.shape != (4, 4) or m.dtype.kind not in 'fiu' or not np.all(np.isfinite(m)):
        raise ValueError(f'{what} is a finite [4, 4] matrix')
    m = m.astype(np.float64)
    if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f'the last row of {what} must be (0, 0, 0, 1)')
    if rigid and (np.abs(m[:3, :3] @ m[:3, :3].T - np.eye(3)).max() > 1e-4 or np.linalg.det(m[:3, :3]) < 0):
        raise ValueError(f'{what} must be rigid: a rotation (determinant + 1) and a translation')
    return m


def _xf12(m):
    return None if m is None else (C.c_float * 12)(*m[:3].astype(np.float32).reshape(-1).tolist())


def _rgb8(v, what):
    col = tuple(v) if np.ndim(v) == 1 else ()
    if len(col) != 3 or any(int(c) != c or not 0 <= int(c) <= 255 for c in col):
        raise ValueError(f'{what} must be three integers 0 .. 255')
    return tuple(int(c) for c in col)


def _on_device(a, dtype, device, what):
    """numpy array or tensor -> contiguous tensor of dtype on device; a tensor must already be of that dtype"""
    if isinstance(a, torch.Tensor):
        if a.dtype != dtype:
            raise ValueError(f'{what} must be {dtype}, got {a.dtype}')
        return a.detach().to(device).contiguous()
    a = np.asarray(a)
    want = np.dtype({torch.float32: 'f4', torch.uint8: 'u1'}[dtype])
    if a.dtype != want and not (dtype == torch.float32 and a.dtype.kind == 'f'):
        raise ValueError(f'{what} must be {want}, got {a.dtype}')
    return torch.from_numpy(np.ascontiguousarray(a, want)).to(device)


class SceneView:
    """Images of a body mesh (``faces`` [F, 3]) inside an optional static scene mesh, with optional spheres, by the rules of the module
    docstring.  The camera and shading arguments are ``BodyRenderer``'s, with ``cull_backface=False`` by default (scene scans are not
    watertight; the open3d script shows back faces).  ``scene_vertices`` [Vs, 3] float32, ``scene_faces`` [Fs, 3], ``scene_colors``
    uint8 [Vs, 3] or None (then ``scene_color`` for every vertex) -- numpy arrays or tensors; ``scene_lit=False`` shows the vertex
    colours unshaded.  ``view`` [4, 4] rigid world -> camera, ``scene_transform`` [4, 4] applied to the scene before it; ``bg_color``
    uint8 triple.  ``device``: where the static layer lives (default: the current GPU)."""

    def __init__(self, faces, scene_vertices=None, scene_faces=None, scene_colors=None, scene_transform=None, view=None,
                 W: int = PROX_RENDER['W'], H: int = PROX_RENDER['H'], fx: float = PROX_RENDER['fx'], fy: float = PROX_RENDER['fy'],
                 cx: float = PROX_RENDER['cx'], cy: float = PROX_RENDER['cy'], znear: float = 0.05, zfar: float = 100.0,
                 cull_backface: bool = False, base_color=(1.0, 1.0, 0.9), ambient: float = 0.3, diffuse: float = 0.7,
                 bg_color=(255, 255, 255), scene_lit: bool = True, scene_color=(204, 204, 204), chunk: int = 16, device=None,
                 _lib: Optional[_hip.HipLib] = None):
        self.lib = _lib or _hip.get_lib()
        if not 1 <= int(chunk) <= MAX_FRAMES:
            raise ValueError(f'chunk must be 1 .. {MAX_FRAMES} frames')
        self.chunk = int(chunk)
        self._cam = _cam(W, H, fx, fy, cx, cy, znear, zfar, cull_backface)
        base = tuple(base_color) if np.ndim(base_color) == 1 else ()
        if len(base) != 3:
            raise ValueError('base_color must be three values in [0, 1]')
        self._shade = _hip.RenderShade((C.c_float * 3)(*[_unit(v, 'base_color') for v in base]), _unit(ambient, 'ambient'),
                                       _unit(diffuse, 'diffuse'))
        bg = _rgb8(bg_color, 'bg_color')
        self._bg = (bg[0] << 16) | (bg[1] << 8) | bg[2]
        self.scene_lit = bool(scene_lit)
        self.topology = _Topology(faces)
        self.W, self.H = self._cam.W, self._cam.H
        self.device = torch.device(device) if device is not None else \
            torch.device('cpu') if self.lib.is_emu else torch.device('cuda', torch.cuda.current_device())
        self._scene_xf = _matrix(scene_transform, 'scene_transform', rigid=False)
        view = _matrix(view, 'view', rigid=True)
        self._scene = None
        self.scene_key = self.scene_rgb = None
        if scene_vertices is None:
            if scene_faces is not None or scene_colors is not None:
                raise ValueError('scene_faces and scene_colors need scene_vertices')
        else:
            if scene_faces is None:
                raise ValueError('scene_vertices need scene_faces')
            topo = _Topology(scene_faces)
            sv = _on_device(scene_vertices, torch.float32, self.device, 'scene_vertices')
            _hip.check_device(self.lib, sv)
            if sv.dim() != 2 or sv.shape[1] != 3 or sv.shape[0] < topo.vmin or sv.shape[0] > 2 ** 24:
                raise ValueError(f'scene_vertices must be float32 [Vs, 3] with the {topo.vmin} vertices the faces name, got {tuple(sv.shape)}')
            if scene_colors is None:
                sc = torch.tensor(_rgb8(scene_color, 'scene_color'), dtype=torch.uint8).repeat(sv.shape[0], 1).to(self.device)
            else:
                sc = _on_device(scene_colors, torch.uint8, self.device, 'scene_colors')
                if tuple(sc.shape) != tuple(sv.shape):
                    raise ValueError(f'scene_colors must be uint8 {tuple(sv.shape)}, got {tuple(sc.shape)}')
            self._scene = (sv, sc, topo)
        self.set_view(view)

    def set_view(self, view=None):
        """another world -> camera [4, 4] (rigid; None: the identity); rasters the static layer again"""
        self._view = _matrix(view, 'view', rigid=True)
        self._view_xf = _xf12(self._view)
        if self._scene is None:
            return
        lib, dev, (sv, sc, topo) = self.lib, self.device, self._scene
        both = [m for m in (self._view, self._scene_xf) if m is not None]
        s = lib.stream(dev)
        Vs = sv.shape[0]
        verts = sv
        if both:
            m = both[0] @ both[1] if len(both) == 2 else both[0]
            if not np.all(np.isfinite(m[:3].astype(np.float32))):
                raise ValueError('view . scene_transform is not finite in float32')
            verts = torch.empty_like(sv)
            lib.check(lib.view_transform(ptr(sv), Vs, _xf12(m), ptr(verts), s), 'view_transform')
        faces = topo.on(dev, Vs)[0]
        normals = None
        if self.scene_lit:
            normals = torch.empty(1, Vs, 3, dtype=torch.float32, device=dev)
            _normals_into(lib, verts[None], topo, normals, None, 1)
        key = torch.empty(self.H, self.W, dtype=torch.int32, device=dev)
        ids = torch.empty(self.H, self.W, dtype=torch.int32, device=dev)
        rgb = torch.empty(self.H, self.W, 3, dtype=torch.uint8, device=dev)
        cam = C.byref(self._cam)
        lib.check(lib.render_ids(ptr(verts), 1, Vs, ptr(faces), faces.shape[0], cam, ptr(key), ptr(ids), None, s), 'render_ids')
        lib.check(lib.view_scene_resolve(ptr(verts), ptr(normals), Vs, ptr(faces), faces.shape[0], cam, ptr(ids), ptr(sc), self._shade.ambient,
                                         self._shade.diffuse, int(self.scene_lit), ptr(rgb), s), 'view_scene_resolve')
        self.scene_key, self.scene_rgb = key, rgb

    def _spheres(self, spheres, sphere_radius, sphere_colors, B, dev):
        if spheres is None:
            return None, None, None, 0
        if not isinstance(spheres, torch.Tensor):
            raise ValueError('spheres must be a torch tensor on the device')
        _hip.check_device(self.lib, spheres)
        if spheres.dim() != 3 or spheres.shape[-1] != 3 or spheres.dtype != torch.float32 or spheres.shape[0] != B or \
                not 1 <= spheres.shape[1] <= MAX_SPHERES:
            raise ValueError(f'spheres must be float32 [B = {B}, P, 3] with 1 <= P <= {MAX_SPHERES}, got {spheres.dtype} {tuple(spheres.shape)}')
        if spheres.device != dev:
            raise ValueError('spheres and vertices are on different devices')
        P = spheres.shape[1]
        if np.ndim(sphere_radius) == 0 and not isinstance(sphere_radius, torch.Tensor):
            radius = torch.full((P,), float(sphere_radius), dtype=torch.float32, device=dev)
        else:
            radius = _on_device(sphere_radius, torch.float32, dev, 'sphere_radius')
            if tuple(radius.shape) != (P,):
                raise ValueError(f'sphere_radius must be a number or float32 [P = {P}], got {tuple(radius.shape)}')
        if sphere_colors is None:
            raise ValueError('spheres need sphere_colors, uint8 [P, 3] or [B, P, 3]')
        cols = _on_device(sphere_colors, torch.uint8, dev, 'sphere_colors')
        if tuple(cols.shape) not in ((P, 3), (B, P, 3)):
            raise ValueError(f'sphere_colors must be uint8 [{P}, 3] or [{B}, {P}, 3], got {tuple(cols.shape)}')
        return spheres.detach().contiguous(), radius, cols, P

    def __call__(self, vertices: torch.Tensor, spheres: Optional[torch.Tensor] = None, sphere_radius=0.02, sphere_colors=None,
                 return_depth: bool = False, return_owner: bool = False):
        """vertices [B, V, 3] float32 in world coordinates -> uint8 [B, H, W, 3]; ``spheres`` [B, P <= 256, 3] float32 world centres
        with ``sphere_radius`` (a number or [P]) and ``sphere_colors`` uint8 [P, 3] or [B, P, 3].  Optional further outputs, in this
        order: depth float32 [B, H, W] (the nearest of all layers, 0: nothing), owner int32 [B, H, W] (-1 background, 0 scene, 1 body,
        2 + s sphere s)."""
        lib, topo = self.lib, self.topology
        verts = _verts(lib, vertices, topo.vmin)
        B, V = verts.shape[:2]
        dev = verts.device
        if self._scene is not None and dev != self.scene_key.device:
            raise ValueError('vertices and the scene are on different devices')
        sph, radius, cols, P = self._spheres(spheres, sphere_radius, sphere_colors, B, dev)
        H, W, n = self.H, self.W, min(B, self.chunk)
        faces = topo.on(dev, V)[0]
        img = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
        depth = torch.empty(B, H, W, dtype=torch.float32, device=dev) if return_depth else None
        owner = torch.empty(B, H, W, dtype=torch.int32, device=dev) if return_owner else None
        keys = torch.empty(n, H, W, dtype=torch.int32, device=dev)
        ids = torch.empty(n, H, W, dtype=torch.int32, device=dev)
        normals = torch.empty(n, V, 3, dtype=torch.float32, device=dev)
        moved = torch.empty(n, V, 3, dtype=torch.float32, device=dev) if self._view is not None else None
        s = lib.stream(dev)
        cam = C.byref(self._cam)
        for lo in range(0, B, self.chunk):
            hi = min(B, lo + self.chunk)
            sub = lambda t: None if t is None else ptr(t[lo:hi])
            v = verts[lo:hi]
            if moved is not None:
                lib.check(lib.view_transform(ptr(v), (hi - lo) * V, self._view_xf, ptr(moved), s), 'view_transform')
                v = moved[:hi - lo]
            _normals_into(lib, v, topo, normals, None, self.chunk)
            lib.check(lib.render_ids(ptr(v), hi - lo, V, ptr(faces), faces.shape[0], cam, ptr(keys), ptr(ids), None, s), 'render_ids')
            lib.check(lib.view_compose(ptr(v), ptr(normals), hi - lo, V, ptr(faces), faces.shape[0], cam, ptr(keys), ptr(ids),
                                       C.byref(self._shade), ptr(self.scene_key), ptr(self.scene_rgb), sub(sph), P, ptr(radius),
                                       ptr(cols) if cols is None or cols.dim() == 2 else sub(cols), int(cols is None or cols.dim() == 2),
                                       self._view_xf, self._bg, sub(img), sub(depth), sub(owner), s), 'view_compose')
        extra = tuple(t for t in (depth, owner) if t is not None)
        return (img,) + extra if extra else img
