"""RaycastingScene: o3d.t.geometry.RaycastingScene's queries on one mesh handle.

    scene = RaycastingScene()
    scene.add_triangles(mesh)                  # a holder with .vertices / .triangles, a _lib.Mesh, or (vertices, triangles)
    scene.cast_rays(rays)                      # the closest hit                                   
    scene.count_intersections(rays)            # how many triangles a ray crosses                  (s4.24)
    scene.list_intersections(rays)             # every crossing, per ray by t then triangle index  (s4.24)
    scene.test_occlusions(rays, tnear, tfar)   # whether a crossing lies in [tnear, tfar]          (s4.24)
    scene.compute_closest_points(points), compute_distance(points)                                 (s4.16)
    scene.compute_signed_distance(points), compute_occupancy(points)                               (s4.18)

The scene holds ONE geometry: add_triangles returns 0, a second call raises NotImplementedError.  Rays are ... x 6
[origin | direction] and points ... x 3, numpy arrays or CUDA tensors; results take the leading shape and the caller's
kind, as surface_distance's do.  Shapes and bounds are checked before the device is touched: the device mesh is built by
the first query.  The all-hits queries' rule is the cast's own pair test (edges inclusive), not Embree's.
"""
import ctypes as C

import numpy as np

from . import _lib, surface_distance as sd
from ._bridge import as_array, as_kind, device_of, empty, launch, ptr

MAX_RAYS = (1 << 31) - 17      # the all-hits queries' bound


def _leading_rays(name, rays):
    """(leading shape, number of rays) of a query's rays, checked: ... x 6, a floating type."""
    shape = tuple(rays.shape) if hasattr(rays, "shape") and hasattr(rays, "dtype") else None
    if shape is None or len(shape) < 1 or shape[-1] != 6:
        raise _lib.PedpError(f"{name}: rays must be ... x 6, got {shape if shape is not None else type(rays).__name__}")
    kind = str(rays.dtype).replace("torch.", "")
    if kind not in ("float16", "float32", "float64"):
        raise _lib.PedpError(f"{name}: rays must be floating point, got {kind}")
    n = int(np.prod(shape[:-1], dtype=np.int64))
    if n > MAX_RAYS:
        raise _lib.PedpError(f"{name}: at most {MAX_RAYS} rays, got {n}")
    return shape[:-1], n


def _torch():
    import torch

    return torch


def _bound(name, what, x):
    """tnear / tfar as a Python float: one real number (NaN is allowed: such a bound holds for no t)."""
    try:
        if np.ndim(x) != 0:
            raise TypeError
        return float(x)
    except (TypeError, ValueError):
        raise _lib.PedpError(f"{name}: {what} must be one real number, got {x!r}") from None


class RaycastingScene:
    def __init__(self, ctx=None):
        self.ctx = ctx
        self._source = None      # what add_triangles was given: a _lib.Mesh, or the checked (vertices f64, triangles u32)
        self._mesh = None        # the device mesh, built by the first query
        self._solid = None       # the topology handle of the signed queries, likewise

    def add_triangles(self, mesh_or_vertices, triangles=None):
        """The scene's geometry: a _lib.Mesh (used as posed), a holder with .vertices / .triangles, or vertices (V x 3
        float) with triangles (F x 3 integer).  Returns its geometry id, 0."""
        if self._source is not None:
            raise NotImplementedError("RaycastingScene holds one geometry: add_triangles was called before")
        if isinstance(mesh_or_vertices, _lib.Mesh):
            if triangles is not None:
                raise _lib.PedpError("RaycastingScene.add_triangles: a _lib.Mesh brings its own triangles")
            if self.ctx is not None and self.ctx is not mesh_or_vertices.ctx:
                raise _lib.PedpError("RaycastingScene.add_triangles: the mesh belongs to another context than the scene")
            self._source = self._mesh = mesh_or_vertices
            return 0
        from .defect_map import _model_arrays

        try:
            v, t = _model_arrays(mesh_or_vertices if triangles is None else (mesh_or_vertices, triangles))
        except _lib.PedpError as e:
            raise _lib.PedpError(str(e).replace("DefectMap:", "RaycastingScene.add_triangles:")) from None
        if len(t) == 0:
            raise _lib.PedpError("RaycastingScene.add_triangles: the mesh has no triangles")
        if not np.isfinite(v).all():
            raise _lib.PedpError("RaycastingScene.add_triangles: vertices must be finite (found NaN or infinite coordinates)")
        self._source = (v, t)
        return 0

    # ---------------------------------------------------------------- the device side, on first use
    def _device_mesh(self, name, dev):
        if self._source is None:
            raise _lib.PedpError(f"RaycastingScene.{name}: the scene is empty: call add_triangles first")
        if self._mesh is None:
            ctx = self.ctx
            if ctx is None and dev is not None:
                import torch
                from ._bridge import stream_context

                ctx = stream_context(dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
            self.ctx = ctx or _lib.default_context()
            v, t = self._source
            self._mesh = _lib.Mesh(self.ctx, v.astype(np.float32), t)    # from_legacy's cast
        if dev is not None and (dev.index or 0) != self._mesh.ctx.device:
            raise _lib.PedpError(f"RaycastingScene.{name}: the arguments are on {dev}, the mesh on cuda:{self._mesh.ctx.device}")
        return self._mesh

    def _model_solid(self, name):
        if isinstance(self._source, _lib.Mesh):
            raise _lib.PedpError(f"RaycastingScene.{name}: a _lib.Mesh keeps no model to build the solid from: "
                                 "add the vertices and triangles instead")
        if self._solid is None:
            self._solid = _lib.Solid(self._mesh.ctx, *self._source)
        return self._solid

    def _rays(self, name, rays):
        lead, n = _leading_rays(name, rays)
        dev = device_of(rays)
        m = self._device_mesh(name, dev)
        return lead, n, dev, m, as_array(rays, dev, np.float32).reshape(n, 6)

    # ---------------------------------------------------------------- rays
    def cast_rays(self, rays):
        """dict(t_hit f32, inf on a miss; geometry_ids u32, 0 or 0xFFFFFFFF; primitive_ids u32, 0xFFFFFFFF on a miss;
        primitive_uvs f32 ... x 2): the closest hit, ties to the smaller t, then the smaller triangle index."""
        lead, n, dev, m, r = self._rays("cast_rays", rays)
        t, ids, uv = empty(dev, (n,), np.float32), empty(dev, (n,), np.uint32), empty(dev, (n, 2), np.float32)
        if n:
            launch(dev, "pedp_raycast", lambda lib, h, mem: lib.pedp_raycast(h, m._h, ptr(r), n, mem, ptr(t), ptr(ids), ptr(uv)), m.ctx)
        # a triangle index is below 2^31 and a miss is all ones: the sign bit, spread, is the geometry id
        geo = (ids.view(np.int32) >> 31).view(np.uint32) if dev is None else (ids.view(_torch().int32) >> 31).view(_torch().uint32)
        out = {"t_hit": t.reshape(lead), "geometry_ids": geo.reshape(lead), "primitive_ids": ids.reshape(lead),
               "primitive_uvs": uv.reshape(lead + (2,))}
        return {k: as_kind(v, rays) for k, v in out.items()}

    def count_intersections(self, rays):
        """int32, the leading shape: the number of triangles each ray intersects."""
        lead, n, dev, m, r = self._rays("count_intersections", rays)
        out = empty(dev, (n,), np.int32)
        if n:
            launch(dev, "pedp_count_intersections", lambda lib, h, mem: lib.pedp_count_intersections(h, m._h, ptr(r), n, mem, ptr(out)),
                   m.ctx)
        return as_kind(out.reshape(lead), rays)

    def test_occlusions(self, rays, tnear=0.0, tfar=float("inf")):
        """bool, the leading shape: whether a triangle the ray intersects has tnear <= t <= tfar (float32, both inclusive)."""
        lo, hi = _bound("test_occlusions", "tnear", tnear), _bound("test_occlusions", "tfar", tfar)
        lead, n, dev, m, r = self._rays("test_occlusions", rays)
        out = empty(dev, (n,), np.uint8)
        if n:
            launch(dev, "pedp_test_occlusions", lambda lib, h, mem: lib.pedp_test_occlusions(
                h, m._h, ptr(r), n, mem, C.c_float(lo), C.c_float(hi), ptr(out)), m.ctx)
        out = out.reshape(lead)
        return as_kind(out.view(np.bool_) if dev is None else out.bool(), rays)

    def list_intersections(self, rays):
        """dict(ray_splits int64 N + 1, ray_ids int64 M, t_hit f32 M, geometry_ids u32 zeros M, primitive_ids u32 M,
        primitive_uvs f32 M x 2) over the N rays in row-major order of the leading shape; a ray's entries by ascending t,
        then triangle index, so its first entry is its cast_rays result."""
        lead, n, dev, m, r = self._rays("list_intersections", rays)
        cap = m._list_cap or max(4 * n, 1024)
        total = C.c_int64()
        while True:
            splits = empty(dev, (n + 1,), np.int64)
            ids, t = empty(dev, (cap,), np.int64), empty(dev, (cap,), np.float32)
            prim, uv = empty(dev, (cap,), np.uint32), empty(dev, (cap, 2), np.float32)

            def call(lib, h, mem):
                rc = lib.pedp_list_intersections(h, m._h, ptr(r), n, mem, cap, ptr(splits), ptr(ids), ptr(t), ptr(prim), ptr(uv),
                                                 C.byref(total))
                return 0 if rc != 0 and total.value > cap else rc     # (more entries than room: once more, below)

            launch(dev, "pedp_list_intersections", call, m.ctx)
            if total.value <= cap:
                break
            cap = total.value
        k = total.value
        m._list_cap = k + k // 4 + 1024
        out = {"ray_splits": splits, "ray_ids": ids[:k], "t_hit": t[:k], "geometry_ids": empty(dev, (k,), np.uint32),
               "primitive_ids": prim[:k], "primitive_uvs": uv[:k]}
        if dev is None:
            out["geometry_ids"][:] = 0
        else:
            out["geometry_ids"].zero_()
        return {key: as_kind(v, rays) for key, v in out.items()}

    # ---------------------------------------------------------------- points
    def _points(self, name, points):
        sd._leading_shape(name, points)          # (shape and type, before the device)
        return self._device_mesh(name, device_of(points))

    def compute_closest_points(self, points):
        return sd.closest_points(self._points("compute_closest_points", points), points)

    def compute_distance(self, points):
        return sd.compute_distance(self._points("compute_distance", points), points)

    def compute_signed_distance(self, points):
        m = self._points("compute_signed_distance", points)
        return sd.compute_signed_distance(m, points, solid=self._model_solid("compute_signed_distance"))

    def compute_occupancy(self, points):
        m = self._points("compute_occupancy", points)
        return sd.compute_occupancy(m, points, solid=self._model_solid("compute_occupancy"))
