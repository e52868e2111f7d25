"""Exact cloud-to-mesh distance and the deviation heat map built on it.

    closest_points, compute_distance   RaycastingScene.compute_closest_points / compute_distance on the mesh handle the ray
                                       caster uses (pedp_closest_points, csrc/pedp_closest.hip)
    align_to_mesh                      align_to_surface with the exact closest point of the triangles in the place of the
                                       nearest model vertex (defect_projection.py:417-460 snaps to vertices)
    deviation_heatmap                  the distance of every measured depth point from the posed CAD surface as the heat map
                                       that ray_tracing / Mesh.project_heatmap consume (run.py:64 leaves a dummy there)
    Solid, compute_signed_distance,    RaycastingScene.compute_signed_distance / compute_occupancy: the distance with the
    compute_occupancy,                 sign of the solid's inside (negative) and outside, by the angle-weighted pseudonormal
    signed_closest_points              of the closest face, edge or vertex (pedp_signed_distance, csrc/pedp_solid.hip)
    signed_deviation, split_deviation  a frame's signed distances, and the two heat maps they split into: excess material
                                       (outside the CAD solid) and missing material (inside it)

CUDA tensors stay on their device: the query is enqueued on the caller's current stream without a host wait when the
mesh's context was created on that stream (otherwise the two streams are synchronised around the call), and CUDA
tensors come back.  numpy arrays and CPU tensors use host memory and get their own kind back.  The contract (the
triangle as the ray caster stores it, float64 with no contraction, Ericson's regions, ties to the lowest index, the
culled search bit-equal to the exhaustive one) is DESIGN.md s4.16; the signed queries' is s4.18.
"""
import numpy as np

from . import _lib
from ._bridge import as_array, as_kind, device_of, empty, is_torch, launch, ptr, stream_context

MAX_POINTS = 1 << 24       # pedp_closest_points' bound

_OUTPUTS = ("points", "distances", "primitive_ids", "primitive_uvs", "sides")


def _mesh_of(name, mesh, ctx, dev):
    """The device mesh of `mesh` (a _lib.Mesh, or a holder with .vertices / .triangles converted like from_legacy)."""
    if isinstance(mesh, _lib.Mesh):
        if ctx is not None and ctx is not mesh.ctx:
            raise _lib.PedpError(f"{name}: the mesh belongs to another context than ctx")
        return mesh
    if not (hasattr(mesh, "vertices") and hasattr(mesh, "triangles")):
        raise _lib.PedpError(f"{name}: mesh must be a _lib.Mesh or hold .vertices and .triangles, got {type(mesh).__name__}")
    if ctx is None:
        if dev is not None:
            import torch

            ctx = stream_context(dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
        else:
            ctx = _lib.default_context()
    from .ray_projection import _device_mesh

    return _device_mesh(mesh, ctx)


def _leading_shape(name, points):
    """(leading shape, number of rows) of a query's points, checked: ... x 3, float32 or float64, at most MAX_POINTS rows."""
    shape = tuple(points.shape) if hasattr(points, "shape") else None
    if shape is None or len(shape) < 1 or shape[-1] != 3:
        raise _lib.PedpError(f"{name}: points must be ... x 3, got {shape if shape is not None else type(points).__name__}")
    kind = str(points.dtype).replace("torch.", "")
    if kind not in ("float32", "float64"):
        raise _lib.PedpError(f"{name}: points must be float32 or float64, got {kind}")
    lead = shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    if n > MAX_POINTS:
        raise _lib.PedpError(f"{name}: at most {MAX_POINTS} points, got {n}")
    return lead, n


def _query(name, mesh, points, want, ctx=None):
    lead, n = _leading_shape(name, points)
    dev = device_of(points)
    m = _mesh_of(name, mesh, ctx, dev)
    if dev is not None and (dev.index or 0) != m.ctx.device:
        raise _lib.PedpError(f"{name}: points are on {dev}, the mesh on cuda:{m.ctx.device}")
    p = as_array(points, dev, np.float64).reshape(n, 3)
    out = {k: empty(dev, lead + (() if w is None else (w,)), t) for k, (w, t) in _lib.Mesh.CLOSEST_OUTPUTS.items() if k in want}
    if n:
        launch(dev, "pedp_closest_points", lambda lib, h, mem: lib.pedp_closest_points(
            h, m._h, ptr(p), n, mem, ptr(out.get("points")), ptr(out.get("distances")), ptr(out.get("primitive_ids")),
            ptr(out.get("primitive_uvs")), ptr(out.get("sides"))), m.ctx)
    return {k: as_kind(v, points) for k, v in out.items()}, m


def closest_points(mesh, points, ctx=None):
    """RaycastingScene.compute_closest_points: for every row of `points` (... x 3, float32 or float64; numpy, a CPU
    tensor or a CUDA tensor) the closest point of the mesh as posed.  `mesh` is a _lib.Mesh or a holder with .vertices /
    .triangles (float32 vertices, like from_legacy).  Returns a dict with the leading shape of `points` and the caller's
    kind: points (... x 3 float64), distances (float64), primitive_ids (uint32, 0xFFFFFFFF: none), primitive_uvs
    (... x 2 float64, the barycentrics (v, w) of a + ab v + ac w), sides (int8: the side of the chosen face's normal,
    -1 / 0 / +1; exact where the closest point is inside a face, a convention on edges and vertices)."""
    return _query("closest_points", mesh, points, _OUTPUTS, ctx)[0]


def compute_distance(mesh, points, ctx=None):
    """RaycastingScene.compute_distance: the distances of closest_points alone."""
    return _query("compute_distance", mesh, points, ("distances",), ctx)[0]["distances"]


_SIGNED = ("signed_distances", "occupancy", "features", "normals")


def Solid(mesh, ctx=None):
    """The topology handle (_lib.Solid) of a model: `mesh` is a holder with .vertices / .triangles or a (vertices,
    triangles) pair in the model frame.  Built once per model, whatever the pose; `.info` reports whether the mesh is
    closed (boundary_edges, nonmanifold_edges, flipped_edges), its orientation and its volume."""
    from .defect_map import _model_arrays

    try:
        v, t = _model_arrays(mesh)
    except _lib.PedpError as e:
        raise _lib.PedpError(str(e).replace("DefectMap:", "Solid:")) from None
    return _lib.Solid(ctx or _lib.default_context(), v, t)


def _context_of(ctx, solid):
    """The context a signed query builds a holder's device mesh on: the caller's, else the solid's, else _mesh_of's choice."""
    return ctx if ctx is not None or solid is None else solid.ctx


def _signed_query(name, mesh, points, want, solid, ctx):
    lead, n = _leading_shape(name, points)
    if solid is not None and not isinstance(solid, _lib.Solid):
        raise _lib.PedpError(f"{name}: solid must be a Solid, got {type(solid).__name__}")
    if solid is None and isinstance(mesh, _lib.Mesh):
        raise _lib.PedpError(f"{name}: a _lib.Mesh keeps no model to build the solid from: pass solid=Solid(model)")
    dev = device_of(points)
    m = _mesh_of(name, mesh, _context_of(ctx, solid), dev)
    if dev is not None and (dev.index or 0) != m.ctx.device:
        raise _lib.PedpError(f"{name}: points are on {dev}, the mesh on cuda:{m.ctx.device}")
    own = solid is None
    if own:
        solid = Solid(mesh, m.ctx)
    elif solid.ctx is not m.ctx:
        raise _lib.PedpError(f"{name}: the solid belongs to another context than the mesh")
    p = as_array(points, dev, np.float64).reshape(n, 3)
    out = {k: empty(dev, lead + (() if w is None else (w,)), t) for k, (w, t) in _lib.Solid.SIGNED_OUTPUTS.items() if k in want}
    try:
        if n:
            launch(dev, "pedp_signed_distance", lambda lib, h, mem: lib.pedp_signed_distance(
                h, m._h, solid._h, ptr(p), n, mem, ptr(out.get("signed_distances")), ptr(out.get("occupancy")),
                ptr(out.get("features")), ptr(out.get("normals"))), m.ctx)
    finally:
        if own:                        # the call's solid goes with the call: nothing enqueued may still read it
            if dev is not None:
                m.ctx.synchronize()
            solid.close()
    return {k: as_kind(v, points) for k, v in out.items()}


def compute_signed_distance(mesh, points, solid=None, ctx=None):
    """RaycastingScene.compute_signed_distance: compute_distance with the sign of the solid, negative inside.  `mesh` and
    `points` as for closest_points; `solid` is the model's Solid (required when `mesh` is a _lib.Mesh; built for the call
    from a holder's own vertices and triangles when None).  Exact for a closed, consistently oriented mesh and a point
    off the surface; a mesh that bounds no solid is refused."""
    return _signed_query("compute_signed_distance", mesh, points, ("signed_distances",), solid, ctx)["signed_distances"]


def compute_occupancy(mesh, points, solid=None, ctx=None):
    """RaycastingScene.compute_occupancy: int8, 1 where the point is inside the solid (signed distance < 0), else 0."""
    return _signed_query("compute_occupancy", mesh, points, ("occupancy",), solid, ctx)["occupancy"]


def signed_closest_points(mesh, points, solid=None, ctx=None):
    """closest_points' dict and, with it, signed_distances (float64), occupancy (int8), features (uint8: 0 face, 1 edge,
    2 vertex, 255 none) and normals (... x 3 float64: the outward unit pseudonormal of the closest feature)."""
    name = "signed_closest_points"
    if not isinstance(mesh, _lib.Mesh) and hasattr(mesh, "vertices"):      # one device mesh, one solid for both calls
        m = _mesh_of(name, mesh, _context_of(ctx, solid), device_of(points))
        own = Solid(mesh, m.ctx) if solid is None else None
        try:
            return signed_closest_points(m, points, own or solid, m.ctx)
        finally:
            if own is not None:
                m.ctx.synchronize()
                own.close()
    out = _query(name, mesh, points, _OUTPUTS, _context_of(ctx, solid))[0]
    out.update(_signed_query(name, mesh, points, _SIGNED, solid, ctx))
    return out


def signed_deviation(depth, K, mesh, solid, unit=1000.0, mask=None, zmin=0.001, ctx=None):
    """The signed distance of every measured depth point from the posed CAD solid: H x W float64 of the caller's kind,
    negative where the measured surface lies inside the solid (a dent), positive outside (a bump), NaN where the pixel is
    invalid by deviation_heatmap's rule (depth < zmin, or `mask` unset).  depth, K, unit, mask and zmin as for
    deviation_heatmap; `solid` as for compute_signed_distance."""
    shape = tuple(depth.shape) if hasattr(depth, "shape") else None
    if shape is None or len(shape) != 2:
        raise _lib.PedpError(f"signed_deviation: depth must be H x W, got {shape if shape is not None else type(depth).__name__}")
    if mask is not None and tuple(mask.shape) != shape:
        raise _lib.PedpError(f"signed_deviation: mask must be {shape[0]} x {shape[1]} like depth, got {tuple(mask.shape)}")
    from .depth_filters import depth2xyzmap

    if is_torch(depth) and not depth.is_cuda:
        import torch

        return torch.from_numpy(signed_deviation(depth.numpy(), K, mesh, solid, unit, None if mask is None else np.asarray(mask),
                                                 zmin, ctx))
    xyz = depth2xyzmap(depth, K)
    pts = (xyz.double() if is_torch(xyz) else xyz.astype(np.float64)) * unit
    sd = compute_signed_distance(mesh, pts, solid, ctx)
    if is_torch(sd):
        import torch

        keep = depth >= zmin
        if mask is not None:
            keep = keep & torch.as_tensor(mask, device=sd.device).bool()
        return torch.where(keep, sd, torch.full_like(sd, float("nan")))
    keep = np.asarray(depth) >= zmin
    if mask is not None:
        keep &= np.asarray(mask).astype(bool)
    return np.where(keep, sd, np.nan)


def split_deviation(sd, saturation, gate):
    """(excess, missing): the two heat maps of a frame's signed distances `sd` (signed_deviation's), deviation_heatmap's
    arithmetic on |sd| -- min(|sd| / saturation, 1) where |sd| <= gate, 0 elsewhere and where sd is NaN -- kept where
    sd > 0 (outside the solid: excess material) and where sd < 0 (inside: missing material).  Each is ready for
    project_heatmap / DefectMap.add_projection, and excess + missing is deviation_heatmap of the same frame."""
    if not (saturation > 0 and gate >= 0):
        raise _lib.PedpError(f"split_deviation: saturation must be positive and gate non-negative, got {saturation} and {gate}")
    if is_torch(sd):
        import torch

        dist = sd.abs()
        heat = torch.where(dist <= gate, torch.clamp(dist / saturation, max=1.0), torch.zeros_like(dist))
        zero = torch.zeros_like(heat)
        return torch.where(sd > 0, heat, zero), torch.where(sd < 0, heat, zero)
    sd = np.asarray(sd, dtype=np.float64)
    dist = np.abs(sd)
    with np.errstate(invalid="ignore"):
        heat = np.where(dist <= gate, np.minimum(dist / saturation, 1.0), 0.0)
        return np.where(sd > 0, heat, 0.0), np.where(sd < 0, heat, 0.0)


def align_to_mesh(defect_points, mesh, offset=0.1, ctx=None):
    """align_to_surface on the triangles: every defect point [x, y, z, ...] goes to its exact closest point of the
    mesh and is lifted by `offset` along the chosen triangle's unit normal ab x ac, oriented to the side the point is
    on (the normal's own direction for a point on the face's plane).  Returns (offset_points, aligned_points)."""
    if len(defect_points) == 0:
        return np.array([]), np.array([])
    pts = np.asarray(defect_points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise _lib.PedpError(f"align_to_mesh: defect_points must be N x 3 (or wider), got shape {pts.shape}")
    res, m = _query("align_to_mesh", mesh, np.ascontiguousarray(pts[:, :3]), ("points", "primitive_ids", "sides"), ctx)
    aligned = res["points"]
    sign = np.where(res["sides"] < 0, -1.0, 1.0)
    return aligned + m.face_normals(res["primitive_ids"]) * sign[:, None] * offset, aligned


def heat_from_distances(depth, dist, saturation, gate, mask=None, zmin=0.001):
    """deviation_heatmap's arithmetic on a frame's distances: min(dist / saturation, 1) where depth >= zmin, dist <= gate
    and the mask (if any) is set, 0 elsewhere; float64, numpy or torch by `dist`."""
    if is_torch(dist):
        import torch

        keep = (depth >= zmin) & (dist <= gate)
        if mask is not None:
            keep = keep & torch.as_tensor(mask, device=dist.device).bool()
        return torch.where(keep, torch.clamp(dist / saturation, max=1.0), torch.zeros_like(dist))
    keep = (np.asarray(depth) >= zmin) & (dist <= gate)
    if mask is not None:
        keep &= np.asarray(mask).astype(bool)
    with np.errstate(invalid="ignore"):
        return np.where(keep, np.minimum(dist / saturation, 1.0), 0.0)


def deviation_heatmap(depth, K, mesh, saturation, gate, unit=1000.0, mask=None, zmin=0.001, ctx=None):
    """The geometric deviation of a depth frame from the posed CAD surface as a heat map.  depth: H x W in the units
    FoundationPose gets (metres), numpy, a CPU tensor or a CUDA tensor; the measured points are
    float64(depth2xyzmap(depth, K)) * unit in the frame the mesh is posed in.  heat = min(distance / saturation, 1) where
    depth >= zmin, distance <= gate and `mask` (H x W, optional) is set, 0 elsewhere: H x W float64 of the caller's kind,
    ready for ray_tracing(..., heatmap, ...) / Mesh.project_heatmap.  `saturation` and `gate` are in the mesh's units."""
    shape = tuple(depth.shape) if hasattr(depth, "shape") else None
    if shape is None or len(shape) != 2:
        raise _lib.PedpError(f"deviation_heatmap: depth must be H x W, got {shape if shape is not None else type(depth).__name__}")
    if not (saturation > 0 and gate >= 0):
        raise _lib.PedpError(f"deviation_heatmap: saturation must be positive and gate non-negative, got {saturation} and {gate}")
    if mask is not None and tuple(mask.shape) != shape:
        raise _lib.PedpError(f"deviation_heatmap: mask must be {shape[0]} x {shape[1]} like depth, got {tuple(mask.shape)}")
    from .depth_filters import depth2xyzmap

    if is_torch(depth) and not depth.is_cuda:
        import torch

        return torch.from_numpy(deviation_heatmap(depth.numpy(), K, mesh, saturation, gate, unit,
                                                  None if mask is None else np.asarray(mask), zmin, ctx))
    xyz = depth2xyzmap(depth, K)
    pts = (xyz.double() if is_torch(xyz) else xyz.astype(np.float64)) * unit
    return heat_from_distances(depth, compute_distance(mesh, pts, ctx), saturation, gate, mask, zmin)
