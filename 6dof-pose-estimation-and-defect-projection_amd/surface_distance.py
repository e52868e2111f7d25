"""Exact cloud-to-mesh distance and the deviation heat map built on it.

    closest_points, compute_distance   RaycastingScene.compute_closest_points / compute_distance on the mesh handle the ray
                                       caster uses (pedp_closest_points, csrc/pedp_closest.hip)
    align_to_mesh                      align_to_surface with the exact closest point of the triangles in the place of the
                                       nearest model vertex (defect_projection.py:417-460 snaps to vertices)
    deviation_heatmap                  the distance of every measured depth point from the posed CAD surface as the heat map
                                       that ray_tracing / Mesh.project_heatmap consume (run.py:64 leaves a dummy there)

CUDA tensors stay on their device: the query is enqueued on the caller's current stream without a host wait when the
mesh's context was created on that stream (otherwise the two streams are synchronised around the call), and CUDA
tensors come back.  numpy arrays and CPU tensors use host memory and get their own kind back.  The contract (the
triangle as the ray caster stores it, float64 with no contraction, Ericson's regions, ties to the lowest index, the
culled search bit-equal to the exhaustive one) is DESIGN.md s4.16.
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


def _query(name, mesh, points, want, ctx=None):
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
