"""Mesh refinement: give a CAD model the resolution that the per-face maps need.

    refine_mesh(mesh, max_edge)      every edge longer than max_edge bisected until none is left (pedp_mesh_refine,
                                     csrc/pedp_refine.hip); each refined face knows the CAD face it came from
    RefinedMesh.reduce_to_parent     a per-face column of the refined model folded back to one value per CAD face
    edge_for_camera(K, distance)     the max_edge whose faces are about two pixel footprints wide at that distance

DefectMap, CoverageMap, DeviationMap and ViewPlanner all speak per face of the model, and a CAD export makes a flat side
two triangles: one defective pixel then marks half a side.  The reference loads a separately prepared model file for the
same need (datareader.py:720-724).  Call refine_mesh once, before the maps and the device mesh are created, build them
all on the result, and read them back per CAD face with reduce_to_parent.  The contract (the bit-symmetric edge test,
one midpoint per welded edge in key order, the four templates, termination) is DESIGN.md s4.25.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import as_array, device_of, empty, is_torch, launch, ptr, stream_context
from .geometry import TriangleMesh

REDUCE_OPS = {"max": 0, "min": 1, "sum": 2}     # PEDP_REDUCE_*
MISS = 0xFFFFFFFF


def edge_for_camera(K, distance, pixels=2.0):
    """pixels * distance / min(fx, fy): the edge length whose faces are about `pixels` pixel footprints wide when the
    camera with intrinsic matrix K (3 x 3, or a holder with .intrinsic_matrix) looks at them square-on from `distance`.
    Choose refine_mesh's max_edge from it: with the working distance of the inspection and pixels = 2 a refined face is
    of the size that one frame can say something about; a smaller max_edge only multiplies faces no pixel tells apart."""
    K = np.asarray(getattr(K, "intrinsic_matrix", K), dtype=np.float64)
    if K.shape != (3, 3):
        raise _lib.PedpError(f"edge_for_camera: K must be 3 x 3, got shape {K.shape}")
    f = min(float(K[0, 0]), float(K[1, 1]))
    distance, pixels = float(distance), float(pixels)
    if not (f > 0.0 and np.isfinite(f) and distance > 0.0 and np.isfinite(distance) and pixels > 0.0 and np.isfinite(pixels)):
        raise _lib.PedpError(f"edge_for_camera: focal lengths, distance and pixels must be positive and finite, got "
                             f"fx = {K[0, 0]}, fy = {K[1, 1]}, distance = {distance}, pixels = {pixels}")
    return pixels * distance / f


def _mesh_arrays(mesh, who="refine_mesh"):
    """(vertices V x 3 float64, triangles F x 3 as 32-bit indices, device) on the side the mesh came from; `who` names the
    caller in the errors."""
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        v, t = mesh
    elif hasattr(mesh, "vertices") and hasattr(mesh, "triangles"):
        v, t = mesh.vertices, mesh.triangles
    else:
        raise _lib.PedpError(f"{who}: mesh must hold .vertices and .triangles or be a (vertices, triangles) pair, "
                             f"got {type(mesh).__name__}")
    dev = device_of(v, t)
    if dev is None:
        v = v.detach().numpy() if is_torch(v) else np.asarray(v)
        t = t.detach().numpy() if is_torch(t) else np.asarray(t)
    for name, a in (("vertices", v), ("triangles", t)):
        if not hasattr(a, "shape") or not hasattr(a, "dtype"):
            raise _lib.PedpError(f"{who}: {name} must be an array or a tensor, got {type(a).__name__}")
    kind_v, kind_t = str(v.dtype).replace("torch.", ""), str(t.dtype).replace("torch.", "")
    if len(v.shape) != 2 or v.shape[1] != 3 or kind_v not in ("float32", "float64"):
        raise _lib.PedpError(f"{who}: vertices must be a V x 3 float array, got {kind_v} of shape {tuple(v.shape)}")
    if int(np.prod(tuple(t.shape))) == 0:
        t = t.reshape(0, 3)
    if len(t.shape) != 2 or t.shape[1] != 3 or kind_t not in (("int32", "uint32", "int64") + (("uint64",) if dev is None else ())):
        raise _lib.PedpError(f"{who}: triangles must be an F x 3 integer array, got {kind_t} of shape {tuple(t.shape)}")
    if dev is not None:
        import torch

        v = as_array(v, dev, np.float64)
        t = t.to(dev)
        if t.dtype == torch.int64:
            if t.numel() and (int(t.min()) < 0 or int(t.max()) > MISS):
                raise _lib.PedpError(f"{who}: triangle indices must lie in [0, 2^32)")
            t = torch.where(t > 0x7FFFFFFF, t - (1 << 32), t).to(torch.int32)      # the same 32 bits
        elif t.dtype != torch.int32:
            t = t.contiguous().view(torch.int32)
        return v, t.contiguous(), dev
    if len(t) and (t.min() < 0 or t.max() > MISS):
        raise _lib.PedpError(f"{who}: triangle indices must lie in [0, 2^32)")
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.uint32), None


class RefinedMesh(TriangleMesh):
    """What refine_mesh returns: a TriangleMesh whose `vertices` (V x 3 float64) and `triangles` (F x 3; uint32 on the host,
    the same bits as int32 in a CUDA tensor) are on the side the input came from, so it goes as it is into _lib.Mesh,
    DefectMap, CoverageMap, DeviationMap, Solid and RaycastingScene.add_triangles.

        parent_face      F int32: the CAD face (the input's face index) of every refined face; non-decreasing
        n_parent_faces   the input's face count
        rounds           rounds that split something (0: the input came back unchanged)
        max_edge         what it was refined to

    The input's vertices are kept, in order, ahead of the new ones."""

    def __init__(self, ctx, handle, vertices, triangles, parent_face, n_parent_faces, rounds, max_edge):
        self.ctx, self._h = ctx, handle
        self.vertices, self.triangles, self.parent_face = vertices, triangles, parent_face
        self.vertex_normals = np.zeros((0, 3))
        self.triangle_normals = np.zeros((0, 3))
        self.n_parent_faces, self.rounds, self.max_edge = int(n_parent_faces), int(rounds), float(max_edge)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().pedp_refined_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def parent_of(self, face_ids):
        """The CAD faces of refined face ids (a cast's primitive_ids, a region's first_face ...): an int32 array or tensor
        of face_ids' shape and side; ids outside [0, F), the miss id 0xFFFFFFFF among them, give -1."""
        if is_torch(face_ids):
            import torch

            ids = face_ids.to(torch.int64)
            if face_ids.dtype == torch.int32:       # uint32 ids kept as int32 bits: -1 is the miss id
                ids = ids & MISS
            pf = self.parent_face if is_torch(self.parent_face) else torch.from_numpy(self.parent_face)
            pf = torch.cat([pf.to(ids.device), torch.full((1,), -1, dtype=torch.int32, device=ids.device)])
            ok = (ids >= 0) & (ids < len(pf) - 1)
            return pf[torch.where(ok, ids, torch.full_like(ids, len(pf) - 1))]
        ids = np.asarray(face_ids).astype(np.int64)
        pf = self.parent_face.cpu().numpy() if is_torch(self.parent_face) else self.parent_face
        pf = np.concatenate([pf, np.full(1, -1, np.int32)])
        ok = (ids >= 0) & (ids < len(pf) - 1)
        return pf[np.where(ok, ids, len(pf) - 1)]

    def reduce_to_parent(self, values, how="max"):
        """One value per CAD face from one value per refined face (a map's peak, hits, coverage ...): `how` = "max", "min"
        or "sum" over each CAD face's run of children, in ascending child order (pedp_refined_reduce).  values: F numbers,
        a numpy array or a CUDA tensor, taken as float64; the result (n_parent_faces float64) is on values' side."""
        if how not in REDUCE_OPS:
            raise _lib.PedpError(f"RefinedMesh.reduce_to_parent: how must be one of {', '.join(REDUCE_OPS)}, got {how!r}")
        if not hasattr(values, "shape") or tuple(values.shape) != (len(self.triangles),):
            raise _lib.PedpError(f"RefinedMesh.reduce_to_parent: values must have shape ({len(self.triangles)},), got "
                                 f"{tuple(getattr(values, 'shape', ())) or type(values).__name__}")
        dev = device_of(values)
        if dev is not None and (dev.index or 0) != self.ctx.device:
            raise _lib.PedpError(f"RefinedMesh.reduce_to_parent: the values are on {dev}, the mesh on cuda:{self.ctx.device}")
        x = as_array(values, dev, np.float64)
        out = empty(dev, (self.n_parent_faces,), np.float64)
        launch(dev, "pedp_refined_reduce", lambda lib, h, mem: lib.pedp_refined_reduce(self._h, REDUCE_OPS[how], mem, ptr(x), ptr(out)),
               self.ctx)
        return out


def refine_mesh(mesh, max_edge, max_faces=1 << 24, ctx=None):
    """Split the faces of `mesh` until no edge is longer than max_edge (choose it with edge_for_camera): a RefinedMesh.

    mesh: a TriangleMesh-like holder (.vertices V x 3, .triangles F x 3) or a (vertices, triangles) pair, numpy arrays or
    CUDA tensors; the result's arrays are on the same side.  The refinement is conforming (both faces at an edge split it
    at the same new vertex, also across duplicated vertices), keeps the surface, the winding and closedness, and is a pure
    function of the arrays and max_edge.  More than max_faces faces, a vertex index outside the vertices, a non-finite
    coordinate or a max_edge that is not positive and finite raise PedpError."""
    v, t, dev = _mesh_arrays(mesh)
    try:
        max_edge, max_faces = float(max_edge), int(max_faces)
    except (TypeError, ValueError):
        raise _lib.PedpError(f"refine_mesh: max_edge must be a number and max_faces an integer, got {max_edge!r}, {max_faces!r}") from None
    if dev is not None:
        import torch

        if ctx is None:
            ctx = stream_context(dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
        elif ctx.device != (dev.index or 0):
            raise _lib.PedpError(f"refine_mesh: the mesh is on {dev}, the context on cuda:{ctx.device}")
    ctx = ctx or _lib.default_context()
    h, reached = C.c_void_p(), C.c_int64()
    n_v, n_f = int(v.shape[0]), int(t.shape[0])
    launch(dev, "pedp_mesh_refine",
           lambda lib, ch, mem: lib.pedp_mesh_refine(ch, ptr(v), n_v, ptr(t), n_f, mem, max_edge, max_faces, C.byref(h), C.byref(reached)),
           ctx)
    lib = _lib.load()
    try:
        V, F, rounds = C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(lib.pedp_refined_size(h, C.byref(V), C.byref(F), C.byref(rounds)), "pedp_refined_size")
        out_v = empty(dev, (V.value, 3), np.float64)
        out_t = empty(dev, (F.value, 3), np.int32 if dev is not None else np.uint32)
        out_p = empty(dev, (F.value,), np.int32)
        launch(dev, "pedp_refined_read", lambda lib, ch, mem: lib.pedp_refined_read(h, mem, ptr(out_v), ptr(out_t), ptr(out_p)), ctx)
    except Exception:
        lib.pedp_refined_destroy(h)
        raise
    return RefinedMesh(ctx, h, out_v, out_t, out_p, n_f, rounds.value, max_edge)
