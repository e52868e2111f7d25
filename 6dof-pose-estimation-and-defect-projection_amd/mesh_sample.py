"""Surface sampling: the model's point cloud (model.ply) made from the model's mesh (model.obj).

    sample_points_uniformly(mesh, n)          n points drawn uniformly by area (pedp_mesh_sample, csrc/pedp_sample.hip)
    sample_points_poisson_disk(mesh, N)       N evenly spaced points: 5 N drawn, thinned to the largest spacing that keeps N
    sample_points_poisson_disk(mesh, spacing=r)   the thinning of a draw at spacing r itself
    thin_to_spacing(points, r)                the same thinning on any cloud: the kept indices
    mesh_to_pcd(mesh, param)                  src/pose_estimation.py:453-464

The reference makes these clouds with Open3D (TriangleMesh.sample_points_poisson_disk), whose choice of points is seeded
by std::random_device.  Here every result is a pure function of (mesh, seed, spacing): a counter-based generator
(Philox4x32-10), the face chosen from an integer prefix sum, and an elimination rule with exactly one answer -- the set a
visit in ascending key order keeps -- found on the device in rounds of final decisions.  Each sample carries its face id
and barycentrics, so it maps back to CAD faces through RefinedMesh.parent_of.  The contract is DESIGN.md s4.26;
tests/_sample_ref.py restates it in numpy, bit for bit.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._bridge import as_array, device_of, empty, is_torch, launch, ptr, stream_context
from .geometry import PointCloud
from .mesh_refine import _mesh_arrays

NORMALS_NONE, NORMALS_VERTEX, NORMALS_TRIANGLE = 0, 1, 2     # PEDP_SAMPLE_NORMALS_*


class _Info(C.Structure):                                       # pedp_mesh_sampler_info_t
    _fields_ = [("vertices", C.c_int64), ("faces", C.c_int64), ("unsampled_faces", C.c_int64), ("total_weight", C.c_uint64),
                ("area", C.c_double), ("largest_area", C.c_double), ("has_vertex_normals", C.c_int32), ("reserved", C.c_int32)]


class SampledCloud(PointCloud):
    """What the sampling functions return: a PointCloud (`points`, and `normals` when they are defined) that also carries

        face_ids       n int32: the mesh face of every point (None for a thinned `pcl`)
        barycentric    n x 3 float64: (a, b, c) with point = (a v0 + b v1) + c v2 of that face (None for a thinned `pcl`)
        index          the disk forms: the sample number (or the `pcl` row) of every point, ascending
        spacing        the disk forms: no two points are closer than this (r* of the count form, or the spacing given)
        drawn, rounds, probes   the disk forms: samples drawn, rounds of the last thinning, thinnings run

    For a mesh given as CUDA tensors the arrays above are tensors on that device, and so are `device_points` and
    `device_normals`; `points` / `normals` are the holder's usual numpy arrays, read from them."""

    face_ids = barycentric = index = spacing = drawn = rounds = probes = device_points = device_normals = None


def _cloud(dev, points, normals, **extra):
    if dev is None:
        out = SampledCloud.adopt(points, normals)
    else:
        out = SampledCloud(points, None if normals is None else normals.cpu().numpy(), _adopt=True)
        out.device_points, out.device_normals = points, normals
    for k, v in extra.items():
        setattr(out, k, v)
    return out


def _seed(who, seed):
    try:
        ok = int(seed) == seed and 0 <= int(seed) < 1 << 64
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise _lib.PedpError(f"{who}: seed must be an integer in [0, 2^64), got {seed!r}")
    return int(seed)


def _count(who, name, x, lowest=1):
    try:
        ok = int(x) == x and int(x) >= lowest
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise _lib.PedpError(f"{who}: {name} must be an integer >= {lowest}, got {x!r}")
    return int(x)


def _spacing(who, spacing, positive=False):
    try:
        r = float(spacing)
    except (TypeError, ValueError):
        r = math.nan
    if not (math.isfinite(r) and (r > 0.0 if positive else r >= 0.0)):
        raise _lib.PedpError(f"{who}: spacing must be a finite number {'> 0' if positive else '>= 0'}, got {spacing!r}")
    return r


def _context(who, dev, ctx):
    if dev is not None:
        import torch

        if ctx is None:
            ctx = stream_context(dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
        elif ctx.device != (dev.index or 0):
            raise _lib.PedpError(f"{who}: the input is on {dev}, the context on cuda:{ctx.device}")
    return ctx or _lib.default_context()


class MeshSampler:
    """The sampler of one mesh (pedp_mesh_sampler_create): the faces' areas, their 32-bit weights and the integer prefix
    sum, on the device.  Build it once and draw from it as often as needed; the module's functions build one per call.

    mesh: a TriangleMesh-like holder (.vertices V x 3, .triangles F x 3, optionally vertex normals) or a (vertices,
    triangles) pair, numpy arrays or CUDA tensors; results are on the same side."""

    def __init__(self, mesh, ctx=None, who="MeshSampler"):
        self._h = None
        v, t, dev = _mesh_arrays(mesh, who)
        if int(t.shape[0]) < 1:
            raise _lib.PedpError(f"{who}: triangles: the mesh has no face")
        vn = None
        if hasattr(mesh, "has_vertex_normals") and mesh.has_vertex_normals():
            vn = as_array(mesh.vertex_normals, dev, np.float64)
            if tuple(vn.shape) != tuple(v.shape):
                raise _lib.PedpError(f"{who}: vertex_normals must have the vertices' shape {tuple(v.shape)}, got {tuple(vn.shape)}")
        self.ctx, self.dev = _context(who, dev, ctx), dev
        h = C.c_void_p()
        launch(dev, "pedp_mesh_sampler_create",
               lambda lib, ch, mem: lib.pedp_mesh_sampler_create(ch, ptr(v), int(v.shape[0]), ptr(t), int(t.shape[0]), ptr(vn), mem, C.byref(h)),
               self.ctx)
        self._h = h
        info = _Info()
        _lib.check(_lib.load().pedp_mesh_sampler_info(h, C.byref(info)), "pedp_mesh_sampler_info")
        self.n_vertices, self.n_faces, self.unsampled_faces = info.vertices, info.faces, info.unsampled_faces
        self.total_weight, self.area, self.largest_area = info.total_weight, info.area, info.largest_area
        self.has_vertex_normals = bool(info.has_vertex_normals)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().pedp_mesh_sampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def normals_mode(self, use_triangle_normal):
        """Open3D's rule: the face's normal on request, else the interpolated vertex normals if the mesh has them."""
        return NORMALS_TRIANGLE if use_triangle_normal else (NORMALS_VERTEX if self.has_vertex_normals else NORMALS_NONE)

    def sample(self, number_of_points, use_triangle_normal=False, seed=0, first=0, who="MeshSampler.sample"):
        """Samples [first, first + number_of_points) of the seed's sequence: a SampledCloud."""
        n, seed, first = _count(who, "number_of_points", number_of_points), _seed(who, seed), _count(who, "first", first, 0)
        if first >= 1 << 64:
            raise _lib.PedpError(f"{who}: first must be below 2^64, got {first}")
        mode, dev = self.normals_mode(use_triangle_normal), self.dev
        pts, face, bary = empty(dev, (n, 3), np.float64), empty(dev, (n,), np.int32), empty(dev, (n, 3), np.float64)
        nrm = empty(dev, (n, 3), np.float64) if mode else None
        launch(dev, "pedp_mesh_sample",
               lambda lib, ch, mem: lib.pedp_mesh_sample(self._h, seed, first, n, mode, mem, ptr(pts), ptr(face), ptr(bary), ptr(nrm)), self.ctx)
        return _cloud(dev, pts, nrm, face_ids=face, barycentric=bary)

    def sample_disk(self, number_of_points=None, spacing=None, init_factor=5, use_triangle_normal=False, seed=0,
                    who="MeshSampler.sample_disk"):
        """The count form (number_of_points) or the spacing form (spacing) of sample_points_poisson_disk: a SampledCloud."""
        if (number_of_points is None) == (spacing is None):
            raise _lib.PedpError(f"{who}: give number_of_points or spacing, one of them, got number_of_points = {number_of_points!r} "
                                 f"and spacing = {spacing!r}")
        n = 0 if number_of_points is None else _count(who, "number_of_points", number_of_points)
        r = -1.0 if spacing is None else _spacing(who, spacing, positive=True)
        factor, seed = _count(who, "init_factor", init_factor), _seed(who, seed)
        mode, dev = self.normals_mode(use_triangle_normal), self.dev
        count, drawn, r_out, rounds, probes = C.c_int64(), C.c_int64(), C.c_double(), C.c_int32(), C.c_int32()
        launch(dev, "pedp_mesh_sample_disk",
               lambda lib, ch, mem: lib.pedp_mesh_sample_disk(self._h, seed, n, r, factor, mode, C.byref(count), C.byref(drawn), C.byref(r_out),
                                                              C.byref(rounds), C.byref(probes)), self.ctx)
        k = count.value
        pts, face, bary = empty(dev, (k, 3), np.float64), empty(dev, (k,), np.int32), empty(dev, (k, 3), np.float64)
        nrm = empty(dev, (k, 3), np.float64) if mode else None
        index = empty(dev, (k,), np.int32)
        launch(dev, "pedp_mesh_sample_disk_read",
               lambda lib, ch, mem: lib.pedp_mesh_sample_disk_read(self._h, mem, ptr(pts), ptr(face), ptr(bary), ptr(nrm), ptr(index)), self.ctx)
        return _cloud(dev, pts, nrm, face_ids=face, barycentric=bary, index=index, spacing=r_out.value, drawn=drawn.value,
                      rounds=rounds.value, probes=probes.value)


def sample_points_uniformly(mesh, number_of_points=100, use_triangle_normal=False, seed=0, first=0, ctx=None):
    """TriangleMesh.sample_points_uniformly: number_of_points points drawn uniformly by area, samples [first, first +
    number_of_points) of the seed's endless sequence (so clouds can be drawn in pieces).  Normals as in Open3D: the face's
    unit normal with use_triangle_normal, else the interpolated (not renormalised) vertex normals if the mesh has them,
    else none.  A SampledCloud on the mesh's side, with face_ids and barycentric."""
    who = "sample_points_uniformly"
    _count(who, "number_of_points", number_of_points)
    with MeshSampler(mesh, ctx, who) as s:
        return s.sample(number_of_points, use_triangle_normal, seed, first, who)


def _points_array(who, points):
    if hasattr(points, "points") and not hasattr(points, "shape"):
        points = getattr(points, "_dev_points", None) if getattr(points, "_points", 0) is None else points.points
    dev = device_of(points)
    if not hasattr(points, "shape") or len(points.shape) != 2 or points.shape[1] != 3:
        raise _lib.PedpError(f"{who}: points must be an N x 3 array, got {tuple(getattr(points, 'shape', ())) or type(points).__name__}")
    return as_array(points, dev, np.float64), dev


def thin_to_spacing(points, spacing, seed=0, ctx=None):
    """The thinning of the Poisson-disk forms on any cloud (points: N x 3, a numpy array, a CUDA tensor or a PointCloud):
    the indices, ascending, of the one subset S(spacing) that a visit in ascending key order keeps -- the keys are a hash
    of (index, seed), so the input's order (a depth camera's rows) shapes nothing.  No two kept points are closer than
    spacing, and every point is closer than spacing to a kept one.  int32, on the points' side."""
    who = "thin_to_spacing"
    p, dev = _points_array(who, points)
    r, seed, n = _spacing(who, spacing), _seed(who, seed), int(p.shape[0])
    ctx = _context(who, dev, ctx)
    kept, count, rounds = empty(dev, (n,), np.int32), C.c_int64(), C.c_int32()
    launch(dev, "pedp_points_thin",
           lambda lib, ch, mem: lib.pedp_points_thin(ch, ptr(p), n, r, seed, mem, n, ptr(kept), C.byref(count), C.byref(rounds)), ctx)
    return kept[:count.value]


def sample_points_poisson_disk(mesh, number_of_points=None, init_factor=5, pcl=None, use_triangle_normal=False, spacing=None, seed=0,
                               ctx=None):
    """TriangleMesh.sample_points_poisson_disk: number_of_points evenly spaced points of the surface.

    init_factor * number_of_points samples are drawn (or `pcl`, a cloud of at least number_of_points points, is taken in
    their place) and thinned at the largest spacing -- bisected for 24 halvings on [0, 2 sqrt(area / number_of_points)] --
    that keeps number_of_points of them; the result's `spacing` says what it was.  With spacing = r in the place of a count:
    the thinning at r of ceil(init_factor * area / r^2) samples (or of pcl).  A SampledCloud on the mesh's side."""
    who = "sample_points_poisson_disk"
    if (number_of_points is None) == (spacing is None):
        raise _lib.PedpError(f"{who}: give number_of_points or spacing, one of them, got number_of_points = {number_of_points!r} and "
                             f"spacing = {spacing!r}")
    if number_of_points is not None:
        _count(who, "number_of_points", number_of_points)
    else:
        _spacing(who, spacing, positive=pcl is None)
    _count(who, "init_factor", init_factor)
    with MeshSampler(mesh, ctx, who) as s:
        if pcl is None:
            return s.sample_disk(number_of_points, spacing, init_factor, use_triangle_normal, seed, who)
        p, dev = _points_array(who, pcl)
        seed, n = _seed(who, seed), int(p.shape[0])
        nrm = pcl.normals if hasattr(pcl, "has_normals") and pcl.has_normals() else None
        if number_of_points is None:
            kept = thin_to_spacing(p, spacing, seed, ctx)
            r_out, rounds, probes = float(spacing), None, 1
        else:
            k = int(number_of_points)
            if k > n:
                raise _lib.PedpError(f"{who}: number_of_points = {k} exceeds the {n} points of pcl")
            r_max = 2.0 * np.sqrt(s.area / k)
            kept, r, rounds, probes = empty(dev, (k,), np.int32), C.c_double(), C.c_int32(), C.c_int32()
            launch(dev, "pedp_points_thin_count",
                   lambda lib, ch, mem: lib.pedp_points_thin_count(ch, ptr(p), n, k, float(r_max), seed, mem, ptr(kept), C.byref(r),
                                                                   C.byref(rounds), C.byref(probes)), _context(who, dev, ctx))
            r_out, rounds, probes = r.value, rounds.value, probes.value
        rows = kept.long() if is_torch(kept) else kept
        if nrm is not None:
            nrm = as_array(nrm, dev, np.float64)[rows]
        return _cloud(dev, p[rows], nrm, index=kept, spacing=r_out, drawn=n, rounds=rounds, probes=probes)


def mesh_to_pcd(mesh_out, param):
    """src/pose_estimation.py:453-464: param['mesh']['number_of_points'] Poisson-disk samples of the mesh, their normals
    estimated from the cloud like every other cloud of the pipeline (hybrid search, radius 2, at most 5 neighbours)."""
    from .icp_refine import estimate_normals

    params = param["mesh"]
    pcd = sample_points_poisson_disk(mesh_out, params["number_of_points"])
    estimate_normals(pcd, params)
    return pcd
