"""The defect map: what the projected heat maps of many frames say about the CAD model itself.

    DefectMap(mesh)          per face of the model: peak intensity, hits, frames that saw it (pedp_defect_map_add), and
                             the connected regions of the marked faces with their sizes (pedp_defect_map_regions,
                             csrc/pedp_defectmap.hip)

run.py:61, :119, :196-201 keeps a growing list of hit clouds and moves every earlier cloud by relative_transformation
at each new detection.  Triangle indices keep the input's order in every mesh handle whatever the pose, so the map is
kept per face in the model frame: a constant-size object per model that is never transformed.  The contract (the
order-preserving integer key of the maximum, once-per-observation frames, the welded edge adjacency, growth, regions by
lowest face, the fixed order of the sums) is DESIGN.md s4.17.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import as_array, device_of, is_torch, launch, ptr

MISS = 0xFFFFFFFF
MAX_GROW = 64


# pedp_defect_region (include/pedp.h), 136 bytes a row
REGION_DTYPE = np.dtype([("first_face", np.int32), ("n_faces", np.int32), ("n_seed_faces", np.int32), ("max_frames", np.int32),
                         ("hits", np.int64), ("area", np.float64), ("centroid", np.float64, (3,)), ("moment", np.float64, (3,)),
                         ("peak", np.float64), ("lo", np.float64, (3,)), ("hi", np.float64, (3,))])
assert REGION_DTYPE.itemsize == 136


def _model_arrays(mesh):
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        v, t = mesh
    elif hasattr(mesh, "vertices") and hasattr(mesh, "triangles"):
        v, t = mesh.vertices, mesh.triangles
    else:
        raise _lib.PedpError(f"DefectMap: mesh must hold .vertices and .triangles or be a (vertices, triangles) pair, "
                             f"got {type(mesh).__name__}")
    v, t = np.asarray(v), np.asarray(t)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype.kind != "f":
        raise _lib.PedpError(f"DefectMap: vertices must be a V x 3 float array, got {v.dtype} of shape {v.shape}")
    if t.size == 0:
        t = t.reshape(0, 3).astype(np.uint32)
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise _lib.PedpError(f"DefectMap: triangles must be an F x 3 integer array, got {t.dtype} of shape {t.shape}")
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise _lib.PedpError(f"DefectMap: triangle indices must lie in [0, {len(v)}), got {t.min()} ... {t.max()}")
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.uint32)


def _check_rows(ids, x):
    """DefectMap.add's arguments: two 1-D arrays or tensors of one length, integer ids and floating intensities."""
    for name, a in (("primitive_ids", ids), ("intensities", x)):
        if not hasattr(a, "shape") or not hasattr(a, "dtype"):
            raise _lib.PedpError(f"DefectMap.add: {name} must be an array or a tensor, got {type(a).__name__}")
    if len(ids.shape) != 1 or tuple(ids.shape) != tuple(x.shape):
        raise _lib.PedpError(f"DefectMap.add: primitive_ids and intensities must be 1-D of one length, got shapes "
                             f"{tuple(ids.shape)} and {tuple(x.shape)}")
    kind_i, kind_x = str(ids.dtype).replace("torch.", ""), str(x.dtype).replace("torch.", "")
    if kind_i not in ("uint32", "int32", "int64"):
        raise _lib.PedpError(f"DefectMap.add: primitive_ids must be uint32, int32 or int64, got {kind_i}")
    if kind_x not in ("float32", "float64"):
        raise _lib.PedpError(f"DefectMap.add: intensities must be float32 or float64, got {kind_x}")


def _check_region_args(min_frames, grow):
    if isinstance(grow, bool) or not isinstance(grow, (int, np.integer)) or not 0 <= grow <= MAX_GROW:
        raise _lib.PedpError(f"DefectMap.regions: grow must be an integer in 0 ... {MAX_GROW}, got {grow!r}")
    if isinstance(min_frames, bool) or not isinstance(min_frames, (int, np.integer)):
        raise _lib.PedpError(f"DefectMap.regions: min_frames must be an integer, got {min_frames!r}")


class DefectMap:
    """Per-face accumulation of projected heat maps on one model, and the defect regions they form.

    mesh: a holder with .vertices / .triangles or a (vertices, triangles) pair, in the model frame (float64 as given).
    The map is tied to the device meshes it is fed from only by the shared triangle order."""

    def __init__(self, mesh, ctx=None):
        v, t = _model_arrays(mesh)
        self.ctx = ctx or _lib.default_context()
        self.V, self.F = len(v), len(t)
        self._h = C.c_void_p()
        self._hit_cap = 0
        _lib.check(_lib.load().pedp_defect_map_create(self.ctx._h, _lib._ptr(v), self.V, _lib._ptr(t), self.F, C.byref(self._h)),
                   "pedp_defect_map_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().pedp_defect_map_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ accumulating
    def add(self, primitive_ids, intensities):
        """One observation (one frame's hits): primitive_ids N (uint32, int32 or int64; 0xFFFFFFFF, -1 and every other id
        outside [0, F) are ignored and counted) and intensities N (float32 or float64; NaN rows are ignored and counted).
        numpy arrays, CPU tensors or CUDA tensors; CUDA tensors stay on the device."""
        ids, x = primitive_ids, intensities
        _check_rows(ids, x)
        dev = device_of(ids, x)
        if dev is not None and (dev.index or 0) != self.ctx.device:
            raise _lib.PedpError(f"DefectMap.add: the rows are on {dev}, the map on cuda:{self.ctx.device}")
        n = int(ids.shape[0])
        if dev is not None:
            import torch

            ids = ids.to(dev)
            if ids.dtype == torch.int64:            # ids outside uint32 (negative or huge) become the miss id, -1 as int32
                ids = torch.where((ids < 0) | (ids >= MISS), torch.full_like(ids, -1), ids)
                ids = torch.where(ids > 0x7FFFFFFF, ids - (1 << 32), ids).to(torch.int32)   # the same 32 bits
            elif ids.dtype != torch.int32:
                ids = ids.contiguous().view(torch.int32)
            ids = ids.contiguous()                  # int32 bits read as uint32: -1 is the miss id
            x = as_array(x, dev, np.float64)
        else:
            ids = ids.detach().cpu().numpy() if is_torch(ids) else np.asarray(ids)
            if ids.dtype == np.int64:
                ids = np.where((ids < 0) | (ids > MISS), MISS, ids)
            ids = np.ascontiguousarray(ids.astype(np.uint32) if ids.dtype != np.int32 else ids.view(np.uint32))
            x = as_array(x, None, np.float64)
        launch(dev, "pedp_defect_map_add", lambda lib, h, mem: lib.pedp_defect_map_add(self._h, ptr(ids), ptr(x), n, mem), self.ctx)

    def add_projection(self, mesh, heatmap, intrinsic_matrix, threshold=0.5, origin=(0.0, 0.0, 0.0)):
        """One observation from a heat map: pedp_project_heatmap_ex on `mesh` (a _lib.Mesh of the map's context with the
        map's F, posed as the frame sees it) with device outputs, fed to pedp_defect_map_add without the hits leaving the
        device.  heatmap: H x W float64 or float32, a numpy array or a CUDA tensor.  Returns the number of hits."""
        import torch

        if not isinstance(mesh, _lib.Mesh):
            raise _lib.PedpError(f"DefectMap.add_projection: mesh must be a _lib.Mesh, got {type(mesh).__name__}")
        if mesh.ctx is not self.ctx:
            raise _lib.PedpError("DefectMap.add_projection: the mesh belongs to another context than the map")
        if mesh.F != self.F:
            raise _lib.PedpError(f"DefectMap.add_projection: the mesh has {mesh.F} faces, the map {self.F}")
        opts = _lib.ProjectOpts(0, _lib.HOST, None, None, None)
        if is_torch(heatmap):
            if not heatmap.is_cuda or (heatmap.device.index or 0) != self.ctx.device:
                raise _lib.PedpError(f"DefectMap.add_projection: a heat map tensor must be on cuda:{self.ctx.device}")
            h = (heatmap if heatmap.dtype in (torch.float32, torch.float64) else heatmap.double()).contiguous()
            torch.cuda.current_stream(h.device).synchronize()       # the library reads it on the context's stream
            opts.heat_f32, opts.heat_mem, h_ptr, shape = int(h.dtype == torch.float32), _lib.DEVICE, C.c_void_p(h.data_ptr()), tuple(h.shape)
        else:
            h = np.asarray(heatmap)
            h = np.ascontiguousarray(h, dtype=np.float32 if h.dtype == np.float32 else np.float64)
            opts.heat_f32, h_ptr, shape = int(h.dtype == np.float32), _lib._ptr(h), h.shape
        if len(shape) != 2:
            raise _lib.PedpError(f"DefectMap.add_projection: the heat map must be H x W, got shape {tuple(shape)}")
        K = np.asarray(intrinsic_matrix, dtype=np.float64)
        if K.shape != (3, 3):
            raise _lib.PedpError(f"DefectMap.add_projection: intrinsic_matrix must be 3 x 3, got shape {K.shape}")
        cam = _lib.Pinhole(K[0, 0], K[1, 1], K[0, 2], K[1, 2], shape[1], shape[0])
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        dev = torch.device("cuda", self.ctx.device)
        cap = self._hit_cap if self._hit_cap > 0 else max(shape[0] * shape[1], 1)
        lib = _lib.load()
        while True:
            pts = torch.empty((cap, 3), dtype=torch.float64, device=dev)
            inten = torch.empty((cap,), dtype=torch.float64, device=dev)
            prim = torch.empty((cap,), dtype=torch.int32, device=dev)
            n_rays, n_hits = C.c_int64(), C.c_int64()
            rc = lib.pedp_project_heatmap_ex(self.ctx._h, mesh._h, C.byref(cam), h_ptr, float(threshold), _lib._ptr(o), _lib.DEVICE,
                                             cap, ptr(pts), ptr(inten), None, ptr(prim), C.byref(n_rays), C.byref(n_hits),
                                             C.byref(opts))
            if rc != 0 and n_hits.value > cap:      # more hits than room (the count is reported): once more with room
                cap = n_hits.value
                continue
            _lib.check(rc, "pedp_project_heatmap_ex")
            break
        m = n_hits.value
        self._hit_cap = m + m // 4 + 1024
        _lib.check(lib.pedp_defect_map_add(self._h, ptr(prim), ptr(inten), m, _lib.DEVICE), "pedp_defect_map_add")
        self.ctx.synchronize()                      # the buffers go back to torch's allocator
        return m

    def clear(self):
        _lib.check(_lib.load().pedp_defect_map_clear(self._h), "pedp_defect_map_clear")

    # ------------------------------------------------------------ reading
    def faces(self):
        """dict(peak F float64, hits F int64, frames F int32); a face never hit reads 0, 0, 0."""
        out = {"peak": np.empty(self.F, np.float64), "hits": np.empty(self.F, np.int64), "frames": np.empty(self.F, np.int32)}
        _lib.check(_lib.load().pedp_defect_map_faces(self._h, _lib.HOST, _lib._ptr(out["peak"]), _lib._ptr(out["hits"]),
                                                     _lib._ptr(out["frames"])), "pedp_defect_map_faces")
        return out

    def stats(self):
        """dict(observations, rows_added, rows_ignored) since the last clear (waits for the stream)."""
        o, a, i = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.load().pedp_defect_map_stats(self._h, C.byref(o), C.byref(a), C.byref(i)), "pedp_defect_map_stats")
        return {"observations": o.value, "rows_added": a.value, "rows_ignored": i.value}

    def regions(self, threshold=0.5, min_frames=1, grow=0, capacity=None):
        """The defect regions: faces with hits > 0, peak > threshold and frames >= min_frames, grown `grow` times over the
        edge adjacency, split into connected components numbered by their lowest face.  Returns dict(labels F int32
        (-1: in no region), n_regions, and one array of length R per column of pedp_defect_region: first_face, n_faces,
        n_seed_faces, max_frames, hits, area, centroid R x 3, moment R x 3, peak, lo R x 3, hi R x 3)."""
        _check_region_args(min_frames, grow)
        cap = min(self.F, 1024) if capacity is None else int(capacity)
        labels = np.empty(self.F, np.int32)
        lib = _lib.load()
        while True:
            table = np.zeros(cap, REGION_DTYPE)
            n = C.c_int64()
            rc = lib.pedp_defect_map_regions(self._h, float(threshold), int(min_frames), int(grow), _lib.HOST, _lib._ptr(labels), cap,
                                             _lib._ptr(table) if cap else None, C.byref(n))
            if rc != 0 and n.value > cap and capacity is None:   # more regions than the guess: once more with room
                cap = n.value
                continue
            _lib.check(rc, "pedp_defect_map_regions")
            break
        out = {"labels": labels, "n_regions": n.value}
        for name in REGION_DTYPE.names:
            out[name] = np.ascontiguousarray(table[name][:n.value])
        return out

    def face_colors(self, jet_lut=None, unhit=(0.5, 0.5, 0.5)):
        """F x 3 float64 colours for the viewer's mesh: jet_lut[clip(trunc(s * 256), 0, 255)] of the peaks min-max
        normalised over the hit faces (create_intersection_pcd's arithmetic; equal peaks divide by zero like it: NaN ->
        black), `unhit` for the faces never hit.  On the host; jet_lut defaults to ray_projection's table."""
        from .ray_projection import _jet_lut

        lut = _jet_lut() if jet_lut is None else np.ascontiguousarray(jet_lut, dtype=np.float64)
        if lut.shape != (256, 3):
            raise _lib.PedpError(f"DefectMap.face_colors: jet_lut must be 256 x 3, got shape {lut.shape}")
        f = self.faces()
        hit = f["hits"] > 0
        colors = np.tile(np.asarray(unhit, dtype=np.float64).reshape(1, 3), (self.F, 1))
        if hit.any():
            p = f["peak"][hit]
            with np.errstate(invalid="ignore", divide="ignore"):
                x = (p - p.min()) / (p.max() - p.min()) * 256.0
            bad = x != x
            x[bad] = 0.0
            rgb = np.take(lut, np.clip(x, 0.0, 255.0).astype(np.intp), axis=0)
            rgb[bad] = 0.0
            colors[hit] = rgb
        return colors
