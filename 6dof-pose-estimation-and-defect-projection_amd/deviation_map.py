"""The deviation map: how far off the part is on every face, measured over everything the camera saw.

    DeviationMap(model)      per face of the model: the count, mean, spread, extremes and frames of the SIGNED distance of
                             the depth points that fell on it (pedp_deviation_map_add / _add_points,
                             csrc/pedp_deviationmap.hip); the regions of faces whose mean is off, with the volume of
                             excess or missing material (pedp_deviation_map_regions), and the totals (_summary)

A DefectMap keeps the PEAK of a projected heat image per face; a peak over frames of a noisy measurement grows with every
frame added, loses the sign and saturates the millimetres.  The deviation map keeps exact integer sums of the quantised
signed distance instead, so that the noise of the mean shrinks with sqrt(n).  The face of a point is the one the
closest-point search found, so a frame's points go in with one search and no ray cast.  The reference has no counterpart.
The state lies over the faces of a DefectMap and borrows its areas, adjacency and region machinery; the contract (the
rows taken, the quantisation, integer atomics, the exact variance, the marking, the fixed order of the sums) is
DESIGN.md s4.23.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import as_array, device_of, is_torch, launch, ptr
from .defect_map import MAX_GROW, MISS, REGION_DTYPE, DefectMap

MAX_GATE = 1024.0          # pedp_deviation_map_add's bound: |q| = |d| 2^20 <= 2^30
Q = 2.0 ** -20             # the unit of the quantised distance

# pedp_deviation_region (include/pedp.h): pedp_defect_region and five more columns, 176 bytes a row
DEVIATION_REGION_DTYPE = np.dtype(REGION_DTYPE.descr + [("measured_area", np.float64), ("volume", np.float64), ("mean", np.float64),
                                                        ("min_mean", np.float64), ("max_mean", np.float64)])
assert DEVIATION_REGION_DTYPE.itemsize == 176

_FACE_COLUMNS = (("n", np.int64), ("frames", np.int32), ("s1", np.int64), ("s2_hi", np.uint64), ("s2_lo", np.uint64),
                 ("min", np.float64), ("max", np.float64), ("mean", np.float64), ("std", np.float64))


def _dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def _check_gate(who, gate):
    if isinstance(gate, bool) or not isinstance(gate, (int, float, np.integer, np.floating)) or not 0.0 <= float(gate) <= MAX_GATE:
        raise _lib.PedpError(f"{who}: gate must be a number in 0 ... {MAX_GATE:g} (mesh units), got {gate!r}")
    return float(gate)


def _check_rows(who, ids, d):
    for name, a in (("primitive_ids", ids), ("signed_distances", d)):
        if not hasattr(a, "shape") or not hasattr(a, "dtype"):
            raise _lib.PedpError(f"{who}: {name} must be an array or a tensor, got {type(a).__name__}")
    if len(ids.shape) != 1 or tuple(ids.shape) != tuple(d.shape):
        raise _lib.PedpError(f"{who}: primitive_ids and signed_distances must be 1-D of one length, got shapes "
                             f"{tuple(ids.shape)} and {tuple(d.shape)}")
    if _dtype_name(ids) not in ("uint32", "int32", "int64"):
        raise _lib.PedpError(f"{who}: primitive_ids must be uint32, int32 or int64, got {_dtype_name(ids)}")
    if _dtype_name(d) not in ("float32", "float64"):
        raise _lib.PedpError(f"{who}: signed_distances must be float32 or float64, got {_dtype_name(d)}")


def _check_criteria(who, threshold=0.0, sign=0, min_samples=1, min_frames=1, z=0.0):
    for name, x in (("threshold", threshold), ("z", z)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or x != x:
            raise _lib.PedpError(f"{who}: {name} must be a number, got {x!r}")
    if isinstance(sign, bool) or not isinstance(sign, (int, np.integer)) or sign not in (-1, 0, 1):
        raise _lib.PedpError(f"{who}: sign must be -1 (missing material), 0 (either) or +1 (excess material), got {sign!r}")
    for name, x, bits in (("min_samples", min_samples, 63), ("min_frames", min_frames, 31)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not -2 ** bits <= x < 2 ** bits:
            raise _lib.PedpError(f"{who}: {name} must be an int{bits + 1}, got {x!r}")
    return _lib.DeviationCriteria(float(threshold), float(z), int(min_samples), int(min_frames), int(sign))


class DeviationMap:
    """Per-face statistics of the signed deviation over frames, over the faces of a DefectMap.

    model_or_defect_map: a DefectMap to share (its areas, adjacency and region scratch serve both; it is kept alive and
    stays the caller's to close, after this map), or what DefectMap takes, of which the deviation map then makes a
    DefectMap of its own (`.defect_map`) and closes it with itself.  The library's handle points into the defect map:
    once that is closed every call here raises."""

    def __init__(self, model_or_defect_map, ctx=None):
        self._owns_map = not isinstance(model_or_defect_map, DefectMap)
        if not self._owns_map:
            self.defect_map = model_or_defect_map
            if ctx is not None and ctx is not self.defect_map.ctx:
                raise _lib.PedpError("DeviationMap: the defect map belongs to another context than ctx")
        else:
            self.defect_map = DefectMap(model_or_defect_map, ctx)
        self.ctx = self.defect_map.ctx
        self.V, self.F = self.defect_map.V, self.defect_map.F
        self._h = C.c_void_p()
        if not self.defect_map._h:
            raise _lib.PedpError("DeviationMap: the defect map is closed")
        _lib.check(_lib.load().pedp_deviation_map_create(self.defect_map._h, C.byref(self._h)), "pedp_deviation_map_create")

    def _handle(self, who):
        """The library's handle, while it and the defect map it points into are open."""
        if not self._h:
            raise _lib.PedpError(f"{who}: the deviation map is closed")
        if not self.defect_map._h:
            raise _lib.PedpError(f"{who}: the defect map under the deviation map is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().pedp_deviation_map_destroy(self._h)
            self._h = C.c_void_p()
        if getattr(self, "_owns_map", False):           # behind the handle that points into it
            self.defect_map.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ accumulating
    def add(self, primitive_ids, signed_distances, gate=MAX_GATE):
        """One observation (one frame's rows): primitive_ids N (uint32, int32 or int64; 0xFFFFFFFF, -1 and every other id
        outside [0, F) are ignored and counted) and signed_distances N (float32 or float64, mesh units, negative inside the
        solid; NaN rows are ignored, rows with |d| > gate are gated, both counted).  numpy arrays, CPU tensors or CUDA
        tensors; CUDA tensors stay on the device."""
        who = "DeviationMap.add"
        ids, d = primitive_ids, signed_distances
        _check_rows(who, ids, d)
        gate = _check_gate(who, gate)
        handle = self._handle(who)
        dev = device_of(ids, d)
        if dev is not None and (dev.index or 0) != self.ctx.device:
            raise _lib.PedpError(f"{who}: the rows are on {dev}, the map on cuda:{self.ctx.device}")
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
        else:
            ids = ids.detach().cpu().numpy() if is_torch(ids) else np.asarray(ids)
            if ids.dtype == np.int64:
                ids = np.where((ids < 0) | (ids > MISS), MISS, ids)
            ids = np.ascontiguousarray(ids.astype(np.uint32) if ids.dtype != np.int32 else ids.view(np.uint32))
        x = as_array(d, dev, np.float64)
        launch(dev, "pedp_deviation_map_add", lambda lib, h, mem: lib.pedp_deviation_map_add(handle, ptr(ids), ptr(x), n, gate, mem),
               self.ctx)

    def add_points(self, mesh, points, solid, gate=MAX_GATE, origin=None):
        """One observation from a frame's points with ONE search: the closest face and the signed distance of every row of
        `points` (N x 3 float32 or float64, the mesh's frame; numpy, a CPU tensor or a CUDA tensor, which stays on the
        device) go into the map without an N-sized result.  mesh: a _lib.Mesh of the map's context with the map's F, posed
        as the frame sees it; solid: the model's Solid.  origin (3 numbers, the camera centre in the mesh's frame): rows
        whose closest feature faces away from it are dropped and counted as backfacing."""
        who = "DeviationMap.add_points"
        if not isinstance(mesh, _lib.Mesh):
            raise _lib.PedpError(f"{who}: mesh must be a _lib.Mesh, got {type(mesh).__name__}")
        if not isinstance(solid, _lib.Solid):
            raise _lib.PedpError(f"{who}: solid must be a Solid, got {type(solid).__name__}")
        if mesh.ctx is not self.ctx or solid.ctx is not self.ctx:
            raise _lib.PedpError(f"{who}: the {'mesh' if mesh.ctx is not self.ctx else 'solid'} belongs to another context than the map")
        if mesh.F != self.F:
            raise _lib.PedpError(f"{who}: the mesh has {mesh.F} faces, the map {self.F}")
        shape = tuple(points.shape) if hasattr(points, "shape") and hasattr(points, "dtype") else None
        if shape is None or len(shape) != 2 or shape[1] != 3:
            raise _lib.PedpError(f"{who}: points must be N x 3, got {shape if shape is not None else type(points).__name__}")
        if _dtype_name(points) not in ("float32", "float64"):
            raise _lib.PedpError(f"{who}: points must be float32 or float64, got {_dtype_name(points)}")
        gate = _check_gate(who, gate)
        o = None
        if origin is not None:
            o = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
            if o.shape != (3,) or not np.isfinite(o).all():
                raise _lib.PedpError(f"{who}: origin must be 3 finite numbers, got {origin!r}")
        handle = self._handle(who)
        dev = device_of(points)
        if dev is not None and (dev.index or 0) != self.ctx.device:
            raise _lib.PedpError(f"{who}: the points are on {dev}, the map on cuda:{self.ctx.device}")
        n = shape[0]
        p = as_array(points, dev, np.float64)
        launch(dev, "pedp_deviation_map_add_points",
               lambda lib, h, mem: lib.pedp_deviation_map_add_points(handle, mesh._h, solid._h, ptr(p), n, mem, gate, ptr(o)), self.ctx)

    def add_frame(self, depth, K, mesh, solid, unit=1000.0, mask=None, zmin=0.001, gate=MAX_GATE, backfacing=True):
        """One observation from a depth frame: the valid pixels' points (surface_fit.frame_points: depth >= zmin and
        `mask`, if any, set; float64(depth2xyzmap(depth, K)) * unit) through add_points on `mesh` as posed in the camera's
        frame.  backfacing=True drops the rows whose closest feature faces away from the camera centre, the origin of
        that frame.  A CUDA depth tensor stays on the device.  Returns the number of points."""
        from .surface_fit import frame_points

        pts = frame_points(depth, K, unit, mask, zmin)
        self.add_points(mesh, pts, solid, gate=gate, origin=(0.0, 0.0, 0.0) if backfacing else None)
        return int(pts.shape[0])

    def clear(self):
        handle = self._handle("DeviationMap.clear")
        _lib.check(_lib.load().pedp_deviation_map_clear(handle), "pedp_deviation_map_clear")

    # ------------------------------------------------------------ reading
    def faces(self):
        """dict of F values each: n int64, frames int32, s1 int64 (the sum of q = rint(d 2^20)), s2_hi / s2_lo uint64 (the
        sum of q^2 in 128 bits), min, max, mean, std float64 in mesh units, and sem = std / sqrt(n).  A face without rows
        reads n 0, frames 0 and NaN for the rest."""
        handle = self._handle("DeviationMap.faces")
        out = {k: np.empty(self.F, t) for k, t in _FACE_COLUMNS}
        _lib.check(_lib.load().pedp_deviation_map_faces(handle, _lib.HOST,
                                                        *[_lib._ptr(out[k]) for k, _ in _FACE_COLUMNS]), "pedp_deviation_map_faces")
        with np.errstate(invalid="ignore", divide="ignore"):
            out["sem"] = out["std"] / np.sqrt(out["n"].astype(np.float64))
        return out

    def stats(self):
        """dict(observations, rows_taken, rows_ignored, rows_gated, rows_backfacing) since the last clear (waits for the
        stream)."""
        handle = self._handle("DeviationMap.stats")
        v = [C.c_int64() for _ in range(5)]
        _lib.check(_lib.load().pedp_deviation_map_stats(handle, *[C.byref(x) for x in v]),
                   "pedp_deviation_map_stats")
        return dict(zip(("observations", "rows_taken", "rows_ignored", "rows_gated", "rows_backfacing"), (x.value for x in v)))

    def summary(self, **criteria):
        """The totals over the measured faces (n > 0 and n >= min_samples) under regions()' criteria: dict(faces,
        measured_faces, marked_faces, max_face, total_area, measured_area, marked_area, mean, rms, max_abs_mean); the sums
        are formed on the device in a fixed order (the same bits on every call)."""
        c = _check_criteria("DeviationMap.summary", **criteria)
        handle = self._handle("DeviationMap.summary")
        out = _lib.DeviationTotals()
        _lib.check(_lib.load().pedp_deviation_map_summary(handle, C.byref(c), C.byref(out)),
                   "pedp_deviation_map_summary")
        return {name: getattr(out, name) for name, _ in _lib.DeviationTotals._fields_}

    def regions(self, threshold, sign=0, min_samples=1, min_frames=1, z=0.0, grow=0, capacity=None):
        """The regions of the faces whose mean deviation is off: n >= min_samples, frames >= min_frames, the sign test
        (0: |mean| > threshold; +1: mean > threshold, excess material; -1: mean < -threshold, missing material) and, with
        z > 0, |mean| sqrt(n) > z std; grown `grow` times and split into connected components numbered by their lowest
        face.  DefectMap.regions' dict (hits = the faces' n summed, peak = the largest |mean|) with measured_area, volume
        (sum of area x mean over the measured faces: unit^3, signed), mean = volume / measured_area, min_mean, max_mean."""
        who = "DeviationMap.regions"
        if isinstance(grow, bool) or not isinstance(grow, (int, np.integer)) or not 0 <= grow <= MAX_GROW:
            raise _lib.PedpError(f"{who}: grow must be an integer in 0 ... {MAX_GROW}, got {grow!r}")
        c = _check_criteria(who, threshold, sign, min_samples, min_frames, z)
        handle = self._handle(who)
        cap = min(self.F, 1024) if capacity is None else int(capacity)
        labels = np.empty(self.F, np.int32)
        lib = _lib.load()
        while True:
            table = np.zeros(cap, DEVIATION_REGION_DTYPE)
            n = C.c_int64()
            rc = lib.pedp_deviation_map_regions(handle, C.byref(c), int(grow), _lib.HOST, _lib._ptr(labels), cap,
                                                _lib._ptr(table) if cap else None, C.byref(n))
            if rc != 0 and n.value > cap and capacity is None:   # more regions than the guess: once more with room
                cap = n.value
                continue
            _lib.check(rc, "pedp_deviation_map_regions")
            break
        out = {"labels": labels, "n_regions": n.value}
        for name in DEVIATION_REGION_DTYPE.names:
            out[name] = np.ascontiguousarray(table[name][:n.value])
        return out

    def face_colors(self, limit, unmeasured=(0.5, 0.5, 0.5)):
        """F x 3 float64 colours for the viewer's mesh: a diverging blue - white - red on s = clip(mean / limit, -1, 1)
        (blue: missing material, red: excess), `unmeasured` for the faces without rows.  On the host."""
        if isinstance(limit, bool) or not isinstance(limit, (int, float, np.integer, np.floating)) or not float(limit) > 0.0:
            raise _lib.PedpError(f"DeviationMap.face_colors: limit must be a positive number (mesh units), got {limit!r}")
        f = self.faces()
        colors = np.tile(np.asarray(unmeasured, dtype=np.float64).reshape(1, 3), (self.F, 1))
        have = f["n"] > 0
        s = np.clip(f["mean"][have] / float(limit), -1.0, 1.0)
        fade = 1.0 - np.abs(s)
        colors[have] = np.stack([np.where(s > 0, 1.0, fade), fade, np.where(s < 0, 1.0, fade)], axis=1)
        return colors
