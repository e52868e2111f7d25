"""The inspection coverage map: which faces of the CAD model the camera has seen, and how well.

    CoverageMap(model)       per face of the model: the pixels that saw it, the views, the best cosine between a ray and
                             its normal, the smallest footprint of a pixel on it and the pixels where something stood in
                             front of it (pedp_coverage_add, csrc/pedp_coverage.hip); the covered share of the surface
                             and the connected regions of what is still uncovered (pedp_coverage_summary / _regions)

A DefectMap says which faces are defective; a face it reads as `peak 0, hits 0, frames 0` is either clean or never seen.
The coverage map closes an inspection with the other half: was the whole part looked at?  The reference has no
counterpart (run.py shows hit clouds and never says what was not inspected).  The state lies over the faces of a
DefectMap and borrows its areas, adjacency and region machinery; the contract (the ray, the seven classes, the footprint,
integer atomics, the fixed order of the sums) is DESIGN.md s4.20.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import as_array, device_of, empty, is_torch, launch, on_torch_stream, ptr
from .defect_map import MAX_GROW, REGION_DTYPE, DefectMap

CLASSES = ("masked", "miss", "no_depth", "occluded", "behind", "grazing", "seen")
MASKED, MISS, NO_DEPTH, OCCLUDED, BEHIND, GRAZING, SEEN = range(7)
Z_MIN = 0.001


def pixel_rays6(K, W, H):
    """The [origin | direction] float32 rows of every pixel of a pinhole camera, row-major (pixel y W + x), from the
    origin: d = (xn, yn, 1) / sqrt((xn xn + yn yn) + 1), xn = (x - cx) / fx, yn = (y - cy) / fy in float64
    (compute_rays' arithmetic, which pedp_coverage_add repeats per pixel)."""
    ys, xs = np.mgrid[0:H, 0:W]
    xn = (xs.reshape(-1).astype(np.float64) - K[0, 2]) / K[0, 0]
    yn = (ys.reshape(-1).astype(np.float64) - K[1, 2]) / K[1, 1]
    length = np.sqrt((xn * xn + yn * yn) + 1.0)
    rays = np.zeros((W * H, 6), np.float32)
    rays[:, 3], rays[:, 4], rays[:, 5] = xn / length, yn / length, 1.0 / length
    return rays


def _dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def _check_camera(who, intrinsic_matrix):
    K = np.asarray(intrinsic_matrix, dtype=np.float64)
    if K.shape != (3, 3):
        raise _lib.PedpError(f"{who}: intrinsic_matrix must be 3 x 3, got shape {K.shape}")
    if not np.isfinite(K[:2]).all() or K[0, 0] <= 0 or K[1, 1] <= 0:
        raise _lib.PedpError(f"{who}: the focal lengths must be positive and the intrinsics finite, got fx = {K[0, 0]}, fy = {K[1, 1]}")
    return K


def _check_view(who, cov, mesh, depth, depth_scale, depth_tol, min_cos):
    """What every view needs whatever it is made from: the mesh, the parameters.  Returns the parameter record."""
    if not isinstance(mesh, _lib.Mesh):
        raise _lib.PedpError(f"{who}: mesh must be a _lib.Mesh, got {type(mesh).__name__}")
    if mesh.ctx is not cov.ctx:
        raise _lib.PedpError(f"{who}: the mesh belongs to another context than the coverage map")
    if mesh.F != cov.F:
        raise _lib.PedpError(f"{who}: the mesh has {mesh.F} faces, the map {cov.F}")
    if depth is not None:
        if depth_tol is None:
            raise _lib.PedpError(f"{who}: depth needs depth_tol (mesh units): it is the sensor's and has no default")
        if not float(depth_tol) >= 0.0:
            raise _lib.PedpError(f"{who}: depth_tol must be >= 0, got {depth_tol!r}")
    if not 0.0 <= float(min_cos) <= 1.0:
        raise _lib.PedpError(f"{who}: min_cos must lie in [0, 1], got {min_cos!r}")
    if not np.isfinite(float(depth_scale)):
        raise _lib.PedpError(f"{who}: depth_scale must be finite, got {depth_scale!r}")
    return _lib.CoverageView(float(depth_scale), 0.0 if depth_tol is None else float(depth_tol), float(min_cos), Z_MIN)


def _check_image(who, name, a, shape, kinds):
    if not hasattr(a, "shape") or not hasattr(a, "dtype"):
        raise _lib.PedpError(f"{who}: {name} must be an array or a tensor, got {type(a).__name__}")
    if tuple(a.shape) != tuple(shape):
        raise _lib.PedpError(f"{who}: {name} must be H x W = {shape[0]} x {shape[1]}, got shape {tuple(a.shape)}")
    if _dtype_name(a) not in kinds:
        raise _lib.PedpError(f"{who}: {name} must be {' or '.join(kinds)}, got {_dtype_name(a)}")


def _check_cast(who, t_hit, primitive_ids, depth, mask):
    """The images of add_cast: H x W each, of one shape.  Returns (H, W)."""
    if not hasattr(t_hit, "shape") or len(t_hit.shape) != 2 or 0 in tuple(t_hit.shape):
        raise _lib.PedpError(f"{who}: t_hit must be a non-empty H x W array or tensor, got "
                             f"{'shape ' + str(tuple(t_hit.shape)) if hasattr(t_hit, 'shape') else type(t_hit).__name__}")
    shape = tuple(int(s) for s in t_hit.shape)
    _check_image(who, "t_hit", t_hit, shape, ("float32",))
    _check_image(who, "primitive_ids", primitive_ids, shape, ("uint32", "int32"))
    if depth is not None:
        _check_image(who, "depth", depth, shape, ("float32",))
    if mask is not None:
        _check_image(who, "mask", mask, shape, ("uint8", "bool"))
    return shape


def _check_criteria(who, min_views=1, min_pixels=1, min_cos=0.0, max_footprint=np.inf):
    for name, x in (("min_views", min_views), ("min_pixels", min_pixels)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise _lib.PedpError(f"{who}: {name} must be an integer, got {x!r}")
    if not -2 ** 31 <= min_views < 2 ** 31:
        raise _lib.PedpError(f"{who}: min_views = {min_views} is no int32")
    if not -2 ** 63 <= min_pixels < 2 ** 63:
        raise _lib.PedpError(f"{who}: min_pixels = {min_pixels} is no int64")
    for name, x in (("min_cos", min_cos), ("max_footprint", max_footprint)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or x != x:
            raise _lib.PedpError(f"{who}: {name} must be a number, got {x!r}")
    return _lib.CoverageCriteria(int(min_views), int(min_pixels), float(min_cos), float(max_footprint))


def _check_region_args(who, grow):
    if isinstance(grow, bool) or not isinstance(grow, (int, np.integer)) or not 0 <= grow <= MAX_GROW:
        raise _lib.PedpError(f"{who}: grow must be an integer in 0 ... {MAX_GROW}, got {grow!r}")


def _as_mask(mask, dev):
    if mask is None:
        return None
    if _dtype_name(mask) == "bool":
        if is_torch(mask):
            import torch

            mask = mask.to(torch.uint8)
        else:
            mask = np.asarray(mask).view(np.uint8)
    return as_array(mask, dev, np.uint8, u8_ok=True)


class CoverageMap:
    """Per-face evidence that the camera observed the model, over the faces of a DefectMap.

    model_or_defect_map: a DefectMap to share (its areas, adjacency and region scratch serve both; it is kept alive and
    stays the caller's to close, after this map), or what DefectMap takes (a holder with .vertices / .triangles or a
    (vertices, triangles) pair), of which the coverage map then makes a DefectMap of its own (`.defect_map`) and closes it
    with itself.  The library's handle points into the defect map: once that is closed every call here raises."""

    def __init__(self, model_or_defect_map, ctx=None):
        self._owns_map = not isinstance(model_or_defect_map, DefectMap)
        if not self._owns_map:
            self.defect_map = model_or_defect_map
            if ctx is not None and ctx is not self.defect_map.ctx:
                raise _lib.PedpError("CoverageMap: the defect map belongs to another context than ctx")
        else:
            self.defect_map = DefectMap(model_or_defect_map, ctx)
        self.ctx = self.defect_map.ctx
        self.V, self.F = self.defect_map.V, self.defect_map.F
        self._cameras = {}       # (K, W, H) -> (RaySet, t_hit, primitive_ids): one resident ray set per camera
        self._h = C.c_void_p()
        if not self.defect_map._h:
            raise _lib.PedpError("CoverageMap: the defect map is closed")
        _lib.check(_lib.load().pedp_coverage_create(self.defect_map._h, C.byref(self._h)), "pedp_coverage_create")

    def _handle(self, who):
        """The library's handle, while it and the defect map it points into are open."""
        if not self._h:
            raise _lib.PedpError(f"{who}: the coverage map is closed")
        if not self.defect_map._h:
            raise _lib.PedpError(f"{who}: the defect map under the coverage map is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().pedp_coverage_destroy(self._h)
            self._h = C.c_void_p()
        for rayset, _, _ in getattr(self, "_cameras", {}).values():
            rayset.close()
        self._cameras = {}
        if getattr(self, "_owns_map", False):           # behind the handle that points into it
            self.defect_map.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ accumulating
    def add_cast(self, mesh, intrinsic_matrix, t_hit, primitive_ids, depth=None, mask=None, depth_scale=1.0, depth_tol=None,
                 min_cos=0.0, want_status=False):
        """One view from a cast that was made elsewhere.  mesh: a _lib.Mesh of the map's context with the map's F, posed
        as the frame sees it; t_hit H x W float32 and primitive_ids H x W uint32 / int32: the cast of the camera's pixel
        rays (pixel_rays6) against it; depth H x W float32 (with depth_tol, in mesh units; z = depth * depth_scale) and
        mask H x W uint8 / bool are optional.  numpy arrays or CUDA tensors; tensors stay on the device.  Returns the
        H x W uint8 class image (MASKED ... SEEN) with want_status, else None."""
        who = "CoverageMap.add_cast"
        prm = _check_view(who, self, mesh, depth, depth_scale, depth_tol, min_cos)
        K = _check_camera(who, intrinsic_matrix)
        H, W = _check_cast(who, t_hit, primitive_ids, depth, mask)
        handle = self._handle(who)
        dev = device_of(t_hit, primitive_ids, depth, mask)
        if dev is not None and (dev.index or 0) != self.ctx.device:
            raise _lib.PedpError(f"{who}: the images are on {dev}, the map on cuda:{self.ctx.device}")
        t = as_array(t_hit, dev, np.float32)
        if dev is not None:
            import torch

            ids = primitive_ids if is_torch(primitive_ids) else torch.from_numpy(np.ascontiguousarray(primitive_ids).view(np.int32))
            ids = ids.to(dev).contiguous()                # int32 bits read as uint32: -1 is the miss id
        else:
            ids = primitive_ids.detach().cpu().numpy() if is_torch(primitive_ids) else np.asarray(primitive_ids)
            ids = np.ascontiguousarray(ids).view(np.uint32)
        d = None if depth is None else as_array(depth, dev, np.float32)
        m = _as_mask(mask, dev)
        status = empty(dev, (H, W), np.uint8) if want_status else None
        cam = _lib.Pinhole(K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H)
        launch(dev, "pedp_coverage_add",
               lambda lib, h, mem: lib.pedp_coverage_add(handle, mesh._h, C.byref(cam), ptr(t), ptr(ids), ptr(d), ptr(m), C.byref(prm),
                                                         mem, ptr(status)), self.ctx)
        return status

    def _camera(self, K, W, H):
        import torch

        key = (K.tobytes(), W, H)
        if key not in self._cameras:
            dev = torch.device("cuda", self.ctx.device)
            self._cameras[key] = (_lib.RaySet(self.ctx, pixel_rays6(K, W, H)),
                                  torch.empty((H, W), dtype=torch.float32, device=dev),
                                  torch.empty((H, W), dtype=torch.int32, device=dev))
        return self._cameras[key]

    def add_view(self, mesh, intrinsic_matrix, shape, depth=None, mask=None, depth_scale=1.0, depth_tol=None, min_cos=0.0,
                 want_status=False):
        """One view of the camera (intrinsic_matrix, shape = (H, W)) on `mesh` as posed: the camera's resident ray set
        (one per (K, W, H), built on first use) is cast with cast_rayset_device and the result fed to pedp_coverage_add
        without leaving the device.  depth, mask and the parameters as for add_cast (numpy arrays or CUDA tensors).
        Returns the H x W uint8 class image as a CUDA tensor with want_status, else None."""
        who = "CoverageMap.add_view"
        prm = _check_view(who, self, mesh, depth, depth_scale, depth_tol, min_cos)
        K = _check_camera(who, intrinsic_matrix)
        if not isinstance(shape, (tuple, list)) or len(shape) != 2 or not all(isinstance(s, (int, np.integer)) and s > 0 for s in shape):
            raise _lib.PedpError(f"{who}: shape must be (H, W), two positive integers, got {shape!r}")
        H, W = int(shape[0]), int(shape[1])
        if depth is not None:
            _check_image(who, "depth", depth, (H, W), ("float32",))
        if mask is not None:
            _check_image(who, "mask", mask, (H, W), ("uint8", "bool"))
        handle = self._handle(who)
        import torch

        dev = torch.device("cuda", self.ctx.device)
        new_camera = (K.tobytes(), W, H) not in self._cameras
        rayset, t, ids = self._camera(K, W, H)
        d = None if depth is None else as_array(depth, dev, np.float32)
        m = _as_mask(mask, dev)
        status = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_status else None
        # On torch's current stream the context's launches are ordered with torch's work and nothing waits (the rule of
        # _bridge.launch).  Otherwise the host waits for torch before the library touches memory that torch has just
        # handed out or filled (the caller's images, a new status image, a new camera's buffers), and for the library
        # before such memory goes back to torch; the camera's own buffers are used on the context's stream alone.
        apart = not on_torch_stream(self.ctx, dev)
        theirs = d is not None or m is not None or status is not None
        if apart and (theirs or new_camera):
            torch.cuda.current_stream(dev).synchronize()
        mesh.cast_rayset_device(rayset, t.data_ptr(), ids.data_ptr())
        cam = _lib.Pinhole(K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H)
        _lib.check(_lib.load().pedp_coverage_add(handle, mesh._h, C.byref(cam), ptr(t), ptr(ids), ptr(d), ptr(m), C.byref(prm),
                                                 _lib.DEVICE, ptr(status)), "pedp_coverage_add")
        if apart and theirs:
            self.ctx.synchronize()
        return status

    def clear(self):
        _lib.check(_lib.load().pedp_coverage_clear(self._handle("CoverageMap.clear")), "pedp_coverage_clear")

    # ------------------------------------------------------------ reading
    def faces(self):
        """dict(pixels F int64, views F int32, best_cos F float64, min_footprint F float64, blocked F int64); a face never
        seen reads 0, 0, 0.0, +inf, 0."""
        out = {"pixels": np.empty(self.F, np.int64), "views": np.empty(self.F, np.int32), "best_cos": np.empty(self.F, np.float64),
               "min_footprint": np.empty(self.F, np.float64), "blocked": np.empty(self.F, np.int64)}
        _lib.check(_lib.load().pedp_coverage_faces(self._handle("CoverageMap.faces"), _lib.HOST, _lib._ptr(out["pixels"]), _lib._ptr(out["views"]),
                                                   _lib._ptr(out["best_cos"]), _lib._ptr(out["min_footprint"]),
                                                   _lib._ptr(out["blocked"])), "pedp_coverage_faces")
        return out

    def covered(self, **criteria):
        """F bool: views >= min_views [1] and pixels >= min_pixels [1] and best_cos >= min_cos [0] and min_footprint <=
        max_footprint [inf], the rule of pedp_coverage_summary / _regions on the values of faces()."""
        c = _check_criteria("CoverageMap.covered", **criteria)
        f = self.faces()
        return ((f["views"] >= c.min_views) & (f["pixels"] >= c.min_pixels) & (f["best_cos"] >= c.min_cos)
                & (f["min_footprint"] <= c.max_footprint))

    def summary(self, **criteria):
        """dict(covered_faces, faces, covered_area, total_area, fraction = covered_area / total_area) under the criteria
        of covered(); the areas are summed on the device in a fixed order (the same bits on every call)."""
        c = _check_criteria("CoverageMap.summary", **criteria)
        out = _lib.CoverageTotals()
        _lib.check(_lib.load().pedp_coverage_summary(self._handle("CoverageMap.summary"), C.byref(c), C.byref(out)), "pedp_coverage_summary")
        return {"covered_faces": out.covered_faces, "faces": out.faces, "covered_area": out.covered_area, "total_area": out.total_area,
                "fraction": out.covered_area / out.total_area if out.total_area > 0 else float("nan")}

    def stats(self):
        """dict(views, masked, miss, no_depth, occluded, behind, grazing, seen): the views and the pixels of each class since
        the last clear (waits for the stream)."""
        views, classes = C.c_int64(), (C.c_int64 * 7)()
        _lib.check(_lib.load().pedp_coverage_stats(self._handle("CoverageMap.stats"), C.byref(views), classes), "pedp_coverage_stats")
        return dict({"views": views.value}, **{name: classes[k] for k, name in enumerate(CLASSES)})

    def regions(self, covered=False, grow=0, capacity=None, **criteria):
        """The connected regions of the UNCOVERED faces (covered=False: where to point the camera next) or of the covered
        ones, grown `grow` times, numbered by their lowest face: DefectMap.regions' dict, with hits = the faces' pixels
        summed, max_frames = their largest views and peak = the largest best_cos over the faces with pixels."""
        who = "CoverageMap.regions"
        _check_region_args(who, grow)
        c = _check_criteria(who, **criteria)
        handle = self._handle(who)
        cap = min(self.F, 1024) if capacity is None else int(capacity)
        labels = np.empty(self.F, np.int32)
        lib = _lib.load()
        while True:
            table = np.zeros(cap, REGION_DTYPE)
            n = C.c_int64()
            rc = lib.pedp_coverage_regions(handle, C.byref(c), int(bool(covered)), int(grow), _lib.HOST, _lib._ptr(labels), cap,
                                           _lib._ptr(table) if cap else None, C.byref(n))
            if rc != 0 and n.value > cap and capacity is None:   # more regions than the guess: once more with room
                cap = n.value
                continue
            _lib.check(rc, "pedp_coverage_regions")
            break
        out = {"labels": labels, "n_regions": n.value}
        for name in REGION_DTYPE.names:
            out[name] = np.ascontiguousarray(table[name][:n.value])
        return out

    def face_colors(self, by="views", jet_lut=None, unseen=(0.5, 0.5, 0.5)):
        """F x 3 float64 colours for the viewer's mesh: jet_lut[clip(trunc(s * 256), 0, 255)] of `by` ("views", "best_cos"
        or "min_footprint") min-max normalised over the seen faces (DefectMap.face_colors' arithmetic; equal values
        divide by zero like it: NaN -> black, as is an infinite footprint), `unseen` for the faces never seen.  On the
        host."""
        from .ray_projection import _jet_lut

        if by not in ("views", "best_cos", "min_footprint"):
            raise _lib.PedpError(f"CoverageMap.face_colors: by must be 'views', 'best_cos' or 'min_footprint', got {by!r}")
        lut = _jet_lut() if jet_lut is None else np.ascontiguousarray(jet_lut, dtype=np.float64)
        if lut.shape != (256, 3):
            raise _lib.PedpError(f"CoverageMap.face_colors: jet_lut must be 256 x 3, got shape {lut.shape}")
        f = self.faces()
        seen = f["pixels"] > 0
        colors = np.tile(np.asarray(unseen, dtype=np.float64).reshape(1, 3), (self.F, 1))
        if seen.any():
            p = f[by][seen].astype(np.float64)
            ok = np.isfinite(p)
            with np.errstate(invalid="ignore", divide="ignore"):
                lo, hi = (p[ok].min(), p[ok].max()) if ok.any() else (0.0, 0.0)
                x = (p - lo) / (hi - lo) * 256.0
            bad = ~np.isfinite(x)
            x[bad] = 0.0
            rgb = np.take(lut, np.clip(x, 0.0, 255.0).astype(np.intp), axis=0)
            rgb[bad] = 0.0
            colors[seen] = rgb
        return colors
