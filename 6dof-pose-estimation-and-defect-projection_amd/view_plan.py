"""Next-best-view planning over the coverage map: which camera poses to take next.

    ViewPlanner(coverage, model, K, shape)   what each of a set of candidate poses would add to a CoverageMap
                             (pedp_view_plan_observe), the gain of every candidate against a working copy of the map's
                             state (pedp_view_plan_score) and the greedy choice of the next k poses
                             (pedp_view_plan_select, csrc/pedp_viewplan.hip)
    orbit_views(centre, radius, n_views)      candidate poses on a sphere around the part

CoverageMap.regions(covered=False) says where the part was not looked at; the planner turns that into camera poses.  A
candidate is an object pose (model to camera, what Mesh.set_pose takes) under the planner's camera; its observation is
what CoverageMap.add_view of that pose would add without depth and mask, by the same per-pixel rule.  The coverage map is
only ever read.  The contract (the merge, a face's progress, the gain and the fixed order of its sum, the greedy rule and
its ties) is DESIGN.md s4.22.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import on_torch_stream
from .coverage import CoverageMap, _check_camera, _check_criteria, pixel_rays6
from .defect_map import _model_arrays


def orbit_views(centre, radius, n_views):
    """N x 4 x 4 float64 object-in-camera poses: the cameras of estimator.sample_views_icosphere(n_views, radius=radius)
    (one per icosphere vertex: 12, 42, 162, ...) looking at `centre` (model frame) from `radius` away; each pose is the
    inverse of that cam_in_ob moved to `centre`."""
    c = np.asarray(centre, dtype=np.float64)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise _lib.PedpError(f"orbit_views: centre must be three finite numbers, got {centre!r}")
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or not 0.0 < radius < np.inf:
        raise _lib.PedpError(f"orbit_views: radius must be a positive number, got {radius!r}")
    if isinstance(n_views, bool) or not isinstance(n_views, (int, np.integer)) or n_views < 1:
        raise _lib.PedpError(f"orbit_views: n_views must be a positive integer, got {n_views!r}")
    from .estimator import sample_views_icosphere

    cams = sample_views_icosphere(int(n_views), radius=float(radius))
    cams[:, :3, 3] += c
    return np.ascontiguousarray(np.linalg.inv(cams))


def _check_index(who, name, x, lo=0):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < lo:
        raise _lib.PedpError(f"{who}: {name} must be an integer >= {lo}, got {x!r}")
    return int(x)


class ViewPlanner:
    """Candidate views of one camera on one model, scored against a CoverageMap.

    coverage: the CoverageMap to plan for (kept alive; it stays the caller's to close, after the planner).  model: what
    DefectMap takes (a holder with .vertices / .triangles or a (vertices, triangles) pair) with the map's face count; the
    planner poses a mesh handle of its own, so the caller's meshes and their poses are never touched.  intrinsic_matrix
    3 x 3 and shape = (H, W): the camera of every candidate, whose ray set is built once.  min_cos: the GRAZING threshold
    of the candidates' views.  capacity: the most candidates at a time (capacity x F x 20 bytes on the device).

    The WORKING STATE is the planner's copy of the map's per-face state: the map's at construction and after reset(),
    moved on by commit() and left by select() as its rounds made it."""

    def __init__(self, coverage, model, intrinsic_matrix, shape, min_cos=0.0, capacity=64):
        who = "ViewPlanner"
        if not isinstance(coverage, CoverageMap):
            raise _lib.PedpError(f"{who}: coverage must be a CoverageMap, got {type(coverage).__name__}")
        v, t = _model_arrays(model)
        if len(t) != coverage.F:
            raise _lib.PedpError(f"{who}: the model has {len(t)} faces, the map {coverage.F}")
        K = _check_camera(who, intrinsic_matrix)
        if not isinstance(shape, (tuple, list)) or len(shape) != 2 or not all(isinstance(s, (int, np.integer)) and not isinstance(s, bool)
                                                                             and s > 0 for s in shape):
            raise _lib.PedpError(f"{who}: shape must be (H, W), two positive integers, got {shape!r}")
        if isinstance(min_cos, bool) or not isinstance(min_cos, (int, float, np.integer, np.floating)) or not 0.0 <= min_cos <= 1.0:
            raise _lib.PedpError(f"{who}: min_cos must lie in [0, 1], got {min_cos!r}")
        self.capacity = _check_index(who, "capacity", capacity, 1)
        self.coverage, self.ctx, self.F = coverage, coverage.ctx, coverage.F
        self.K, self.H, self.W, self.min_cos = K, int(shape[0]), int(shape[1]), float(min_cos)
        self.n = 0
        self._h = C.c_void_p()
        self._mesh = self._rayset = self._t = self._ids = None
        handle = coverage._handle(who)
        import torch

        dev = torch.device("cuda", self.ctx.device)
        self._mesh = _lib.Mesh(self.ctx, v, t, posable=True)
        self._rayset = _lib.RaySet(self.ctx, pixel_rays6(K, self.W, self.H))
        self._t = torch.empty((self.H, self.W), dtype=torch.float32, device=dev)
        self._ids = torch.empty((self.H, self.W), dtype=torch.int32, device=dev)
        if not on_torch_stream(self.ctx, dev):
            torch.cuda.current_stream(dev).synchronize()    # the cast buffers are used on the context's stream alone from here on
        _lib.check(_lib.load().pedp_view_plan_create(handle, self.capacity, C.byref(self._h)), "pedp_view_plan_create")
        self.reset()

    def _handle(self, who):
        """The library's handle, while it and the coverage map it points into are open."""
        if not self._h:
            raise _lib.PedpError(f"{who}: the view planner is closed")
        self.coverage._handle(who)
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.load().pedp_view_plan_destroy(self._h)
            self._h = C.c_void_p()
        for h in (getattr(self, "_rayset", None), getattr(self, "_mesh", None)):
            if h is not None:
                h.close()
        self._rayset = self._mesh = self._t = self._ids = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ candidates
    def add_candidates(self, poses):
        """poses V x 4 x 4 (or one 4 x 4), model to camera: per pose the planner's mesh is posed, the camera's ray set cast
        and the result observed into the next row, all enqueued on the context's stream without a host wait.  Returns the
        candidates' indices."""
        who = "ViewPlanner.add_candidates"
        try:
            T = np.asarray(poses, dtype=np.float64)
        except (TypeError, ValueError):
            raise _lib.PedpError(f"{who}: poses must be V x 4 x 4 numbers, got {type(poses).__name__}") from None
        if T.ndim == 2 and T.shape == (4, 4):
            T = T[None]
        if T.ndim != 3 or T.shape[1:] != (4, 4):
            raise _lib.PedpError(f"{who}: poses must be V x 4 x 4, got shape {T.shape}")
        if not np.isfinite(T).all():
            raise _lib.PedpError(f"{who}: poses must be finite")
        if self.n + len(T) > self.capacity:
            raise _lib.PedpError(f"{who}: the plan is full: {self.n} candidates and {len(T)} more, room for {self.capacity}")
        handle = self._handle(who)
        lib = _lib.load()
        cam = _lib.Pinhole(self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2], self.W, self.H)
        first = self.n
        for pose in np.ascontiguousarray(T):
            self._mesh.set_pose(pose)
            self._mesh.cast_rayset_device(self._rayset, self._t.data_ptr(), self._ids.data_ptr())
            index = C.c_int64()
            _lib.check(lib.pedp_view_plan_observe(handle, self._mesh._h, C.byref(cam), C.c_void_p(self._t.data_ptr()),
                                                  C.c_void_p(self._ids.data_ptr()), self.min_cos, _lib.DEVICE, C.byref(index)),
                       "pedp_view_plan_observe")
            self.n = index.value + 1
        return list(range(first, self.n))

    def candidate(self, v):
        """dict(pixels F int64, best_cos F float64, min_footprint F float64): what candidate v would add, in the units of
        CoverageMap.faces(); a face the view does not see reads 0, 0.0, +inf."""
        who = "ViewPlanner.candidate"
        v = _check_index(who, "v", v)
        if v >= self.n:
            raise _lib.PedpError(f"{who}: candidate {v} of {self.n}")
        handle = self._handle(who)
        out = {"pixels": np.empty(self.F, np.int64), "best_cos": np.empty(self.F, np.float64), "min_footprint": np.empty(self.F, np.float64)}
        _lib.check(_lib.load().pedp_view_plan_candidate(handle, v, _lib.HOST, _lib._ptr(out["pixels"]), _lib._ptr(out["best_cos"]),
                                                        _lib._ptr(out["min_footprint"])), "pedp_view_plan_candidate")
        return out

    def clear(self):
        """Forget the candidates (the working state stays)."""
        handle = self._handle("ViewPlanner.clear")
        _lib.check(_lib.load().pedp_view_plan_clear(handle), "pedp_view_plan_clear")
        self.n = 0

    # ------------------------------------------------------------ the working state
    def reset(self):
        """The working state becomes the coverage map's state as it is now."""
        handle = self._handle("ViewPlanner.reset")
        _lib.check(_lib.load().pedp_view_plan_reset(handle), "pedp_view_plan_reset")

    def commit(self, v):
        """Candidate v is merged into the working state: what the map would hold after add_view at that pose."""
        who = "ViewPlanner.commit"
        v = _check_index(who, "v", v)
        if v >= self.n:
            raise _lib.PedpError(f"{who}: candidate {v} of {self.n}")
        handle = self._handle(who)
        _lib.check(_lib.load().pedp_view_plan_commit(handle, v), "pedp_view_plan_commit")

    # ------------------------------------------------------------ gains
    def score(self, **criteria):
        """dict(gain_area V float64, gain_faces V int64) of every candidate against the working state under the criteria
        of CoverageMap.covered(): with min_views = 1 the area and the faces that add_view at that pose would newly cover
        (with more, a view that brings a face one view nearer earns 1 / min_views of its area).  Summed on the device in a
        fixed order: the same bits on every call."""
        who = "ViewPlanner.score"
        c = _check_criteria(who, **criteria)
        handle = self._handle(who)
        out = {"gain_area": np.zeros(self.n, np.float64), "gain_faces": np.zeros(self.n, np.int64)}
        _lib.check(_lib.load().pedp_view_plan_score(handle, C.byref(c), _lib.HOST, _lib._ptr(out["gain_area"]), _lib._ptr(out["gain_faces"])),
                   "pedp_view_plan_score")
        return out

    def select(self, k, min_gain=0.0, **criteria):
        """The next k views, greedily: from the coverage map's state as it is now, k times the candidate not yet chosen
        with the largest gain_area (the lowest index among equals) is merged into the working state, until none gains more
        than min_gain.  The rounds run on the device back to back; the host waits once.  Returns dict(order n int32,
        gain_area n float64, gain_faces n int64: the chosen candidates and what each added when it was chosen;
        covered_faces, covered_area, total_area, fraction: CoverageMap.summary() of the working state afterwards)."""
        who = "ViewPlanner.select"
        k = _check_index(who, "k", k)
        if isinstance(min_gain, bool) or not isinstance(min_gain, (int, float, np.integer, np.floating)) or min_gain != min_gain:
            raise _lib.PedpError(f"{who}: min_gain must be a number, got {min_gain!r}")
        c = _check_criteria(who, **criteria)
        handle = self._handle(who)
        room = min(k, self.n)
        order, area, faces = np.empty(room, np.int32), np.empty(room, np.float64), np.empty(room, np.int64)
        n, totals = C.c_int64(), _lib.CoverageTotals()
        _lib.check(_lib.load().pedp_view_plan_select(handle, C.byref(c), k, float(min_gain), _lib._ptr(order), _lib._ptr(area),
                                                     _lib._ptr(faces), C.byref(n), C.byref(totals)), "pedp_view_plan_select")
        return {"order": order[:n.value].copy(), "gain_area": area[:n.value].copy(), "gain_faces": faces[:n.value].copy(),
                "covered_faces": totals.covered_faces, "covered_area": totals.covered_area, "total_area": totals.total_area,
                "fraction": totals.covered_area / totals.total_area if totals.total_area > 0 else float("nan")}
