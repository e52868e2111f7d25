"""Robust best fit of a scene cloud to the posed CAD surface: the pose an inspection is measured in.

    fit_to_surface         iteratively re-weighted Gauss-Newton of a point cloud onto the mesh as posed, over the exact
                           closest-point search (pedp_fit_to_surface, csrc/pedp_surface_fit.hip); the whole loop on the device
    refit_pose             the object pose that a fit implies when the scene stayed fixed and the mesh was posed by `pose`
    fit_frame_to_surface   fit_to_surface of the valid pixels of a depth frame, the points formed as deviation_heatmap does

It belongs between refine_pose_with_icp and deviation_heatmap: the ICP pose, found against a subsampled vertex cloud of the
model, is the start value, and the fit against the triangles themselves, with a loss that a dent cannot pull, is the pose
the deviation is measured in.  CUDA tensors stay on their stream (no host wait; the numbers of the result are read when
the result is built); numpy arrays and CPU tensors use host memory.  The contract is DESIGN.md s4.21.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import as_array, device_of, empty, is_torch, launch, ptr
from .geometry import RegistrationResult
from .surface_distance import _leading_shape, _mesh_of

LOSSES = {"l2": 0, "huber": 1, "tukey": 2}      # PEDP_FIT_L2 / _HUBER / _TUKEY
STATS_DOUBLES = 40                              # PEDP_FIT_STATS_DOUBLES
MAX_ITERATION = 1000


def _behind(a, count):
    """The pointer `count` float64 values into the array or tensor a."""
    return C.c_void_p(ptr(a).value + 8 * count)


def fit_to_surface(mesh, points, init=None, loss="tukey", scale=None, gate=float("inf"), max_iteration=30,
                   relative_fitness=1e-6, relative_rmse=1e-6, trace=False, ctx=None):
    """The rigid correction T that brings `points` (... x 3, float32 or float64; numpy, a CPU tensor or a CUDA tensor) onto
    the surface of `mesh` (a _lib.Mesh or a holder with .vertices / .triangles) as posed, starting from `init` (4 x 4, the
    identity by default).  loss: "l2", "huber" (weight 1 up to `scale`, scale / d beyond) or "tukey" (weight
    (1 - (d / scale)^2)^2 below `scale`, 0 from there on); `scale`, in the mesh's units, is required for the robust two.
    Rows farther than `gate` from the surface take no part.  Stops after `max_iteration` updates or when fitness and
    rmse both change by less than the two thresholds, like registration_icp.

    Returns a RegistrationResult: transformation (4 x 4 float64 numpy), fitness (inliers over finite rows), inlier_rmse,
    and with them iterations (updates applied), inliers, weight_sum, singular (a solve was refused: the pose is the last
    good one), packet (the 30 sums of the last pass) and trace (None, or one row per pass: fitness, rmse, the 16 of T)."""
    name = "fit_to_surface"
    if loss not in LOSSES:
        raise _lib.PedpError(f"{name}: loss must be one of {', '.join(LOSSES)}, got {loss!r}")
    if loss != "l2" and not (scale is not None and scale > 0):
        raise _lib.PedpError(f"{name}: loss {loss!r} needs a positive scale (in the mesh's units), got {scale!r}")
    if not gate >= 0:
        raise _lib.PedpError(f"{name}: gate must not be negative, got {gate!r}")
    if not 0 <= int(max_iteration) <= MAX_ITERATION:
        raise _lib.PedpError(f"{name}: max_iteration must be 0 ... {MAX_ITERATION}, got {max_iteration!r}")
    _, n = _leading_shape(name, points)
    start = np.eye(4) if init is None else np.ascontiguousarray(
        init.detach().cpu().numpy() if is_torch(init) else init, dtype=np.float64)
    if start.shape != (4, 4) or not np.isfinite(start).all():
        raise _lib.PedpError(f"{name}: init must be a finite 4 x 4 matrix, got shape {start.shape}")
    dev = device_of(points)
    m = _mesh_of(name, mesh, ctx, dev)
    if dev is not None and (dev.index or 0) != m.ctx.device:
        raise _lib.PedpError(f"{name}: points are on {dev}, the mesh on cuda:{m.ctx.device}")
    p = as_array(points, dev, np.float64).reshape(n, 3)
    rows = int(max_iteration) + 1
    out = empty(dev, (16 + STATS_DOUBLES,), np.float64)
    tr = None
    if trace:
        tr = empty(dev, (rows, 18), np.float64)
        if dev is not None:
            tr.zero_()
    launch(dev, "pedp_fit_to_surface", lambda lib, h, mem: lib.pedp_fit_to_surface(
        h, m._h, ptr(p) if n else None, n, mem, _lib._ptr(start), LOSSES[loss], float(scale or 0.0), float(gate),
        int(max_iteration), float(relative_fitness), float(relative_rmse), ptr(out), _behind(out, 16), ptr(tr)), m.ctx)
    got = out.cpu().numpy() if is_torch(out) else out           # (a CUDA result: the one wait, on the caller's stream)
    stats = got[16:]
    res = RegistrationResult(got[:16].reshape(4, 4))
    res.fitness = float(stats[0])
    res.inlier_rmse = float(stats[1])
    res.iterations = int(stats[2])
    res.inliers = int(stats[3])
    res.weight_sum = float(stats[4])
    res.singular = bool(stats[5])
    res.finite_rows = int(stats[6])
    res.packet = stats[8:38].copy()
    res.trace = None
    if trace:
        full = tr.cpu().numpy() if is_torch(tr) else tr
        res.trace = full[:res.iterations + 1].copy() if n else full[:0].copy()
    return res


def refit_pose(pose, result):
    """The object pose after a fit: fit_to_surface moved the SCENE by result.transformation onto the mesh posed by `pose`;
    with the scene where it is, the object stands at inv(result.transformation) @ pose.  `result` is a RegistrationResult
    or a 4 x 4 matrix."""
    T = np.asarray(getattr(result, "transformation", result), dtype=np.float64)
    pose = np.asarray(pose.detach().cpu().numpy() if is_torch(pose) else pose, dtype=np.float64)
    if T.shape != (4, 4) or pose.shape != (4, 4):
        raise _lib.PedpError(f"refit_pose: pose and transformation must be 4 x 4, got {pose.shape} and {T.shape}")
    return np.linalg.inv(T) @ pose


def frame_points(depth, K, unit=1000.0, mask=None, zmin=0.001):
    """The measured points of a depth frame that deviation_heatmap would test, float64(depth2xyzmap(depth, K)) * unit, at
    the valid pixels alone (depth >= zmin and `mask`, if any, set), in row-major pixel order: M x 3 of depth's kind."""
    shape = tuple(depth.shape) if hasattr(depth, "shape") else None
    if shape is None or len(shape) != 2:
        raise _lib.PedpError(f"fit_frame_to_surface: depth must be H x W, got {shape if shape is not None else type(depth).__name__}")
    if mask is not None and tuple(mask.shape) != shape:
        raise _lib.PedpError(f"fit_frame_to_surface: mask must be {shape[0]} x {shape[1]} like depth, got {tuple(mask.shape)}")
    from .depth_filters import depth2xyzmap

    if is_torch(depth) and not depth.is_cuda:
        import torch

        return torch.from_numpy(frame_points(depth.numpy(), K, unit, None if mask is None else np.asarray(mask), zmin))
    xyz = depth2xyzmap(depth, K)
    if is_torch(xyz):
        import torch

        keep = depth >= zmin
        if mask is not None:
            keep = keep & torch.as_tensor(mask, device=xyz.device).bool()
        return (xyz.double() * unit)[keep]
    keep = np.asarray(depth) >= zmin
    if mask is not None:
        keep &= np.asarray(mask).astype(bool)
    return np.ascontiguousarray((xyz.astype(np.float64) * unit)[keep])


def fit_frame_to_surface(depth, K, mesh, unit=1000.0, mask=None, zmin=0.001, **fit):
    """fit_to_surface of a depth frame's measured points: depth, K, unit, mask and zmin as for deviation_heatmap; only the
    valid pixels are passed on (an invalid one would cost a search and take no part).  `fit`: fit_to_surface's keywords."""
    return fit_to_surface(mesh, frame_points(depth, K, unit, mask, zmin), **fit)
