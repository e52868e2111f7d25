"""Pose arithmetic of FoundationPose's refinement loop on the device (csrc/pedp_pose.hip).

    pose_update         the refiner's network output -> next poses, one lane per pose (pedp_pose_update)
    max_pair_distance   the largest distance between two points of a cloud (pedp_max_pair_distance), the maximum in
                        compute_mesh_diameter without a frame-sized n x n x 3 array on the host

CUDA tensors run on the caller's current stream; pose_update returns without a host wait.  numpy arrays and CPU tensors
use host memory.  The contract (float32 with no contraction, tanh / sin / cos in float64 rounded once, pytorch3d 0.7's
rotation formulas, unpinned) is DESIGN.md s4.10.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import as_array, check_out, device_of, empty, launch, ptr

_ROT = {"axis_angle": _lib.ROT_AXIS_ANGLE, "6d": _lib.ROT_6D}


def update_params(trans_rep="tracknet", rot_rep="axis_angle", normalize_xyz=False, trans_normalizer=1.0, rot_normalizer=1.0,
                  mesh_diameter=1.0):
    """pedp_pose_update_params from a refiner configuration.  trans_rep: 'tracknet' (tanh, scaled) or any other name
    (the output as it is); 'deepim' is not supported.  rot_rep: 'axis_angle' or '6d'.  trans_normalizer: one number or
    three."""
    if trans_rep == "deepim":
        raise NotImplementedError("trans_rep 'deepim' is not supported")
    if rot_rep not in _ROT:
        raise RuntimeError(f"unknown rot_rep {rot_rep!r}")
    tn = np.asarray(trans_normalizer, dtype=np.float64).astype(np.float32).reshape(-1)
    if tn.size not in (1, 3):
        raise _lib.PedpError(f"trans_normalizer: one value or three, got {tn.size}")
    prm = _lib.PoseUpdateParams()
    prm.trans_rep = _lib.TRANS_TRACKNET if trans_rep == "tracknet" else _lib.TRANS_RAW
    prm.rot_rep = _ROT[rot_rep]
    prm.normalize_xyz = int(bool(normalize_xyz))
    prm.trans_normalizer[:] = [float(x) for x in np.broadcast_to(tn, (3,))]
    prm.rot_normalizer = float(np.float32(rot_normalizer))
    prm.mesh_diameter = float(mesh_diameter)
    return prm


def pose_update(trans, rot, poseA, params=None, out=None, want_deltas=False, **kw):
    """trans N x 3, rot N x 3 (axis_angle) or N x 6 (6d), poseA N x 4 x 4, float32 -> (poses N x 4 x 4, trans_delta
    N x 3, rot_mat_delta N x 3 x 3); the deltas are None unless want_deltas.  `params` comes from update_params, or its
    keywords are given here (not both).  `out` receives the poses: a C-contiguous N x 4 x 4 float32 array where the
    inputs are (a CUDA tensor on their device, else a numpy array or CPU tensor); poseA itself is allowed."""
    if params is not None and kw:
        raise TypeError(f"pose_update: give params or update_params' keywords, not both ({', '.join(kw)})")
    prm = params if params is not None else update_params(**kw)
    shape = tuple(poseA.shape)
    if len(shape) != 3 or shape[1:] != (4, 4):
        raise _lib.PedpError(f"pose_update: poseA must be N x 4 x 4, got {shape}")
    n = shape[0]
    width = 6 if prm.rot_rep == _lib.ROT_6D else 3
    dev = device_of(trans, rot, poseA)

    def take(x, k, what):
        a = as_array(x, dev)
        if int(np.prod(tuple(a.shape))) != n * k or (k < 16 and tuple(a.shape) not in ((n, k), (n * k,))):
            raise _lib.PedpError(f"pose_update: {what} must be {n} x {k}, got {tuple(a.shape)}")
        return a

    pa, t, r = take(poseA, 16, "poseA"), take(trans, 3, "trans"), take(rot, width, "rot")
    if out is None:
        out = empty(dev, (n, 4, 4))
    else:
        check_out("pose_update", out, (n, 4, 4), np.float32, dev, f"C-contiguous {n} x 4 x 4 float32 array")
    td, rd = (empty(dev, (n, 3)), empty(dev, (n, 3, 3))) if want_deltas else (None, None)
    launch(dev, "pedp_pose_update", lambda lib, h, mem: lib.pedp_pose_update(
        h, C.byref(prm), n, ptr(t), ptr(r), ptr(pa), mem, ptr(out), ptr(td), ptr(rd)))
    return out, td, rd


def max_pair_distance(pts):
    """The largest distance between two of the n x 3 points (numpy, CPU or CUDA tensor; float64), equal bit for bit to
    numpy's `np.linalg.norm(p[None] - p[:, None], axis=-1).max()`; NaN if a coordinate is not finite, 0.0 for one
    point.  Returns a Python float (the call waits for it)."""
    dev = device_of(pts)
    p = as_array(pts, dev, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise _lib.PedpError(f"max_pair_distance: expected n x 3 points, got {tuple(p.shape)}")
    res = C.c_double()
    launch(dev, "pedp_max_pair_distance", lambda lib, h, mem: lib.pedp_max_pair_distance(
        h, ptr(p), int(p.shape[0]), mem, C.byref(res)))
    return res.value
