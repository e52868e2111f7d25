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
from .crop import _device_of, _launch, _ptr, _to_device
from .depth_filters import _is_torch

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
    dev = _device_of(trans, rot, poseA)

    def take(x, k, what):
        if dev is not None:
            a = _to_device(x, dev).contiguous()
        else:
            a = np.ascontiguousarray(x.detach().cpu().numpy() if _is_torch(x) else x, dtype=np.float32)
        if int(np.prod(tuple(a.shape))) != n * k or (k < 16 and tuple(a.shape) not in ((n, k), (n * k,))):
            raise _lib.PedpError(f"pose_update: {what} must be {n} x {k}, got {tuple(a.shape)}")
        return a

    def new(*s):
        if dev is None:
            return np.empty(s, np.float32)
        import torch

        return torch.empty(s, dtype=torch.float32, device=dev)

    pa, t, r = take(poseA, 16, "poseA"), take(trans, 3, "trans"), take(rot, width, "rot")
    if out is None:
        out = new(n, 4, 4)
    else:
        _check_out(out, n, dev)
    td, rd = (new(n, 3), new(n, 3, 3)) if want_deltas else (None, None)
    _launch(dev, "pedp_pose_update", lambda lib, h, mem: lib.pedp_pose_update(
        h, C.byref(prm), n, _ptr(t), _ptr(r), _ptr(pa), mem, _ptr(out), _ptr(td), _ptr(rd)))
    return out, td, rd


def _check_out(out, n, dev):
    """The kernel writes 16 n float32 values through out's pointer, on the inputs' side: anything else is refused."""
    where = f"on {dev}" if dev is not None else "in host memory"
    if _is_torch(out):
        import torch

        ok = (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, 4, 4)
              and (out.device == dev if dev is not None else not out.is_cuda))
        kind = f"{out.dtype} tensor of shape {tuple(out.shape)} on {out.device}{'' if out.is_contiguous() else ', strided'}"
    else:
        a = out if isinstance(out, np.ndarray) else None
        ok = (dev is None and a is not None and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable
              and a.shape == (n, 4, 4))
        kind = (f"{type(out).__name__}" if a is None else
                f"{a.dtype} array of shape {a.shape}{'' if a.flags.c_contiguous else ', strided'}")
    if not ok:
        raise _lib.PedpError(f"pose_update: out must be a C-contiguous {n} x 4 x 4 float32 array {where}, got a {kind}")


def max_pair_distance(pts):
    """The largest distance between two of the n x 3 points (numpy, CPU or CUDA tensor; float64), equal bit for bit to
    numpy's `np.linalg.norm(p[None] - p[:, None], axis=-1).max()`; NaN if a coordinate is not finite, 0.0 for one
    point.  Returns a Python float (the call waits for it)."""
    dev = _device_of(pts)
    if dev is not None:
        import torch

        p = pts.to(torch.float64).contiguous()
    else:
        p = np.ascontiguousarray(pts.detach().cpu().numpy() if _is_torch(pts) else pts, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise _lib.PedpError(f"max_pair_distance: expected n x 3 points, got {tuple(p.shape)}")
    res = C.c_double()
    _launch(dev, "pedp_max_pair_distance", lambda lib, h, mem: lib.pedp_max_pair_distance(
        h, _ptr(p), int(p.shape[0]), mem, C.byref(res)))
    return res.value
