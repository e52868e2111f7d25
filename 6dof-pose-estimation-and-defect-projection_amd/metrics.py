"""Pose errors against a ground truth: FoundationPose's evaluation metrics (Utils.py:232-266, :806-834).

    add_err, adds_err               the reference's single-pose functions (np.float64)
    add_err_batch, adds_err_batch   B poses in one library call (pedp_pose_errors, csrc/pedp_metrics.hip)
    compute_auc_sklearn             the area under the accuracy-threshold curve, host numpy (no sklearn at run time)
    symmetry_tfs_from_info          a BOP models_info entry -> the symmetry_tfs FoundationPose and the batch functions take

CUDA tensors stay on their device: the batch functions enqueue on the caller's current stream and return a CUDA tensor
without a host wait (host arrays given alongside go up through page-locked memory on that stream).  numpy arrays and CPU
tensors use host memory and get their own kind back.  The contract (float64 with no contraction, the transform's and the
mean's order, ADD-S as the nearest pred point of every gt point, symmetries as a minimum over pred . sym, NaN for
non-finite inputs) is DESIGN.md s4.15.
"""
import numpy as np

from . import _lib
from ._bridge import as_array, as_kind, check_out, device_of, empty, is_torch, launch, ptr

MAX_POSES = 65535          # pedp_pose_errors' bounds
MAX_POINTS = 1 << 22


def _errors(kind, name, preds, gts, model_pts, symmetry_tfs, out):
    shape, gshape, pshape = tuple(preds.shape), tuple(gts.shape), tuple(model_pts.shape)
    if len(shape) != 3 or shape[1:] != (4, 4):
        raise _lib.PedpError(f"{name}: preds must be B x 4 x 4, got {shape}")
    B = shape[0]
    if gshape != (4, 4) and (len(gshape) != 3 or gshape[1:] != (4, 4) or gshape[0] not in (1, B)):
        raise _lib.PedpError(f"{name}: gts must be 4 x 4 or {B} x 4 x 4, got {gshape}")
    G = 1 if len(gshape) == 2 else gshape[0]
    if len(pshape) != 2 or pshape[1] != 3 or pshape[0] < 1:
        raise _lib.PedpError(f"{name}: model_pts must be N x 3 with N >= 1, got {pshape}")
    N = pshape[0]
    if B > MAX_POSES or N > MAX_POINTS:
        raise _lib.PedpError(f"{name}: at most {MAX_POSES} poses and {MAX_POINTS} points, got {B} and {N}")
    S = 0
    if symmetry_tfs is not None:
        sshape = tuple(symmetry_tfs.shape)
        if sshape != (4, 4) and (len(sshape) != 3 or sshape[1:] != (4, 4) or sshape[0] < 1):
            raise _lib.PedpError(f"{name}: symmetry_tfs must be S x 4 x 4 with S >= 1, got {sshape}")
        S = 1 if len(sshape) == 2 else sshape[0]
        if S > MAX_POSES:
            raise _lib.PedpError(f"{name}: at most {MAX_POSES} symmetries, got {S}")
    dev = device_of(preds, gts, model_pts, symmetry_tfs)
    if out is not None:
        check_out(name, out, (B,), np.float64, dev, f"C-contiguous float64 array of {B} values")
    else:
        out = empty(dev, B, np.float64)
    if B:
        p, g, m = (as_array(x, dev, np.float64) for x in (preds, gts, model_pts))
        s = as_array(symmetry_tfs, dev, np.float64) if S else None
        launch(dev, "pedp_pose_errors", lambda lib, h, mem: lib.pedp_pose_errors(
            h, ptr(m), N, ptr(p), B, ptr(g), G, ptr(s), S, kind, mem, ptr(out)))
    return as_kind(out, preds)


def add_err_batch(preds, gts, model_pts, symmetry_tfs=None, out=None):
    """ADD of B poses: the mean distance between the model points under preds[b] and under the ground truth.  preds
    B x 4 x 4; gts 4 x 4 (one for all) or B x 4 x 4; model_pts N x 3; float32 or float64, numpy, CPU or CUDA tensors.
    With symmetry_tfs (S x 4 x 4) the error of a pose is the minimum over s of the error of preds[b] @ symmetry_tfs[s].
    Returns B float64 values where the inputs are (a CUDA tensor on their device, enqueued on the current stream with
    no host wait; else numpy, or a CPU tensor if preds is one); `out` receives them if given (a C-contiguous float64
    array of B values on that side)."""
    return _errors(_lib.ERR_ADD, "add_err_batch", preds, gts, model_pts, symmetry_tfs, out)


def adds_err_batch(preds, gts, model_pts, symmetry_tfs=None, out=None):
    """ADD-S of B poses: the mean, over the model points under the ground truth, of the distance to the nearest model
    point under preds[b] (the direction of the reference's tree).  Arguments and result as add_err_batch."""
    return _errors(_lib.ERR_ADDS, "adds_err_batch", preds, gts, model_pts, symmetry_tfs, out)


def _one(fn, name, pred, gt, model_pts):
    if tuple(pred.shape) != (4, 4) or tuple(gt.shape) != (4, 4):
        raise _lib.PedpError(f"{name}: pred and gt must be 4 x 4, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    e = fn(pred.reshape(1, 4, 4), gt, model_pts)
    return np.float64(e.cpu().numpy()[0] if is_torch(e) else e[0])


def add_err(pred, gt, model_pts, symetry_tfs=None):
    """Average Distance of Model Points (Hinterstoisser et al., ACCV 2012) of one pose, an np.float64 (the call waits
    for it).  `symetry_tfs` is accepted and ignored, as the reference ignores it (and spelt as the reference spells it):
    for an error that is minimised over symmetries use add_err_batch."""
    return _one(add_err_batch, "add_err", pred, gt, model_pts)


def adds_err(pred, gt, model_pts):
    """ADD-S of one pose (pred and gt 4 x 4, model_pts N x 3), an np.float64 (the call waits for it)."""
    return _one(adds_err_batch, "adds_err", pred, gt, model_pts)


def compute_auc_sklearn(errs, max_val=0.1, step=0.001):
    """The area under the curve of "share of errs <= x" over x in np.arange(0, max_val + step, step), divided by
    max_val.  The curve is filled threshold by threshold until it first reaches 1 and stays at 1 from there (the
    reference's early break); the area is numpy's trapezoid rule, which is what sklearn.metrics.auc computes."""
    errs = np.sort(np.array(errs))
    X = np.arange(0, max_val + step, step)
    Y = np.ones(len(X))
    for i, x in enumerate(X):
        y = (errs <= x).sum() / len(errs)
        Y[i] = y
        if y >= 1:
            break
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    return trapezoid(Y, X) / (max_val * 1)


def symmetry_tfs_from_info(info, rot_angle_discrete=5):
    """The symmetry transforms (S x 4 x 4 float64, the identity first) of a BOP `models_info` entry: its
    'symmetries_discrete' matrices in order with their translations taken from millimetres to metres, then, for
    'symmetries_continuous', the rotations about the entry's first axis (x, y or z, whichever component is positive
    first) in steps of rot_angle_discrete degrees from 0 up to 360, each carrying the entry's offset as it is."""
    from .estimator import euler_matrix

    tfs = [np.eye(4)]
    if "symmetries_discrete" in info:
        discrete = np.array(info["symmetries_discrete"]).reshape(-1, 4, 4)
        discrete[..., :3, 3] *= 0.001
        tfs += list(discrete)
    if "symmetries_continuous" in info:
        first = info["symmetries_continuous"][0]
        axis = np.array(first["axis"]).reshape(3)
        turning = next((k for k in range(3) if axis[k] > 0), None)
        angles = [[0], [0], [0]]
        if turning is not None:
            angles[turning] = np.arange(0, 360, rot_angle_discrete) / 180.0 * np.pi
        for rx in angles[0]:
            for ry in angles[1]:
                for rz in angles[2]:
                    tf = euler_matrix(rx, ry, rz)
                    tf[:3, 3] = first["offset"]
                    tfs.append(tf)
    return np.array(tfs)
