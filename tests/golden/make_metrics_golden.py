"""Writes tests/golden/g11_metrics.npz from the reference's own add_err, adds_err and compute_auc_sklearn.

    python tests/golden/make_metrics_golden.py /path/to/reference

Runs only where the reference tree exists; no test calls it.  transform_pts, add_err, adds_err and compute_auc_sklearn
are taken out of Utils.py with `ast` (make_reference_golden.py's `take`), so the file's imports never execute, and run on
the CPU against the installed numpy, scipy (cKDTree) and sklearn (metrics.auc).  The fixture holds names and numbers
only: every input the functions were given and every output they gave.

Layout:
    pts/<N>_<scale>          N x 3 float64 model points (float32 values: the estimator's points are float32), scale m
                             (coordinates ~0.05) or mm (the same cloud x 1000)
    cases                    names <N>_<scale>_<offset>
    <case>/gt                4 x 4 float64 (distance ~0.6 m); for the offset 'same' it is the prediction itself
    <case>/pred              4 x 4 float32: gt turned by the offset's angle about a random axis and shifted, rounded
                             through float32 as the estimator's poses are
    <case>/add, <case>/adds  what the reference returned for (pred widened to float64, gt, pts)
    auc/cases                names; auc/<case>/errs, max_val, step and the reference's out
"""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_golden import rotations, take  # noqa: E402

SIZES = (1, 2, 63, 257, 1025, 3001)
# name -> (angle in radians, shift in metres)
OFFSETS = {"same": (0.0, 0.0), "1e-9": (1e-9, 0.0), "1e-3": (1e-3, 1e-4), "0.3": (0.3, 0.01), "3.1": (3.1, 0.05)}


def axis_angle(axis, angle):
    x, y, z = axis / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def main(ref_root):
    add_err, adds_err, auc = take(ref_root, "Utils.py", ["transform_pts", "add_err", "adds_err", "compute_auc_sklearn"],
                                  {"np": np, "cKDTree": cKDTree})[1:]
    rng = np.random.default_rng(1101)
    out, names = {}, []
    for n in SIZES:
        cloud = rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
        for scale, k in (("m", 1.0), ("mm", 1000.0)):
            pts = (cloud * np.float32(k)).astype(np.float64)
            out[f"pts/{n}_{scale}"] = pts
            for off, (angle, shift) in OFFSETS.items():
                gt = np.eye(4)
                gt[:3, :3] = rotations(rng, 1)[0]
                gt[:3, 3] = rng.uniform(-0.2, 0.2, 3) * k + np.array([0, 0, 0.6 * k])
                pred = gt.copy()
                pred[:3, :3] = axis_angle(rng.standard_normal(3), angle) @ gt[:3, :3]
                d = rng.standard_normal(3)
                pred[:3, 3] += shift * k * d / np.linalg.norm(d)
                pred = pred.astype(np.float32)
                if off == "same":
                    gt = pred.astype(np.float64)
                name = f"{n}_{scale}_{off}"
                names.append(name)
                out[f"{name}/gt"], out[f"{name}/pred"] = gt, pred
                out[f"{name}/add"] = np.float64(add_err(pred.astype(np.float64), gt.copy(), pts.copy()))
                out[f"{name}/adds"] = np.float64(adds_err(pred.astype(np.float64), gt.copy(), pts.copy()))
                print(f"{name}: add {float(out[f'{name}/add'])!r} adds {float(out[f'{name}/adds'])!r}")
    out["cases"] = np.array(names)
    aucs = {
        "no_hits": (rng.uniform(0.11, 0.5, 40), 0.1, 0.001),            # nothing at or below max_val: the curve stays 0
        "all_below_step": (rng.uniform(0, 0.0009, 25), 0.1, 0.001),     # 1 from the second threshold on: the early break
        "straddle": (rng.uniform(0.0, 0.2, 200), 0.1, 0.001),           # half of them beyond max_val
        "one": (np.array([0.0123]), 0.1, 0.001),
        "one_beyond": (np.array([0.25]), 0.1, 0.001),
        "ties_on_thresholds": (np.arange(0, 0.1, 0.004), 0.1, 0.001),   # errors equal to thresholds as arange forms them
        "other_grid": (rng.uniform(0.0, 0.06, 100), 0.05, 0.0005),
        "millimetres": (rng.uniform(0.0, 30.0, 100), 20.0, 0.1),
    }
    out["auc/cases"] = np.array(list(aucs))
    for name, (errs, max_val, step) in aucs.items():
        out[f"auc/{name}/errs"], out[f"auc/{name}/max_val"], out[f"auc/{name}/step"] = errs, np.float64(max_val), np.float64(step)
        out[f"auc/{name}/out"] = np.float64(auc(errs.copy(), max_val=max_val, step=step))
        print(f"auc/{name}: {len(errs)} errors, {float(out[f'auc/{name}/out'])!r}")
    path = os.path.join(HERE, "g11_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
