"""Times of the pose-error metrics on cuda:0 -> profiles/metrics_time.json (or the path given).

    python tools/metrics_time.py [OUT.json]

Both kinds (ADD, ADD-S) at B in {1, 252} poses x N in {2048, 8192} model points.  Two paths start from the same state, the
poses as float32 CUDA tensors (what the estimator holds) and the points on both sides, and end with B float64 values on the
host; they alternate inside one loop:

    device      add_err_batch / adds_err_batch on the CUDA tensors, then the result's download (which waits for it)
    reference   the shape of the reference's evaluation loop: the poses' download, then per pose numpy's transform of the
                points and either the mean norm (ADD) or scipy's cKDTree over the pred points queried with the gt points
                (ADD-S); the reference asks for workers=-1, which here is the 16 CPUs a job may use (WORKERS)

Host wall clock; every shape runs twice unmeasured first.  Nothing falls back: without a GPU the first call raises."""
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pedp_hip.compat import add_err_batch, adds_err_batch  # noqa: E402

WORKERS = min(16, len(os.sched_getaffinity(0)))
SHAPES = [(B, N) for B in (1, 252) for N in (2048, 8192)]
BUDGET_S = 4.0      # measured time per path and shape, at least MIN_REPS calls
MIN_REPS, MAX_REPS = 5, 200


def inputs(B, N, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.05, 0.05, (N, 3)).astype(np.float32)
    q = rng.standard_normal((B + 1, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(B + 1, 3, 3)
    poses = np.tile(np.eye(4, dtype=np.float32), (B + 1, 1, 1))
    poses[:, :3, :3] = R
    poses[:, :3, 3] = rng.uniform(-0.1, 0.1, (B + 1, 3)) + [0, 0, 0.6]
    return pts, poses[1:], poses[0].astype(np.float64)


def reference_path(kind, preds_cuda, gt, pts):
    preds = preds_cuda.cpu().numpy().astype(np.float64)
    gt_pts = pts @ gt[:3, :3].T + gt[:3, 3]
    out = np.empty(len(preds))
    for b, P in enumerate(preds):
        pred_pts = pts @ P[:3, :3].T + P[:3, 3]
        if kind == "add":
            out[b] = np.linalg.norm(pred_pts - gt_pts, axis=-1).mean()
        else:
            out[b] = cKDTree(pred_pts).query(gt_pts, k=1, workers=WORKERS)[0].mean()
    return out


def device_path(fn, preds_cuda, gt_cuda, pts_cuda):
    return fn(preds_cuda, gt_cuda, pts_cuda).cpu().numpy()


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median": float(np.median(ms)), "min": float(ms[0]), "max": float(ms[-1])}


def main(out_path):
    assert torch.cuda.is_available(), "metrics_time.py measures on a GPU"
    rows = []
    for kind, fn in (("add", add_err_batch), ("adds", adds_err_batch)):
        for B, N in SHAPES:
            pts, preds, gt = inputs(B, N, 7 * B + N)
            pts64 = pts.astype(np.float64)
            dp, dg, dm = torch.as_tensor(preds, device="cuda"), torch.as_tensor(gt, device="cuda"), torch.as_tensor(pts, device="cuda")
            for _ in range(2):
                got, want = device_path(fn, dp, dg, dm), reference_path(kind, dp, gt, pts64)
            worst = float(np.abs(got - want).max())
            assert worst < 1e-12, f"{kind} B={B} N={N}: the two paths differ by {worst}"
            dev_ms, ref_ms = [], []
            while len(dev_ms) < MIN_REPS or (sum(ref_ms) < BUDGET_S * 1e3 and len(dev_ms) < MAX_REPS):
                t0 = time.perf_counter()
                device_path(fn, dp, dg, dm)
                t1 = time.perf_counter()
                reference_path(kind, dp, gt, pts64)
                t2 = time.perf_counter()
                dev_ms.append((t1 - t0) * 1e3)
                ref_ms.append((t2 - t1) * 1e3)
            row = {"kind": kind, "B": B, "N": N, "reps": len(dev_ms), "device_ms": stats(dev_ms), "reference_ms": stats(ref_ms),
                   "max_abs_difference": worst}
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "cpu_workers": WORKERS,
              "what": "host wall clock per call in ms, the two paths alternating in one loop; both start from float32 CUDA "
                      "poses and end with float64 values on the host", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "metrics_time.json"))
