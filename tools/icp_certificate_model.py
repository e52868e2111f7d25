"""CPU model of the fused ICP pass's nearest-neighbour certificates (numpy + scipy + the oracle, no GPU):

    python tools/icp_certificate_model.py [bench_100k|parity|tiny]

Runs the oracle's 21-pass registration of the configuration's frame, takes the pose every pass started from out of its
trace, and applies the certificate rule of csrc/icp/fused_pass.h to the TRUE first and second neighbour distances (the
kernel's bound on the second neighbour is looser by the fp32 filter's slack): a slot that searches in pass p within
rho = min(r, KAPPA d_prev) keeps c = min(rho, d_second); the next pass moves the point by m and certifies the slot when
d(p', t_prev) < c - m, carrying c - m on.  Rebuild passes (the motion bound of csrc/icp/fused_close.h) certify nothing.
It prints, per pass, the largest and the median motion of a candidate point and, for each KAPPA, the share of certified
slots and of fully certified 16-slot runs (candidates of each 64-point half of the scene's Hilbert order, in order)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KAPPAS = (1.25, 1.5, 2.0)


def rebuild_passes(trace, r, lo, hi):
    """Passes that run as rebuild passes: pass 0, and the pass behind every close whose motion bound reaches 0.95 margin."""
    margin, c = 2.0 * r, 0.5 * (lo + hi)
    reach = r + margin + np.sqrt((0.25 * (hi - lo) ** 2).sum())
    th = ta = 0.0
    out = {0}
    for p in range(len(trace) - 1):
        U = trace[p + 1, 2:].reshape(4, 4) @ np.linalg.inv(trace[p, 2:].reshape(4, 4))
        D = U[:3, :3] - np.eye(3)
        th += np.sqrt((D * D).sum())
        ta += np.linalg.norm(U[:3, 3] + D @ c)
        if not th * reach + ta < 0.95 * margin:
            out.add(p + 1)
            th = ta = 0.0
    return out


def model(config="bench_100k"):
    from scipy.spatial import cKDTree
    import pedp_oracle as oracle
    from pedp_hip import synth
    from target_tiles_model import hilbert_order

    f = synth.Frame(config)
    scene = f.scene(oracle.raycast(f.verts_posed, f.tris, f.rays6)["t_hit"])
    r = f.max_correspondence_distance
    ro = oracle.icp(scene, f.model_points, f.normals, r, f.icp_init(), max_iter=20, rel_fitness=-1, rel_rmse=-1)
    trace = ro["trace"]
    rebuilds = rebuild_passes(trace, r, f.model_points.min(0), f.model_points.max(0))
    tree = cKDTree(f.model_points)
    pos = np.empty(len(scene), np.int64)  # position of a point in the scene's spatial order
    pos[hilbert_order(scene)] = np.arange(len(scene))
    print(f"{config}: {len(scene)} scene points, {len(f.model_points)} target points, r = {r}, rebuild passes {sorted(rebuilds)}")
    print("pass  cand   motion max / median (mm)   " + "   ".join(f"kappa {k}: slots runs" for k in KAPPAS))
    state = {k: dict(c=np.zeros(len(scene))) for k in KAPPAS}
    prev_pts = prev_nn = None
    above = {k: 0 for k in KAPPAS}
    for p in range(len(trace)):
        T = trace[p, 2:].reshape(4, 4)
        pts = scene @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(pts, k=2, distance_upper_bound=4.0 * r)
        cand = d[:, 0] < r
        m = np.zeros(len(scene)) if prev_pts is None else np.sqrt(((pts - prev_pts) ** 2).sum(1))
        dprev = np.full(len(scene), np.inf)
        if prev_nn is not None:
            had = prev_nn >= 0
            dprev[had] = np.sqrt(((pts[had] - f.model_points[prev_nn[had]]) ** 2).sum(1))
        line = f"{p:4d} {cand.sum():6d}   {m[cand].max() if cand.any() else 0:10.3e} / {np.median(m[cand]) if cand.any() else 0:9.3e}   "
        for k in KAPPAS:
            s = state[k]
            c_new = s["c"] - m
            ok = cand & (dprev < c_new) & (p not in rebuilds)
            rho = np.minimum(r, k * dprev)
            s["c"] = np.where(ok, c_new, np.where(cand, np.minimum(rho, d[:, 1]), 0.0))
            # 16-slot runs: the candidates of a half, in order, sixteen at a time
            idx = np.nonzero(cand)[0]
            idx = idx[np.argsort(pos[idx])]
            h = pos[idx] // 64
            start = np.r_[0, np.nonzero(np.diff(h))[0] + 1]
            rank = np.arange(len(idx)) - np.repeat(start, np.diff(np.r_[start, len(idx)]))
            run = h * 4 + rank // 16
            _, inv = np.unique(run, return_inverse=True)
            full = np.bincount(inv, weights=~ok[idx]) == 0
            share = ok[cand].mean() if cand.any() else 0.0
            above[k] += share > 0.9
            line += f"   {share:14.3f} {full.mean() if len(full) else 0:5.3f}"
        print(line)
        prev_pts, prev_nn = pts, np.where(cand, j[:, 0], -1)
    for k in KAPPAS:
        print(f"kappa {k}: {above[k]} of {len(trace)} passes above 90 % certified slots")


if __name__ == "__main__":
    model(sys.argv[1] if len(sys.argv) > 1 else "bench_100k")
