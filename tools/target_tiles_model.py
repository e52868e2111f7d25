"""CPU model of what an ICP pass lists on the target side, per order of the target pack's rows (numpy + scipy, no GPU):

    python tools/target_tiles_model.py [bench_100k|parity|tiny|bench_1m]

A tile (16 rows) is listed for a scene node when |c_node - c_tile| <= rho + rad_node + rad_tile; a 1024-row word
likewise.  The model: the configuration's mesh vertices as the target; box-centre spheres as tile_sphere_kernel makes
them; scene proxy = the camera-facing vertices, doubled, with sigma = 0.6 mm jitter, in the model frame (a steady pass:
the pose has converged); scene nodes = 16 consecutive points of the scene's Hilbert order; rho = the node's largest
true nearest-neighbour distance.  It prints the tile radii and the tiles and words listed per node for the Hilbert
runs and for the balanced k-d split of csrc/icp/target_order.h, whose rule `compact_order` restates, and for the split
with Ritter's spheres in place of box-centre ones."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def hilbert_order(pts, bits=16):
    """Stable order of the rows by the Skilling Hilbert index of their cell in a (2^bits)^3 grid over their own box."""
    p = np.asarray(pts, np.float64)
    lo, hi = p.min(0), p.max(0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    X = np.minimum(((p - lo) / ext * (1 << bits) * (1.0 - 1e-9)).astype(np.int64), (1 << bits) - 1).T.copy()
    M = 1 << (bits - 1)
    Q = M
    while Q > 1:
        P = Q - 1
        for i in range(3):
            on = (X[i] & Q) != 0
            X[0] = np.where(on, X[0] ^ P, X[0])
            t = np.where(on, 0, (X[0] ^ X[i]) & P)
            X[0] ^= t
            X[i] ^= t
        Q >>= 1
    X[1] ^= X[0]
    X[2] ^= X[1]
    t = np.zeros_like(X[0])
    Q = M
    while Q > 1:
        t = np.where((X[2] & Q) != 0, t ^ (Q - 1), t)
        Q >>= 1
    X ^= t
    h = np.zeros(len(p), np.uint64)
    for b in range(bits - 1, -1, -1):
        for i in range(3):
            h = (h << np.uint64(1)) | ((X[i] >> b) & 1).astype(np.uint64)
    return np.argsort(h, kind="stable")


def left_rows(m):
    """Rows the left part of a segment of m > 16 rows takes."""
    u = 1024 if m > 1024 else 64 if m > 64 else 16
    return u * -(-m // (2 * u))


def compact_order(xyz, log=None):
    """Balanced k-d split of rows given in Hilbert order (centred float32 coordinates): their positions in the new order.
    While a segment has more than 16 rows: axis = widest float32 extent (ties: lowest axis); stable sort by that
    coordinate (ties: the position so far); the left part takes left_rows(m) rows.  log, if a list, receives
    (start, rows, axis, left rows) of every split."""
    xyz = np.asarray(xyz, np.float32)
    order = np.arange(len(xyz))
    todo = [(0, len(xyz))]
    while todo:
        s, m = todo.pop()
        if m <= 16:
            continue
        seg = order[s:s + m]
        p = xyz[seg]
        ext = p.max(0) - p.min(0)
        axis = 0
        if ext[1] > ext[axis]:
            axis = 1
        if ext[2] > ext[axis]:
            axis = 2
        order[s:s + m] = seg[np.argsort(p[:, axis], kind="stable")]
        h = left_rows(m)
        if log is not None:
            log.append((s, m, axis, h))
        todo += [(s, h), (s + h, m - h)]
    return order


def ritter_sphere(p):
    """Ritter's two passes: the farthest pair found from the first row, then the sphere grown over every row outside it."""
    a = p[((p - p[0]) ** 2).sum(1).argmax()]
    b = p[((p - a) ** 2).sum(1).argmax()]
    m, r = 0.5 * (a + b), 0.5 * np.linalg.norm(b - a)
    for q in p:
        d = np.linalg.norm(q - m)
        if d > r:
            r_new = 0.5 * (r + d)
            m = m + (q - m) * ((d - r_new) / d)
            r = r_new
    return m, max(r, np.sqrt(((p - m) ** 2).sum(1).max()))


def unit_spheres(rows, unit, ritter=False):
    """Bounding spheres (centre, radius) of every `unit` consecutive rows: box centre + farthest row, as
    tile_sphere_kernel makes them, or Ritter's."""
    n = len(rows)
    c, r = [], []
    for k in range(0, n, unit):
        p = rows[k:k + unit]
        if ritter:
            m, rad = ritter_sphere(p)
        else:
            m = 0.5 * (p.min(0) + p.max(0))
            rad = np.sqrt(((p - m) ** 2).sum(1).max())
        c.append(m)
        r.append(rad)
    return np.array(c), np.array(r)


def listed_per_node(node_c, node_reach, sph_c, sph_r):
    """Spheres listed per node: |c_node - c| <= reach_node + r."""
    from scipy.spatial import cKDTree

    tree = cKDTree(sph_c)
    near = tree.query_ball_point(node_c, node_reach + sph_r.max())
    out = np.empty(len(node_c), np.int64)
    for i, cand in enumerate(near):
        cand = np.asarray(cand, np.int64)
        d = np.linalg.norm(sph_c[cand] - node_c[i], axis=1)
        out[i] = int((d <= node_reach[i] + sph_r[cand]).sum())
    return out


def model(config="bench_100k", sigma=0.6, seed=0):
    from scipy.spatial import cKDTree
    from pedp_hip import synth

    f = synth.Frame(config)
    tgt = f.model_points
    centred = (tgt - tgt.mean(0)).astype(np.float32)
    hil = hilbert_order(tgt)
    orders = {"Hilbert runs": hil, "balanced k-d split": hil[compact_order(centred[hil])]}
    # scene proxy in the model frame: the vertices that face the camera of the ground-truth pose
    R, t = f.T_gt[:3, :3], f.T_gt[:3, 3]
    facing = np.einsum("ij,ij->i", f.normals @ R.T, tgt @ R.T + t) < 0.0
    rng = np.random.default_rng(seed)
    scene = np.repeat(tgt[facing], 2, axis=0)
    scene = scene + rng.normal(0.0, sigma, scene.shape)
    scene = scene[hilbert_order(scene)]
    rho = cKDTree(tgt).query(scene)[0]
    node_c, node_r = unit_spheres(scene, 16)
    node_rho = np.array([rho[k:k + 16].max() for k in range(0, len(scene), 16)])
    rows = []
    for name, order, ritter in [(k, v, False) for k, v in orders.items()] + [("k-d split, Ritter spheres", orders["balanced k-d split"], True)]:
        p = centred[order].astype(np.float64) + tgt.mean(0)
        c16, r16 = unit_spheres(p, 16, ritter)
        cw, rw = unit_spheres(p, 1024, ritter)
        tiles = listed_per_node(node_c, node_rho + node_r, c16, r16)
        words = listed_per_node(node_c, node_rho + node_r, cw, rw)
        rows.append((name, np.median(r16), np.percentile(r16, 90), tiles.mean(), np.median(tiles), words.mean()))
    return rows


if __name__ == "__main__":
    config = sys.argv[1] if len(sys.argv) > 1 else "bench_100k"
    print(f"{config}: order of target rows | tile radius median / p90 (mm) | tiles listed per node (mean / median) | 1,024-row words per node")
    res = model(config)
    for name, r50, r90, tm, t50, wm in res:
        print(f"  {name:26s} | {r50:.2f} / {r90:.2f} | {tm:.1f} / {t50:.0f} | {wm:.1f}")
    print(f"  tiles listed, split / Hilbert: {res[1][3] / res[0][3]:.2f}; Ritter spheres / box-centre spheres on the split: {res[2][3] / res[1][3]:.2f}")
