"""Independent numpy / scipy statements of the point-cloud operations (test_cloudops_matrix_cpu.py holds the oracle
against them on every geometry of _cloud_cases; test_oracle_cpu.py on its fixtures).  Nothing here shares code with
oracle/cloudops.c or the library: a KD-tree where those sweep, numpy's eigen solver where those use a closed form,
running sums where those add in blocks."""
import numpy as np
from scipy.spatial import cKDTree


def d2(a, b):
    """Squared distance in the operations' order of additions, (dx^2 + dy^2) + dz^2: the strict tests are exact."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def voxel_means(pts, v):
    """Group by floor((p - (min - v / 2)) / v), lexicographic order of the voxel index, mean per group."""
    idx = np.floor((pts - (pts.min(axis=0) - v * 0.5)) / v).astype(np.int64)
    _, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.ravel()
    return np.stack([np.bincount(inv, pts[:, k]) for k in range(3)], 1) / np.bincount(inv)[:, None]


def knn_mean(pts, k):
    """Mean distance to the k nearest (the point itself is one of them); fewer points than k: all of them."""
    k = min(k, len(pts))
    d, _ = cKDTree(pts).query(pts, k=k)
    return d.reshape(len(pts), k).mean(axis=1)


def neighbours(pts, r):
    """Per point the ascending indices j with d^2 < r^2 strictly (itself included): a ball query slightly larger than
    r, filtered by the exact float64 distance."""
    lists = cKDTree(pts).query_ball_point(pts, r * (1.0 + 1e-9) + 1e-300)
    out = []
    for i, js in enumerate(lists):
        js = np.array(sorted(js), np.int64)
        out.append(js[d2(pts[js], pts[i]) < r * r])
    return out


def dbscan(pts, eps, min_points):
    """(labels, core): neighbours d^2 < eps^2, core points have >= min_points of them (themselves included), clusters
    grow breadth-first from the lowest unvisited core index and are numbered in that order; a border point keeps the
    first cluster that reaches it -- the smallest id among its core neighbours; noise is -1."""
    nb = neighbours(pts, eps)
    n = len(pts)
    core = np.array([len(x) >= min_points for x in nb], bool)
    labels = np.full(n, -1, np.int32)
    cid = 0
    for s in range(n):
        if not core[s] or labels[s] >= 0:
            continue
        labels[s] = cid
        queue = [s]
        while queue:
            q = queue.pop(0)
            if not core[q]:
                continue
            for j in nb[q]:
                if labels[j] < 0:
                    labels[j] = cid
                    queue.append(int(j))
        cid += 1
    return labels, core, nb


def check_dbscan(labels, pts, eps, min_points):
    """The properties of pedp.h's cluster_dbscan paragraph, of `labels` against the restatement."""
    ref, core, nb = dbscan(pts, eps, min_points)
    assert np.array_equal(labels == -1, ref == -1)                                     # the noise set
    assert not np.any(labels[core] == -1)                                              # no core point is noise
    pairs = set(zip(labels[core].tolist(), ref[core].tolist()))
    assert len(pairs) == len(set(a for a, _ in pairs)) == len(set(b for _, b in pairs))  # one-to-one on the core points
    for i in np.flatnonzero(~core & (labels >= 0)):                                    # border points
        assert labels[i] == min(labels[j] for j in nb[i] if core[j]), i
    ids = np.unique(labels[labels >= 0])
    assert np.array_equal(ids, np.arange(len(ids)))
    first = [np.flatnonzero(core & (labels == c))[0] for c in ids]                    # numbered by the smallest core index
    assert first == sorted(first)
    return ref, core


def hybrid_sets(pts, radius, max_nn):
    """Per point the max_nn nearest with d^2 < radius^2, ascending (d^2, index)."""
    out = []
    for i, js in enumerate(neighbours(pts, radius)):
        dd = d2(pts[js], pts[i])
        out.append(js[np.lexsort((js, dd))][:max_nn])
    return out


def check_normals(est, pts, radius, max_nn, sets=None):
    """Where the neighbourhood's covariance has a separated smallest eigenvalue, (l1 - l0) > 1e-6 l2, the normal is
    numpy's eigenvector up to sign within 1e-6; elsewhere it is finite and (0, 0, 1) or of unit length within 1e-12.
    Returns the mask of the points the eigenvector rule decided."""
    sets = hybrid_sets(pts, radius, max_nn) if sets is None else sets
    decided = np.zeros(len(pts), bool)
    assert np.isfinite(est).all()
    for i, js in enumerate(sets):
        if len(js) >= 3:
            w, V = np.linalg.eigh(np.cov(pts[js].T, bias=True))
            if w[1] - w[0] > 1e-6 * w[2]:
                assert abs(abs(est[i] @ V[:, 0]) - 1.0) < 1e-6, (i, est[i], V[:, 0])
                decided[i] = True
                continue
        assert np.array_equal(est[i], [0.0, 0.0, 1.0]) or abs(np.linalg.norm(est[i]) - 1.0) < 1e-12, (i, est[i])
    return decided


def plane_from_points(pts, idx):
    """Open3D's GetPlaneFromPoints over pts[idx] with running sums (np.cumsum(...)[-1] per moment): centroid, the six
    second moments about it, the cross products of the largest-determinant axis."""
    q = pts[np.asarray(idx, np.int64)]
    if len(q) < 3:
        return np.zeros(4)
    c = np.array([np.cumsum(q[:, k])[-1] for k in range(3)]) / len(q)
    r = q - c
    xx, xy, xz, yy, yz, zz = (np.cumsum(r[:, a] * r[:, b])[-1] for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))
    det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
    if det_x >= det_y and det_x >= det_z:
        n = np.array([det_x, xz * yz - xy * zz, xy * yz - xz * yy])
    elif det_y >= det_z:
        n = np.array([xz * yz - xy * zz, det_y, xy * xz - yz * xx])
    else:
        n = np.array([xy * yz - xz * yy, xy * xz - yz * xx, det_z])
    norm = np.linalg.norm(n)
    if not norm > 0.0:
        return np.zeros(4)
    n = n / norm
    return np.array([n[0], n[1], n[2], -(n @ c)])


def feature_match(fs, ft):
    """argmin over the targets of the squared L2 distance, lowest index on ties; a distance that is NaN or +inf is
    never the nearest, a source row without a finite distance gets -1 (the registration's rule for non-finite rows)."""
    out = np.full(len(fs), -1, np.int32)
    for i, a in enumerate(fs):
        with np.errstate(invalid="ignore", over="ignore"):
            d = ((a[None, :] - ft) ** 2).sum(axis=1) if len(ft) else np.zeros(0)
        ok = np.isfinite(d)
        if ok.any():
            out[i] = int(np.flatnonzero(ok)[np.argmin(d[ok])])
    return out


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def fpfh_order_ties(pts, nrm, radius, max_nn, ulps=4):
    """For a report, not a check: Feature.cpp orders a pair by acos(|a1|) > acos(|a2|).  Counts the pairs whose two angles
    are within `ulps` of each other (two libms may order them differently) and returns a function of the mask of differing
    rows -> (pairs, such pairs, rows whose own or a neighbour's SPFH reads one, differing rows that read none)."""
    sets = hybrid_sets(pts, radius, max_nn)
    owner = np.zeros(len(pts), bool)
    pairs = ties = 0
    for i, js in enumerate(sets):
        for j in js[1:]:
            dp = pts[j] - pts[i]
            dist = np.sqrt(_dot(dp, dp))
            if dist == 0.0:
                continue
            pairs += 1
            with np.errstate(invalid="ignore"):
                c1, c2 = np.arccos(abs(_dot(nrm[i], dp) / dist)), np.arccos(abs(_dot(nrm[j], dp) / dist))
            if np.isfinite(c1) and np.isfinite(c2) and abs(c1 - c2) <= ulps * np.spacing(max(c1, c2)):
                ties += 1
                owner[i] = True
    reads = np.array([owner[js].any() for js in sets], bool)
    return lambda differing: (pairs, ties, int(reads.sum()), int((differing & ~reads).sum()))


def fpfh(pts, nrm, radius, max_nn):
    """Independent restatement of Open3D's ComputeFPFHFeature (vector form, numpy's acos / arctan2).  Dot products of
    three terms are written out: numpy's `@` goes through BLAS, whose accumulator starts at +0 (so a sum of negative
    zeros loses its sign) and may fuse multiply and add.  Both decide a feature where the exact value sits on a cut: on
    an exactly planar cloud with opposite normals the first angle is atan2(+-0, -1) = +-pi, bin 10 or bin 0, and on a
    lattice the two angles whose comparison orders the pair are equal in exact arithmetic."""
    n = len(pts)
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    lists = []
    for i in range(n):
        cand = np.flatnonzero(d2[i] < radius * radius)
        cand = cand[np.lexsort((cand, d2[i, cand]))][:max_nn]
        lists.append(cand)
    spfh = np.zeros((n, 33))
    for i, cand in enumerate(lists):
        if len(cand) <= 1:
            continue
        incr = 100.0 / (len(cand) - 1)
        for j in cand[1:]:
            dp = pts[j] - pts[i]
            dist = np.sqrt(_dot(dp, dp))
            f = np.zeros(3)
            if dist != 0.0:
                a, b = nrm[i], nrm[j]
                a1, a2 = _dot(a, dp) / dist, _dot(b, dp) / dist
                with np.errstate(invalid="ignore"):      # |a1| = 1 + an ulp: acos is NaN, the comparison false, as in C
                    swap = np.arccos(abs(a1)) > np.arccos(abs(a2))
                if swap:
                    a, b, dp, f[2] = nrm[j], nrm[i], -dp, -a2
                else:
                    f[2] = a1
                v = np.cross(dp, a)
                vn = np.sqrt(_dot(v, v))
                if vn == 0.0:
                    f[:] = 0.0
                else:
                    v = v / vn
                    w = np.cross(a, v)
                    f[1] = _dot(v, b)
                    f[0] = np.arctan2(_dot(w, b), _dot(a, b))
            for k, x in enumerate((11 * (f[0] + np.pi) / (2 * np.pi), 11 * (f[1] + 1) * 0.5, 11 * (f[2] + 1) * 0.5)):
                spfh[i, 11 * k + min(max(int(np.floor(x)), 0), 10)] += incr
    out = np.zeros((n, 33))
    for i, cand in enumerate(lists):
        if len(cand) <= 1:
            continue
        s = np.zeros(3)
        for j in cand[1:]:
            if d2[i, j] == 0.0:
                continue
            val = spfh[j] / d2[i, j]
            out[i] += val
            s += val.reshape(3, 11).sum(1)
        s = np.where(s != 0.0, 100.0 / np.where(s != 0.0, s, 1.0), 0.0)
        out[i] = out[i] * np.repeat(s, 11) + spfh[i]
    return out
