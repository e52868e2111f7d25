"""Named, seeded geometries for the nearest-neighbour / registration case matrix
(test_nn_matrix_gpu.py) and the oracle's own agreement test (test_oracle_cpu.py).

Every generator returns (src, tgt, normals) as float64 arrays; `normals` are unit vectors, one per
target row, so point-to-plane can run on every geometry.  The source lies near the target (a
subset of it, jittered) unless the geometry says otherwise, so a registration has inliers."""
import numpy as np


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _near(rng, tgt, ns, sigma):
    """ns source points: target rows drawn with replacement, jittered by sigma."""
    pick = rng.integers(0, len(tgt), ns) if len(tgt) else np.zeros(0, np.int64)
    return tgt[pick] + rng.normal(0.0, sigma, (ns, 3))


def blob(ns, nt, seed, scale=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    tgt = rng.normal(0.0, 1.0, (nt, 3)) * scale + offset
    src = _near(rng, tgt, ns, 0.02 * scale)
    return src, tgt, _unit(rng.normal(size=(nt, 3)))


def far(ns, nt, seed):
    """mm far from the origin: the blob translated by 1e5."""
    return blob(ns, nt, seed, scale=1.0, offset=1e5)


def small(ns, nt, seed):
    """Extents of 1e-4."""
    return blob(ns, nt, seed, scale=1e-4)


def clusters(ns, nt, seed):
    """Two blobs 1e4 apart: a mostly empty bounding box."""
    rng = np.random.default_rng(seed)
    tgt = rng.normal(0.0, 1.0, (nt, 3))
    tgt[nt // 2:, 0] += 1e4
    src = _near(rng, tgt, ns, 0.02)
    return src, tgt, _unit(rng.normal(size=(nt, 3)))


def planar(ns, nt, seed):
    """z = 0 exactly (one zero extent), normals +z."""
    rng = np.random.default_rng(seed)
    tgt = np.zeros((nt, 3))
    tgt[:, :2] = rng.normal(0.0, 1.0, (nt, 2))
    src = _near(rng, tgt, ns, 0.02)
    return src, tgt, np.tile([0.0, 0.0, 1.0], (nt, 1))


def collinear(ns, nt, seed):
    """On the x axis (two zero extents), normals +z."""
    rng = np.random.default_rng(seed)
    tgt = np.zeros((nt, 3))
    tgt[:, 0] = rng.normal(0.0, 1.0, nt)
    src = _near(rng, tgt, ns, 0.02)
    return src, tgt, np.tile([0.0, 0.0, 1.0], (nt, 1))


def duplicated(ns, nt, seed):
    """Every target row twice (rows 2k and 2k + 1 equal): exact ties, lowest index wins."""
    src, base, nrm = blob(ns, (nt + 1) // 2, seed)
    return src, np.repeat(base, 2, axis=0)[:nt], np.repeat(nrm, 2, axis=0)[:nt]


def one_point(ns, nt, seed):
    """All target rows are the same point: every query ties nt ways."""
    rng = np.random.default_rng(seed)
    tgt = np.tile([0.25, -0.5, 1.0], (nt, 1))
    src = tgt[:1] + rng.normal(0.0, 0.3, (ns, 3))
    return src, tgt, np.tile([0.0, 0.0, 1.0], (nt, 1))


def lattice(ns, nt, seed):
    """Integer lattice of spacing 2 (about nt points); queries on cell centres, face centres and
    edge midpoints: exact 8-, 4- and 2-way ties at squared distances 3, 2 and 1."""
    rng = np.random.default_rng(seed)
    m = max(2, int(round(nt ** (1 / 3))))
    g = np.arange(m, dtype=np.float64) * 2.0
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:nt]
    offs = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    base = tgt[rng.integers(0, len(tgt), ns)]
    src = base + offs[np.arange(ns) % 3]
    return src, tgt, _unit(rng.normal(size=(len(tgt), 3)))


def boundary(ns, nt, seed):
    """Sparse integer targets (spacing 100) and queries at offset (3, 4, 0) of one of them: the
    nearest neighbour is at exactly d = 5 (d^2 == 25 in float64), every other one beyond 90."""
    rng = np.random.default_rng(seed)
    m = max(2, int(round(nt ** (1 / 3))))
    g = np.arange(m, dtype=np.float64) * 100.0
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:nt]
    src = tgt[rng.integers(0, len(tgt), ns)] + [3.0, 4.0, 0.0]
    return src, tgt, np.tile([0.0, 0.0, 1.0], (len(tgt), 1))


def nonfinite_source(ns, nt, seed):
    """The blob with NaN, +inf and -inf source rows: scattered single coordinates, and a run of
    (ns % 128) + 128 all-NaN rows from row 128 on.  Non-finite rows go last in the spatial order, so
    the last partial chunk and the whole 128-point chunk before it hold nothing else."""
    src, tgt, nrm = blob(ns, nt, seed)
    rng = np.random.default_rng(seed + 1)
    bad = rng.choice(ns, max(3, ns // 20), replace=False)
    for j, i in enumerate(bad):
        src[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    run = ns % 128 + 128
    if ns >= 128 + run:
        src[128:128 + run] = np.nan
    return src, tgt, nrm


def nonfinite_target(ns, nt, seed):
    """The blob with NaN, +inf and -inf target rows (never a neighbour)."""
    src, tgt, nrm = blob(ns, nt, seed)
    rng = np.random.default_rng(seed + 2)
    bad = rng.choice(nt, max(3, nt // 20), replace=False)
    for j, i in enumerate(bad):
        tgt[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    return src, tgt, nrm


GEOMETRIES = {
    "blob": blob, "far": far, "small": small, "clusters": clusters, "planar": planar, "collinear": collinear,
    "duplicated": duplicated, "one_point": one_point, "lattice": lattice, "boundary": boundary,
    "nonfinite_source": nonfinite_source, "nonfinite_target": nonfinite_target,
}


def extent(tgt):
    """Diagonal of the target's bounding box over its finite rows (like the library's box: a row with a
    NaN or infinite coordinate is left out)."""
    t = np.asarray(tgt, np.float64)
    t = t[np.isfinite(t).all(1)]
    if len(t) == 0:
        return 0.0
    lo, hi = t.min(axis=0), t.max(axis=0)
    return float(np.sqrt(np.sum((hi - lo) ** 2)))
