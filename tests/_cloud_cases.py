"""Named, seeded clouds and per-geometry parameters for the point-cloud operations' case matrix
(test_cloudops_matrix_cpu.py, test_cloudops_matrix_gpu.py).

The clouds are the target clouds of _nn_cases.GEOMETRIES (without the nonfinite_* ones) and `two_sheets`.  Every
parameter follows the cloud's own length h -- the median non-zero distance to the 8 nearest neighbours, 1.0 where
there is none -- so the same table of factors gives a meaningful neighbourhood at mm scale, 1e5 from the origin and
at extents of 1e-4."""
import numpy as np
from scipy.spatial import cKDTree

import _nn_cases

NAMES = ("blob", "far", "small", "clusters", "planar", "collinear", "duplicated", "one_point", "lattice", "boundary")
SEED = 3
SIZES = (700, 5000)


def two_sheets(n=600, seed=SEED):
    """n / 2 points with z = 0 exactly and n / 2 with z = 10 exactly, x and y uniform in [0, 20); even rows lie on
    the lower sheet and odd rows on the upper one, so the sheets interleave in index order.  Both sheets hold the
    same number of points: every sample of three points of one sheet has n / 2 inliers, and which sheet
    segment_plane returns is decided by the tie rule alone (the earliest iteration)."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 3))
    pts[:, :2] = rng.uniform(0.0, 20.0, (n, 2))
    pts[1::2, 2] = 10.0
    return pts


def cloud(name, n, seed=SEED):
    if name == "two_sheets":
        return two_sheets(n, seed)
    return np.ascontiguousarray(_nn_cases.GEOMETRIES[name](8, n, seed)[1])


def length(pts):
    """h: the median non-zero distance to the 8 nearest neighbours, 1.0 if there is none."""
    pts = np.asarray(pts, np.float64)
    if len(pts) < 2:
        return 1.0
    d, _ = cKDTree(pts).query(pts, k=min(9, len(pts)))
    d = d[:, 1:]
    d = d[d > 0]
    return float(np.median(d)) if len(d) else 1.0


def params(pts):
    """The operations' parameters for a cloud, by its length h."""
    h = length(pts)
    return {"h": h, "voxel": 2.5 * h, "k": 8, "eps": 3.0 * h, "min_points": 5, "normal_radius": 4.0 * h, "normal_max_nn": 30,
            "fpfh_radius": 5.0 * h, "fpfh_max_nn": 50, "plane_threshold": 0.5 * h, "plane_iterations": 60, "plane_seed": 2}


def blob(n, seed, scale=1.0, offset=0.0):
    return _nn_cases.blob(8, n, seed, scale, offset)[1]


def sheet(n, seed, span=100.0, amp=2.0):
    """A wavy sheet: x, y uniform in [0, span), z = amp sin(x / 9) cos(y / 7) and 0.05 of noise."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, span, (n, 2))
    return np.column_stack([xy, amp * np.sin(xy[:, 0] / 9.0) * np.cos(xy[:, 1] / 7.0) + rng.normal(0.0, 0.05, n)])


def fuzz(seed):
    """(geometry name, cloud, parameters) of a fuzz seed: N uniform in [1, 600], the geometry and the parameters
    drawn from the seed -- eps, radius and voxel from [0.5 h, 8 h], k from [1, 40], max_nn from [1, 128]."""
    rng = np.random.default_rng(5000 + seed)   # (seeds 0..15 from this base reach N = 1, k >= N and sparse neighbourhoods)
    n = int(rng.integers(1, 601))
    name = NAMES[int(rng.integers(0, len(NAMES)))]
    pts = cloud(name, n, seed)
    h = length(pts)
    u = lambda: float(rng.uniform(0.5, 8.0)) * h
    return name, pts, {"h": h, "voxel": u(), "k": int(rng.integers(1, 41)), "eps": u(), "min_points": int(rng.integers(1, 12)),
                       "normal_radius": u(), "normal_max_nn": int(rng.integers(1, 129)), "fpfh_radius": u(),
                       "fpfh_max_nn": int(rng.integers(1, 129)), "plane_threshold": float(rng.uniform(0.1, 2.0)) * h,
                       "plane_iterations": int(rng.integers(1, 130)), "plane_seed": seed}
