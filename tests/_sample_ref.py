"""The contract of the surface sampler (pedp_sample.hip) restated in numpy: Philox4x32-10 on uint64
arrays, the integer prefix sum of the faces' weights and the 64 x 64 -> high 64 multiply through Python integers, Open3D's
point formula in float64, the thinning as the serial greedy visit in ascending key order over a cKDTree candidate list
(the strict comparison done by hand in the contract's arithmetic), the round-based form of the same set, and the
bisection of the count form.  The device is compared with this bit for bit (test_mesh_sample_gpu.py); the restatement
itself is pinned by test_mesh_sample_cpu.py."""
import numpy as np
from scipy.spatial import cKDTree

from _refine_ref import cube, icosphere, refine  # noqa: F401  (the mesh builders of the refinement's tests)

U = np.uint64
MASK = U(0xFFFFFFFF)
M0, M1 = U(0xD2511F53), U(0xCD9E8D57)
W0, W1 = U(0x9E3779B9), U(0xBB67AE85)
NORMALS_NONE, NORMALS_VERTEX, NORMALS_TRIANGLE = 0, 1, 2


# ---------------------------------------------------------------- the generator
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0, c1, c2, c3) and keys (k0, k1): four uint64 arrays of 32-bit words."""
    x0, x1, x2, x3, k0, k1 = np.broadcast_arrays(*[np.atleast_1d(np.asarray(a, dtype=U)) for a in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = M0 * x0, M1 * x2                                  # 32 x 32 bits: no overflow in 64
        x0, x1, x2, x3 = (p1 >> U(32)) ^ x1 ^ k0, p1 & MASK, (p0 >> U(32)) ^ x3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return x0, x1, x2, x3


def draw(k, which, seed):
    """Block `which` (0: x, 1: y, 2: a given cloud's thinning key) of samples k (uint64) under a 64-bit seed."""
    k = np.asarray(k, dtype=U)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox(k & MASK, k >> U(32), which, 0, seed & 0xFFFFFFFF, seed >> 32)


def mulhi64(a, w):
    w = int(w)
    return np.array([(int(x) * w) >> 64 for x in a], dtype=U)


def sample_numbers(first, n):
    """k = first + i mod 2^64"""
    return np.array([(int(first) + i) & 0xFFFFFFFFFFFFFFFF for i in range(n)], dtype=U)


# ---------------------------------------------------------------- the faces' table
def _cross(e1, e2):
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                     e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _norm(c):
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def face_table(v, t):
    """area (F), amax, w (F uint64), C (F uint64, inclusive), W, A (the areas summed in face order)"""
    v, t = np.asarray(v, np.float64), np.asarray(t).astype(np.int64)
    with np.errstate(all="ignore"):
        area = 0.5 * _norm(_cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]))
        finite = np.isfinite(area)
        amax = area[finite].max() if finite.any() else 0.0
        w = np.zeros(len(t), U)
        ok = finite & (area > 0.0)
        w[ok] = np.floor((area[ok] / amax) * 4294967296.0).astype(U)
    c = np.cumsum(w, dtype=U)
    return area, amax, w, c, int(c[-1]), float(np.cumsum(area)[-1])   # cumsum adds in order; np.sum would add pairwise


def sample(v, t, n, seed=0, first=0, normals=NORMALS_NONE, vertex_normals=None):
    """Samples [first, first + n): a dict of points, face_ids (int32), barycentric, normals (or None) and z (y2)."""
    v, t = np.asarray(v, np.float64), np.asarray(t).astype(np.int64)
    _, _, _, c, w_total, _ = face_table(v, t)
    k = sample_numbers(first, n)
    x, y = draw(k, 0, seed), draw(k, 1, seed)
    f = np.searchsorted(c, mulhi64((x[0] << U(32)) | x[1], w_total), "right")
    u1 = (((x[2] << U(32)) | x[3]) >> U(11)).astype(np.float64) * 2.0 ** -53
    u2 = (((y[0] << U(32)) | y[1]) >> U(11)).astype(np.float64) * 2.0 ** -53
    s = np.sqrt(u1)
    a, b, cc = 1.0 - s, s * (1.0 - u2), s * u2
    v0, v1, v2 = v[t[f, 0]], v[t[f, 1]], v[t[f, 2]]
    nrm = None
    if normals == NORMALS_VERTEX:
        q = np.asarray(vertex_normals, np.float64)
        nrm = (a[:, None] * q[t[f, 0]] + b[:, None] * q[t[f, 1]]) + cc[:, None] * q[t[f, 2]]
    elif normals == NORMALS_TRIANGLE:
        cr = _cross(v1 - v0, v2 - v0)
        nrm = cr / _norm(cr)[:, None]
    return {"points": (a[:, None] * v0 + b[:, None] * v1) + cc[:, None] * v2, "face_ids": f.astype(np.int32),
            "barycentric": np.stack([a, b, cc], axis=1), "normals": nrm, "z": y[2]}


# ---------------------------------------------------------------- thinning
def keys(z):
    """(z_i << 32) | (i mod 2^32)"""
    z = np.asarray(z, dtype=U)
    return (z << U(32)) | (np.arange(len(z), dtype=U) & MASK)


def cloud_keys(n, seed=0):
    return keys(draw(np.arange(n, dtype=U), 2, seed)[0])


def _dist2(p, q):
    d = p - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def thin(p, key, r):
    """S(r): the serial greedy in ascending key order.  A bool mask of the kept points."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    r2 = r * r
    if len(p) == 0 or not r2 > 0.0:
        return np.ones(len(p), bool)
    tree = cKDTree(p)
    kept, removed = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for i in np.argsort(key, kind="stable"):
        if removed[i]:
            continue
        kept[i] = True
        cand = np.asarray(tree.query_ball_point(p[i], r * (1.0 + 1e-6)), dtype=np.int64)
        cand = cand[cand != i]
        removed[cand[_dist2(p[cand], p[i][None, :]) < r2]] = True
    return kept


def conflict_pairs(p, r):
    """every pair i < j with ((dx^2 + dy^2) + dz^2) < r * r"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    if len(p) < 2 or not r * r > 0.0:
        return np.zeros((0, 2), np.int64)
    pairs = cKDTree(p).query_pairs(r * (1.0 + 1e-6), output_type="ndarray").astype(np.int64).reshape(-1, 2)
    return pairs[_dist2(p[pairs[:, 0]], p[pairs[:, 1]]) < r * r]


def thin_rounds(p, key, r):
    """The same set in synchronous rounds (states read from before the round): the kept mask and the rounds taken."""
    n = len(p)
    pairs = conflict_pairs(p, r)
    swap = key[pairs[:, 0]] > key[pairs[:, 1]]
    low, high = np.where(swap, pairs[:, 1], pairs[:, 0]), np.where(swap, pairs[:, 0], pairs[:, 1])
    state, rounds = np.zeros(n, np.int8), 0                       # 0 undecided, 1 kept, 2 removed
    while (state == 0).any():
        open_ = state[high] == 0
        gone = np.zeros(n, bool)
        gone[high[open_ & (state[low] == 1)]] = True
        held = np.zeros(n, bool)
        held[high[open_ & (state[low] == 0)]] = True
        und = state == 0
        state[und & gone] = 2
        state[und & ~gone & ~held] = 1
        rounds += 1
    return state == 1, rounds


def thin_to_count(p, key, n_points, r_hi):
    """The count form: (the N kept indices in ascending order, r*)."""
    lo, hi = 0.0, r_hi
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        if int(thin(p, key, mid).sum()) >= n_points:
            lo = mid
        else:
            hi = mid
    kept = np.flatnonzero(thin(p, key, lo))
    kept = kept[np.argsort(key[kept], kind="stable")[:n_points]]
    return np.sort(kept).astype(np.int32), lo


def _rows(s, idx):
    return {k: (None if a is None else a[idx]) for k, a in s.items()}


def sample_disk(v, t, number_of_points=None, spacing=None, init_factor=5, seed=0, normals=NORMALS_NONE, vertex_normals=None):
    """sample_points_poisson_disk on the mesh: the kept samples' rows, `index` (their sample numbers), `spacing`, `drawn`."""
    area = face_table(v, t)[5]
    if number_of_points is not None:
        m = init_factor * number_of_points
        s = sample(v, t, m, seed, 0, normals, vertex_normals)
        idx, r = thin_to_count(s["points"], keys(s["z"]), number_of_points, 2.0 * np.sqrt(area / number_of_points))
    else:
        m = max(int(np.ceil((float(init_factor) * area) / (spacing * spacing))), 1)
        s = sample(v, t, m, seed, 0, normals, vertex_normals)
        idx, r = np.flatnonzero(thin(s["points"], keys(s["z"]), spacing)).astype(np.int32), spacing
    out = _rows(s, idx)
    out.update(index=idx, spacing=float(r), drawn=m)
    return out


# ---------------------------------------------------------------- meshes
def one_triangle():
    return np.array([[0.25, -1.0, 2.0], [3.0, 0.5, 1.0], [-0.5, 2.0, 0.125]], np.float64), np.array([[0, 1, 2]], np.uint32)


def two_triangles_1_3():
    """areas 0.5 and 1.5"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 1], [0, 1, 1]], np.float64)
    return v, np.array([[0, 1, 2], [3, 4, 5]], np.uint32)


def strip(n_faces, height=1.0):
    """n_faces triangles of equal area over a unit-step strip"""
    n = n_faces + 2
    v = np.array([[0.5 * i, height * (i % 2), 0.0] for i in range(n)], np.float64)
    t = np.array([[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n_faces)], np.uint32)
    return v, t


def with_dead_faces():
    """two live triangles around a zero-area face (index 1) and one below 2^-32 of the largest (index 3)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],           # 0: area 0.5
                  [2, 2, 2], [3, 3, 3], [4, 4, 4],           # 1: collinear
                  [0, 0, 1], [1, 0, 1], [0, 1, 1],           # 2: area 0.5
                  [5, 0, 0], [5 + 2.0 ** -17, 0, 0], [5, 2.0 ** -17, 0]], np.float64)   # 3: area 2^-35
    return v, np.arange(12, dtype=np.uint32).reshape(4, 3)


def vertex_normals(v, t):
    """area-weighted vertex normals (any smooth per-vertex vectors would do)"""
    v, t = np.asarray(v, np.float64), np.asarray(t).astype(np.int64)
    fn = _cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, t[:, k], fn)
    ln = np.linalg.norm(acc, axis=1, keepdims=True)
    return acc / np.where(ln > 0, ln, 1.0)


def separated_squares(size=100.0, shrink=0.8):
    """The six sides of a cube, each shrunk about its centre and with vertices of its own: 12 faces, outward winding.  The
    sides' rims are 0.1 sqrt(2) size apart, so a cloud sampled more densely than that pairs every point of another
    sampling with a point of the same plane."""
    v, t, c = [], [], 0.5 * size
    for axis in range(3):
        for side in (0.0, size):
            u, w = [a for a in range(3) if a != axis]
            q = np.zeros((4, 3))
            q[:, axis] = side
            q[:, u] = [c - shrink * c, c + shrink * c, c + shrink * c, c - shrink * c]
            q[:, w] = [c - shrink * c, c - shrink * c, c + shrink * c, c + shrink * c]
            b = len(v)
            v += list(q)
            flip = (side == 0.0) != (axis == 1)          # (u, w, axis) is right-handed except for axis 1
            t += [[b, b + 2, b + 1], [b, b + 3, b + 2]] if flip else [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    return np.array(v, np.float64), np.array(t, np.uint32)
