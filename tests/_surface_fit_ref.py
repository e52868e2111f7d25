"""numpy restatement of the surface fit's contract (include/pedp.h pedp_fit_to_surface) on top of
_closest_ref: the same expressions in the same order, float64.  The search is _closest_ref's point_triangle with the
lexicographic (d^2, index) minimum; the sums are plain running sums in index order (or in the reverse order, which is
how the tests measure what a summation order may move); the solve is the pivoted LDLT of csrc/icp/solve.h."""
import functools
import math

import numpy as np

import _closest_ref as ref

NONE = ref.NONE
LOSSES = ("l2", "huber", "tukey")

# What the order of the sums alone moves in a fit: the reference with its running sums forwards against the reference with
# them reversed, over the five cases below (test_surface_fit_cpu measures it again and holds it to these figures).
# Measured: T 5.61e-14 (the soup, Huber), rmse 4.98e-15 (the clean torus).  The device sums in a tree, a third order, so
# it is allowed 100 times the floor.
FLOOR_T, FLOOR_RMSE = 5.7e-14, 5.0e-15
BOUND_T, BOUND_RMSE = 100 * FLOOR_T, 100 * FLOOR_RMSE


# ---------------------------------------------------------------- the search

def _spheres(a, ab, ac):
    """A sphere around every record: the centroid and the largest vertex distance, widened."""
    cen = a + (ab + ac) / 3.0
    rad = np.sqrt(np.maximum.reduce([((v - cen) ** 2).sum(axis=1) for v in (a, a + ab, a + ac)]))
    return cen, rad * (1.0 + 1e-9) + 1e-9


def closest(recs, q):
    """(c, d, face) of the rows of q (all finite) against the records: _closest_ref.closest_ref's points, distances and
    primitive_ids.  Only the pairs that can win are evaluated -- a triangle whose sphere lies farther than the nearest
    sphere's far side (by a margin far above the rounding of the bound) cannot -- and each of them by the same
    point_triangle, so the result has closest_ref's bits (test_surface_fit_cpu checks that it does)."""
    a, ab, ac, skip = recs
    n = len(q)
    c = np.full((n, 3), np.nan)
    d = np.full(n, np.inf)
    face = np.full(n, NONE, np.uint32)
    use = np.nonzero(~skip)[0]
    if n == 0 or len(use) == 0:
        return c, d, face
    cen, rad = _spheres(a[use], ab[use], ac[use])
    step = max(1, (1 << 22) // len(use))
    for i0 in range(0, n, step):
        qq = q[i0:i0 + step]
        gap = np.sqrt(((qq[:, None, :] - cen[None]) ** 2).sum(axis=2))
        upper = (gap + rad[None]).min(axis=1)
        i, k = np.nonzero(gap - rad[None] <= (upper * (1.0 + 1e-9) + 1e-9)[:, None])
        f = use[k]
        with np.errstate(all="ignore"):
            dd = ref.point_triangle(qq[i], a[f], ab[f], ac[f])[4]
        dd = np.where(np.isnan(dd), np.inf, dd)
        order = np.lexsort((f, dd, i))                  # by row, then d^2, then index: the first of a row wins
        i, f, dd = i[order], f[order], dd[order]
        first = np.r_[True, i[1:] != i[:-1]]
        i, f, dd = i[first], f[first], dd[first]
        hit = dd < np.inf
        i, f = i[hit], f[hit]
        _, _, cc, _, d2 = ref.point_triangle(qq[i], a[f], ab[f], ac[f])
        c[i0 + i] = cc
        d[i0 + i] = np.sqrt(d2)
        face[i0 + i] = f.astype(np.uint32)
    return c, d, face


# ---------------------------------------------------------------- rows

def move(T, p):
    """q = R p + t, each component ((T[k,0] x + T[k,1] y) + T[k,2] z) + T[k,3]."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)], axis=1)


def cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2],
                     x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=1)


def weight(loss, scale, d):
    """The weight of an inlier at distance d (an array)."""
    d = np.asarray(d, dtype=np.float64)
    if loss == "l2":
        return np.ones_like(d)
    with np.errstate(all="ignore"):
        if loss == "huber":
            return np.where(d <= scale, 1.0, scale / d)
        if loss == "tukey":
            u = d / scale
            t = 1.0 - u * u
            return np.where(d < scale, t * t, 0.0)
    raise ValueError(loss)


def row_terms(recs, pts, T, loss, scale, gate):
    """(terms, rows, finite): the 30 terms of every row that takes part (M x 30, in index order), the indices of those
    rows, and the number of finite rows.  Columns: 21 of w J J^T (upper triangle, row by row), 6 of w J d, d d, 1, w."""
    a, ab, ac, _ = recs
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    fin = np.nonzero(np.isfinite(p).all(axis=1))[0]
    q = move(T, p[fin])
    c, d, face = closest(recs, q)
    with np.errstate(invalid="ignore"):
        take = (face != NONE) & (d <= gate)
    q, c, d, f = q[take], c[take], d[take], face[take].astype(np.int64)
    nf = cross(ab[f], ac[f])
    with np.errstate(all="ignore"):
        nf = nf / np.sqrt(ref.dot(nf, nf))[:, None]
        n = np.where((d > 0.0)[:, None], (q - c) / d[:, None], nf)
    w = weight(loss, scale, d)
    J = np.concatenate([cross(q, n), n], axis=1)
    wJ = w[:, None] * J
    cols = [wJ[:, i] * J[:, j] for i in range(6) for j in range(i, 6)]
    cols += [wJ[:, i] * d for i in range(6)]
    cols += [d * d, np.ones_like(d), w]
    return np.stack(cols, axis=1).reshape(-1, 30), fin[take], len(fin)


def running_sum(terms, reverse=False):
    """The 30 sums of the terms, one after the other in index order (or from the last row to the first)."""
    if len(terms) == 0:
        return np.zeros(terms.shape[1])
    return np.cumsum(terms[::-1] if reverse else terms, axis=0)[-1]


def exact_sum(terms):
    """math.fsum of every column, and the sum of the absolute values: what a summation bound is stated against."""
    return (np.array([math.fsum(col) for col in terms.T]), np.array([math.fsum(np.abs(col)) for col in terms.T]))


# ---------------------------------------------------------------- close

def solve6_ldlt(Ain, b):
    """csrc/icp/solve.h solve6_ldlt: (x, ok)."""
    n = 6
    A = np.array(Ain, dtype=np.float64).reshape(6, 6).copy()
    tr = [0] * n
    for k in range(n):
        p, big = k, abs(A[k, k])
        for i in range(k + 1, n):
            if abs(A[i, i]) > big:
                big, p = abs(A[i, i]), i
        tr[k] = p
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
        if k > 0:
            tmp = [A[j, j] * A[k, j] for j in range(k)]
            s = 0.0
            for j in range(k):
                s += A[k, j] * tmp[j]
            A[k, k] -= s
            for i in range(k + 1, n):
                u = 0.0
                for j in range(k):
                    u += A[i, j] * tmp[j]
                A[i, k] -= u
        akk = A[k, k]
        if abs(akk) > 0.0:
            for i in range(k + 1, n):
                A[i, k] /= akk
    y = [float(v) for v in b]
    for k in range(n):
        if tr[k] != k:
            y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(n):
        for j in range(i):
            y[i] -= A[i, j] * y[j]
    for i in range(n):
        y[i] = y[i] / A[i, i] if abs(A[i, i]) > 2.2250738585072014e-308 else 0.0
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] -= A[j, i] * y[j]
    for k in range(n - 1, -1, -1):
        if tr[k] != k:
            y[k], y[tr[k]] = y[tr[k]], y[k]
    x = np.array(y)
    return x, bool(np.isfinite(x).all())


def vec6_to_T(x):
    """csrc/icp/solve.h vec6_to_T."""
    sa, ca, sb, cb, sc, cc = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    return np.array([[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, x[3]],
                     [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def mat4_mul(A, B):
    """csrc/icp/solve.h mat4_mul_dev: every entry a running sum over k from 0."""
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += A[i, k] * B[k, j]
            C[i, j] = s
    return C


def fit(verts, tris, pts, init=None, loss="tukey", scale=None, gate=np.inf, max_iteration=30, relative_fitness=1e-6,
        relative_rmse=1e-6, reverse=False):
    """The loop of pedp_fit_to_surface.  Returns a dict: T, fitness, rmse, iterations, K, weight_sum, singular, and trace
    (one row per pass: fitness, rmse, K, then the 16 of T as the pass found it)."""
    recs = ref.records(verts, tris)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    fitness = rmse = 0.0
    trace, singular, p = [], False, 0
    while True:
        terms, _, n_finite = row_terms(recs, pts, T, loss, scale, gate)
        pk = running_sum(terms, reverse)
        K = pk[28]
        prev = (fitness, rmse)
        fitness, rmse = (K / n_finite, math.sqrt(pk[27] / K)) if K > 0 else (0.0, 0.0)
        trace.append(np.r_[fitness, rmse, K, T.reshape(-1)])
        if p >= max_iteration or not K > 0:
            break
        if p > 0 and abs(prev[0] - fitness) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
        A = np.zeros((6, 6))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                A[i, j] = A[j, i] = pk[k]
                k += 1
        x, ok = solve6_ldlt(A, -pk[21:27])
        nxt = mat4_mul(vec6_to_T(x), T) if ok else T
        if not (ok and np.isfinite(nxt).all()):
            singular = True
            break
        T = nxt
        p += 1
    return {"T": T, "fitness": fitness, "rmse": rmse, "iterations": p, "K": int(pk[28]), "weight_sum": float(pk[29]),
            "singular": singular, "trace": np.array(trace)}


# ---------------------------------------------------------------- the cases the CPU and the GPU tests share

def rigid(rotvec, t):
    """The 4 x 4 of a rotation vector (Rodrigues) and a translation."""
    rotvec = np.asarray(rotvec, dtype=np.float64)
    th = np.linalg.norm(rotvec)
    k = rotvec / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * Kx + (1.0 - math.cos(th)) * (Kx @ Kx)
    T[:3, 3] = t
    return T


def pose_errors(T, want):
    """(rotation error in degrees, translation error) of T against `want`."""
    R = T[:3, :3] @ want[:3, :3].T
    return (math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0)))),
            float(np.linalg.norm(T[:3, 3] - want[:3, 3])))


MOTION = rigid(np.deg2rad(2.7) * np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0), 1.1 * np.array([0.5, -0.7, 0.5]) / math.sqrt(0.99))


def torus_mesh():
    from pedp_hip import synth

    v, t, _ = synth.bumpy_torus(50, 40)
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(t)


@functools.lru_cache(maxsize=None)
def torus_case(dent, n=2000, seed=7):
    """(verts, tris, points, motion): n points on the triangles of the 50 x 40 torus, with dent=True the ones within
    0.35 rad of azimuth 1.0 lifted 3 units along their face's normal, all moved by inv(MOTION): the fit that brings them
    back is MOTION."""
    verts, tris = torus_mesh()
    a, ab, ac, skip = ref.records(verts, tris)
    rng = np.random.default_rng(seed)
    f = rng.choice(np.nonzero(~skip)[0], n)
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = u + v > 1.0
    u, v = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - v, v)
    s = a[f] + ab[f] * u[:, None] + ac[f] * v[:, None]
    if dent:
        nrm = np.cross(ab[f], ac[f])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        az = np.arctan2(s[:, 1], s[:, 0])
        patch = np.abs(np.angle(np.exp(1j * (az - 1.0)))) < 0.35
        s = s + 3.0 * patch[:, None] * nrm
    inv = np.linalg.inv(MOTION)
    pts = np.ascontiguousarray(s @ inv[:3, :3].T + inv[:3, 3])
    for arr in (verts, tris, pts):
        arr.setflags(write=False)
    return verts, tris, pts, MOTION


def soup(F, seed):
    """F random triangles of 1 .. 12 mm in a 100 mm box, the second one degenerate (test_closest_gpu's generator)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-50.0, 50.0, (F, 1, 3))
    verts = (centre + rng.normal(0.0, rng.uniform(1.0, 12.0, (F, 1, 1)), (F, 3, 3))).reshape(-1, 3).astype(np.float32)
    if F > 2:
        verts[5] = verts[4]
    return verts, np.arange(3 * F, dtype=np.uint32).reshape(F, 3)


def queries(verts, tris, n, seed):
    """n points in turn on vertices, on edge midpoints, at centroids, 0.5 off and 200 off the faces, and scattered
    (test_closest_gpu's generator): d = 0 on vertices and edges, the far ones beyond any sensible gate."""
    rng = np.random.default_rng(seed)
    v = verts.astype(np.float64)
    f = rng.integers(0, len(tris), n)
    a, b, c = v[tris[f, 0]], v[tris[f, 1]], v[tris[f, 2]]
    nrm = np.cross(b - a, c - a)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    cen = (a + b + c) / 3.0
    sign = rng.choice([-1.0, 1.0], (n, 1))
    kinds = [a, c, 0.5 * (a + b), 0.5 * (b + c), cen, cen + 0.5 * sign * nrm, cen + 200.0 * sign * nrm,
             rng.uniform(-120.0, 120.0, (n, 3))]
    pick = np.arange(n) % len(kinds)
    return np.ascontiguousarray(np.stack(kinds)[pick, np.arange(n)])


SOUP_FIT = dict(loss="huber", scale=1.0, gate=20.0, max_iteration=6)


@functools.lru_cache(maxsize=None)
def soup_case():
    """(verts, tris, points): 3072 of `queries` on the 1025-triangle soup, moved by inv(MOTION)."""
    verts, tris = soup(1025, 3)
    inv = np.linalg.inv(MOTION)
    pts = np.ascontiguousarray(queries(verts, tris, 3072, 3072) @ inv[:3, :3].T + inv[:3, 3])
    for arr in (verts, tris, pts):
        arr.setflags(write=False)
    return verts, tris, pts


@functools.lru_cache(maxsize=None)
def soup_fit(reverse=False):
    verts, tris, pts = soup_case()
    return fit(verts, tris, pts, reverse=reverse, **SOUP_FIT)


CASES = {"clean": dict(dent=False, loss="l2", scale=None, gate=np.inf), "dent_l2": dict(dent=True, loss="l2", scale=None, gate=10.0),
         "dent_huber": dict(dent=True, loss="huber", scale=0.5, gate=10.0),
         "dent_tukey": dict(dent=True, loss="tukey", scale=1.5, gate=10.0)}


@functools.lru_cache(maxsize=None)
def torus_fit(name, reverse=False):
    """The reference fit of one of CASES (computed once per process, shared by the tests; the arrays are not to be written)."""
    case = CASES[name]
    verts, tris, pts, _ = torus_case(case["dent"])
    return fit(verts, tris, pts, loss=case["loss"], scale=case["scale"], gate=case["gate"], reverse=reverse)
