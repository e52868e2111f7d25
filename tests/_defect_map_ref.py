"""The defect map restated on the host: numpy for the faces' geometry and the weld, a dict of edges for
the adjacency, scipy's connected components for the regions, math.fsum for the sums.  Also the meshes of the tests."""
import math

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

MISS = 0xFFFFFFFF
SIGN = np.uint64(1 << 63)
INT_COLUMNS = ("first_face", "n_faces", "n_seed_faces", "max_frames", "hits")
BIT_COLUMNS = ("peak", "lo", "hi")


# ------------------------------------------------------------------ the order-preserving key
def key_of(x):
    """uint64 keys with key(a) < key(b) <=> a < b for non-NaN doubles, -0 below +0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | SIGN)


def value_of(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~SIGN, ~k).view(np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the model
def weld(verts):
    """w[v]: the lowest index of a vertex whose coordinates compare equal with == (-0 == +0; NaN equals nothing)."""
    v = np.asarray(verts, dtype=np.float64) + 0.0           # -0 + 0 = +0: one representation per value
    w = np.arange(len(v), dtype=np.int64)
    ok = ~np.isnan(v).any(axis=1)
    if ok.any():
        idx = np.nonzero(ok)[0]
        _, first, inverse = np.unique(v[ok], axis=0, return_index=True, return_inverse=True)
        w[idx] = idx[first[inverse.reshape(-1)]]            # np.unique's index is that of the first occurrence
    return w


class Model:
    """Areas, centroids, boxes, welded ids and neighbour lists of a triangle mesh, float64 in the contract's order."""

    def __init__(self, verts, tris, welded=True):
        self.verts = v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        self.tris = t = np.ascontiguousarray(tris, dtype=np.uint32).reshape(-1, 3)
        self.F = F = len(t)
        a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
        ab, ac = b - a, c - a
        with np.errstate(invalid="ignore", over="ignore"):
            n0 = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
            n1 = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
            n2 = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
            self.area = 0.5 * np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
            self.centroid = ((a + b) + c) / 3.0
        corners = np.stack([a, b, c], axis=1)               # F x 3 corners x 3 axes
        keys = key_of(corners)
        nan = np.isnan(corners)
        self.lo_key = np.where(nan, key_of(np.inf), keys).min(axis=1) if F else np.zeros((0, 3), np.uint64)
        self.hi_key = np.where(nan, key_of(-np.inf), keys).max(axis=1) if F else np.zeros((0, 3), np.uint64)
        self.w = w = weld(v) if welded else np.arange(len(v), dtype=np.int64)   # welded=False: by the raw indices
        edges = {}
        for f in range(F):
            for k in range(3):
                i, j = int(w[t[f, k]]), int(w[t[f, (k + 1) % 3]])
                if i != j:
                    edges.setdefault((min(i, j), max(i, j)), []).append(f)
        nbr = [set() for _ in range(F)]
        for faces in edges.values():
            for f in faces:
                nbr[f].update(faces)
        self.neighbours = [np.array(sorted(s - {f}), dtype=np.int64) for f, s in enumerate(nbr)]
        rows = np.concatenate([np.full(len(n), f) for f, n in enumerate(self.neighbours)]) if F else np.zeros(0, np.int64)
        cols = np.concatenate(self.neighbours) if F else np.zeros(0, np.int64)
        self.graph = csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(F, F))


# ------------------------------------------------------------------ accumulating
class State:
    def __init__(self, F):
        self.F = F
        self.key = np.zeros(F, np.uint64)
        self.hits = np.zeros(F, np.int64)
        self.frames = np.zeros(F, np.int32)
        self.observations = self.rows_added = self.rows_ignored = 0

    def add(self, ids, x):
        ids = np.asarray(ids).astype(np.int64)
        x = np.asarray(x, dtype=np.float64)
        ok = (ids >= 0) & (ids < self.F) & ~np.isnan(x)
        f = ids[ok]
        np.maximum.at(self.key, f, key_of(x[ok]))
        np.add.at(self.hits, f, 1)
        self.frames[np.unique(f)] += 1
        self.observations += 1
        self.rows_added += int(ok.sum())
        self.rows_ignored += int((~ok).sum())
        return self

    @property
    def peak(self):
        return np.where(self.hits > 0, value_of(self.key), 0.0)

    def faces(self):
        return {"peak": self.peak, "hits": self.hits, "frames": self.frames}

    def stats(self):
        return {"observations": self.observations, "rows_added": self.rows_added, "rows_ignored": self.rows_ignored}


# ------------------------------------------------------------------ regions
def grown(model, mark, grow):
    mark = np.asarray(mark, dtype=bool).copy()
    for _ in range(grow):
        mark = mark | (model.graph.dot(mark.astype(np.int32)) > 0)
    return mark


def regions(model, state, threshold=0.5, min_frames=1, grow=0):
    """labels and the table's columns; area and moment as math.fsum (exact sum, rounded once), with abs_moment =
    fsum |area * centroid| for the bound of the tests."""
    F = model.F
    seed = (state.hits > 0) & (state.peak > threshold) & (state.frames >= min_frames)
    mark = grown(model, seed, grow)
    labels = np.full(F, -1, np.int32)
    idx = np.nonzero(mark)[0]
    R = 0
    if len(idx):
        _, comp = connected_components(model.graph[idx][:, idx], directed=False)
        _, first = np.unique(comp, return_index=True)       # a component's first (lowest) marked face
        rank = np.empty(len(first), np.int64)
        rank[np.argsort(first)] = np.arange(len(first))     # numbered by the lowest face
        labels[idx] = rank[comp]
        R = len(first)
    out = {"labels": labels, "n_regions": R,
           "first_face": np.zeros(R, np.int32), "n_faces": np.zeros(R, np.int32), "n_seed_faces": np.zeros(R, np.int32),
           "max_frames": np.zeros(R, np.int32), "hits": np.zeros(R, np.int64), "area": np.zeros(R), "centroid": np.zeros((R, 3)),
           "moment": np.zeros((R, 3)), "abs_moment": np.zeros((R, 3)), "peak": np.zeros(R), "lo": np.zeros((R, 3)),
           "hi": np.zeros((R, 3))}
    order = np.argsort(labels[idx], kind="stable")
    members = np.split(idx[order], np.cumsum(np.bincount(labels[idx], minlength=R))[:-1]) if R else []
    for r, fs in enumerate(members):
        out["first_face"][r] = fs[0]
        out["n_faces"][r] = len(fs)
        out["n_seed_faces"][r] = seed[fs].sum()
        out["max_frames"][r] = state.frames[fs].max()
        out["hits"][r] = state.hits[fs].sum()
        area = math.fsum(model.area[fs])
        out["area"][r] = area
        with np.errstate(invalid="ignore", over="ignore"):
            terms = model.area[fs, None] * model.centroid[fs]
        for d in range(3):
            out["moment"][r, d] = math.fsum(terms[:, d]) if np.isfinite(terms[:, d]).all() else terms[:, d].sum()
            out["abs_moment"][r, d] = math.fsum(np.abs(terms[:, d])) if np.isfinite(terms[:, d]).all() else np.inf
        hit = fs[state.hits[fs] > 0]
        out["peak"][r] = value_of(state.key[hit].max(keepdims=True))[0]
        out["lo"][r] = value_of(model.lo_key[fs].min(axis=0))
        out["hi"][r] = value_of(model.hi_key[fs].max(axis=0))
        with np.errstate(invalid="ignore", divide="ignore"):
            out["centroid"][r] = out["moment"][r] / area if area > 0 or area != area else np.nan
    return out


# ------------------------------------------------------------------ meshes
def cube():
    v = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])       # index 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # x = 0, 1; y = 0, 1; z = 0, 1
    t = [tri for (a, b, c, d) in quads for tri in ((a, b, c), (a, c, d))]
    return v, np.array(t, dtype=np.uint32)


def unwelded(verts, tris):
    """Every face with vertices of its own: only the weld holds the mesh together."""
    t = np.asarray(tris)
    return np.ascontiguousarray(np.asarray(verts, dtype=np.float64)[t.reshape(-1)]), np.arange(t.size, dtype=np.uint32).reshape(-1, 3)


def torus(W, H, R=40.0, r=15.0, centre=(0.0, 0.0, 0.0)):
    """A W x H grid torus: W H vertices, 2 W H faces."""
    u, v = np.meshgrid(np.arange(W) * 2 * np.pi / W, np.arange(H) * 2 * np.pi / H, indexing="ij")
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    a, b = i * H + j, ((i + 1) % W) * H + j
    c, d = ((i + 1) % W) * H + (j + 1) % H, i * H + (j + 1) % H
    tris = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=2).reshape(-1, 3)
    return verts + np.asarray(centre, dtype=np.float64), tris.astype(np.uint32)


def torus_with_seam(W, H, seed=3):
    """The torus with the ring of vertices at i = 0 duplicated (the faces of the last column of quads use the copies,
    like an OBJ's UV seam) and the triangles in a shuffled order."""
    verts, tris = torus(W, H)
    ring = np.arange(H)                                      # vertices with i = 0
    copies = len(verts) + ring
    verts = np.concatenate([verts, verts[ring]])
    last = np.arange(2 * (W - 1) * H, 2 * W * H)             # faces of the quads with i = W - 1
    t = tris.astype(np.int64)
    sub = t[last]
    sub[sub < H] += W * H                                    # index j -> its copy
    t[last] = sub
    assert set(np.unique(t[last][t[last] >= W * H])) == set(copies)
    perm = np.random.default_rng(seed).permutation(len(t))
    return verts, np.ascontiguousarray(t[perm]).astype(np.uint32)


def two_tori(W, H):
    v1, t1 = torus(W, H)
    v2, t2 = torus(W, H, centre=(200.0, 0.0, 0.0))
    return np.concatenate([v1, v2]), np.concatenate([t1, t2 + np.uint32(len(v1))])


def fin():
    """Three faces on the edge (0, 1): non-manifold, all neighbours of each other."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.5, -1.0, 0.0], [0.5, 0.0, 1.0]])
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.uint32)


def strip(n):
    """n triangles in a row between two rails: a path graph (face f touches f - 1 and f + 1 alone)."""
    k = np.arange(n + 2)
    v = np.stack([0.5 * k, (k % 2).astype(np.float64), 0.01 * np.sin(k)], axis=1)
    f = np.arange(n)
    t = np.stack([f, f + 1, f + 2], axis=1)
    t[1::2] = t[1::2][:, [1, 0, 2]]
    return v, t.astype(np.uint32)


def oddities():
    """The 16-face torus with a zero-area face (three corners on a line), a face with a repeated index, a face on a
    vertex with a NaN, and vertices at -0 / +0 that weld."""
    v, t = torus(4, 2)
    n = len(v)
    extra = np.array([[0.0, 0.0, 50.0], [1.0, 0.0, 50.0], [2.0, 0.0, 50.0],      # n .. n + 2: collinear
                      [np.nan, 1.0, 50.0],                                        # n + 3
                      [-0.0, 5.0, 60.0], [0.0, 5.0, 60.0], [1.0, 5.0, 60.0], [0.0, 6.0, 60.0], [1.0, 6.0, 61.0]])  # n + 4 ..
    faces = np.array([[n, n + 1, n + 2], [n, n + 1, n + 1], [n + 1, n + 2, n + 3],
                      [n + 4, n + 6, n + 7], [n + 5, n + 8, n + 6]], dtype=np.uint32)   # the last two meet on (+-0, 5, 60) - (1, 5, 60)
    return np.concatenate([v, extra]), np.concatenate([t, faces])
