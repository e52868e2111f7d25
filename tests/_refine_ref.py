"""A numpy restatement of pedp_mesh_refine's contract (include/pedp.h), the meshes and single-triangle
cases its tests share, and the checks of a refined closed mesh.

    refine(v, t, max_edge)         vectorised per round; the new vertices' order comes from np.unique on the 64-bit keys
    refine_loop(v, t, max_edge)    the same contract as plain loops over faces, for tiny meshes
Both return (vertices V x 3 float64, triangles F x 3 uint32, parent_face F int32, rounds).  numpy's elementwise
operations neither contract nor reassociate, so every expression below is evaluated as written.
"""
import numpy as np

MAX_ROUNDS = 64
NXT = [1, 2, 0]


def weld(v):
    """w[i] = the lowest index of a vertex at v[i]'s position, compared with == (-0 equals +0)."""
    _, inv = np.unique(v + 0.0, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    low = np.full(inv.max() + 1 if len(inv) else 0, len(v), np.int64)
    np.minimum.at(low, inv, np.arange(len(v)))
    return low[inv]


def len2(a, b):
    d = b - a
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _check(v, t, max_edge):
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(t).astype(np.int64).reshape(-1, 3)
    if not (max_edge > 0 and np.isfinite(max_edge)):
        raise ValueError("max_edge must be a positive finite number")
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle index is outside the vertices")
    if not np.isfinite(v).all():
        raise ValueError("a vertex has a non-finite coordinate")
    return v, t


def _rot(c, r):
    return np.take_along_axis(c, (r[:, None] + np.arange(3)[None, :]) % 3, axis=1)


def refine_round(v, t, pf, w, limit2):
    """One round on (v, t int64, pf, w); None when no edge is long."""
    p = v[t]
    is_long = len2(p, p[:, NXT]) > limit2                                  # F x 3: edge k = (c_k, c_(k+1)%3)
    if not is_long.any():
        return None
    wa, wb = w[t], w[t[:, NXT]]
    key = (np.minimum(wa, wb).astype(np.uint64) << np.uint64(32)) | np.maximum(wa, wb).astype(np.uint64)
    _, first, inv = np.unique(key[is_long], return_index=True, return_inverse=True)
    V = len(v)
    mid = np.full(t.shape, -1, np.int64)
    mid[is_long] = V + inv.reshape(-1)
    new_v = 0.5 * (p[is_long][first] + p[:, NXT][is_long][first])
    v2 = np.concatenate([v, new_v])
    w2 = np.concatenate([w, np.arange(V, V + len(new_v))])
    n = is_long.sum(axis=1)
    off = np.concatenate([[0], np.cumsum(1 + n)])
    out = np.full((off[-1], 3), -1, np.int64)
    pf2 = np.repeat(pf, 1 + n)

    def put(sel, k, a, b, c):
        out[off[:-1][sel] + k] = np.stack([a, b, c], axis=1)

    s = n == 0
    put(s, 0, t[s, 0], t[s, 1], t[s, 2])
    s = n == 1
    r = np.argmax(is_long[s], axis=1)                                      # rotated so that the long edge is edge 0
    c, m = _rot(t[s], r), _rot(mid[s], r)
    put(s, 0, c[:, 0], m[:, 0], c[:, 2])
    put(s, 1, m[:, 0], c[:, 1], c[:, 2])
    s = n == 2
    r = (np.argmin(is_long[s], axis=1) + 1) % 3                            # rotated so that the short edge is edge 2
    c, m = _rot(t[s], r), _rot(mid[s], r)
    m0, m1 = m[:, 0], m[:, 1]
    near = len2(v2[m0], v2[c[:, 2]]) <= len2(v2[m1], v2[c[:, 0]])
    put(s, 0, m0, c[:, 1], m1)
    put(s, 1, c[:, 0], m0, np.where(near, c[:, 2], m1))
    put(s, 2, np.where(near, m0, c[:, 0]), m1, c[:, 2])
    s = n == 3
    c, m = t[s], mid[s]
    put(s, 0, c[:, 0], m[:, 0], m[:, 2])
    put(s, 1, m[:, 0], c[:, 1], m[:, 1])
    put(s, 2, m[:, 2], m[:, 1], c[:, 2])
    put(s, 3, m[:, 0], m[:, 1], m[:, 2])
    return v2, out, pf2, w2


def refine(v, t, max_edge, max_faces=1 << 24):
    v, t = _check(v, t, max_edge)
    w = weld(v)
    pf = np.arange(len(t), dtype=np.int32)
    limit2 = np.float64(max_edge) * np.float64(max_edge)
    rounds = 0
    while True:
        step = refine_round(v, t, pf, w, limit2)
        if step is None:
            return v, t.astype(np.uint32), pf, rounds
        if rounds == MAX_ROUNDS or len(step[1]) > max_faces:
            raise ValueError(f"{len(step[1])} faces in round {rounds + 1}")
        v, t, pf, w = step
        rounds += 1


def refine_loop(v, t, max_edge):
    """The contract as plain loops; for tiny meshes."""
    v, t = _check(v, t, max_edge)
    v = [tuple(float(x) for x in row) for row in v]
    t = [tuple(int(i) for i in row) for row in t]
    w = []
    for i, p in enumerate(v):
        w.append(next(j for j in range(i + 1) if v[j] == p))
    pf = list(range(len(t)))
    limit2 = float(max_edge) * float(max_edge)

    def l2(a, b):
        dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
        return (dx * dx + dy * dy) + dz * dz

    rounds = 0
    while True:
        flags, keys = [], {}
        for c in t:
            fl = []
            for k in range(3):
                a, b = c[k], c[(k + 1) % 3]
                fl.append(l2(v[a], v[b]) > limit2)
                if fl[-1]:
                    keys.setdefault((min(w[a], w[b]), max(w[a], w[b])), (a, b))
            flags.append(fl)
        if not keys:
            break
        V = len(v)
        ids = {}
        for q in sorted(keys):
            a, b = keys[q]
            ids[q] = len(v)
            v.append(tuple(0.5 * (v[a][d] + v[b][d]) for d in range(3)))
        w.extend(range(V, len(v)))
        t2, pf2 = [], []
        for c, fl, parent in zip(t, flags, pf):
            m = [ids[(min(w[c[k]], w[c[(k + 1) % 3]]), max(w[c[k]], w[c[(k + 1) % 3]]))] if fl[k] else None for k in range(3)]
            n = sum(fl)
            if n == 0:
                kids = [c]
            elif n == 1:
                r = fl.index(True)
                c0, c1, c2 = c[r], c[(r + 1) % 3], c[(r + 2) % 3]
                kids = [(c0, m[r], c2), (m[r], c1, c2)]
            elif n == 2:
                r = (fl.index(False) + 1) % 3
                c0, c1, c2, m0, m1 = c[r], c[(r + 1) % 3], c[(r + 2) % 3], m[r], m[(r + 1) % 3]
                kids = [(m0, c1, m1)]
                if l2(v[m0], v[c2]) <= l2(v[m1], v[c0]):
                    kids += [(c0, m0, c2), (m0, m1, c2)]
                else:
                    kids += [(c0, m0, m1), (c0, m1, c2)]
            else:
                kids = [(c[0], m[0], m[2]), (m[0], c[1], m[1]), (m[2], m[1], c[2]), (m[0], m[1], m[2])]
            t2 += kids
            pf2 += [parent] * len(kids)
        t, pf = t2, pf2
        rounds += 1
        assert rounds <= MAX_ROUNDS
    return (np.array(v, np.float64).reshape(-1, 3), np.array(t, np.uint32).reshape(-1, 3), np.array(pf, np.int32), rounds)


# ---------------------------------------------------------------- meshes

def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * 0.7
    t = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.uint32)
    return v, t


def cube(lo=0.0, hi=1.0):
    """The cube [lo, hi]^3: 8 vertices, 12 triangles, normals out.  Faces 2 s and 2 s + 1 are side s; side 5 is z = hi."""
    v = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], np.float64)
    t = np.array([[0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3],
                  [0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6]], np.uint32)
    return v, t


def icosphere(subdivisions, radius=1.0):
    """20 * 4^subdivisions faces on the sphere, shared vertices, normals out."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        cache, t2 = {}, []

        def mid(a, b):
            q = (min(a, b), max(a, b))
            if q not in cache:
                p = v[a] + v[b]
                cache[q] = len(v)
                v.append(p / np.linalg.norm(p))
            return cache[q]

        for a, b, c in t:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            t2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = t2
    return np.array(v, np.float64) * radius, np.array(t, np.uint32)


def split_vertices(v, t, faces):
    """The mesh with the corners of `faces` given vertices of their own (duplicates at the same positions), as an OBJ
    export with split normals has them along a crease."""
    v, t = [tuple(p) for p in v], np.array(t, np.int64)
    for f in faces:
        for k in range(3):
            v.append(v[t[f, k]])
            t[f, k] = len(v) - 1
    return np.array(v, np.float64), t.astype(np.uint32)


# ---------------------------------------------------------------- the four templates on one triangle, by hand
def single_triangle_cases():
    """(name, vertices, triangles, max_edge, expected vertices, expected triangles): one round each, written by hand."""
    cases = []
    A, B, C = (0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (0.75, 0.5, 0.0)        # AB long; AC = BC = sqrt(0.8125) short
    cases.append(("none", [A, (0.5, 0.0, 0.0), (0.25, 0.5, 0.0)], [(0, 1, 2)], 1.0, [A, (0.5, 0.0, 0.0), (0.25, 0.5, 0.0)], [(0, 1, 2)]))
    for k, tri in enumerate([(0, 1, 2), (2, 0, 1), (1, 2, 0)]):           # the long edge (0, 1) as edge k
        cases.append((f"one-edge{k}", [A, B, C], [tri], 1.0, [A, B, C, (0.75, 0.0, 0.0)], [(0, 3, 2), (3, 1, 2)]))
    # two long edges (0, 1), (1, 2); the short one (2, 0) has length 1 = max_edge exactly: not long
    P0, P2 = (-0.5, 0.0, 0.0), (0.5, 0.0, 0.0)
    for name, apex, m0, m1, rest in [
            ("tie", (0.0, 1.0, 0.0), (-0.25, 0.5, 0.0), (0.25, 0.5, 0.0), [(0, 3, 2), (3, 4, 2)]),          # |m0 c2|^2 == |m1 c0|^2: <=
            ("near", (0.25, 1.0, 0.0), (-0.125, 0.5, 0.0), (0.375, 0.5, 0.0), [(0, 3, 2), (3, 4, 2)]),      # 0.640625 < 1.015625
            ("far", (-0.25, 1.0, 0.0), (-0.375, 0.5, 0.0), (0.125, 0.5, 0.0), [(0, 3, 4), (0, 4, 2)])]:     # 1.015625 > 0.640625
        for k, tri in enumerate([(0, 1, 2), (1, 2, 0), (2, 0, 1)]):       # the short edge (2, 0) as edge 2, 1, 0
            cases.append((f"two-{name}-short{(2 - k) % 3}", [P0, apex, P2], [tri], 1.0, [P0, apex, P2, m0, m1], [(3, 1, 4)] + rest))
    # three long edges: the midpoints in key order (0, 1) -> 3, (0, 2) -> 4, (1, 2) -> 5
    Q = [(0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (0.75, 1.25, 0.0)]
    mids = [(0.75, 0.0, 0.0), (0.375, 0.625, 0.0), (1.125, 0.625, 0.0)]
    cases.append(("three-rot0", Q, [(0, 1, 2)], 1.0, Q + mids, [(0, 3, 4), (3, 1, 5), (4, 5, 2), (3, 5, 4)]))
    cases.append(("three-rot1", Q, [(1, 2, 0)], 1.0, Q + mids, [(1, 5, 3), (5, 2, 4), (3, 4, 0), (5, 4, 3)]))
    cases.append(("three-rot2", Q, [(2, 0, 1)], 1.0, Q + mids, [(2, 4, 5), (4, 0, 3), (5, 3, 1), (4, 3, 5)]))
    return [(n, np.array(v, np.float64), np.array(t, np.uint32), e, np.array(ev, np.float64), np.array(et, np.uint32))
            for n, v, t, e, ev, et in cases]


# ---------------------------------------------------------------- checks of a refined mesh
def longest_edge(v, t):
    p = v[np.asarray(t, np.int64)]
    return float(np.sqrt(len2(p, p[:, NXT]).max()))


def face_areas(v, t):
    p = v[np.asarray(t, np.int64)]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def signed_volume(v, t):
    p = v[np.asarray(t, np.int64)]
    return float(np.sum(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2]))) / 6.0)


def edge_pairing(v, t):
    """(edges with other than two faces, two-face edges run through in the same direction) under the weld."""
    wt = weld(v)[np.asarray(t, np.int64)]
    a, b = wt.reshape(-1), wt[:, NXT].reshape(-1)
    keep = a != b
    a, b = a[keep], b[keep]
    key = np.minimum(a, b) * (len(v) + 1) + np.maximum(a, b)
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    direction = np.zeros(len(uniq), np.int64)
    np.add.at(direction, inv.reshape(-1), np.where(a < b, 1, -1))
    return int((cnt != 2).sum()), int(((cnt == 2) & (direction != 0)).sum())


def plane_distance_ulps(v0, t0, v, t, pf):
    """The largest distance of a refined face's corner from the plane of its CAD face, in units of ulp(max |coordinate|);
    formed in extended precision so that the measurement adds nothing of its own."""
    L = np.longdouble
    p = v0.astype(L)[np.asarray(t0, np.int64)][pf]                         # the CAD face of every refined face
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n = n / np.sqrt((n * n).sum(axis=1))[:, None]
    q = v.astype(L)[np.asarray(t, np.int64)]
    d = np.abs(((q - p[:, :1]) * n[:, None, :]).sum(axis=2))
    return float(d.max() / L(np.spacing(np.abs(v0).max())))
