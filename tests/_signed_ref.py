"""numpy restatement of the signed-distance contract (include/pedp.h pedp_signed_distance) on the record
arithmetic of tests/_closest_ref.py: the closest point and Ericson's rule of the chosen triangle, the angle-weighted
pseudonormal of the closest face, edge or vertex from a dict-based adjacency, and the sign of (p - c) . N.  Beside it, as
an independent yardstick that knows nothing of closest points or features, the generalised winding number."""
import numpy as np

from _closest_ref import closest_ref, dot, point_triangle, records, region

FACE, EDGE, VERTEX, NO_FEATURE = 0, 1, 2, 255
FEATURE_OF_RULE = {1: VERTEX, 2: VERTEX, 4: VERTEX, 3: EDGE, 6: EDGE, 5: EDGE, 7: FACE}
CORNER_OF_RULE = {1: 0, 2: 1, 4: 2}
SLOT_OF_RULE = {3: 0, 6: 1, 5: 2}


# ---------------------------------------------------------------- topology
def weld(verts):
    """w[v]: the lowest index of a vertex at v's position (==: -0 equals +0; a vertex with a NaN welds to nothing)."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    first, w = {}, np.arange(len(v))
    for i, p in enumerate(v):
        if np.isnan(p).any():
            continue
        key = tuple(float(x) + 0.0 for x in p)          # -0.0 + 0.0 is +0.0
        w[i] = first.setdefault(key, i)
    return w


def topology(verts, tris):
    """pedp_solid_info as a dict, with `twin` (3 F: the twin of every edge slot or -1) and `corners` (welded vertex ->
    its corners (face, corner) in that order)."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    w = weld(v)
    wt = w[t] if len(t) else t
    edges, corners = {}, {}
    for f in range(len(t)):
        for k in range(3):
            corners.setdefault(int(wt[f, k]), []).append((f, k))
            a, b = int(wt[f, k]), int(wt[f, (k + 1) % 3])
            if a != b:
                edges.setdefault((min(a, b), max(a, b)), []).append((3 * f + k, a < b))
    twin = np.full(3 * len(t), -1, np.int64)
    boundary = nonmanifold = flipped = 0
    for slots in edges.values():
        if len(slots) == 1:
            boundary += 1
        elif len(slots) > 2:
            nonmanifold += 1
        elif slots[0][1] == slots[1][1]:
            flipped += 1
        else:
            twin[slots[0][0]], twin[slots[1][0]] = slots[1][0], slots[0][0]
    a, b, c = (v[t[:, k]] for k in range(3)) if len(t) else (np.zeros((0, 3)),) * 3
    volume = float(np.sum(dot(a, np.cross(b, c)) / 6.0))
    return {"V": len(v), "F": len(t), "welded_vertices": int((w == np.arange(len(v))).sum()), "edges": len(edges),
            "boundary_edges": boundary, "nonmanifold_edges": nonmanifold, "flipped_edges": flipped,
            "degenerate_faces": int(sum(len({int(x) for x in row}) < 3 for row in wt)),
            "closed": int(boundary == 0 and nonmanifold == 0 and flipped == 0 and len(t) > 0),
            "orientation": int(np.sign(volume)), "volume": volume, "twin": twin, "corners": corners, "weld": w}


# ---------------------------------------------------------------- pseudonormals on the records
def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def unit_normals(ab, ac):
    c = cross(ab, ac)
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / np.sqrt(dot(c, c))[:, None]


def vertex_table(topo, ab, ac, skip, nh):
    """welded vertex -> sum over its corners, in (face, corner) order from 0, of n(face) * atan2(|q x s|, q . s)."""
    table = {}
    for wv, lst in topo["corners"].items():
        N = np.zeros(3)
        for f, k in lst:
            if skip[f] or np.isnan(nh[f, 0]):
                continue
            q, s = ((ab[f], ac[f]), (ac[f] - ab[f], -ab[f]), (-ac[f], ab[f] - ac[f]))[k]
            qs = cross(q, s)
            N = N + nh[f] * np.arctan2(np.sqrt(dot(qs, qs)), dot(q, s))
        table[wv] = N
    return table


def signed_ref(verts, tris, pts, model=None):
    """pedp_signed_distance's outputs for float32 vertices `verts` (the mesh as posed), the triangles and N x 3 float64
    points, as a dict: signed_distances, occupancy, features, normals, and closest_ref's own entries.  `model`: the
    vertices the solid is built from (the topology and the orientation), `verts` when None."""
    t = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    topo = topology(verts if model is None else model, t)
    cl = closest_ref(verts, t, pts)
    a, ab, ac, skip = records(verts, t)
    nh = unit_normals(ab, ac)
    table = vertex_table(topo, ab, ac, skip, nh)
    wt = topo["weld"][t]
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    out = dict(cl)
    out.update(signed_distances=cl["distances"].copy(), occupancy=np.zeros(n, np.int8), features=np.full(n, NO_FEATURE, np.uint8),
               normals=np.full((n, 3), np.nan), rules=np.zeros(n, np.uint8))
    orient = float(topo["orientation"])
    for i in np.nonzero(cl["primitive_ids"] != 0xFFFFFFFF)[0]:
        f = int(cl["primitive_ids"][i])
        rule = region(p[i], a[f], ab[f], ac[f])
        if rule in CORNER_OF_RULE:
            N = table[int(wt[f, CORNER_OF_RULE[rule]])]
        elif rule in SLOT_OF_RULE:
            tw = int(topo["twin"][3 * f + SLOT_OF_RULE[rule]])
            N = nh[f].copy()
            if tw >= 0 and not skip[tw // 3] and not np.isnan(nh[tw // 3, 0]):
                N = N + nh[tw // 3]
        else:
            N = nh[f]
        r = p[i] - cl["points"][i]
        s = dot(r, N) * orient
        d = cl["distances"][i]
        out["rules"][i] = rule
        out["signed_distances"][i] = -d if s < 0 else d
        out["occupancy"][i] = 1 if (s < 0 and d > 0) else 0
        out["features"][i] = FEATURE_OF_RULE[rule]
        with np.errstate(invalid="ignore", divide="ignore"):
            out["normals"][i] = (N / np.sqrt(dot(N, N))) * orient
    return out


def decided(verts, tris, pts):
    """Per point: the best and the second-best triangle's d^2 differ (a tie between two triangles may pick either's rule)."""
    a, ab, ac, skip = records(verts, tris)
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    out = np.ones(len(p), bool)
    if len(a) < 2:
        return out
    for i0 in range(0, len(p), 512):
        dd = point_triangle(p[i0:i0 + 512, None, :], a[None], ab[None], ac[None])[4]
        dd = np.sort(np.where(np.isnan(dd) | skip[None, :], np.inf, dd), axis=1)
        out[i0:i0 + 512] = dd[:, 0] != dd[:, 1]
    return out


# ---------------------------------------------------------------- the yardstick
def winding_number(verts, tris, pts):
    """The generalised winding number of the mesh about every point (Van Oosterom & Strackee: the solid angle of a
    triangle is 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|)), over 4 pi: 1 inside a closed
    mesh whose normals point out, 0 outside.  float64 on the vertices as given; no closest point, no feature."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(p))
    for i0 in range(0, len(p), 1024):
        q = p[i0:i0 + 1024, None, :]
        a, b, c = (v[t[:, k]][None] - q for k in range(3))
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        det = np.einsum("...k,...k->...", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("...k,...k->...", a, b) * lc + np.einsum("...k,...k->...", b, c) * la + \
            np.einsum("...k,...k->...", c, a) * lb
        out[i0:i0 + 1024] = (2.0 * np.arctan2(det, den)).sum(axis=1) / (4.0 * np.pi)
    return out


# ---------------------------------------------------------------- fixture meshes (outward normals)
def _prism(poly, z0=0.0, z1=1.0, cap_tris=None):
    """The prism over a counter-clockwise polygon (n x 2): n side quads of two triangles, two caps by `cap_tris` (index
    triples into the polygon, counter-clockwise; a fan from corner 0 when None)."""
    poly = np.asarray(poly, dtype=np.float64)
    n = len(poly)
    verts = np.concatenate([np.column_stack([poly, np.full(n, z0)]), np.column_stack([poly, np.full(n, z1)])])
    cap = [(0, k, k + 1) for k in range(1, n - 1)] if cap_tris is None else cap_tris
    tris = []
    for k in range(n):
        j = (k + 1) % n
        tris += [(k, j, n + j), (k, n + j, n + k)]
    tris += [(c, b, a) for a, b, c in cap] + [(n + a, n + b, n + c) for a, b, c in cap]
    return verts, np.asarray(tris, dtype=np.uint32)


def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.uint32)


def cube():
    return _prism([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])


def pyramid():
    """A tall pyramid: the apex 4 above the centre of a unit base."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.5, 4.0]])
    t = [(0, 2, 1), (0, 3, 2)] + [(k, (k + 1) % 4, 4) for k in range(4)]
    return v, np.asarray(t, dtype=np.uint32)


WEDGE_LENGTH = 2.0


def wedge():
    """A 20 degree wedge prism: its first two faces lie in the plane y = 0 exactly, and meet the slanted face in the sharp
    edge x = y = 0; the face x = WEDGE_LENGTH closes it."""
    L = WEDGE_LENGTH
    v, t = _prism([[0.0, 0.0], [L, 0.0], [L, L * np.tan(np.radians(20.0))]])
    assert (v[t[:2].reshape(-1), 1] == 0.0).all()
    return v, t


def l_prism():
    poly = [[0.0, 0.0], [2.0, 0.0], [2.0, 1.0], [1.0, 1.0], [1.0, 2.0], [0.0, 2.0]]     # the concave edge is at (1, 1)
    return _prism(poly, cap_tris=[(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)])


def torus(W, H, R=2.0, r=0.7):
    i, j = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    u, v = 2.0 * np.pi * i / W, 2.0 * np.pi * j / H
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)

    def vid(a, b):
        return (a % W) * H + (b % H)

    a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
    tris = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=2).reshape(-1, 3)
    return verts, np.ascontiguousarray(tris, dtype=np.uint32)


def stl_cube():
    """The cube as an STL file holds it: 36 vertices, none shared; one of the copies of a corner has -0.0 for 0.0."""
    v, t = cube()
    verts = v[t.reshape(-1)].copy()
    k = int(np.nonzero(verts[:, 0] == 0.0)[0][3])
    verts[k, 0] = -0.0
    assert np.signbit(verts[k, 0])
    return verts, np.arange(36, dtype=np.uint32).reshape(12, 3)


MESHES = {"tetrahedron": (tetrahedron, 4), "cube": (cube, 12), "pyramid": (pyramid, 6), "wedge": (wedge, 8), "l_prism": (l_prism, 20),
          "torus_12x8": (lambda: torus(12, 8), 192), "torus_24x22": (lambda: torus(24, 22), 1056), "stl_cube": (stl_cube, 12)}
N_QUERIES = 4000
SEED = 7


def fixture(name):
    """(float32 vertices, triangles, N_QUERIES uniform float64 points in the mesh's box enlarged by 0.5)."""
    make, faces = MESHES[name]
    v, t = make()
    assert len(t) == faces
    v32 = np.ascontiguousarray(v, dtype=np.float32)
    rng = np.random.default_rng(SEED + sorted(MESHES).index(name))
    lo, hi = v.min(axis=0) - 0.5, v.max(axis=0) + 0.5
    return v32, t, np.ascontiguousarray(rng.uniform(lo, hi, (N_QUERIES, 3)))


_CACHE = {}


def reference(name):
    """The restatement and the yardstick of a fixture, computed once: (verts32, tris, pts, signed_ref dict, winding)."""
    if name not in _CACHE:
        v32, t, pts = fixture(name)
        ref = signed_ref(v32, t, pts)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        wn = winding_number(v32, t, pts)
        wn.setflags(write=False)
        _CACHE[name] = (v32, t, pts, ref, wn)
    return _CACHE[name]
