"""numpy restatement of the closest-point contract (include/pedp.h pedp_closest_points): the same
expressions in the same order, float64, every point against every triangle, the minimum with ties to the lowest index."""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)
PAIRS_PER_CHUNK = 1 << 20      # rows x triangles of one table: ~40 float64 temporaries of that size stay below 400 MB


def records(verts, tris):
    """(a, ab, ac, skipped) as tri_setup_kernel stores them: e1 = b - a and e2 = c - a in float32, m = e2 x e1 with each
    component fma(x, y, -(z * w)) in float32; a record whose m is all zero is skipped.  a, ab, ac promoted to float64."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    a = v[t[:, 0]]
    e1 = v[t[:, 1]] - a
    e2 = v[t[:, 2]] - a
    assert e1.dtype == np.float32

    def fms(x, y, z, w):    # float32 fma(x, y, -(float32)(z * w)): the product x y is exact in float64
        with np.errstate(under="ignore", over="ignore", invalid="ignore"):
            return (x.astype(np.float64) * y.astype(np.float64) - (z * w).astype(np.float64)).astype(np.float32)

    m = np.stack([fms(e2[:, 1], e1[:, 2], e2[:, 2], e1[:, 1]), fms(e2[:, 2], e1[:, 0], e2[:, 0], e1[:, 2]),
                  fms(e2[:, 0], e1[:, 1], e2[:, 1], e1[:, 0])], axis=1)
    return a.astype(np.float64), e1.astype(np.float64), e2.astype(np.float64), np.all(m == 0, axis=1)


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def point_triangle(p, a, ab, ac):
    """(v, w, c, r, d2) of points p against triangles (a, ab, ac), broadcast over the leading axes."""
    with np.errstate(all="ignore"):
        ap = p - a
        bp = ap - ab
        cp = ap - ac
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / ((va + vb) + vc)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        v = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, 1.0 - e], vb * den)
        w = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), e], vc * den)
        c = (a + ab * v[..., None]) + ac * w[..., None]
        r = p - c
        dd = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
    return v, w, c, r, dd


def region(p, a, ab, ac):
    """The number (1 .. 7) of the rule that decides (v, w) for one point and one triangle."""
    ap = p - a
    bp = ap - ab
    cp = ap - ac
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [d1 <= 0 and d2 <= 0, d3 >= 0 and d4 <= d3, vc <= 0 and d1 >= 0 and d3 <= 0, d6 >= 0 and d5 <= d6,
             vb <= 0 and d2 >= 0 and d6 <= 0, va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0, True]
    return conds.index(True) + 1


def closest_ref(verts, tris, pts):
    """The five outputs of pedp_closest_points for float32 vertices, triangles and N x 3 float64 points, as a dict with
    Mesh.closest_points' keys, and `unskipped`, the number of triangles that take part."""
    a, ab, ac, skip = records(verts, tris)
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    N, F = len(p), len(a)
    out = {"points": np.full((N, 3), np.nan), "distances": np.full(N, np.nan), "primitive_ids": np.full(N, NONE, np.uint32),
           "primitive_uvs": np.full((N, 2), np.nan), "sides": np.zeros(N, np.int8), "unskipped": int((~skip).sum())}
    finite = np.isfinite(p).all(axis=1)
    out["distances"][finite] = np.inf
    if F == 0:
        return out
    rows = np.nonzero(finite)[0]
    step = max(1, PAIRS_PER_CHUNK // F)
    for i0 in range(0, len(rows), step):
        idx = rows[i0:i0 + step]
        q = p[idx]
        dd = point_triangle(q[:, None, :], a[None], ab[None], ac[None])[4]
        dd = np.where(np.isnan(dd) | skip[None, :], np.inf, dd)
        f = np.argmin(dd, axis=1)                      # the first of equal minima: the lowest index
        hit = dd[np.arange(len(idx)), f] < np.inf
        idx, q, f = idx[hit], q[hit], f[hit]
        v, w, c, r, d2 = point_triangle(q, a[f], ab[f], ac[f])
        x, y = ab[f], ac[f]
        nrm = np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2],
                        x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=1)
        out["points"][idx] = c
        out["distances"][idx] = np.sqrt(d2)
        out["primitive_ids"][idx] = f.astype(np.uint32)
        out["primitive_uvs"][idx] = np.stack([v, w], axis=1)
        out["sides"][idx] = np.sign(dot(r, nrm)).astype(np.int8)
    return out


KEYS = ("points", "distances", "primitive_ids", "primitive_uvs", "sides")


def same_bits(got, ref, keys=KEYS):
    """The first key whose arrays differ in any bit (NaNs compare by their bits' class: both NaN), or None."""
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if g.shape != r.shape or g.dtype != r.dtype:
            return f"{k}: {g.dtype}{g.shape} against {r.dtype}{r.shape}"
        if g.dtype.kind == "f":
            bad = ~((g.view(np.uint64) == r.view(np.uint64)) | (np.isnan(g) & np.isnan(r)))
        else:
            bad = g != r
        if bad.any():
            i = np.argwhere(bad)[0]
            return f"{k}: {int(bad.sum())} differ, first at {tuple(i)}: {g[tuple(i)]!r} against {r[tuple(i)]!r}"
    return None


def torus_surface(u, v):
    """Points of synth.bumpy_torus' surface at the angles u, v (float64, any shape -> ... x 3)."""
    r = 25.0 * (1.0 + 0.15 * np.sin(5.0 * u) * np.cos(3.0 * v))
    R = 60.0
    return np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v) + 0.0 * u], axis=-1)


def coherent_queries(groups=48, seed=0):
    """The queries of the culling condition: `groups` runs of 64 neighbouring surface points with 0.5 mm noise."""
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 0.12, 8)
    out = []
    for _ in range(groups):
        u0 = rng.uniform(0.0, 2.0 * np.pi)
        v0 = rng.uniform(0.0, 2.0 * np.pi)
        u = (u0 + s)[:, None] + 0.0 * s[None, :]          # i outer
        v = (v0 + 1.5 * s)[None, :] + 0.0 * s[:, None]
        out.append(torus_surface(u, v).reshape(64, 3) + rng.normal(0.0, 0.5, (64, 3)))
    return np.ascontiguousarray(np.concatenate(out))
