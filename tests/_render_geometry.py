"""Scenes whose renders follow from float64 geometry, and the checks that hold a render to them.

The renderer's contract says where every output pixel looks: output row i, column j is the ray through
camera pixel (j + 0.5, i + 0.5), or (umin + (j + 0.5)(umax - umin) / w, vmin + (i + 0.5)(vmax - vmin) / h) under a
bbox2d window.  With attributes that are affine functions of the model position, every covered pixel's colour and
normal then follow from its xyz, and for a plane the covered set follows from the projected outline.  These checks cost
O(pixels), so they run at the refiner's sizes; they do not share arithmetic with the restatement tests/_render_ref.py.
Each check also measures two wrong conventions (screen-space interpolation, pixel centres at integers) at the same
pixels, so that a scene too gentle to tell them apart fails instead of passing.
"""
import numpy as np

RAY_TOL = 2e-3      # px: xyz projects onto its pixel centre
PLANE_TOL = 1e-6    # of the depth: xyz lies on the quad's plane
ATTR_TOL = 1e-5     # colour, normal, sampled texture
OUTLINE = 1e-3      # px: coverage is not judged this close to the quad's projected outline
MARGIN = 100.0      # a wrong convention must miss a tolerance by this factor ...
MISS_FRAC = 0.10    # ... on at least this fraction of the quad's pixels

# 480 x 640 camera with fx != fy and an off-centre principal point
K_FRAME = np.array([[520.0, 0.0, 321.3], [0.0, 500.0, 238.7], [0.0, 0.0, 1.0]])


def grazing_quad(tilt_deg=10.0):
    """Two triangles of one plane whose normal is 90 - tilt_deg degrees from the view axis, in the camera frame of the
    identity pose: depth runs from 0.2 m (near edge, image row ~470 of K_FRAME) to 3 m (far edge, row ~172)."""
    a = np.tan(np.deg2rad(tilt_deg))

    def y(z):
        return 0.0925 - (z - 0.2) * a

    v = np.array([[-0.1, y(0.2), 0.2], [0.1, y(0.2), 0.2], [0.6, y(3.0), 3.0], [-0.6, y(3.0), 3.0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def quad_poses(n, seed):
    """Rotations of up to 3 degrees about a pivot 1 m in front of the camera and shifts of up to 1 cm: every vertex
    stays in front (z >= 0.15), the tilt stays within 75-85 degrees of the view axis."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 4, 4), np.float32)
    pivot = np.array([0.0, 0.0, 1.0])
    for i in range(n):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = np.deg2rad(rng.uniform(0, 3))
        kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = pivot - R @ pivot + rng.uniform(-0.01, 0.01, 3)
        out[i] = T
    return out


def affine_field(verts, lo, hi, seed, dims=3):
    """(A, b) of float64 with A p + b inside [lo, hi] per channel over the convex hull of `verts` (the extremes of an
    affine function lie at vertices); the values of each channel reach lo and hi."""
    rng = np.random.default_rng(seed)
    p = np.asarray(verts, np.float64)
    A = rng.normal(size=(dims, 3))
    val = p @ A.T
    lo_v, hi_v = val.min(0), val.max(0)
    s = (np.asarray(hi, np.float64) - lo) / (hi_v - lo_v)
    return A * s[:, None], lo - lo_v * s


def normal_field(verts, seed):
    """(A_n, b_n): a field of non-unit normals, |A_n p + b_n| >= 0.5 over the hull."""
    rng = np.random.default_rng(seed)
    p = np.asarray(verts, np.float64)
    c = p.mean(0)
    ext = np.abs(p - c).max()
    A = rng.normal(size=(3, 3)) * (0.15 / ext)
    b = np.array([0.3, -0.4, 1.0]) - A @ c
    return A, b


def ramp_texture(th, tw, const=0.3):
    """texel (i, j) = ((j + 0.5) / tw, (i + 0.5) / th, const): bilinear sampling returns (u, v, const) wherever none of
    the four taps wraps."""
    ii, jj = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
    return np.stack([(jj + 0.5) / tw, (ii + 0.5) / th, np.full((th, tw), const)], -1).astype(np.float32)


def vertex_values(verts, field):
    A, b = field
    return (np.asarray(verts, np.float64) @ A.T + b).astype(np.float32)


def pixel_centres(h, w, bbox=None, half=0.5):
    """Camera pixel coordinates (u, v) that output pixel (i, j) looks through (h x w each); `half` is the centre offset
    (0.5 in the contract; 0 gives the integer convention)."""
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64) + half, np.arange(h, dtype=np.float64) + half)
    if bbox is None:
        return jj, ii
    umin, vmin, umax, vmax = (float(x) for x in np.asarray(bbox, np.float32))
    return umin + jj * (umax - umin) / w, vmin + ii * (vmax - vmin) / h


def _project(K, X):
    z = X[..., 2]
    return (K[0, 0] * X[..., 0] + K[0, 1] * X[..., 1]) / z + K[0, 2], K[1, 1] * X[..., 1] / z + K[1, 2]


def _edge_dist(a, b, qu, qv):
    """Signed distance (px) of points q from the line a -> b, positive on its left."""
    d = b - a
    return (d[0] * (qv - a[1]) - d[1] * (qu - a[0])) / np.hypot(d[0], d[1])


def _bary2(P, qu, qv):
    """2-D barycentrics of q in triangle P (3 x 2)."""
    (x0, y0), (x1, y1), (x2, y2) = P
    det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    l1 = ((qu - x0) * (y2 - y0) - (x2 - x0) * (qv - y0)) / det
    l2 = ((x1 - x0) * (qv - y0) - (qu - x0) * (y1 - y0)) / det
    return 1 - l1 - l2, l1, l2


def check_pose(maps, T, K, verts, faces, color_field, normal_field_=None, uv_field=None, tex_const=None, bbox=None,
               quad=False):
    """Hold one pose's render to float64 geometry.  maps: (color h x w x 3, depth h x w, normal h x w x 3 or None,
    xyz h x w x 3), rows in image order.  Returns a dict of measurements; raises AssertionError where a check fails."""
    color, depth, normal, xyz = (None if m is None else np.asarray(m) for m in maps)
    h, w = depth.shape
    T = np.asarray(T, np.float32).astype(np.float64)
    R, t = T[:3, :3], T[:3, 3]
    st = {}
    assert np.array_equal(depth.view(np.uint32), np.ascontiguousarray(xyz[..., 2]).view(np.uint32)), "depth != xyz.z"
    cov = depth != 0
    bg = ~cov
    for name, m in (("color", color), ("normal", normal), ("xyz", xyz)):
        if m is not None:
            assert not m[bg].any(), f"{name}: {int((m[bg] != 0).any(-1).sum())} background pixels are not zero"
    st["covered"] = int(cov.sum())
    qu, qv = pixel_centres(h, w, bbox)
    X = xyz[cov].astype(np.float64)
    pu, pv = _project(K, X)
    res = np.hypot(pu - qu[cov], pv - qv[cov])
    st["ray_max"] = float(res.max()) if res.size else 0.0
    assert st["ray_max"] <= RAY_TOL, f"xyz off its pixel's ray by {st['ray_max']:.3g} px"
    p = (X - t) @ R                                   # T^-1 xyz
    A, b = color_field
    if uv_field is None:
        want_c = p @ A.T + b
    else:
        Au, bu = uv_field
        uv = p @ Au.T + bu
        want_c = np.concatenate([uv, np.full((len(uv), 1), tex_const)], 1)
    err_c = np.abs(color[cov] - want_c)
    st["color_max"] = float(err_c.max()) if err_c.size else 0.0
    assert st["color_max"] <= ATTR_TOL, f"colour off the affine field by {st['color_max']:.3g}"
    if normal is not None and normal_field_ is not None:
        An, bn = normal_field_
        n_w = (p @ An.T + bn) @ R.T
        n_w /= np.linalg.norm(n_w, axis=1, keepdims=True)
        err_n = np.abs(normal[cov] - n_w)
        st["normal_max"] = float(err_n.max()) if err_n.size else 0.0
        assert st["normal_max"] <= ATTR_TOL, f"normal off the affine field by {st['normal_max']:.3g}"
    if not quad:
        return st

    # the plane, the covered set and the two wrong conventions
    Vc = np.asarray(verts, np.float32).astype(np.float64) @ R.T + t      # camera-space vertices
    nrm = np.cross(Vc[1] - Vc[0], Vc[2] - Vc[0])
    nrm /= np.linalg.norm(nrm)
    plane = np.abs(X @ nrm - Vc[0] @ nrm) / X[:, 2]
    st["plane_max"] = float(plane.max()) if plane.size else 0.0
    assert st["plane_max"] <= PLANE_TOL, f"xyz off the plane by {st['plane_max']:.3g} of the depth"
    P2 = np.stack(_project(K, Vc), 1)                                      # projected outline (convex: all z > 0)
    e1, e2 = P2[1] - P2[0], P2[2] - P2[0]
    sgn = np.sign(e1[0] * e2[1] - e1[1] * e2[0])
    d = np.stack([sgn * _edge_dist(P2[k], P2[(k + 1) % 4], qu, qv) for k in range(4)])
    inside = (d >= 0).all(0)
    clear = (np.abs(d) >= OUTLINE).all(0)
    wrong = (inside != cov) & clear
    st["coverage_mismatch"] = int(wrong.sum())
    st["near_outline"] = int((~clear).sum())
    assert not wrong.any(), f"{int(wrong.sum())} pixels covered unlike the float64 ray test ({int((cov & ~inside & clear).sum())} " \
                            f"extra, {int((inside & ~cov & clear).sum())} missing)"
    sel = cov & clear
    # screen-space interpolation: 2-D barycentrics in whichever triangle holds the pixel centre
    fc = np.asarray(faces, np.int64)
    aff = np.full(qu[sel].shape + (3,), np.nan)
    col_aff = np.full(qu[sel].shape + (3,), np.nan)
    vcol = vertex_values(verts, color_field).astype(np.float64) if uv_field is None else None
    for f in fc:
        lam = _bary2(P2[f], qu[sel], qv[sel])
        inn = np.isnan(aff[:, 0]) & (np.min(lam, axis=0) >= -1e-9)
        L = np.stack(lam, 1)[inn]
        aff[inn] = L @ Vc[f]
        if vcol is not None:
            col_aff[inn] = L @ vcol[f]
    au, av = _project(K, aff)
    ray_aff = np.hypot(au - qu[sel], av - qv[sel])
    iu, iv = pixel_centres(h, w, bbox, half=0.0)
    pu_s, pv_s = _project(K, xyz[sel].astype(np.float64))
    ray_int = np.hypot(pu_s - iu[sel], pv_s - iv[sel])
    alts = {"affine_ray": ray_aff / RAY_TOL, "integer_centre_ray": ray_int / RAY_TOL}
    if vcol is not None:
        alts["affine_color"] = np.abs(col_aff - want_c[sel[cov]]).max(1) / ATTR_TOL
    for k, ratio in alts.items():
        ratio = np.nan_to_num(ratio, nan=np.inf)
        frac = float((ratio >= MARGIN).mean()) if ratio.size else 0.0
        st[k + "_frac"] = frac
        st[k + "_median_ratio"] = float(np.median(ratio)) if ratio.size else 0.0
        assert frac >= MISS_FRAC, f"{k}: the wrong convention misses the tolerance {MARGIN:g}x on only {frac:.1%} of pixels"
    return st


def summarize(stats):
    """Worst case of every measurement over poses (max of errors; min of covered counts, sensitivity fractions and
    ratios)."""
    out = {}
    for s in stats:
        for k, v in s.items():
            worst = min if (k == "covered" or k.endswith("_frac") or k.endswith("_ratio")) else max
            out[k] = v if k not in out else worst(out[k], v)
    return out
