"""Brute-force numpy restatement of the renderer (csrc/pedp_render.hip, DESIGN.md s"Renderer"): every pixel is tested
against every triangle, in float32 with the device code's operation order (no FMA), so that the GPU tests can ask
for bit equality.  Test infrastructure only; slow (F x H x W work per pose), meant for small meshes and images."""
import numpy as np

f32 = np.float32
ONE, ZERO = f32(1.0), f32(0.0)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def pose_records(proj, poses, bbox, H, W):
    """Per pose: clip matrix P . diag(1, -1, -1, 1) . T (16 floats) and the bbox2d window (has, sx, ox, sy, oy)."""
    P = np.asarray(proj, f32).reshape(4, 4)
    T = np.asarray(poses, f32).reshape(-1, 4, 4)
    G = T.copy()
    G[:, 1:3] = -G[:, 1:3]
    M = np.empty_like(G)
    for i in range(4):
        for j in range(4):
            M[:, i, j] = ((P[i, 0] * G[:, 0, j] + P[i, 1] * G[:, 1, j]) + P[i, 2] * G[:, 2, j]) + P[i, 3] * G[:, 3, j]
    win = np.zeros((len(T), 5), f32)
    if bbox is not None:
        bb = np.asarray(bbox, f32).reshape(-1, 4)
        Wf, Hf = f32(W), f32(H)
        l, t, r, b = bb[:, 0], Hf - bb[:, 1], bb[:, 2], Hf - bb[:, 3]
        win[:, 0] = 1
        win[:, 1] = Wf / (r - l)
        win[:, 2] = ((Wf - r) - l) / (r - l)
        win[:, 3] = Hf / (t - b)
        win[:, 4] = ((Hf - t) - b) / (t - b)
    return M, win


def clip_vertices(verts, M, win):
    """V x 4 clip-space vertices of one pose (M 4 x 4, win 5)."""
    v = np.asarray(verts, f32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    rows = [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(4)]
    if win[0] != 0:
        rows[0] = rows[0] * win[1] + rows[3] * win[2]
        rows[1] = rows[1] * win[3] + rows[3] * win[4]
    return np.stack(rows, axis=1).astype(f32)


def _cross(ax, ay, aw, bx, by, bw):
    return ay * bw - aw * by, aw * bx - ax * bw, ax * by - ay * bx


def tri_setup(clip, faces):
    """Edge coefficients (F x 3 x 3, sign-normalised), z (F x 3), w (F x 3) and the mask of triangles kept."""
    faces = np.asarray(faces, np.int64)
    V = len(clip)
    ok = np.all((faces >= 0) & (faces < V), axis=1)
    fi = np.where(faces >= 0, np.minimum(faces, V - 1), 0) if V else faces * 0
    a, b, d = (clip[fi[:, k]] if V else np.zeros((len(faces), 4), f32) for k in range(3))
    for q in (0, 1, 2):  # trivial rejects, every vertex outside one clip plane
        ok &= ~((a[:, q] > a[:, 3]) & (b[:, q] > b[:, 3]) & (d[:, q] > d[:, 3]))
        ok &= ~((a[:, q] < -a[:, 3]) & (b[:, q] < -b[:, 3]) & (d[:, q] < -d[:, 3]))
    ok &= ~((a[:, 3] <= 0) & (b[:, 3] <= 0) & (d[:, 3] <= 0))
    c = np.empty((len(faces), 3, 3), np.float64)  # edge functions in float64 (exact products of float32 inputs)
    a64, b64, d64 = a.astype(np.float64), b.astype(np.float64), d.astype(np.float64)
    for k, (p, q) in enumerate(((b64, d64), (d64, a64), (a64, b64))):
        c[:, k] = np.stack(_cross(p[:, 0], p[:, 1], p[:, 3], q[:, 0], q[:, 1], q[:, 3]), axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        det = (c[:, 0, 0] * a64[:, 0] + c[:, 0, 1] * a64[:, 1]) + c[:, 0, 2] * a64[:, 3]
    ok &= (det != 0) & np.isfinite(det)
    c = np.where((det < 0)[:, None, None], -c, c)
    z = np.stack([a[:, 2], b[:, 2], d[:, 2]], axis=1)
    w = np.stack([a[:, 3], b[:, 3], d[:, 3]], axis=1)
    return c, z, w, ok


def pixel_ndc(i, n):
    return (np.asarray(2 * i + 1, dtype=f32) / f32(n)) - ONE


def cover(c, z, w, px, py):
    """Elementwise coverage test (broadcasting): returns mask, u, v, z/w."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
        e0 = (c[..., 0, 0] * px + c[..., 0, 1] * py) + c[..., 0, 2]
        e1 = (c[..., 1, 0] * px + c[..., 1, 1] * py) + c[..., 1, 2]
        e2 = (c[..., 2, 0] * px + c[..., 2, 1] * py) + c[..., 2, 2]
        S = (e0 + e1) + e2
        m = (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & (S > 0)
        u, v = (e0 / S).astype(f32), (e1 / S).astype(f32)
        t = (ONE - u) - v
        zc = (u * z[..., 0] + v * z[..., 1]) + t * z[..., 2]
        wc = (u * w[..., 0] + v * w[..., 1]) + t * w[..., 2]
        m &= wc > 0
        q = zc / wc
        m &= (q >= -ONE) & (q <= ONE)
    return m, u.astype(f32), v.astype(f32), q.astype(f32)


def _orderable(q):
    b = q.view(np.uint32).astype(np.uint64)
    neg = (b & np.uint64(0x80000000)) != 0
    return np.where(neg, (~b) & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def rasterize_one(clip, faces, H, W):
    """rast (H x W x 4, GL row order): u, v, z/w, triangle id + 1; zero on the background."""
    c, z, w, ok = tri_setup(clip, faces)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = pixel_ndc(cc.reshape(-1), W), pixel_ndc(rr.reshape(-1), H)
    P = H * W
    best = np.full(P, EMPTY, np.uint64)
    idx = np.nonzero(ok)[0]
    step = max(1, (1 << 22) // max(P, 1))
    for s in range(0, len(idx), step):
        t = idx[s:s + step]
        m, u, v, q = cover(c[t][:, None], z[t][:, None], w[t][:, None], px[None], py[None])
        key = np.where(m, (_orderable(q) << np.uint64(32)) | t[:, None].astype(np.uint64), EMPTY)
        best = np.minimum(best, key.min(axis=0))
    rast = np.zeros((P, 4), f32)
    hit = best != EMPTY
    t = (best[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    m, u, v, q = cover(c[t], z[t], w[t], px[hit], py[hit])
    assert m.all()
    rast[hit] = np.stack([u, v, q, (t + 1).astype(f32)], axis=1)
    return rast.reshape(H, W, 4)


def rasterize(pos, faces, H, W):
    return np.stack([rasterize_one(np.asarray(p, f32), faces, H, W) for p in pos]) if len(pos) else np.zeros((0, H, W, 4), f32)


def _lerp(u, v, t, a0, a1, a2):
    return (u * a0 + v * a1) + t * a2


def interpolate(attr, rast, faces):
    """attr V x A or N x V x A -> N x H x W x A.  Zero where the id is not in [1, F] (NaN included; a fractional id
    truncates) and where the triangle names a vertex outside [0, V)."""
    rast = np.asarray(rast, f32)
    N, H, W, _ = rast.shape
    attr = np.asarray(attr, f32)
    V, A = attr.shape[-2], attr.shape[-1]
    out = np.zeros((N, H, W, A), f32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    for n in range(N):
        a = attr[n] if attr.ndim == 3 else attr
        r = rast[n].reshape(-1, 4)
        hit = np.nonzero((r[:, 3] >= 1) & (r[:, 3] <= len(faces)))[0]
        i = faces[r[hit, 3].astype(np.int64) - 1]
        good = np.all((i >= 0) & (i < V), axis=1)
        hit, i = hit[good], i[good]
        u, v = r[hit, 0][:, None], r[hit, 1][:, None]
        out[n].reshape(-1, A)[hit] = _lerp(u, v, (ONE - u) - v, a[i[:, 0]], a[i[:, 1]], a[i[:, 2]])
    return out


def _wrap(f, n):
    m = np.fmod(f, f32(n))
    m = np.where(m < 0, m + f32(n), m)
    i = m.astype(np.int64)
    return np.where((i >= 0) & (i < n), i, 0)


def tex_sample(tex, u, v):
    """tex h x w x C, u, v (P,) -> P x C."""
    th, tw, C = tex.shape
    x, y = u * f32(tw) - f32(0.5), v * f32(th) - f32(0.5)
    good = (np.abs(x) < f32(1e8)) & (np.abs(y) < f32(1e8))
    x, y = np.where(good, x, ZERO), np.where(good, y, ZERO)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    ix0, iy0 = _wrap(x0, tw), _wrap(y0, th)
    ix1, iy1 = np.where(ix0 + 1 == tw, 0, ix0 + 1), np.where(iy0 + 1 == th, 0, iy0 + 1)
    t00, t10, t01, t11 = tex[iy0, ix0], tex[iy0, ix1], tex[iy1, ix0], tex[iy1, ix1]
    a, b = t00 + (t10 - t00) * fx, t01 + (t11 - t01) * fx
    return np.where(good[:, None], a + (b - a) * fy, ZERO).astype(f32)


def texture(tex, uv):
    tex, uv = np.asarray(tex, f32), np.asarray(uv, f32)
    N, H, W, _ = uv.shape
    return np.stack([tex_sample(tex[n if len(tex) > 1 else 0], uv[n, ..., 0].reshape(-1), uv[n, ..., 1].reshape(-1))
                     .reshape(H, W, -1) for n in range(N)])


def _normalize(x):
    n = np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])
    d = np.maximum(n, f32(1e-12))[..., None]
    return (x / d).astype(f32)


def _clip01(x):
    return np.where(x < 0, ZERO, np.where(x > 1, ONE, x)).astype(f32)


def render(verts, faces, vnormals, poses, proj, H, W, out_h, out_w, vcolor=None, uv=None, tex=None, bbox=None,
           get_normal=False, use_light=False, light_dir=(0, 0, 1), light_pos=(0, 0, 0), light_color=None, w_ambient=0.8,
           w_diffuse=0.5):
    """The fused render: (color, depth, normal or None, xyz), rows flipped (output row 0 = GL row out_h - 1)."""
    verts, vnormals = np.asarray(verts, f32), np.asarray(vnormals, f32)
    faces = np.asarray(faces, np.int64)
    poses = np.asarray(poses, f32).reshape(-1, 4, 4)
    N = len(poses)
    M, win = pose_records(proj, poses, bbox, H, W)
    get_normal = get_normal or use_light
    color = np.zeros((N, out_h, out_w, 3), f32)
    depth = np.zeros((N, out_h, out_w), f32)
    normal = np.zeros((N, out_h, out_w, 3), f32) if get_normal else None
    xyz = np.zeros((N, out_h, out_w, 3), f32)
    wa, wd = f32(w_ambient), f32(w_diffuse)
    for n in range(N):
        rast = rasterize_one(clip_vertices(verts, M[n], win[n]), faces, out_h, out_w).reshape(-1, 4)
        hit = rast[:, 3] > 0
        t = rast[hit, 3].astype(np.int64) - 1
        i = faces[t]
        u, v = rast[hit, 0][:, None], rast[hit, 1][:, None]
        bt = (ONE - u) - v
        T = poses[n]
        pc = [((T[None, :3, 0] * verts[i[:, k], 0:1] + T[None, :3, 1] * verts[i[:, k], 1:2]) + T[None, :3, 2] * verts[i[:, k], 2:3])
              + T[None, :3, 3] for k in range(3)]
        nc = [(T[None, :3, 0] * vnormals[i[:, k], 0:1] + T[None, :3, 1] * vnormals[i[:, k], 1:2]) + T[None, :3, 2] * vnormals[i[:, k], 2:3]
              for k in range(3)]
        X = _lerp(u, v, bt, *pc)
        if tex is not None:
            uvv = np.asarray(uv, f32)
            UV = _lerp(u, v, bt, uvv[i[:, 0]], uvv[i[:, 1]], uvv[i[:, 2]])
            col = tex_sample(np.asarray(tex, f32).reshape(np.asarray(tex).shape[-3:]), UV[:, 0], UV[:, 1])
        else:
            vc = np.asarray(vcolor, f32)
            col = _lerp(u, v, bt, vc[i[:, 0]], vc[i[:, 1]], vc[i[:, 2]])
        if use_light:
            dif = []
            for k in range(3):
                nh = _normalize(nc[k])
                if light_dir is not None:
                    ld = np.broadcast_to(-np.asarray(light_dir, f32).reshape(1, 3), nh.shape)
                else:
                    ld = np.asarray(light_pos, f32).reshape(1, 3) - pc[k]
                lh = _normalize(ld)
                dif.append(_clip01((nh[:, 0] * lh[:, 0] + nh[:, 1] * lh[:, 1]) + nh[:, 2] * lh[:, 2])[:, None])
            d = _lerp(u, v, bt, *dif)
            lc = col if light_color is None else np.broadcast_to(np.asarray(light_color, f32).reshape(1, -1), col.shape)
            col = col * wa + (d * lc) * wd
        col = _clip01(col)

        def put(dst, val, k):  # GL row order in, flipped rows out
            gl = np.zeros((out_h * out_w, k), f32)
            gl[hit] = val.reshape(-1, k)
            dst[n] = gl.reshape(dst[n].shape)[::-1]
        put(color, col, 3)
        put(xyz, X, 3)
        put(depth, X[:, 2], 1)
        if get_normal:
            put(normal, _normalize(_lerp(u, v, bt, *nc)), 3)
    return color, depth, normal, xyz
