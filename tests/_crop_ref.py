"""Numpy restatement of the crop contract (csrc/pedp_crop.hip) and a torch float32 restatement of
kornia 0.7.2's warp_perspective, for the crop tests.

The contract: per pose one float64 map from output pixel to grid_sample pixel coordinate, evaluated per pixel in float64
and cast to float32; grid_sample's float32 bilinear (corners nw, ne, sw, se, products then sums, no FMA) or nearest
(round half to even), zeros outside.  numpy's float32 and float64 operations round once each, like the kernels built
with -ffp-contract=off, so the two are bit-equal.
"""
import numpy as np

f32 = np.float32


def inv3(m):
    """Float64 inverse by adjugate / determinant, in the kernel's order; returns (inverse 3 x 3, det)."""
    m = [float(v) for v in np.asarray(m, np.float64).reshape(9)]
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4]
    c10, c11, c12 = m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5]
    c20, c21, c22 = m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]
    det = (m[0] * c00 + m[1] * c10) + m[2] * c20
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.array([c00, c01, c02, c10, c11, c12, c20, c21, c22], np.float64) / np.float64(det)
    return r.reshape(3, 3), det


def make_map(M, H, W, align_corners):
    """warp_perspective's map of one float32 M on an H x W source: (s 3 x 3, bx, by, ok)."""
    Md = np.asarray(M, np.float32).astype(np.float64).reshape(3, 3)
    r, det = inv3(Md)
    ok = bool(np.all(np.isfinite(Md)) and det != 0.0 and np.isfinite(det))
    nx = 2.0 / (1e-14 if W == 1 else float(W - 1))
    ny = 2.0 / (1e-14 if H == 1 else float(H - 1))
    ax = (W - 1) / 2.0 if align_corners else W / 2.0
    ay = (H - 1) / 2.0 if align_corners else H / 2.0
    s = np.empty((3, 3), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(3):
            s[0, j] = ax * (nx * r[0, j] - r[2, j])
            s[1, j] = ay * (ny * r[1, j] - r[2, j])
            s[2, j] = r[2, j]
    return s, (W - 1) / 2.0, (H - 1) / 2.0, ok


def map_coords64(mp, x, y):
    """Float64 grid_sample pixel coordinates of output pixels (x, y) (integer arrays), before the float32 cast."""
    s, bx, by, _ = mp
    xd, yd = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        X = (s[0, 0] * xd + s[0, 1] * yd) + s[0, 2]
        Y = (s[1, 0] * xd + s[1, 1] * yd) + s[1, 2]
        Z = (s[2, 0] * xd + s[2, 1] * yd) + s[2, 2]
        big = np.abs(Z) > 1e-8
        ix = np.where(big, X / np.where(big, Z, 1.0) + bx, X + bx)
        iy = np.where(big, Y / np.where(big, Z, 1.0) + by, Y + by)
    return ix, iy


def map_coords(mp, x, y):
    ix, iy = map_coords64(mp, x, y)
    with np.errstate(over="ignore", invalid="ignore"):
        return ix.astype(np.float32), iy.astype(np.float32)


def nearest_index(ix, iy, H, W):
    """(in-range mask, x index, y index) of grid_sample's nearest sample (round half to even)."""
    xr, yr = np.rint(ix), np.rint(iy)
    with np.errstate(invalid="ignore"):
        ok = (xr >= 0) & (xr <= W - 1) & (yr >= 0) & (yr <= H - 1)
    return ok, np.where(ok, xr, 0).astype(np.int64), np.where(ok, yr, 0).astype(np.int64)


def sample_nearest(img, ix, iy):
    """img C x H x W (any dtype) at float32 coordinates -> C x ... float32, zero outside."""
    C_, H, W = img.shape
    ok, xi, yi = nearest_index(ix, iy, H, W)
    v = img[:, yi, xi].astype(np.float32)
    return np.where(ok[None], v, f32(0))


def sample_bilinear(img, ix, iy):
    """grid_sample bilinear, zeros padding: weights from floor, corners summed nw, ne, sw, se in float32."""
    C_, H, W = img.shape
    with np.errstate(invalid="ignore", over="ignore"):
        x0f, y0f = np.floor(ix), np.floor(iy)
        anyin = (x0f >= -1) & (x0f <= W - 1) & (y0f >= -1) & (y0f <= H - 1)
        x0f = np.where(anyin, x0f, f32(0)).astype(np.float32)
        y0f = np.where(anyin, y0f, f32(0)).astype(np.float32)
        ixs = np.where(anyin, ix, f32(0)).astype(np.float32)
        iys = np.where(anyin, iy, f32(0)).astype(np.float32)
    x1f, y1f = x0f + f32(1), y0f + f32(1)
    w = [(x1f - ixs) * (y1f - iys), (ixs - x0f) * (y1f - iys), (x1f - ixs) * (iys - y0f), (ixs - x0f) * (iys - y0f)]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    corners = [(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)]
    acc = np.zeros((C_,) + np.shape(ix), np.float32)
    for (cx, cy), wk in zip(corners, w):
        inb = anyin & (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
        v = img[:, np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)].astype(np.float32)
        acc = np.where(inb[None], acc + v * wk[None], acc)
    return acc


def warp(src, M, dsize, mode="bilinear", align_corners=True):
    """The contract's warp_perspective: src N x C x H x W (N = B or 1), M B x 3 x 3 -> B x C x h x w float32."""
    src = np.asarray(src)
    M = np.asarray(M, np.float32).reshape(-1, 3, 3)
    B, (h, w) = len(M), dsize
    N, C_, H, W = src.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros((B, C_, h, w), np.float32)
    for b in range(B):
        mp = make_map(M[b], H, W, align_corners)
        if not mp[3]:
            continue
        ix, iy = map_coords(mp, x, y)
        img = src[b if N == B else 0]
        out[b] = sample_nearest(img, ix, iy) if mode == "nearest" else sample_bilinear(img, ix, iy)
    return out


def crop_window(poses, K, radius, out_w, out_h, corner=None):
    """compute_crop_window_tf_batch(method='box_3d') in float32, the kernel's order; K float32; the scales as
    out * float32(1 / extent).  Returns (tf B x 3 x 3, bbox2d B x 4 or None)."""
    P = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    K = np.asarray(K, np.float64).astype(np.float32).reshape(9)
    r = f32(radius)
    t = P[:, :3, 3]
    z0 = f32(0)
    offs = [(z0, z0), (r, z0), (-r, z0), (z0, r), (z0, -r)]
    uv = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for ox, oy in offs:
            X, Y, Z = t[:, 0] + ox, t[:, 1] + oy, t[:, 2] + z0
            u = (K[0] * X + K[1] * Y) + K[2] * Z
            v = (K[3] * X + K[4] * Y) + K[5] * Z
            w_ = (K[6] * X + K[7] * Y) + K[8] * Z
            uv.append((u / w_, v / w_))
        cu, cv = uv[0]
        rad = np.max(np.stack([np.abs(a - cu) for a, _ in uv] + [np.abs(b - cv) for _, b in uv]), axis=0)
        left, right, top, bottom = np.rint(cu - rad), np.rint(cu + rad), np.rint(cv - rad), np.rint(cv + rad)
        # `out_size[0] / (right - left)`: torch divides a number by a tensor as the float32 reciprocal times the number
        s0 = (f32(1) / (right - left)) * f32(out_w)
        s1 = (f32(1) / (bottom - top)) * f32(out_h)
    B = len(P)
    one, zero = np.ones(B, np.float32), np.zeros(B, np.float32)
    nt = [[s0, zero, zero], [zero, s1, zero], [zero, zero, one]]
    tt = [[one, zero, -left], [zero, one, -top], [zero, zero, one]]
    tf = np.empty((B, 3, 3), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            for j in range(3):
                tf[:, i, j] = (nt[i][0] * tt[0][j] + nt[i][1] * tt[1][j]) + nt[i][2] * tt[2][j]
    bbox = None
    if corner is not None:
        bbox = np.empty((B, 4), np.float32)
        cu_, cv_ = float(np.float32(corner[0])), float(np.float32(corner[1]))
        for b in range(B):
            inv, _ = inv3(tf[b])
            bbox[b] = [(inv[0, 0] * 0.0 + inv[0, 1] * 0.0) + inv[0, 2], (inv[1, 0] * 0.0 + inv[1, 1] * 0.0) + inv[1, 2],
                       (inv[0, 0] * cu_ + inv[0, 1] * cv_) + inv[0, 2], (inv[1, 0] * cu_ + inv[1, 1] * cv_) + inv[1, 2]]
    return tf, bbox


def crop_to_ori(tf):
    """The contract's crop_to_oris: float32 of the float64 inverse of each tf_to_crops."""
    return np.stack([inv3(m)[0].astype(np.float32) for m in np.asarray(tf, np.float32).reshape(-1, 3, 3)])


def depth2xyz(depth_b, K):
    """depth2xyzmap_batch's float32 arithmetic on one H x W image, zfar = inf -> H x W x 3."""
    K = np.asarray(K, np.float32).reshape(9)
    H, W = depth_b.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    z = depth_b.astype(np.float32)
    with np.errstate(invalid="ignore"):
        valid = ~((z < f32(0.001)) | (z > f32(np.inf)))
    X = ((u - K[2]) * z) / K[0]
    Y = ((v - K[5]) * z) / K[4]
    out = np.stack([X, Y, z], -1)
    return np.where(valid[..., None], out, f32(0)).astype(np.float32)


def transform_xyz(xyz, t, normalize, z_invalid, diameter):
    """transform_batch on B x 3 x h x w xyz maps: the z test before the translation, x - t, and under normalize_xyz
    x * (1 / (float32(diameter) / 2)) with each channel zeroed where z failed or its own |x| >= 2."""
    xyz = np.asarray(xyz, np.float32)
    zbad = xyz[:, 2:3] < f32(z_invalid)
    out = xyz - np.asarray(t, np.float32).reshape(-1, 3, 1, 1)
    if normalize:
        inv_r = f32(1) / (f32(diameter) / f32(2))
        out = out * inv_r
        out = np.where(zbad | (np.abs(out) >= 2), f32(0), out)
    return out.astype(np.float32)


def scorer_xyzB(depth, tf, K, dsize):
    """The scorer's xyz_mapBs before transform_batch: crop the depth, warp it back to the frame with crop_to_oris,
    back-project, crop again (all nearest, align_corners False) -- the reference's composition on the contract."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    tf = np.asarray(tf, np.float32).reshape(-1, 3, 3)
    dB = warp(depth[None, None], tf, dsize, "nearest", False)
    ori = warp(dB, crop_to_ori(tf), (H, W), "nearest", False)
    xyz = np.stack([depth2xyz(o[0], K) for o in ori]).transpose(0, 3, 1, 2)
    return warp(np.ascontiguousarray(xyz), tf, dsize, "nearest", False)


# ---------------------------------------------------------------- kornia 0.7.2, restated in torch float32

def kornia_warp_perspective(src, M, dsize, mode="bilinear", align_corners=True):
    """kornia.geometry.transform.warp_perspective as kornia 0.7.2 computes it (float32 grid_sample on src's device)."""
    import torch
    import torch.nn.functional as F

    src = torch.as_tensor(src).float()
    dev = src.device
    M = torch.as_tensor(M, device=dev).float()
    M = M.reshape(-1, 3, 3)
    B, (_, _, H, W) = len(M), src.shape
    h, w = dsize

    def norm(hh, ww):
        tr = torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0], [0.0, 0.0, 1.0]], device=dev)
        wd = 1e-14 if ww == 1 else ww - 1.0
        hd = 1e-14 if hh == 1 else hh - 1.0
        tr[0, 0] = tr[0, 0] * 2.0 / wd
        tr[1, 1] = tr[1, 1] * 2.0 / hd
        return tr[None]

    src_norm = norm(H, W)
    A = norm(h, w) @ (M @ torch.linalg.inv(src_norm))
    Ainv = torch.linalg.inv(A)
    xs = (torch.linspace(0, w - 1, w, device=dev) / (w - 1) - 0.5) * 2 if w > 1 else torch.zeros(1, device=dev)
    ys = (torch.linspace(0, h - 1, h, device=dev) / (h - 1) - 0.5) * 2 if h > 1 else torch.zeros(1, device=dev)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    pts = torch.stack([gx, gy, torch.ones_like(gx)], -1).reshape(1, -1, 3).expand(B, -1, -1)
    ph = torch.bmm(pts, Ainv.permute(0, 2, 1))
    z = ph[..., 2:3]
    eps = 1e-8
    scale = torch.where(z.abs() > eps, 1.0 / (z + eps), torch.ones_like(z))
    grid = (ph[..., :2] * scale).reshape(B, h, w, 2)
    return F.grid_sample(src.expand(B, -1, -1, -1), grid, mode=mode, padding_mode="zeros", align_corners=align_corners)
