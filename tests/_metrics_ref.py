"""pedp_pose_errors restated in numpy, operation for operation: float64, every sum in the order
written.  numpy's elementwise float64 +, -, *, /, sqrt are IEEE operations rounded once and numpy never fuses two of them,
so the arrays below hold what the kernel's registers hold.

The order of the mean (it depends on N alone):
    the terms v_0 .. v_{N-1}, padded with +0 to a multiple of CH = 256, in chunks of 256;
    in chunk c, thread t (0 .. 127) adds v[256 c + t] + v[256 c + 128 + t];
    the 64 lanes of a wave are added by halving: a[k] + a[k + 32] for k < 32, then k < 16 with + 16, ... down to + 1;
    the chunk's sum is wave 0's value + wave 1's;
    the sum is ((p_0 + p_1) + p_2) + ... over the chunks, and the mean is that sum / N.
"""
import numpy as np

MT, QPT = 128, 2
CH = MT * QPT          # points of a chunk
TP = 256               # pred points of an LDS tile (the order of a minimum does not matter; the tests straddle it)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def pose_times_sym(P, s):
    """Rows 0 .. 2 of P @ s as ((P_i0 s_0j + P_i1 s_1j) + P_i2 s_2j) + P_i3 s_3j; the bottom row is carried over."""
    P, s = np.asarray(P, np.float64), np.asarray(s, np.float64)
    out = P.copy()
    for i in range(3):
        for j in range(4):
            out[i, j] = ((P[i, 0] * s[0, j] + P[i, 1] * s[1, j]) + P[i, 2] * s[2, j]) + P[i, 3] * s[3, j]
    return out


def transform(M, pts):
    """q_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k -> three arrays."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return [((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3] for k in range(3)]


def mean_in_order(v):
    n = len(v)
    chunks = -(-n // CH)
    a = np.zeros(chunks * CH)
    a[:n] = v
    a = a.reshape(chunks, QPT, MT // 64, 64)
    a = a[:, 0] + a[:, 1]                       # a thread's two terms
    h = 32
    while h:
        a = a[..., :h] + a[..., h:2 * h]        # the lanes by halving
        h //= 2
    p = a[:, 0, 0]
    for w in range(1, MT // 64):
        p = p + a[:, w, 0]                      # the waves in order
    s = p[0]
    for c in range(1, chunks):
        s = s + p[c]                            # the chunks in order
    return s / np.float64(n)


def _one(kind, P, G, pts):
    with np.errstate(all="ignore"):
        a, b = transform(P, pts), transform(G, pts)
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            return np.float64(np.nan)
        if kind == "add":
            dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
            return mean_in_order(np.sqrt((dx * dx + dy * dy) + dz * dz))
        best = np.empty(len(pts))
        for i0 in range(0, len(pts), 512):      # gt points in blocks: every pred point against each
            sl = slice(i0, i0 + 512)
            dx, dy, dz = a[0][None, :] - b[0][sl, None], a[1][None, :] - b[1][sl, None], a[2][None, :] - b[2][sl, None]
            best[sl] = ((dx * dx + dy * dy) + dz * dz).min(axis=1)
        return mean_in_order(np.sqrt(best))


def pose_error(kind, pred, gt, pts, sym=None):
    """The error of one pose: kind 'add' or 'adds'; sym None (nothing is multiplied) or S x 4 x 4."""
    pred, gt, pts = np.asarray(pred, np.float64), np.asarray(gt, np.float64), np.asarray(pts, np.float64)
    if sym is None:
        return _one(kind, pred, gt, pts)
    es = np.array([_one(kind, pose_times_sym(pred, s), gt, pts) for s in np.asarray(sym, np.float64).reshape(-1, 4, 4)])
    return np.float64(np.nan) if np.isnan(es).any() else es.min()


def pose_errors(kind, preds, gts, pts, sym=None):
    gts = np.asarray(gts)
    return np.array([pose_error(kind, p, gts if gts.ndim == 2 else gts[b if len(gts) > 1 else 0], pts, sym)
                     for b, p in enumerate(np.asarray(preds))], np.float64)


def bound(pred, gt, pts, want):
    """The tolerance between two float64 implementations of either error: with u = 2^-53 and
    S = max_i (|x_i| + |y_i| + |z_i|) max|R| + max|t| over both poses, 32 u S + 2 (N + 8) u want."""
    pred, gt, pts = np.asarray(pred, np.float64), np.asarray(gt, np.float64), np.asarray(pts, np.float64)
    u = 2.0 ** -53
    R = max(np.abs(pred[:3, :3]).max(), np.abs(gt[:3, :3]).max())
    t = max(np.abs(pred[:3, 3]).max(), np.abs(gt[:3, 3]).max())
    S = np.abs(pts).sum(axis=1).max() * R + t
    return 32 * u * S + 2 * (len(pts) + 8) * u * abs(float(want))
