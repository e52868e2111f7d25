"""The coverage map restated on the host: one vectorised numpy pass per view for the per-pixel rule and
the per-face state, math.fsum for the area sums, and tests/_defect_map_ref.py's Model, key, growth and labelling for the
regions.  float64, every expression in the contract's order."""
import math

import numpy as np

import _defect_map_ref as dref
from _closest_ref import dot, records

MASKED, MISS, NO_DEPTH, OCCLUDED, BEHIND, GRAZING, SEEN = range(7)
CLASSES = ("masked", "miss", "no_depth", "occluded", "behind", "grazing", "seen")
NEVER = np.uint64(0xFFFFFFFFFFFFFFFF)
Z_MIN = np.float32(0.001)
FACE_KEYS = ("pixels", "views", "best_cos", "min_footprint", "blocked")


# ------------------------------------------------------------------ the camera
def intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def pixel_dirs(K, W, H):
    """N x 3 float64: the direction of every pixel's ray as it was cast (rounded to float32 and widened again)."""
    ys, xs = np.mgrid[0:H, 0:W]
    xn = (xs.reshape(-1).astype(np.float64) - K[0, 2]) / K[0, 0]
    yn = (ys.reshape(-1).astype(np.float64) - K[1, 2]) / K[1, 1]
    length = np.sqrt((xn * xn + yn * yn) + 1.0)
    return np.stack([xn / length, yn / length, 1.0 / length], axis=1).astype(np.float32).astype(np.float64)


def rays6(K, W, H):
    return np.ascontiguousarray(np.hstack([np.zeros((W * H, 3)), pixel_dirs(K, W, H)]).astype(np.float32))


def records64(verts, tris):
    """(a, ab, ac, skipped) without the float32 rounding of a mesh handle's records: for known answers."""
    v = np.asarray(verts, dtype=np.float64)
    t = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    a = v[t[:, 0]]
    return a, v[t[:, 1]] - a, v[t[:, 2]] - a, np.zeros(len(t), bool)


def host_cast(rec, dirs):
    """A brute-force float64 cast of rays from the origin for the tests without a GPU: t_hit N float32 (inf: miss) and
    primitive_ids N uint32 (0xFFFFFFFF: miss), the lowest index among equal distances."""
    a, ab, ac, skip = rec
    d = dirs[:, None, :]
    with np.errstate(all="ignore"):
        p = np.cross(d, ac[None])
        det = (ab[None] * p).sum(-1)
        s = -a[None]
        u = (s * p).sum(-1) / det
        q = np.cross(s, ab[None])
        v = (d * q).sum(-1) / det
        t = (ac[None] * q).sum(-1) / det
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & ~skip[None]
    t = np.where(ok, t, np.inf)
    f = np.argmin(t, axis=1)
    best = t[np.arange(len(dirs)), f]
    return best.astype(np.float32), np.where(np.isfinite(best), f, dref.MISS).astype(np.uint32)


# ------------------------------------------------------------------ the per-pixel rule
def classify(rec, K, W, H, t_hit, prim_id, depth=None, mask=None, depth_scale=1.0, depth_tol=None, min_cos=0.0):
    """dict(status N uint8, face N int64, z_hit, cos, footprint N float64) of one view; rec = records(posed float32
    vertices, triangles).  cos and footprint mean something on the pixels that reach the GRAZING rule alone."""
    a, ab, ac, skip = rec
    F, N = len(a), W * H
    t = np.ascontiguousarray(t_hit, dtype=np.float32).reshape(N)
    ids = np.ascontiguousarray(prim_id).reshape(N).astype(np.int64)
    d = pixel_dirs(K, W, H)
    hit = (ids >= 0) & (ids < F) & np.isfinite(t)
    f = np.where(hit, ids, 0)
    with np.errstate(all="ignore"):
        z_hit = t.astype(np.float64) * d[:, 2]
        if F:
            x, y = ab[f], ac[f]
            c = np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2],
                          x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=1)
            n = c / np.sqrt(dot(c, c))[:, None]
            dp = np.abs(dot(n, d))
            cos = np.where(~skip[f] & (dp > 0.0), np.where(dp < 1.0, dp, 1.0), 0.0)
        else:
            cos = np.zeros(N)
        foot = ((z_hit * z_hit) * d[:, 2]) / ((K[0, 0] * K[1, 1]) * cos)
        status = np.full(N, SEEN, np.uint8)
        status[cos < min_cos] = GRAZING
        if depth is not None:
            if depth_tol is None or not depth_tol >= 0:
                raise ValueError("depth needs depth_tol >= 0")
            dm = np.ascontiguousarray(depth, dtype=np.float32).reshape(N)
            diff = dm.astype(np.float64) * float(depth_scale) - z_hit
            status[diff > depth_tol] = BEHIND
            status[diff < -depth_tol] = OCCLUDED
            status[~(dm >= Z_MIN) | np.isinf(dm)] = NO_DEPTH
    status[~hit] = MISS
    if mask is not None:
        status[np.ascontiguousarray(mask).reshape(N).astype(np.uint8) == 0] = MASKED
    return {"status": status, "face": f, "z_hit": z_hit, "cos": cos, "footprint": foot}


# ------------------------------------------------------------------ the per-face state
class State:
    def __init__(self, F):
        self.F = F
        self.pixels = np.zeros(F, np.int64)
        self.views = np.zeros(F, np.int32)
        self.key = np.zeros(F, np.uint64)               # key_of(best cosine); 0: never
        self.fp_bits = np.full(F, NEVER, np.uint64)     # bits of the smallest footprint; all ones: never
        self.blocked = np.zeros(F, np.int64)
        self.classes = np.zeros(7, np.int64)
        self.n_views = 0
        self.last = None

    def add(self, rec, K, W, H, t_hit, prim_id, **kw):
        c = self.last = classify(rec, K, W, H, t_hit, prim_id, **kw)
        seen, occluded = c["status"] == SEEN, c["status"] == OCCLUDED
        f = c["face"][seen]
        np.add.at(self.pixels, f, 1)
        self.views[np.unique(f)] += 1
        np.maximum.at(self.key, f, dref.key_of(c["cos"][seen]))
        foot = np.ascontiguousarray(c["footprint"][seen])
        ok = ~np.isnan(foot)
        np.minimum.at(self.fp_bits, f[ok], foot[ok].view(np.uint64))
        np.add.at(self.blocked, c["face"][occluded], 1)
        self.classes += np.bincount(c["status"], minlength=7)
        self.n_views += 1
        return self

    @property
    def best_cos(self):
        return np.where(self.key != 0, dref.value_of(self.key), 0.0)

    @property
    def min_footprint(self):
        return np.where(self.fp_bits == NEVER, np.inf, self.fp_bits.view(np.float64))

    def faces(self):
        return {"pixels": self.pixels, "views": self.views, "best_cos": self.best_cos, "min_footprint": self.min_footprint,
                "blocked": self.blocked}

    def stats(self):
        return dict({"views": self.n_views}, **{name: int(self.classes[k]) for k, name in enumerate(CLASSES)})

    def covered(self, min_views=1, min_pixels=1, min_cos=0.0, max_footprint=np.inf):
        return ((self.views >= min_views) & (self.pixels >= min_pixels) & (self.best_cos >= min_cos)
                & (self.min_footprint <= max_footprint))

    def summary(self, model, **criteria):
        cov = self.covered(**criteria)
        ca, ta = math.fsum(model.area[cov]), math.fsum(model.area)
        return {"covered_faces": int(cov.sum()), "faces": self.F, "covered_area": ca, "total_area": ta,
                "fraction": ca / ta if ta > 0 else float("nan")}


# ------------------------------------------------------------------ regions
def regions(model, state, covered=False, grow=0, **criteria):
    """_defect_map_ref.regions on the coverage marking (the covered faces or the uncovered ones), with the three columns
    that come from the per-face state taken from the coverage state: hits = sum of pixels, max_frames = max of views,
    peak = max of best_cos over the faces with pixels (0.0 if none)."""
    mark = state.covered(**criteria) == bool(covered)
    proxy = dref.State(model.F)                         # marked <=> hits 1, peak 1 > 0.5, frames 1 >= 1
    proxy.hits = mark.astype(np.int64)
    proxy.frames = mark.astype(np.int32)
    proxy.key = dref.key_of(np.ones(model.F))
    out = dref.regions(model, proxy, 0.5, 1, grow)
    lab, R = out["labels"], out["n_regions"]
    inside = lab >= 0
    hits, frames, peak = np.zeros(R, np.int64), np.zeros(R, np.int32), np.zeros(R, np.uint64)
    np.add.at(hits, lab[inside], state.pixels[inside])
    np.maximum.at(frames, lab[inside], state.views[inside])
    np.maximum.at(peak, lab[inside], np.where(state.pixels > 0, state.key, np.uint64(0))[inside])
    out["hits"], out["max_frames"] = hits, frames
    out["peak"] = np.where(peak != 0, dref.value_of(peak), 0.0)
    return out
