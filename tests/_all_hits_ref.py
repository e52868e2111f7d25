"""The all-hits queries' reference, from the oracle alone: the pairs oracle.accepted_pairs accepts, each
with the (t, u, v) oracle.mt_test forms on oracle.tri_setup's records, sorted by (ray, bits of t, triangle).  Counts,
splits and occlusion are derived from that list.  accepted_pairs is single-threaded C over every pair: compute a base
array once per module and `patched` rows only for variants of it."""
import numpy as np


class Hits:
    """ray_ids int64 M, t_hit f32 M, primitive_ids u32 M, primitive_uvs f32 M x 2 in the queries' order, over n rays."""

    def __init__(self, n, ray_ids, t, ids, uv):
        self.n = int(n)
        self.ray_ids = np.asarray(ray_ids, np.int64).reshape(-1)
        self.t_hit = np.asarray(t, np.float32).reshape(-1)
        self.primitive_ids = np.asarray(ids, np.uint32).reshape(-1)
        self.primitive_uvs = np.asarray(uv, np.float32).reshape(-1, 2)

    @property
    def counts(self):
        return np.bincount(self.ray_ids, minlength=self.n).astype(np.int32)

    @property
    def ray_splits(self):
        return np.concatenate([[0], np.cumsum(self.counts, dtype=np.int64)]).astype(np.int64)

    def occluded(self, tnear=0.0, tfar=np.inf):
        """any listed t with tnear <= t <= tfar, compared in float32; a NaN bound holds for nothing"""
        lo, hi = np.float32(tnear), np.float32(tfar)
        with np.errstate(invalid="ignore"):
            inside = (lo <= self.t_hit) & (self.t_hit <= hi)
        return np.bincount(self.ray_ids[inside], minlength=self.n) > 0

    def rows(self, keep):
        """the sub-list of the rays `keep` (sorted indices), renumbered 0 .. len(keep) - 1"""
        keep = np.asarray(keep, np.int64)
        new = np.full(self.n, -1, np.int64)
        new[keep] = np.arange(len(keep))
        sel = new[self.ray_ids] >= 0
        return Hits(len(keep), new[self.ray_ids[sel]], self.t_hit[sel], self.primitive_ids[sel], self.primitive_uvs[sel])


def all_hits(oracle, verts, tris, rays6):
    rays = np.ascontiguousarray(rays6, np.float32).reshape(-1, 6)
    pairs = oracle.accepted_pairs(verts, tris, rays)
    rec = oracle.tri_setup(verts, tris)
    t = np.empty(len(pairs), np.float32)
    uv = np.empty((len(pairs), 2), np.float32)
    for k, (i, f) in enumerate(pairs):
        hit, t[k], uv[k, 0], uv[k, 1] = oracle.mt_test(rays[i, :3], rays[i, 3:], rec[f])
        assert hit
    ray, tri = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.uint32)
    order = np.lexsort((tri, t.view(np.uint32), ray))
    return Hits(len(rays), ray[order], t[order], tri[order], uv[order])


def patched(oracle, verts, tris, base_hits, rays6, changed):
    """The reference of rays6, which differs from base_hits' rays in the rows `changed` only: those rows recomputed."""
    rays = np.ascontiguousarray(rays6, np.float32).reshape(-1, 6)
    changed = np.unique(np.asarray(changed, np.int64))
    assert len(rays) == base_hits.n
    fresh = all_hits(oracle, verts, tris, rays[changed])
    keep = ~np.isin(base_hits.ray_ids, changed)
    ray = np.concatenate([base_hits.ray_ids[keep], changed[fresh.ray_ids]])
    t = np.concatenate([base_hits.t_hit[keep], fresh.t_hit])
    ids = np.concatenate([base_hits.primitive_ids[keep], fresh.primitive_ids])
    uv = np.concatenate([base_hits.primitive_uvs[keep], fresh.primitive_uvs])
    order = np.lexsort((ids, t.view(np.uint32), ray))
    return Hits(len(rays), ray[order], t[order], ids[order], uv[order])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_list(got, ref, what=""):
    """a list_intersections dict against a Hits: every array, bit for bit"""
    assert same_bits(got["ray_splits"], ref.ray_splits), f"{what}: ray_splits"
    assert same_bits(got["ray_ids"], ref.ray_ids), f"{what}: ray_ids"
    assert same_bits(got["primitive_ids"], ref.primitive_ids), f"{what}: primitive_ids"
    assert same_bits(got["t_hit"], ref.t_hit), f"{what}: t_hit"
    assert same_bits(got["primitive_uvs"], ref.primitive_uvs), f"{what}: primitive_uvs"
    assert got["geometry_ids"].dtype == np.uint32 and not got["geometry_ids"].any() and len(got["geometry_ids"]) == len(ref.t_hit)
