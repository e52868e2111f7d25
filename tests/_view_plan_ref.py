"""Next-best-view planning restated on the host, in numpy over tests/_coverage_ref.py's classify and
State: a candidate's observation, the merge into a working state, a face's progress, the gain with its sum in s4.17's
block-and-butterfly order (NOT math.fsum: the gains compare bit for bit, so the greedy order is unambiguous), and the
greedy selection."""
import numpy as np

import _coverage_ref as cref

BLOCK = 4096
LANES = np.arange(64)


# ------------------------------------------------------------------ the fixed order of the sums
def wave_sum(x):
    """Lane l adds x[l], x[l + 64], ... one after the other from +0; then the butterfly: in step off = 32 ... 1 every lane
    adds the value of lane l ^ off to its own."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    rows = np.zeros((-(-len(x) // 64) * 64), np.float64)        # padded with +0, which changes no bit of a sum from +0
    rows[:len(x)] = x
    acc = np.zeros(64)
    for row in rows.reshape(-1, 64):
        acc = acc + row
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[LANES ^ off]
    return acc[0]


def ordered_sum(x):
    """Blocks of 4096 consecutive values, a wave_sum each; then one wave_sum of the block sums."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return wave_sum([wave_sum(x[b:b + BLOCK]) for b in range(0, len(x), BLOCK)])


# ------------------------------------------------------------------ candidates and the working state
class Observation:
    """What pedp_coverage_add of one view would add without depth and mask: per face the SEEN pixels, the largest cosine
    key and the bits of the smallest footprint."""

    def __init__(self, F, rec, K, W, H, t_hit, prim_id, min_cos=0.0):
        st = cref.State(F).add(rec, K, W, H, t_hit, prim_id, min_cos=min_cos)
        self.cpix = st.pixels.astype(np.uint32)
        self.ckey = st.key
        self.cfp = st.fp_bits

    def row(self):
        """In the units of pedp_coverage_faces, as pedp_view_plan_candidate reads a row back."""
        import _defect_map_ref as dref

        return {"pixels": self.cpix.astype(np.int64), "best_cos": np.where(self.ckey != 0, dref.value_of(self.ckey), 0.0),
                "min_footprint": np.where(self.cfp == cref.NEVER, np.inf, self.cfp.view(np.float64))}


class Work:
    """The planner's copy of a coverage State's pixels, views, key and fp_bits."""

    def __init__(self, state):
        self.pixels, self.views = state.pixels.copy(), state.views.copy()
        self.key, self.fp_bits = state.key.copy(), state.fp_bits.copy()

    def copy(self):
        return Work(self)

    def merge(self, o):
        """The state pedp_coverage_add of that view would leave."""
        self.pixels += o.cpix.astype(np.int64)
        self.views += (o.cpix > 0).astype(np.int32)
        self.key = np.maximum(self.key, o.ckey)
        self.fp_bits = np.minimum(self.fp_bits, o.cfp)
        return self

    best_cos = cref.State.best_cos
    min_footprint = cref.State.min_footprint
    covered = cref.State.covered


def progress(w, min_views=1, min_pixels=1, min_cos=0.0, max_footprint=np.inf):
    """F int64, 0 ... m with m = max(min_views, 1): m exactly where the face is covered."""
    q = (w.pixels >= min_pixels) & (w.best_cos >= min_cos) & (w.min_footprint <= max_footprint)
    n = np.ones(len(q), np.int64) if min_views <= 0 else np.minimum(w.views.astype(np.int64), min_views)
    return np.where(q, n, 0)


def gain(w, o, area, **criteria):
    """(gain_area, gain_faces) of observation o against working state w."""
    m = max(criteria.get("min_views", 1), 1)
    before, after = progress(w, **criteria), progress(w.copy().merge(o), **criteria)
    delta = after - before
    assert (delta >= 0).all() and not delta[o.cpix == 0].any()
    with np.errstate(invalid="ignore"):
        terms = np.where(delta > 0, (area * delta.astype(np.float64)) / float(m), 0.0)
    return ordered_sum(terms), int(((before < m) & (after == m)).sum())


def score(w, candidates, area, **criteria):
    g = [gain(w, o, area, **criteria) for o in candidates]
    return {"gain_area": np.array([a for a, _ in g], np.float64), "gain_faces": np.array([f for _, f in g], np.int64)}


def totals(w, area, **criteria):
    cov = w.covered(**criteria)
    ca, ta = ordered_sum(np.where(cov, area, 0.0)), ordered_sum(area)
    return {"covered_faces": int(cov.sum()), "covered_area": ca, "total_area": ta, "fraction": ca / ta if ta > 0 else float("nan")}


def select(state, candidates, area, k, min_gain=0.0, **criteria):
    """The greedy selection from coverage State `state`: dict(order, gain_area, gain_faces, the totals of the working state
    afterwards, and that state as "work")."""
    w = Work(state)
    chosen = np.zeros(len(candidates), bool)
    order, areas, faces = [], [], []
    for _ in range(k):
        s = score(w, candidates, area, **criteria)
        best = -1
        for v in range(len(candidates)):
            if not chosen[v] and s["gain_area"][v] > (min_gain if best < 0 else s["gain_area"][best]):
                best = v                                     # `>`: the lowest index among equals, and a NaN never wins
        if best < 0:
            break
        order.append(best)
        areas.append(s["gain_area"][best])
        faces.append(s["gain_faces"][best])
        w.merge(candidates[best])
        chosen[best] = True
    out = {"order": np.array(order, np.int32), "gain_area": np.array(areas, np.float64), "gain_faces": np.array(faces, np.int64), "work": w}
    out.update(totals(w, area, **criteria))
    return out


# ------------------------------------------------------------------ the scenes
def posed_records(verts, tris, T):
    """The records of the model moved by the 4 x 4 T on the host: float64 transform, float32 cast."""
    from _closest_ref import records

    v = np.asarray(verts, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]
    return records(np.ascontiguousarray(v.astype(np.float32)), tris)


def orbit(radius, n_views, centre=(0.0, 0.0, 0.0)):
    """Object-in-camera poses: the inverses of sample_views_icosphere's cameras, moved to `centre`."""
    from pedp_hip.estimator import sample_views_icosphere

    cams = sample_views_icosphere(n_views, radius=radius)
    cams[:, :3, 3] += np.asarray(centre, dtype=np.float64)
    return np.linalg.inv(cams)
