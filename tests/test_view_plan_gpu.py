"""Next-best-view planning on the device (csrc/pedp_viewplan.hip) against its restatement
(tests/_view_plan_ref.py): bit for bit, the gains' floating-point sums included (the restatement sums in the contract's
order)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _coverage_ref as cref
import _defect_map_ref as dref
import _view_plan_ref as ref
from pedp_hip import view_plan  # noqa: F401  (without the feature every test here fails at import)

pytestmark = pytest.mark.gpu

QUAD = (np.array([[-10.0, -10.0, 0.0], [10.0, -10.0, 0.0], [10.0, 10.0, 0.0], [-10.0, 10.0, 0.0]]),
        np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))
MESHES = {
    "quad": lambda: QUAD,                                   # F = 2
    "torus1022": lambda: dref.torus(73, 7),
    "torus4096": lambda: dref.torus(64, 32),                # one full block of the sums
    "torus4098": lambda: dref.torus(683, 3),                # a block and two faces
    "torus8194": lambda: dref.torus(241, 17),               # two blocks and two faces
}
CRITERIA = [{}, dict(min_cos=0.5), dict(min_pixels=2), dict(min_views=2), dict(max_footprint=40.0)]


@functools.lru_cache(maxsize=None)
def model(name):
    return dref.Model(*MESHES[name]())


def camera(W, H, f):
    return cref.intrinsics(f, f, (W - 1) / 2, (H - 1) / 2)


def look_at(eye, target=(0.0, 0.0, 0.0)):
    """The object pose of a camera at `eye` (model frame) that looks at `target`."""
    eye = np.asarray(eye, dtype=np.float64)
    z = np.asarray(target, dtype=np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x = x / np.linalg.norm(x) if x.any() else np.array([1.0, 0.0, 0.0])
    cam = np.eye(4)
    cam[:3, 0], cam[:3, 1], cam[:3, 2], cam[:3, 3] = x, np.cross(z, x), z, eye
    return np.linalg.inv(cam)


ORBIT = ref.orbit(200.0, 12)                                # the 42 poses of the greedy scene
OFF_CENTRE = ref.orbit(200.0, 12, (3.0, -2.0, 5.0))         # the same cameras looking past the torus's centre: no two gains tie
# an orbit thinned out and two cameras close to the outer equator at u = 0, where the first and the last faces meet
EDGE_POSES = np.concatenate([ORBIT[::4], [look_at((150.0, -8.0, 20.0), (50.0, 0.0, 0.0)), look_at((140.0, 10.0, -30.0), (50.0, 0.0, 0.0))]])
SMALL = (32, 24, 60.0)                                      # W, H, focal length
_refs = {}


def reference(ctx, name, poses, W, H, f, min_cos=0.0):
    """(views, candidates) of the restatement: per pose the records as the device poses them, the device's cast of the
    camera's rays, and the observation the restatement makes of it.  Computed once per scene and never changed."""
    from pedp_hip import _lib

    key = (name, W, H, f, np.ascontiguousarray(poses).tobytes(), min_cos)
    if key not in _refs:
        m, K = model(name), camera(W, H, f)
        mesh = _lib.Mesh(ctx, m.verts, m.tris, posable=True)
        rays = _lib.RaySet(ctx, cref.rays6(K, W, H))
        seen, views, cands = {}, [], []
        for T in poses:
            k = T.tobytes()
            if k not in seen:
                mesh.set_pose(T)
                rec = cref.records(mesh.posed_vertices(T).astype(np.float32), m.tris)
                hit = mesh.cast_rayset(rays, want_uv=False)
                view = (rec, hit["t_hit"], hit["primitive_ids"])
                seen[k] = (view, ref.Observation(m.F, rec, K, W, H, view[1], view[2], min_cos=min_cos))
            views.append(seen[k][0])
            cands.append(seen[k][1])
        rays.close()
        mesh.close()
        _refs[key] = (views, cands)
    return _refs[key]


class Scene:
    """A CoverageMap, a ViewPlanner over it with `poses` as candidates, a posable mesh for real views, the restatement."""

    def __init__(self, ctx, name, poses, W, H, f, min_cos=0.0, capacity=None, ref_ctx=None):
        from pedp_hip import CoverageMap, ViewPlanner, _lib

        self.m, self.K, self.W, self.H, self.poses = model(name), camera(W, H, f), W, H, np.ascontiguousarray(poses)
        self.views, self.cands = reference(ref_ctx or ctx, name, self.poses, W, H, f, min_cos)
        self.cov = CoverageMap((self.m.verts, self.m.tris), ctx)
        self.mesh = _lib.Mesh(ctx, self.m.verts, self.m.tris, posable=True)
        self.planner = ViewPlanner(self.cov, (self.m.verts, self.m.tris), self.K, (H, W), min_cos=min_cos,
                                   capacity=len(poses) if capacity is None else capacity)
        self.state = cref.State(self.m.F)
        self.min_cos = min_cos

    def add_all(self):
        assert self.planner.add_candidates(self.poses) == list(range(len(self.poses)))
        return self

    def take(self, v, cov=None):
        """A real view at pose v on the coverage map (and on the restatement's state)."""
        (cov or self.cov).add_view(self.mesh.set_pose(self.poses[v]), self.K, (self.H, self.W), min_cos=self.min_cos)
        if cov is None:
            rec, t, ids = self.views[v]
            self.state.add(rec, self.K, self.W, self.H, t, ids, min_cos=self.min_cos)

    def close(self):
        for h in (self.planner, self.mesh, self.cov):
            h.close()


@pytest.fixture
def scene(ctx):
    made = []

    def make(name, poses, W=SMALL[0], H=SMALL[1], f=SMALL[2], **kw):
        made.append(Scene(ctx, name, poses, W, H, f, **kw))
        return made[-1]

    yield make
    for s in made:
        s.close()


def same_gains(got, want):
    assert got["gain_area"].dtype == np.float64 and dref.same_bits(got["gain_area"], want["gain_area"])
    assert got["gain_faces"].dtype == np.int64 and np.array_equal(got["gain_faces"], want["gain_faces"])


def same_select(got, want):
    assert got["order"].dtype == np.int32 and np.array_equal(got["order"], want["order"]), (got["order"], want["order"])
    same_gains(got, want)
    assert got["covered_faces"] == want["covered_faces"]
    for k in ("covered_area", "total_area", "fraction"):
        assert float(got[k]).hex() == float(want[k]).hex(), k


def same_row(got, want):
    for k in ("pixels", "best_cos", "min_footprint"):
        assert got[k].dtype == want[k].dtype and dref.same_bits(got[k], want[k]), k


def same_faces(got, want):
    for k in cref.FACE_KEYS:
        assert got[k].dtype == want[k].dtype and dref.same_bits(got[k], want[k]), k


# ------------------------------------------------------------------ the C ABI on casts made elsewhere
class RawPlan:
    """pedp_view_plan_* on a coverage map's handle, for casts that are poked or lie in device memory."""

    def __init__(self, cov, capacity):
        from pedp_hip import _lib

        self.lib, self.F, self.h = _lib.load(), cov.F, C.c_void_p()
        _lib.check(self.lib.pedp_view_plan_create(cov._h, capacity, C.byref(self.h)), "pedp_view_plan_create")

    def observe(self, mesh, K, W, H, t, ids, min_cos=0.0, mem=0):
        from pedp_hip import _lib
        from pedp_hip._bridge import ptr

        cam, index = _lib.Pinhole(K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H), C.c_int64(-1)
        rc = self.lib.pedp_view_plan_observe(self.h, mesh._h, C.byref(cam), ptr(t), ptr(ids), min_cos, mem, C.byref(index))
        return rc, index.value

    def candidate(self, v):
        from pedp_hip import _lib

        out = {"pixels": np.empty(self.F, np.int64), "best_cos": np.empty(self.F, np.float64), "min_footprint": np.empty(self.F, np.float64)}
        rc = self.lib.pedp_view_plan_candidate(self.h, v, _lib.HOST, *[_lib._ptr(out[k]) for k in ("pixels", "best_cos", "min_footprint")])
        return rc, out

    def close(self):
        self.lib.pedp_view_plan_destroy(self.h)


def poked(t, ids, F, seed):
    """The cast with rows that take no part put inside the runs: ids >= F, the miss id, NaN and infinite t."""
    t, ids = t.copy().reshape(-1), ids.copy().reshape(-1)
    n = len(t)
    if n >= 63:
        rng = np.random.default_rng(seed)
        where = rng.choice(n, 4 * (n // 16), replace=False).reshape(4, -1)
        ids[where[0]] = rng.integers(F, 2 ** 32 - 1, where.shape[1])
        ids[where[1]] = dref.MISS
        t[where[2]] = np.nan
        t[where[3]] = rng.choice([np.inf, -np.inf], where.shape[1])
    return t, ids


@pytest.mark.parametrize("name", ["quad", "torus1022"])
@pytest.mark.parametrize("W,H", [(1, 1), (63, 1), (64, 1), (65, 1), (257, 1), (241, 17)])
def test_observation_rows(ctx, name, W, H):
    """The two-triangle quad fills every frame: runs cross the wave and block boundaries and every atomic is contended.
    The 1022-face torus is a long way off: most faces are under a pixel, so there are next to no runs."""
    from pedp_hip import CoverageMap, _lib

    m, K = model(name), camera(W, H, 300.0)
    tilt = np.array([[1.0, 0, 0], [0, np.cos(0.6), -np.sin(0.6)], [0, np.sin(0.6), np.cos(0.6)]])
    v = m.verts + [0.0, 0.0, 4.0] if name == "quad" else m.verts @ tilt.T + [0.0, 0.0, 1500.0]
    v = np.ascontiguousarray(v.astype(np.float32))
    rec = cref.records(v, m.tris)
    mesh = _lib.Mesh(ctx, v, m.tris)
    hit = mesh.cast_rays(cref.rays6(K, W, H), want_uv=False)
    t0, ids0 = hit["t_hit"], hit["primitive_ids"]
    if name == "quad":
        assert np.isfinite(t0).all()
    elif W * H > 4000:
        on = ids0[np.isfinite(t0)]
        assert len(on) > 100 and len(np.unique(on)) > 0.5 * len(on)
    cov = CoverageMap((m.verts, m.tris), ctx)
    plan = RawPlan(cov, 3)
    casts = [(t0, ids0, 0.0), poked(t0, ids0, m.F, W) + (0.0,), (t0, ids0, 0.9995)]
    for k, (t, ids, min_cos) in enumerate(casts):
        assert plan.observe(mesh, K, W, H, t, ids, min_cos) == (0, k)
    for k, (t, ids, min_cos) in enumerate(casts):                # read back after all three: a row is its own view's alone
        want = ref.Observation(m.F, rec, K, W, H, t, ids, min_cos=min_cos)
        rc, got = plan.candidate(k)
        assert rc == 0
        same_row(got, want.row())
        if name == "quad" and k == 0:
            assert got["pixels"].sum() == W * H
    assert plan.observe(mesh, K, W, H, t0, ids0)[0] == -1 and b"full" in plan.lib.pedp_last_error()
    assert plan.candidate(3)[0] == -1 and plan.candidate(-1)[0] == -1
    assert not cov.faces()["pixels"].any() and cov.stats()["views"] == 0
    for h in (plan, cov, mesh):
        h.close()


# ------------------------------------------------------------------ the gains
@pytest.mark.parametrize("name", list(MESHES))
def test_score_at_the_block_edges(scene, name):
    """F = 2, 1022, 4096, 4098, 8194: under, at and over one and two blocks of the sums; the candidates see the faces on
    both sides of every block's edge."""
    big = name not in ("quad", "torus1022")
    poses = EDGE_POSES if name != "quad" else ref.orbit(40.0, 12)[::3]
    s = scene(name, poses, *((64, 48, 120.0) if big else SMALL)).add_all()
    F = s.m.F
    seen = np.zeros(F, bool)
    for v, o in enumerate(s.cands):
        same_row(s.planner.candidate(v), o.row())
        seen |= o.cpix > 0
    assert seen[:64].any() and seen[-64:].any()
    if big:                                                                   # faces on both sides of every block's edge
        assert seen[4032:4096].any() and (F == 4096 or seen[4096:4160].any()) and (F < 8192 or (seen[8128:8192].any() and seen[8192:].any()))
    for history in ([], [1], [1, 3, 12]):
        for v in history[s.state.n_views:]:
            s.take(v)
        s.planner.reset()
        for criteria in CRITERIA:
            want = ref.score(ref.Work(s.state), s.cands, s.m.area, **criteria)
            same_gains(s.planner.score(**criteria), want)
            same_gains(s.planner.score(**criteria), want)                     # the same bits on every call
        assert name == "quad" or ref.score(ref.Work(s.state), s.cands, s.m.area)["gain_faces"].max() > 10
    same_faces(s.cov.faces(), s.state.faces())


def test_gain_faces_is_what_a_real_view_newly_covers(ctx, scene):
    """Against a second CoverageMap that replays the history and takes the candidate's view for real."""
    from pedp_hip import CoverageMap

    s = scene("torus1022", ORBIT).add_all()
    other = CoverageMap(s.cov.defect_map)
    criteria = [c for c in CRITERIA if "min_views" not in c]

    def covered(f, min_views=1, min_pixels=1, min_cos=0.0, max_footprint=np.inf):
        return (f["views"] >= min_views) & (f["pixels"] >= min_pixels) & (f["best_cos"] >= min_cos) & (f["min_footprint"] <= max_footprint)

    history = []
    for more in ([], [19], [24, 40]):
        for v in more:
            s.take(v)
        history += more
        s.planner.reset()
        before = s.cov.faces()
        got = [s.planner.score(**c) for c in criteria]
        for v in range(len(s.poses)):
            other.clear()
            for h in history + [v]:
                s.take(h, other)
            after = other.faces()
            for c, g in zip(criteria, got):
                newly = covered(after, **c) & ~covered(before, **c)
                assert g["gain_faces"][v] == newly.sum(), (history, c, v)
        assert sum(int(g["gain_faces"].sum()) for g in got) > 0
    other.close()


# ------------------------------------------------------------------ the greedy selection
@pytest.mark.parametrize("criteria", CRITERIA, ids=lambda c: "-".join(c) or "default")
def test_select_on_the_torus(scene, criteria):
    s = scene("torus1022", ORBIT).add_all()
    got = s.planner.select(12, **criteria)
    want = ref.select(s.state, s.cands, s.m.area, 12, **criteria)
    same_select(got, want)
    assert len(got["order"]) >= 3 and len(set(got["order"])) == len(got["order"])
    if not criteria:
        assert list(got["order"]) == [19, 24, 40, 15, 10, 35, 30, 14, 33, 6, 25, 22] and got["covered_faces"] == 1018
        fresh = ref.score(ref.Work(s.state), s.cands, s.m.area)["gain_area"]
        assert int(got["order"][2]) not in np.argsort(-fresh, kind="stable")[:6]                # greedy, not top-k
    same_select(s.planner.select(12, **criteria), want)                       # a selection starts over: the same bits
    # from a map that has taken views, and a min_gain between two rounds' gains
    s.take(int(got["order"][1]))
    later = ref.select(s.state, s.cands, s.m.area, 12, **criteria)
    same_select(s.planner.select(12, **criteria), later)
    cut = float(later["gain_area"][3])
    stopped = s.planner.select(12, min_gain=cut, **criteria)
    same_select(stopped, ref.select(s.state, s.cands, s.m.area, 12, min_gain=cut, **criteria))
    assert 0 < len(stopped["order"]) <= 3


@pytest.mark.parametrize("V", [1, 2, 64, 65, 130])
def test_select_among_v_candidates(scene, V):
    """One wave looks at 64 candidates at a time: V on both sides of that, the poses repeated, and above 64 the best
    pose of the fresh map (19) as the last candidate alone."""
    idx = (np.arange(V) * 5 + 2) % 42
    if V > 64:
        idx[idx == 19] = 0
        idx[V - 1] = 19
    poses = ORBIT[idx]
    s = scene("torus1022", poses).add_all()
    assert s.planner.n == V
    for criteria in ({}, dict(min_views=2)):
        for k in ((0, 6, V + 5) if V <= 2 else (0, 9)):                        # k > V: no more rounds than candidates
            got, want = s.planner.select(k, **criteria), ref.select(s.state, s.cands, s.m.area, k, **criteria)
            same_select(got, want)
            assert len(got["order"]) <= min(k, V)
        same_gains(s.planner.score(**criteria), ref.score(want["work"], s.cands, s.m.area, **criteria))   # w as the rounds left it
    one = s.planner.select(min(V, 20))                                        # min_views = 1: a copy is never chosen
    chosen = [poses[v].tobytes() for v in one["order"]]
    assert len(set(chosen)) == len(chosen) and (V <= 64 or one["order"][0] == V - 1)


def test_order_of_the_candidates_clear_reset_and_commit(scene):
    s = scene("torus1022", OFF_CENTRE).add_all()
    fresh = s.planner.score()
    want = ref.score(ref.Work(s.state), s.cands, s.m.area)
    same_gains(fresh, want)
    assert len(np.unique(want["gain_area"])) == len(want["gain_area"])        # no ties: the choice cannot hang on the order
    picked = s.planner.select(8)
    same_select(picked, ref.select(s.state, s.cands, s.m.area, 8))
    # another order: the gains permuted, the same poses chosen
    perm = np.random.default_rng(5).permutation(len(s.poses))
    s.planner.clear()
    assert s.planner.n == 0 and len(s.planner.score()["gain_area"]) == 0 and len(s.planner.select(3)["order"]) == 0
    assert s.planner.add_candidates(s.poses[perm]) == list(range(len(perm)))
    s.planner.reset()
    shuffled = s.planner.score()
    assert dref.same_bits(shuffled["gain_area"], fresh["gain_area"][perm]) and np.array_equal(shuffled["gain_faces"], fresh["gain_faces"][perm])
    again = s.planner.select(8)
    assert np.array_equal(perm[again["order"]], picked["order"]) and dref.same_bits(again["gain_area"], picked["gain_area"])
    # clear and re-add: the rows and the gains as at first
    s.planner.clear()
    s.planner.add_candidates(s.poses[:5])
    s.planner.add_candidates(s.poses[5:])
    s.planner.reset()
    same_gains(s.planner.score(), fresh)
    same_row(s.planner.candidate(7), s.cands[7].row())
    # reset after the map took a real view; without it the working state is still the old one
    s.take(int(picked["order"][0]))
    same_gains(s.planner.score(), fresh)
    s.planner.reset()
    after = ref.score(ref.Work(s.state), s.cands, s.m.area)
    same_gains(s.planner.score(), after)
    assert after["gain_faces"][picked["order"][0]] == 0 and not dref.same_bits(after["gain_area"], fresh["gain_area"])
    # commit + score is the next greedy round
    two = s.planner.select(2, min_views=2)
    s.planner.reset()
    s.planner.commit(int(two["order"][0]))
    w = ref.Work(s.state).merge(s.cands[two["order"][0]])
    round_two = s.planner.score(min_views=2)
    same_gains(round_two, ref.score(w, s.cands, s.m.area, min_views=2))
    rest = [v for v in range(len(s.poses)) if v != two["order"][0]]
    best = rest[int(np.argmax(round_two["gain_area"][rest]))]
    assert best == two["order"][1] and round_two["gain_area"][best] == two["gain_area"][1] and round_two["gain_faces"][best] == two["gain_faces"][1]


def test_the_coverage_map_is_not_touched(ctx, scene):
    from pedp_hip import CoverageMap

    s = scene("torus1022", ORBIT)
    s.take(5)
    faces, stats, summary = s.cov.faces(), s.cov.stats(), s.cov.summary()
    s.add_all()
    s.planner.score(min_cos=0.5)
    s.planner.select(6)
    s.planner.commit(3)
    s.planner.select(4, min_views=2)
    s.planner.clear()
    same_faces(s.cov.faces(), faces)
    assert s.cov.stats() == stats and s.cov.summary() == summary
    same_faces(faces, s.state.faces())
    s.take(17)                                                                # a view after planning ...
    plain = CoverageMap(s.cov.defect_map)
    s.take(5, plain)
    s.take(17, plain)                                                         # ... and the same two views without
    same_faces(s.cov.faces(), plain.faces())
    assert s.cov.stats() == plain.stats()
    same_faces(s.cov.faces(), s.state.faces())
    plain.close()


# ------------------------------------------------------------------ memory, streams and handles
def test_host_memory_device_memory_and_a_side_stream(ctx, scene):
    import torch
    from pedp_hip import _lib

    s = scene("torus1022", ORBIT).add_all()
    s.take(19)
    s.planner.reset()
    host, lib, h = s.planner.score(min_cos=0.5), _lib.load(), s.planner._h
    same_gains(host, ref.score(ref.Work(s.state), s.cands, s.m.area, min_cos=0.5))
    crit = _lib.CoverageCriteria(1, 1, 0.5, float("inf"))
    area, faces = torch.empty(42, dtype=torch.float64, device="cuda"), torch.empty(42, dtype=torch.int64, device="cuda")
    row = [torch.empty(s.m.F, dtype=d, device="cuda") for d in (torch.int64, torch.float64, torch.float64)]
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.pedp_view_plan_score(h, C.byref(crit), _lib.DEVICE, vp(area), vp(faces)) == 0
    assert lib.pedp_view_plan_candidate(h, 19, _lib.DEVICE, *[vp(r) for r in row]) == 0
    ctx.synchronize()
    same_gains({"gain_area": area.cpu().numpy(), "gain_faces": faces.cpu().numpy()}, host)
    same_row(dict(zip(("pixels", "best_cos", "min_footprint"), [r.cpu().numpy() for r in row])), s.cands[19].row())
    only = np.empty(42, np.int64)                                             # the pointers are nullable
    assert lib.pedp_view_plan_score(h, C.byref(crit), _lib.HOST, None, _lib._ptr(only)) == 0 and np.array_equal(only, host["gain_faces"])
    spare = np.empty(42, np.float64)
    assert lib.pedp_view_plan_score(h, None, _lib.HOST, _lib._ptr(spare), None) == 0 and (spare >= 0).all()
    assert lib.pedp_view_plan_score(h, None, 7, None, _lib._ptr(only)) == -1 and b"mem" in lib.pedp_last_error()
    n = C.c_int64(-1)
    assert lib.pedp_view_plan_select(h, None, 3, 0.0, None, None, None, C.byref(n), None) == 0 and n.value == 3
    assert lib.pedp_view_plan_select(h, None, -1, 0.0, None, None, None, C.byref(n), None) == -1 and n.value == 0
    assert lib.pedp_view_plan_commit(h, 42) == -1 and lib.pedp_view_plan_commit(h, -1) == -1
    assert lib.pedp_view_plan_create(s.cov._h, 0, C.byref(C.c_void_p())) == -1 and b"capacity" in lib.pedp_last_error()
    # a context on a side stream, which the planner shares with torch: nothing waits, the same bits
    side = torch.cuda.Stream()
    sctx = _lib.Context(0, stream=side.cuda_stream)
    with torch.cuda.stream(side):
        on_side = Scene(sctx, "torus1022", ORBIT, *SMALL, ref_ctx=ctx).add_all()
        on_side.take(19)
        got = on_side.planner.select(5, min_cos=0.5)
    same_select(got, ref.select(s.state, s.cands, s.m.area, 5, min_cos=0.5))
    same_select(s.planner.select(5, min_cos=0.5), got)
    raw = RawPlan(on_side.cov, 1)
    assert raw.observe(s.mesh, s.K, s.W, s.H, s.views[0][1], s.views[0][2])[0] == -1 and b"another context" in lib.pedp_last_error()
    raw.close()
    on_side.close()
    sctx.close()


def test_a_full_plan_and_closed_handles(scene):
    from pedp_hip import CoverageMap, ViewPlanner, _lib

    s = scene("torus1022", ORBIT[:4], capacity=5)
    s.planner.add_candidates(ORBIT[:3])
    with pytest.raises(_lib.PedpError, match="full"):
        s.planner.add_candidates(ORBIT[3:6])
    assert s.planner.n == 3 and s.planner.add_candidates(ORBIT[3]) == [3]
    same_gains(s.planner.score(), ref.score(ref.Work(s.state), s.cands, s.m.area))
    with pytest.raises(_lib.PedpError, match="faces"):
        ViewPlanner(s.cov, dref.torus(73, 14), s.K, (s.H, s.W))
    cov = CoverageMap(s.cov.defect_map)
    planner = ViewPlanner(cov, (s.m.verts, s.m.tris), s.K, (s.H, s.W), capacity=3)
    planner.add_candidates(ORBIT[:2])
    cov.close()
    for call in (lambda: planner.add_candidates(ORBIT[0]), lambda: planner.candidate(0), planner.clear, planner.reset,
                 lambda: planner.commit(0), planner.score, lambda: planner.select(1)):
        with pytest.raises(_lib.PedpError, match="coverage map is closed"):
            call()
    planner.close()
    with pytest.raises(_lib.PedpError, match="view planner is closed"):
        planner.score()
    with pytest.raises(_lib.PedpError, match="closed"):
        ViewPlanner(cov, (s.m.verts, s.m.tris), s.K, (s.H, s.W))


def tiny_view(ctx):
    """A coverage map, the posed mesh and the cast of synth's tiny frame on `ctx`, with the restatement's observation."""
    from pedp_hip import CoverageMap, _lib, synth

    f = synth.Frame("tiny")
    W, H = f.width, f.height
    K = cref.intrinsics(f.f, f.f, f.cx, f.cy)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    hit = mesh.cast_rays(cref.rays6(K, W, H), want_uv=False)
    t, ids = hit["t_hit"].reshape(H, W), hit["primitive_ids"].reshape(H, W)
    cov = CoverageMap((f.verts.astype(np.float64), f.tris), ctx)
    want = ref.Observation(cov.F, cref.records(f.verts_posed, f.tris), K, W, H, t, ids, min_cos=0.1)
    return f, cov, mesh, K, t, ids, want


def test_device_observe_while_a_registration_is_pending(ctx):
    """pedp_view_plan_observe with PEDP_DEVICE, _reset, _commit and a device-memory _score only enqueue: a pending
    registration's result is unchanged.  The calls that wait on the stream are refused."""
    import torch
    from pedp_hip import _lib

    f, cov, mesh, K, t, ids, want = tiny_view(ctx)
    plan = RawPlan(cov, 2)
    scene_pts = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene_pts), _lib.Cloud(ctx, f.model_points, f.normals)
    icp = dict(max_iteration=6, relative_fitness=-1, relative_rmse=-1)
    one = _lib.icp(ctx, src, tgt, 10.0, f.icp_init(), want_corr=True, **icp)
    d_t, d_ids = torch.from_numpy(t).cuda(), torch.from_numpy(ids.view(np.int32)).cuda()
    d_area, d_faces = torch.empty(2, dtype=torch.float64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lib, n = plan.lib, C.c_int64()
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    _lib.icp_begin(ctx, src, tgt, 10.0, f.icp_init(), **icp)
    try:
        assert plan.observe(mesh, K, f.width, f.height, d_t, d_ids, 0.1, _lib.DEVICE) == (0, 0)
        assert lib.pedp_view_plan_reset(plan.h) == 0 and lib.pedp_view_plan_commit(plan.h, 0) == 0 and lib.pedp_view_plan_reset(plan.h) == 0
        assert lib.pedp_view_plan_score(plan.h, None, _lib.DEVICE, vp(d_area), vp(d_faces)) == 0
        assert plan.observe(mesh, K, f.width, f.height, t, ids, 0.1, _lib.HOST)[0] == -1 and b"pending" in lib.pedp_last_error()
        assert plan.candidate(0)[0] == -1
        assert lib.pedp_view_plan_score(plan.h, None, _lib.HOST, None, _lib._ptr(np.empty(2, np.int64))) == -1
        assert lib.pedp_view_plan_select(plan.h, None, 1, 0.0, None, None, None, C.byref(n), None) == -1
        assert lib.pedp_view_plan_create(cov._h, 2, C.byref(C.c_void_p())) == -1
    finally:
        two = _lib.icp_end(ctx, want_corr=True)
    assert np.array_equal(one["T"], two["T"]) and np.array_equal(one["corr"], two["corr"])
    assert one["fitness"] == two["fitness"] and one["inlier_rmse"] == two["inlier_rmse"]
    rc, row = plan.candidate(0)
    assert rc == 0 and plan.candidate(1)[0] == -1                            # the refused observation was not counted
    same_row(row, want.row())
    area = dref.Model(f.verts.astype(np.float64), f.tris).area
    g = ref.score(ref.Work(cref.State(cov.F)), [want], area)
    assert g["gain_faces"][0] > 0
    same_gains({"gain_area": d_area.cpu().numpy()[:1], "gain_faces": d_faces.cpu().numpy()[:1]}, g)
    assert not cov.faces()["pixels"].any()
    plan.close()
    cov.close()
    cov.defect_map.close()


def test_a_context_with_a_history_gives_the_same_bits(ctx, scene):
    from pedp_hip import _lib, synth

    s = scene("torus1022", ORBIT).add_all()                                  # the session's context: whatever ran before
    here = s.planner.select(6, min_views=2)
    fresh_ctx = _lib.Context(0)
    fresh = Scene(fresh_ctx, "torus1022", ORBIT, *SMALL, ref_ctx=ctx).add_all()
    same_select(fresh.planner.select(6, min_views=2), here)
    f = synth.Frame("tiny")
    umesh = _lib.Mesh(fresh_ctx, f.verts_posed, f.tris)
    pts = f.scene(umesh.cast_rays(f.rays6, want_uv=False)["t_hit"])                          # a cast
    _lib.icp(fresh_ctx, _lib.Cloud(fresh_ctx, pts), _lib.Cloud(fresh_ctx, f.model_points, f.normals), 10.0, f.icp_init(), max_iteration=6,
             relative_fitness=-1, relative_rmse=-1)                                         # a registration
    umesh.closest_points(pts[:500])                                                         # a closest-point query
    used = Scene(fresh_ctx, "torus1022", ORBIT, *SMALL, ref_ctx=ctx).add_all()
    same_select(used.planner.select(6, min_views=2), here)
    same_select(here, ref.select(s.state, s.cands, s.m.area, 6, min_views=2))
    for h in (used, fresh, umesh):
        h.close()
    fresh_ctx.close()
