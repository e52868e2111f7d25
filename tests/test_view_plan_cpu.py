"""Next-best-view planning's restatement (tests/_view_plan_ref.py) against known answers and against the
coverage map's restatement, the exports and the Python argument errors: everything here runs without a GPU."""
import functools
import math
import os
import re
import types

import numpy as np
import pytest

import _coverage_ref as cref
import _defect_map_ref as dref
import _view_plan_ref as ref
from pedp_hip import view_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("create", "destroy", "clear", "observe", "candidate", "reset", "commit", "score", "select")
EPS = 2.0 ** -52
CRITERIA = [{}, dict(min_cos=0.5), dict(min_pixels=2), dict(max_footprint=40.0)]


# ------------------------------------------------------------------ the unit cube and its six axis views
def axis_poses():
    """The six object poses that turn each side of the unit cube towards the camera, the cube's centre 3.5 down the axis."""
    def rx(k):
        c, s = round(math.cos(k * math.pi / 2)), round(math.sin(k * math.pi / 2))
        return np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])

    def ry(k):
        c, s = round(math.cos(k * math.pi / 2)), round(math.sin(k * math.pi / 2))
        return np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])

    poses = []
    for R in (rx(0), rx(1), rx(2), rx(3), ry(1), ry(3)):
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = [0.0, 0.0, 3.5] - R @ [0.5, 0.5, 0.5]
        poses.append(T)
    return poses


@functools.lru_cache(maxsize=None)
def cube_scene():
    K, W, H = cref.intrinsics(40.0, 40.0, 7.5, 7.5), 16, 16
    v, t = dref.cube()
    model = dref.Model(v, t)
    cands = []
    for T in axis_poses():
        rec = ref.posed_records(v, t, T)
        th, ids = cref.host_cast(rec, cref.pixel_dirs(K, W, H))
        cands.append(ref.Observation(model.F, rec, K, W, H, th, ids))
    return model, cands


def test_the_six_axis_views_of_the_cube():
    model, cands = cube_scene()
    assert (model.area == 0.5).all()
    fresh = cref.State(12)
    s = ref.score(ref.Work(fresh), cands, model.area)
    assert list(s["gain_area"]) == [1.0] * 6 and list(s["gain_faces"]) == [2] * 6           # every view gains exactly its two faces
    assert sorted(int(f) for o in cands for f in np.nonzero(o.cpix)[0]) == list(range(12))
    out = ref.select(fresh, cands, model.area, 7)                                           # the seventh round stops
    assert list(out["order"]) == [0, 1, 2, 3, 4, 5]                                         # ties go to the lowest index
    assert list(out["gain_area"]) == [1.0] * 6 and list(out["gain_faces"]) == [2] * 6
    assert out["fraction"] == 1.0 and out["covered_faces"] == 12 and out["covered_area"] == out["total_area"] == 6.0
    three = ref.select(fresh, cands, model.area, 3)
    assert list(three["order"]) == [0, 1, 2] and three["fraction"] == 0.5
    assert len(ref.select(fresh, cands, model.area, 0)["order"]) == 0
    assert len(ref.select(fresh, cands, model.area, 6, min_gain=1.0)["order"]) == 0          # not > min_gain: stop at once
    assert len(ref.select(fresh, cands, model.area, 6, min_gain=float("nan"))["order"]) == 0
    # the fresh state is not touched, and a view already taken gains nothing
    assert not fresh.pixels.any()
    w = ref.Work(fresh).merge(cands[2])
    assert ref.gain(w, cands[2], model.area) == (0.0, 0) and ref.gain(w, cands[3], model.area) == (1.0, 2)


def test_two_views_per_face_on_the_cube():
    model, cands = cube_scene()
    twice = cands + cands                                                                   # each view twice
    fresh = cref.State(12)
    s = ref.score(ref.Work(fresh), twice, model.area, min_views=2)
    assert list(s["gain_area"]) == [0.5] * 12 and list(s["gain_faces"]) == [0] * 12         # half the area of two faces
    out = ref.select(fresh, twice, model.area, 12, min_views=2)
    assert list(out["order"]) == list(range(12)) and out["fraction"] == 1.0
    assert list(out["gain_faces"]) == [0] * 6 + [2] * 6 and list(out["gain_area"]) == [0.5] * 12
    assert (out["work"].views == 2).all()
    one = ref.select(fresh, twice, model.area, 12, min_views=1)                             # a copy is never chosen
    assert list(one["order"]) == list(range(6))
    # min_views <= 0 counts no views: one qualifying view covers
    assert ref.gain(ref.Work(fresh), cands[0], model.area, min_views=0) == (1.0, 2)
    assert ref.gain(ref.Work(fresh), cands[0], model.area, min_views=-3) == (1.0, 2)


# ------------------------------------------------------------------ the torus under 42 orbit views
@functools.lru_cache(maxsize=None)
def torus_scene():
    """torus(73, 7), the 42 poses of sample_views_icosphere(12, radius=200), a 32 x 24 frame, fx = fy = 60."""
    v, t = dref.torus(73, 7)
    model = dref.Model(v, t)
    W, H = 32, 24
    K = cref.intrinsics(60.0, 60.0, (W - 1) / 2, (H - 1) / 2)
    poses = ref.orbit(200.0, 12)
    dirs = cref.pixel_dirs(K, W, H)
    views, cands = [], []
    for T in poses:
        rec = ref.posed_records(v, t, T)
        th, ids = cref.host_cast(rec, dirs)
        views.append((rec, th, ids))
        cands.append(ref.Observation(model.F, rec, K, W, H, th, ids))
    return model, K, W, H, views, cands


def test_gain_faces_is_what_add_newly_covers():
    model, K, W, H, views, cands = torus_scene()
    assert model.F == 1022 and len(cands) == 42
    histories = [[], [19], [19, 24, 40]]
    for history in histories:
        st = cref.State(model.F)
        for v in history:
            st.add(*views[v][:1], K, W, H, *views[v][1:])
        w = ref.Work(st)
        for criteria in CRITERIA:
            before = st.covered(**criteria)
            got = ref.score(w, cands, model.area, **criteria)
            newly_total = 0
            for v, (rec, th, ids) in enumerate(views):
                after = cref.State(model.F)
                after.pixels, after.views, after.key, after.fp_bits = st.pixels.copy(), st.views.copy(), st.key.copy(), st.fp_bits.copy()
                after.add(rec, K, W, H, th, ids)
                newly = after.covered(**criteria) & ~before
                assert got["gain_faces"][v] == newly.sum(), (history, criteria, v)
                want = math.fsum(model.area[newly])                                         # min_views = 1: the newly covered area
                assert abs(got["gain_area"][v] - want) <= model.F * EPS * want
                merged = w.copy().merge(cands[v])                                           # the merge IS the state add leaves
                assert np.array_equal(merged.pixels, after.pixels) and np.array_equal(merged.views, after.views)
                assert np.array_equal(merged.key, after.key) and np.array_equal(merged.fp_bits, after.fp_bits)
                newly_total += newly.sum()
            assert newly_total > 0, (history, criteria)
    assert not (ref.score(ref.Work(cref.State(model.F)), cands, model.area, min_cos=0.5)["gain_faces"]
                == ref.score(ref.Work(cref.State(model.F)), cands, model.area)["gain_faces"]).all()


def test_the_fixed_order_sum():
    rng = np.random.default_rng(7)
    for n in (0, 1, 63, 64, 65, 1022, 4096, 4097, 8194, 270000):
        x = rng.uniform(0.0, 1.0, n) ** 8
        got, want = ref.ordered_sum(x), math.fsum(x)
        assert abs(got - want) <= n * EPS * want, n
        assert ref.ordered_sum(x).hex() == got.hex()
    assert ref.ordered_sum([]) == 0.0 and math.copysign(1.0, ref.ordered_sum([])) == 1.0
    # the order is the contract's, not left to right: lane 1 adds x[1] + x[65] before the butterfly brings in lane 0's 1
    x = np.zeros(128)
    x[0], x[1], x[65] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert ref.wave_sum(x) == 1.0 + 2.0 ** -52 and ((x[0] + x[1]) + x[65]) == 1.0
    model, _, _, _, _, cands = torus_scene()
    a = ref.gain(ref.Work(cref.State(model.F)), cands[19], model.area)
    assert a == ref.gain(ref.Work(cref.State(model.F)), cands[19], model.area)


def test_greedy_on_the_torus_is_not_top_k():
    model, K, W, H, views, cands = torus_scene()
    fresh = cref.State(model.F)
    s = ref.score(ref.Work(fresh), cands, model.area)
    out = ref.select(fresh, cands, model.area, 12)
    order = [int(v) for v in out["order"]]
    assert len(order) >= 3
    ranking = [int(v) for v in np.argsort(-s["gain_area"], kind="stable")]                  # top-k on the fresh map
    assert order != ranking[:len(order)] and order[2] not in ranking[:6]
    assert len(set(order)) == len(order)
    assert (np.diff(out["gain_area"]) <= 0).all() and (out["gain_area"] > 0).all()          # coverage gains are submodular
    assert len(np.unique(s["gain_faces"])) < len(s["gain_faces"])                           # ties in faces on the fresh map
    # what this scene was chosen for; a change of the scene shows here first
    assert order == [19, 24, 40, 15, 10, 35, 30, 14, 33, 6, 25, 22] and out["covered_faces"] == 1018
    assert s["gain_faces"][19] == s["gain_faces"][24] == 321
    # the totals are the summary of the state the rounds left, and the recorded gains add up to it
    st = cref.State(model.F)
    for v in order:
        st.add(*views[v][:1], K, W, H, *views[v][1:])
    want = st.summary(model)
    assert out["covered_faces"] == want["covered_faces"] == out["gain_faces"].sum()
    assert abs(out["covered_area"] - want["covered_area"]) <= model.F * EPS * want["covered_area"]
    assert abs(out["gain_area"].sum() - want["covered_area"]) <= 2 * model.F * EPS * want["covered_area"]
    # a min_gain between two rounds' gains stops there
    cut = ref.select(fresh, cands, model.area, 12, min_gain=float(out["gain_area"][4]))
    assert [int(v) for v in cut["order"]] == order[:4]


def test_orbit_views_look_at_the_centre():
    centre = np.array([3.0, -2.0, 5.0])
    poses = view_plan.orbit_views(centre, 200.0, 12)
    assert poses.shape == (42, 4, 4) and poses.dtype == np.float64
    assert np.allclose(poses, ref.orbit(200.0, 12, centre), rtol=0, atol=1e-12)
    at = poses[:, :3, :3] @ centre + poses[:, :3, 3]                                        # the centre in every camera's frame
    assert np.allclose(at, [0.0, 0.0, 200.0], rtol=0, atol=1e-9)
    assert np.allclose(poses[:, :3, :3] @ poses[:, :3, :3].transpose(0, 2, 1), np.eye(3), atol=1e-12)
    assert np.array_equal(view_plan.orbit_views([0.0, 0.0, 0.0], 200.0, 12), ref.orbit(200.0, 12))
    assert len(view_plan.orbit_views(centre, 1.0, 43)) == 162
    for bad in (dict(centre=[0, 0]), dict(centre=[0, 0, np.nan]), dict(radius=0.0), dict(radius="r"), dict(n_views=0), dict(n_views=2.0)):
        with pytest.raises(view_plan._lib.PedpError):
            view_plan.orbit_views(**dict(dict(centre=centre, radius=1.0, n_views=12), **bad))


# ------------------------------------------------------------------ exports and argument errors
def test_exports_in_the_header_the_bindings_the_library_and_compat():
    header = open(os.path.join(ROOT, "include", "pedp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    import pedp_hip
    from pedp_hip import _lib, compat

    lib = _lib.load()
    for name in EXPORTS:
        assert re.search(rf"\bint pedp_view_plan_{name}\s*\(", code), name
        assert f"pedp_view_plan_{name}" in _lib.PROTOTYPES
        assert hasattr(lib, f"pedp_view_plan_{name}")
    assert "typedef struct pedp_view_plan_s *pedp_view_plan_t;" in code
    assert compat.ViewPlanner is view_plan.ViewPlanner is pedp_hip.ViewPlanner and "ViewPlanner" in compat.__all__
    assert compat.orbit_views is view_plan.orbit_views is pedp_hip.orbit_views and "orbit_views" in compat.__all__
    assert "DESIGN.md s4.22" in header
    assert lib.pedp_view_plan_create(None, 4, None) == -1       # a null map is refused before anything else is looked at
    assert lib.pedp_view_plan_destroy(None) == 0
    n = __import__("ctypes").c_int64(5)
    assert lib.pedp_view_plan_select(None, None, 1, 0.0, None, None, None, n, None) == -1


def test_argument_errors_come_before_any_library_call(monkeypatch):
    import ctypes as C

    from pedp_hip import _lib
    from pedp_hip.coverage import CoverageMap
    from pedp_hip.view_plan import ViewPlanner

    def no_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_call)
    monkeypatch.setattr(_lib, "default_context", no_call)
    E = _lib.PedpError
    v, t = dref.cube()
    K = cref.intrinsics(40.0, 40.0, 7.5, 7.5)

    class Cov(CoverageMap):                                     # handles that are never given to the library, nor closed
        def close(self):
            pass

    class Planner(ViewPlanner):
        def close(self):
            pass

    def cov(F=12, open_=True):
        c = object.__new__(Cov)
        c.ctx, c.F, c._cameras, c._owns_map = object(), F, {}, False
        c._h = C.c_void_p(1 if open_ else None)
        c.defect_map = types.SimpleNamespace(_h=C.c_void_p(1))
        return c

    good = dict(coverage=cov(), model=(v, t), intrinsic_matrix=K, shape=(16, 16))
    for what, kw in (("CoverageMap", dict(coverage=object())), ("faces", dict(coverage=cov(F=11))), ("vertices", dict(model=object())),
                     ("V x 3", dict(model=(v[:, :2], t))), ("3 x 3", dict(intrinsic_matrix=np.eye(4))),
                     ("focal", dict(intrinsic_matrix=cref.intrinsics(0.0, 40.0, 1.0, 1.0))), ("shape", dict(shape=(16,))),
                     ("shape", dict(shape=(0, 16))), ("shape", dict(shape=(16.0, 16))), ("min_cos", dict(min_cos=1.5)),
                     ("min_cos", dict(min_cos=float("nan"))), ("min_cos", dict(min_cos="x")), ("capacity", dict(capacity=0)),
                     ("capacity", dict(capacity=2.0)), ("capacity", dict(capacity=True)), ("closed", dict(coverage=cov(open_=False)))):
        with pytest.raises(E, match=what):
            ViewPlanner(**dict(good, **kw))

    def planner(n=3, capacity=4, open_=True, cov_open=True):
        p = object.__new__(Planner)
        p.coverage, p.F, p.K, p.W, p.H, p.min_cos = cov(open_=cov_open), 12, K, 16, 16, 0.0
        p.ctx, p.n, p.capacity = p.coverage.ctx, n, capacity
        p._h = C.c_void_p(1 if open_ else None)
        p._mesh = p._rayset = p._t = p._ids = None
        return p

    p = planner()
    for what, poses in (("V x 4 x 4", np.eye(3)), ("V x 4 x 4", np.zeros((2, 4, 3))), ("V x 4 x 4", "poses"), ("finite", np.full((1, 4, 4), np.nan)),
                        ("full", np.tile(np.eye(4), (2, 1, 1)))):
        with pytest.raises(E, match=what):
            p.add_candidates(poses)
    assert p.n == 3
    for fn in (p.candidate, p.commit):
        for v in (-1, 3, 1.0, True, None):
            with pytest.raises(E):
                fn(v)
    for fn in (p.score, lambda **kw: p.select(2, **kw)):
        for kw in (dict(min_views=1.0), dict(min_pixels=True), dict(min_cos="a"), dict(max_footprint=float("nan")), dict(min_views=2 ** 31),
                   dict(min_pixels=2 ** 63)):
            with pytest.raises(E):
                fn(**kw)
    for k in (-1, 1.0, True, None):
        with pytest.raises(E, match="k must be"):
            p.select(k)
    for g in (float("nan"), "g", None, True):
        with pytest.raises(E, match="min_gain"):
            p.select(2, min_gain=g)
    for q, what in ((planner(open_=False), "view planner is closed"), (planner(cov_open=False), "coverage map is closed")):
        for call in (lambda: q.add_candidates(np.eye(4)), lambda: q.candidate(0), q.clear, q.reset, lambda: q.commit(0), q.score,
                     lambda: q.select(1)):
            with pytest.raises(E, match=what):
                call()
