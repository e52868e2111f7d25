"""The deviation map on the device (csrc/pedp_deviationmap.hip) against its restatement
(tests/_deviation_map_ref.py): bit for bit -- the integers, min, max, mean, std and the labels -- except the
floating-point area and volume sums, which are held to s4.17's bound of any summation order (n_faces 2^-52 relative to
math.fsum) and to repeatability.  add_points is held to the state that the parent's own signed_closest_points + add
leaves."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _coverage_ref as cref
import _defect_map_ref as dref
import _deviation_map_ref as ref
from pedp_hip import deviation_map  # noqa: F401  (without the feature every test here fails at import)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
Q = ref.Q
GATE = 0.75
ROW_COUNTS = (0, 1, 63, 64, 65, 257, 4097)
PATTERNS = ("one_face", "alternating", "runs", "random")
MESHES = {
    "triangle": lambda: (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]], dtype=np.uint32)),
    "quad": lambda: (np.array([[-10.0, -10.0, 4.0], [10.0, -10.0, 4.0], [10.0, 10.0, 4.0], [-10.0, 10.0, 4.0]]),
                     np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)),
    "torus1022": lambda: dref.torus(73, 7),
    "torus32000": lambda: dref.torus(200, 80),
    "torus4000": lambda: dref.torus(50, 40),
}


@functools.lru_cache(maxsize=None)
def model(name):
    return dref.Model(*MESHES[name]())


_maps = {}


@pytest.fixture
def maps(ctx):
    """name -> the (cleared) DeviationMap of that model on the session's context."""
    from pedp_hip import DeviationMap

    def get(name):
        if name not in _maps:
            m = model(name)
            _maps[name] = DeviationMap((m.verts, m.tris), ctx)
        _maps[name].clear()
        return _maps[name]

    return get


def rows(F, n, pattern, seed=0):
    """n rows in `pattern`, with rows that take no part, rows on the gate and ties put inside the runs."""
    rng = np.random.default_rng([seed, n, F])
    if pattern == "one_face":
        ids = np.full(n, F - 1)
    elif pattern == "alternating":
        ids = (np.arange(n) % 2) * (F - 1)
    elif pattern == "runs":                           # sorted runs of 1 ... 300 rows: across wave and block boundaries
        lengths = np.resize([1, 63, 2, 65, 130, 300, 37, 64, 255, 3], max(n, 1))
        ids = (np.repeat(np.arange(len(lengths)), lengths)[:n] * 7) % F
    else:
        ids = rng.integers(0, F, n)
    ids = ids.astype(np.uint32)
    d = rng.normal(0.0, 0.3, n)
    special = [np.nan, np.inf, -np.inf, GATE, -GATE, np.nextafter(GATE, np.inf), -np.nextafter(GATE, np.inf), 0.0, -0.0,
               2.5 * Q, -3.5 * Q, 1000.5 * Q]
    if n > 4 * len(special):
        at = rng.choice(n, 2 * len(special) + 6, replace=False)
        d[at[:len(special)]] = special
        d[at[len(special):2 * len(special)]] = special
        ids[at[-6:]] = [dref.MISS, F, F + 7, dref.MISS, 2 ** 31, F]
    return ids, d


def same_faces(got, want):
    for k in ref.FACE_KEYS:
        assert got[k].dtype == want[k].dtype and dref.same_bits(got[k], want[k]), k


# ------------------------------------------------------------------ add: sizes where the lane, wave and block logic can go wrong
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", ["triangle", "quad", "torus1022", "torus32000"])
def test_add_is_the_restatement_bit_for_bit(maps, name, pattern):
    F = model(name).F
    for n in ROW_COUNTS:
        dm, st = maps(name), ref.State(F)
        for k in range(2):                            # two observations: the second meets a state that is not empty
            ids, d = rows(F, n, pattern, seed=k)
            dm.add(ids, d, gate=GATE)
            st.add(ids, d, GATE)
        same_faces(dm.faces(), st.faces())
        assert dm.stats() == st.stats(), (n, dm.stats(), st.stats())


def test_the_sum_of_squares_crosses_two_to_the_64(maps):
    dm, st = maps("quad"), ref.State(2)
    d = np.full(4097, 1000.0)
    ids = np.ones(4097, np.uint32)
    dm.add(ids, d)
    st.add(ids, d)
    f = dm.faces()
    same_faces(f, st.faces())
    assert f["s2_hi"][1] >= 1 and f["mean"][1] == 1000.0 and f["std"][1] == 0.0 and np.isnan(f["mean"][0])
    d[::2] = -1000.0
    d[1::7] = 1024.0                                  # the largest value the gate can admit
    dm.add(ids, d)
    st.add(ids, d)
    same_faces(dm.faces(), st.faces())
    assert dm.faces()["max"][1] == 1024.0 and dm.faces()["frames"][1] == 2


def test_the_gate_is_checked(maps):
    from pedp_hip import _lib

    dm = maps("quad")
    ids, d = np.zeros(3, np.uint32), np.zeros(3)
    lib = _lib.load()
    for gate in (-1.0, 1024.5, float("nan"), float("inf")):
        assert lib.pedp_deviation_map_add(dm._h, _lib._ptr(ids), _lib._ptr(d), 3, gate, _lib.HOST) == -1, gate
    assert dm.stats()["observations"] == 0
    dm.add(ids, np.array([0.0, -0.0, Q]), gate=0.0)
    assert dm.stats() == {"observations": 1, "rows_taken": 2, "rows_ignored": 0, "rows_gated": 1, "rows_backfacing": 0}


# ------------------------------------------------------------------ what the state does not depend on
def test_order_memory_and_history_change_nothing(ctx, maps):
    import torch

    from pedp_hip import DefectMap, DeviationMap, _lib

    name = "torus1022"
    m = model(name)
    F = m.F
    obs = [rows(F, 4097, p, seed=3) for p in ("runs", "random", "one_face")]
    dm = maps(name)
    for ids, d in obs:
        dm.add(ids, d, gate=GATE)
    want, want_stats = dm.faces(), dm.stats()
    dm.clear()                                        # permuted rows
    rng = np.random.default_rng(5)
    for ids, d in obs:
        p = rng.permutation(len(ids))
        dm.add(ids[p], d[p], gate=GATE)
    same_faces(dm.faces(), want)
    dm.clear()                                        # device memory, int64 ids, float32-exact distances stay float64
    for ids, d in obs:
        dm.add(torch.from_numpy(ids.astype(np.int64)).cuda(), torch.from_numpy(d).cuda(), gate=GATE)
    same_faces(dm.faces(), want)
    assert dm.stats() == want_stats
    dm.clear()                                        # after clear: a fresh map
    empty = dm.faces()
    assert not empty["n"].any() and not empty["frames"].any() and np.isnan(empty["mean"]).all() and np.isnan(empty["min"]).all()
    assert dm.stats() == dict.fromkeys(want_stats, 0)
    # unrelated calls on the context and on the map underneath, between the observations
    shared = DefectMap((m.verts, m.tris), ctx)
    other = DeviationMap(shared, ctx)
    mesh = _lib.Mesh(ctx, m.verts.astype(np.float32), m.tris)
    for k, (ids, d) in enumerate(obs):
        other.add(ids, d, gate=GATE)
        shared.add(ids, np.abs(d))
        shared.regions(threshold=0.1, grow=1)
        mesh.closest_points(np.random.default_rng(k).normal(0.0, 30.0, (500, 3)))
        other.regions(0.1, grow=2)
        other.summary(threshold=0.1)
    same_faces(other.faces(), want)
    shared.close()
    with pytest.raises(_lib.PedpError, match="the defect map under the deviation map is closed"):
        other.faces()
    other.close()
    mesh.close()


_PROBE = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import _defect_map_ref as dref
from pedp_hip import DeviationMap, _lib
z = np.load(sys.argv[2])
ctx = _lib.Context(0)
dm = DeviationMap(dref.torus(73, 7), ctx)
for k in range(int(z["count"])):
    dm.add(z[f"ids{k}"], z[f"d{k}"], gate=float(z["gate"]))
f = dm.faces()
np.savez(sys.argv[3], **f, **{"stat_" + k: v for k, v in dm.stats().items()})
dm.close(); ctx.close()
"""


def test_the_combine_switch_changes_no_bit(tmp_path):
    """The switch is read once per process: two fresh processes, the in-wave combine on and off."""
    F = model("torus1022").F
    obs = [rows(F, 4097, p, seed=9) for p in PATTERNS]
    inp = str(tmp_path / "rows.npz")
    np.savez(inp, count=len(obs), gate=GATE, **{f"ids{k}": o[0] for k, o in enumerate(obs)}, **{f"d{k}": o[1] for k, o in enumerate(obs)})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for flag in ("1", "0"):
        out = str(tmp_path / f"state{flag}.npz")
        env = dict(os.environ, PEDP_DEVIATION_COMBINE=flag)
        p = subprocess.run([sys.executable, "-c", _PROBE, root, inp, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        got[flag] = dict(np.load(out))
    st = ref.State(F)
    for ids, d in obs:
        st.add(ids, d, GATE)
    for flag in got:
        same_faces(got[flag], st.faces())
        assert {k: int(got[flag]["stat_" + k]) for k in st.stats()} == st.stats()


# ------------------------------------------------------------------ add_points: a frame's points with one search
W, H, FOCAL, UNIT = 160, 144, 250.0, 1000.0


def rot_x(a):
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


class Scene:
    """The closed torus posed in front of the camera; the frame's depth points with seeded noise along the ray, a patch
    lifted towards the camera by LIFT, and a few hundred points well inside the tube and well outside the part."""
    LIFT, SIGMA, POINT_GATE = 1.0, 0.05, 3.0

    def __init__(self, ctx):
        from pedp_hip import _lib

        m = model("torus4000")
        self.model = m
        v32 = np.ascontiguousarray((m.verts @ rot_x(0.6).T + [0.0, 0.0, 200.0]).astype(np.float32))
        self.mesh = _lib.Mesh(ctx, v32, m.tris)
        self.solid = _lib.Solid(ctx, m.verts, m.tris)
        self.K = cref.intrinsics(FOCAL, FOCAL, (W - 1) / 2, (H - 1) / 2)
        hit = self.mesh.cast_rays(cref.rays6(self.K, W, H), want_uv=False)
        t, self.hit_ids = hit["t_hit"].astype(np.float64), hit["primitive_ids"]
        self.seen = np.isfinite(t)
        dirs = cref.pixel_dirs(self.K, W, H)
        ys, xs = np.mgrid[0:H, 0:W]
        centre = int(np.argmin(np.where(self.seen, t, np.inf)))                 # the nearest pixel: it faces the camera; the patch lies around it
        self.patch = self.seen & (np.abs(xs.reshape(-1) - centre % W) <= 7) & (np.abs(ys.reshape(-1) - centre // W) <= 7)
        self.t, self.dirs = t, dirs

    def frame(self, seed, lifted=True):
        """(points N x 3 float64, depth H x W float32 in metres): one noisy frame."""
        rng = np.random.default_rng(seed)
        t = np.where(self.seen, self.t + rng.normal(0.0, self.SIGMA, len(self.t)), 0.0)
        if lifted:
            t = np.where(self.patch, t - self.LIFT, t)
        z = (t * self.dirs[:, 2]).reshape(H, W)
        depth = np.where(self.seen.reshape(H, W), z / UNIT, 0.0).astype(np.float32)
        pts = (t[:, None] * self.dirs)[self.seen]
        u = rng.uniform(0.0, 2 * np.pi, 300)
        ring = np.stack([40.0 * np.cos(u), 40.0 * np.sin(u), rng.normal(0.0, 2.0, 300)], axis=1) @ rot_x(0.6).T + [0.0, 0.0, 200.0]
        far = rng.normal(0.0, 1.0, (200, 3)) * [150.0, 150.0, 60.0] + [0.0, 0.0, 420.0]
        return np.ascontiguousarray(np.concatenate([pts, ring, far])), depth


_scene = []


@pytest.fixture
def scene(ctx):
    if not _scene:
        _scene.append(Scene(ctx))
    return _scene[0]


def test_add_points_leaves_the_state_of_signed_closest_points_and_add(ctx, maps, scene):
    from pedp_hip import _lib
    from pedp_hip import surface_distance as sd

    pts, _ = scene.frame(1)
    both = sd.signed_closest_points(scene.mesh, pts, scene.solid)             # the parent's code: two searches
    prim, sdist = both["primitive_ids"], both["signed_distances"]
    assert (sdist < -10.0).sum() >= 250 and (sdist > 50.0).sum() >= 150 and (np.abs(sdist) < 0.3).sum() > 5000
    dm = maps("torus4000")
    dm.add(prim, sdist, gate=scene.POINT_GATE)
    want, want_stats = dm.faces(), dm.stats()
    assert want_stats["rows_gated"] >= 400 and want_stats["rows_taken"] > 5000
    st = ref.State(dm.F).add(prim, sdist, scene.POINT_GATE)
    same_faces(want, st.faces())
    dm.clear()
    dm.add_points(scene.mesh, pts, scene.solid, gate=scene.POINT_GATE)
    same_faces(dm.faces(), want)
    assert dm.stats() == want_stats
    try:                                              # the search's other kernels: the same rows
        for mode in (1, 2, 3):
            _lib.closest_configure(ctx, mode)
            dm.clear()
            dm.add_points(scene.mesh, pts, scene.solid, gate=scene.POINT_GATE)
            same_faces(dm.faces(), want)
    finally:
        _lib.closest_configure(ctx, 0)
    import torch

    dm.clear()                                        # device memory, float32-exact points widen exactly
    dm.add_points(scene.mesh, torch.from_numpy(pts).cuda(), scene.solid, gate=scene.POINT_GATE)
    same_faces(dm.faces(), want)
    dm.add_points(scene.mesh, np.zeros((0, 3)), scene.solid)                   # no rows: an observation all the same
    assert dm.stats()["observations"] == 2 and dm.faces()["frames"].max() == 1


def test_the_origin_drops_the_rows_that_face_away(maps, scene):
    from pedp_hip import surface_distance as sd

    pts, _ = scene.frame(2)
    both = sd.signed_closest_points(scene.mesh, pts, scene.solid)
    c, nrm = both["points"], both["normals"]
    for origin in ((0.0, 0.0, 0.0), (30.0, -500.0, 200.0)):
        r = np.asarray(origin) - c
        terms = r * nrm
        dot = (terms[:, 0] + terms[:, 1]) + terms[:, 2]
        back = ~(dot > 0.0)                           # on the device's own outputs
        # The kernel takes the sign of (r . N) orientation on the pseudonormal before it is normalised; `normals` is N / |N|
        # times the orientation, each component rounded.  The two agree in sign unless r . n cancels to within its own
        # rounding, 8 x 2^-52 of its terms' magnitudes: a condition on the input (the seeds of the frame) that no row is
        # that close to edge on, checked here and not a tolerance on the result.
        doubtful = ~(np.abs(dot) > 8 * EPS * np.abs(terms).sum(axis=1))
        assert not doubtful[np.isfinite(dot)].any(), f"{int(doubtful.sum())} rows within rounding of edge on: take another seed"
        st = ref.State(scene.model.F).add(both["primitive_ids"], both["signed_distances"], scene.POINT_GATE, backfacing=back)
        dm = maps("torus4000")
        dm.add_points(scene.mesh, pts, scene.solid, gate=scene.POINT_GATE, origin=origin)
        same_faces(dm.faces(), st.faces())
        assert dm.stats() == st.stats() and st.rows_backfacing > 50 and st.rows_taken > 1000, st.stats()


def test_add_frame_from_a_cuda_depth_tensor_is_add_points_on_its_rows(maps, scene):
    import torch

    from pedp_hip.surface_fit import frame_points

    _, depth = scene.frame(3)
    mask = np.ones((H, W), np.uint8)
    mask[:, :20] = 0
    cuda_depth = torch.from_numpy(depth).cuda()
    pts = frame_points(cuda_depth, scene.K, UNIT, mask)
    assert pts.is_cuda and 5000 < len(pts) == int(((depth >= 0.001) & (mask > 0)).sum())
    dm = maps("torus4000")
    dm.add_points(scene.mesh, pts, scene.solid, gate=scene.POINT_GATE, origin=(0.0, 0.0, 0.0))
    want, want_stats = dm.faces(), dm.stats()
    assert want_stats["rows_taken"] > 5000
    dm.clear()
    n = dm.add_frame(cuda_depth, scene.K, scene.mesh, scene.solid, unit=UNIT, mask=mask, gate=scene.POINT_GATE)
    assert n == len(pts)
    same_faces(dm.faces(), want)
    assert dm.stats() == want_stats
    dm.clear()
    dm.add_frame(depth, scene.K, scene.mesh, scene.solid, unit=UNIT, mask=mask, gate=scene.POINT_GATE, backfacing=False)
    assert dm.stats()["rows_backfacing"] == 0 and dm.stats()["rows_taken"] >= want_stats["rows_taken"]


# ------------------------------------------------------------------ regions and totals
def same_regions(got, want):
    assert got["n_regions"] == want["n_regions"]
    assert np.array_equal(got["labels"], want["labels"])
    for k in dref.INT_COLUMNS:
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    for k in dref.BIT_COLUMNS + ref.REGION_BIT_COLUMNS:
        assert dref.same_bits(got[k], want[k]), k
    n, nm = want["n_faces"].astype(np.float64), want["n_measured"].astype(np.float64)
    assert (np.abs(got["area"] - want["area"]) <= n * EPS * want["area"]).all(), "area beyond n_faces 2^-52 of fsum"
    assert (np.abs(got["measured_area"] - want["measured_area"]) <= nm * EPS * want["measured_area"]).all()
    assert (np.abs(got["volume"] - want["volume"]) <= nm * EPS * want["abs_volume"]).all(), "volume beyond n_faces 2^-52 of fsum"
    with np.errstate(invalid="ignore", divide="ignore"):
        assert dref.same_bits(got["mean"], np.where(nm > 0, got["volume"] / got["measured_area"], np.nan))


def same_table_bits(a, b):
    assert a["n_regions"] == b["n_regions"] and np.array_equal(a["labels"], b["labels"])
    for k in deviation_map.DEVIATION_REGION_DTYPE.names:
        assert dref.same_bits(a[k], b[k]), k


def same_summary(got, want, F):
    for k in ("faces", "measured_faces", "marked_faces", "max_face"):
        assert got[k] == want[k], k
    for k in ("total_area", "measured_area", "marked_area"):
        assert abs(got[k] - want[k]) <= F * EPS * want[k], k
    if want["measured_faces"]:
        assert got["max_abs_mean"] == want["max_abs_mean"]
        # each sum is within F 2^-52 of fsum relative to its terms' magnitudes; the quotient adds the area's error and a rounding
        assert abs(got["mean"] - want["s1"] / want["measured_area"]) <= (2 * F + 2) * EPS * want["abs_s1"] / want["measured_area"]
        rms = np.sqrt(want["s2"] / want["measured_area"])
        assert abs(got["rms"] - rms) <= (F + 2) * EPS * rms
    else:
        assert np.isnan(got["mean"]) and np.isnan(got["rms"]) and np.isnan(got["max_abs_mean"])


def test_the_lifted_patch_is_one_region_with_its_volume(maps, scene):
    dm = maps("torus4000")
    st = ref.State(scene.model.F)
    from pedp_hip import surface_distance as sd

    for k in range(4):
        pts, _ = scene.frame(10 + k)
        dm.add_points(scene.mesh, pts, scene.solid, gate=scene.POINT_GATE, origin=(0.0, 0.0, 0.0))
        both = sd.signed_closest_points(scene.mesh, pts, scene.solid)
        c, nrm = both["points"], both["normals"]
        back = ~(((0.0 - c[:, 0]) * nrm[:, 0] + (0.0 - c[:, 1]) * nrm[:, 1]) + (0.0 - c[:, 2]) * nrm[:, 2] > 0.0)
        st.add(both["primitive_ids"], both["signed_distances"], scene.POINT_GATE, backfacing=back)
    same_faces(dm.faces(), st.faces())
    crit = dict(threshold=0.4, sign=+1, min_samples=2)
    got, want = dm.regions(**crit), ref.regions(scene.model, st, **crit)
    print(f"lifted patch: {want['n_regions']} region(s), faces {want['n_faces']}, volume {want['volume']}, area {want['measured_area']}")
    same_regions(got, want)
    assert want["n_regions"] == 1 and 0.4 * want["measured_area"][0] < want["volume"][0] < (scene.LIFT + 0.2) * want["measured_area"][0]
    assert dm.regions(sign=-1, threshold=0.4, min_samples=2)["n_regions"] == 0
    same_table_bits(dm.regions(**crit), got)          # the same bits on every call
    for kw in (dict(crit, grow=2), dict(threshold=0.02, z=3.0), dict(threshold=0.05, sign=-1), dict(threshold=0.0, min_frames=4, grow=1)):
        same_regions(dm.regions(**kw), ref.regions(scene.model, st, **kw))
    for kw in (crit, dict(threshold=0.02, z=3.0, min_samples=4), dict(threshold=1e9)):
        s = dm.summary(**kw)
        same_summary(s, ref.summary(scene.model, st, **kw), scene.model.F)
        again = dm.summary(**kw)
        assert all(np.array_equal(s[k], again[k], equal_nan=True) for k in s)     # the same bits on every call
    colors = dm.face_colors(1.0)
    f = dm.faces()
    assert colors.shape == (dm.F, 3) and (colors[f["n"] == 0] == 0.5).all() and (colors[got["labels"] == 0][:, 0] == 1.0).all()


def test_regions_on_every_model_and_an_empty_map(maps):
    for name in ("triangle", "quad", "torus1022", "torus32000"):
        m = model(name)
        dm, st = maps(name), ref.State(m.F)
        empty = dm.regions(0.0)
        assert empty["n_regions"] == 0 and (empty["labels"] == -1).all()
        same_summary(dm.summary(), ref.summary(m, st), m.F)
        rng = np.random.default_rng(m.F)
        for k in range(3):
            ids = rng.integers(0, m.F, 4097).astype(np.uint32) if m.F > 2 else rows(m.F, 4097, "alternating", k)[0]
            bump = 0.5 * np.exp(-((ids.astype(np.float64) - m.F / 3) / (0.02 * m.F + 1)) ** 2) - 0.4 * (ids > 0.9 * m.F)
            d = bump + rng.normal(0.0, 0.05, len(ids))
            dm.add(ids, d, gate=GATE)
            st.add(ids, d, GATE)
        for kw in (dict(threshold=0.2), dict(threshold=0.2, sign=-1, grow=1), dict(threshold=0.1, sign=+1, min_frames=2, z=2.0)):
            same_regions(dm.regions(**kw), ref.regions(m, st, **kw))
            crit = {k: v for k, v in kw.items() if k != "grow"}
            same_summary(dm.summary(**crit), ref.summary(m, st, **crit), m.F)


CLEAN_SCENE = dict(frames=16, first_seed=100, z=4.0, min_samples=32)


def test_a_clean_noisy_scene_marks_what_the_restatement_marks(maps, scene):
    """The scene's frame without the lifted patch, 16 times with fresh noise, through add_points with the camera centre:
    the device marks the faces the restatement marks on the device's own signed_closest_points rows, at z = 4 and z = 2.
    The z rule needs min_samples beside it: a face with one row has std 0, so any mean passes at any z, and a handful of
    rows have the heavy tails of Student's t.  Even so a posed frame is NOT the clean input of the test below: measured
    on the MI355X, of the 1,588 faces with 32 rows or more the restatement marks 6, 2, 8 and 4 at z = 4 for the first
    seeds 100, 200, 300 and 400 (26, 23, 27, 23 without min_samples), where noise alone would mark one face in ten such
    runs.  The rows a face gets are chosen by the search, which depends on the noise itself, so a face's rows are not a
    fair sample of the noise (supposed, not shown: the marked faces were not looked at one by one).  No seed meets the
    condition `no face marked`, so it is not asserted here; the agreement with the restatement is."""
    from pedp_hip import surface_distance as sd

    c = CLEAN_SCENE
    dm, st = maps("torus4000"), ref.State(scene.model.F)
    for k in range(c["frames"]):
        pts, _ = scene.frame(c["first_seed"] + k, lifted=False)
        dm.add_points(scene.mesh, pts, scene.solid, gate=scene.POINT_GATE, origin=(0.0, 0.0, 0.0))
        both = sd.signed_closest_points(scene.mesh, pts, scene.solid)
        r, nrm = -both["points"], both["normals"]
        back = ~((r[:, 0] * nrm[:, 0] + r[:, 1] * nrm[:, 1]) + r[:, 2] * nrm[:, 2] > 0.0)
        st.add(both["primitive_ids"], both["signed_distances"], scene.POINT_GATE, backfacing=back)
    f = st.faces()
    same_faces(dm.faces(), f)
    assert (f["n"] >= c["min_samples"]).sum() > 1000 and st.observations == c["frames"]
    for z in (c["z"], 2.0):
        crit = dict(z=z, min_samples=c["min_samples"])
        want = ref.regions(scene.model, st, **crit)
        print(f"clean scene, z = {z}: {int(ref.marked(f, **crit).sum())} of {int((f['n'] >= c['min_samples']).sum())} faces with "
              f"{c['min_samples']} rows or more marked, {want['n_regions']} regions; {int(ref.marked(f, z=z).sum())} without min_samples")
        same_regions(dm.regions(0.0, **crit), want)
        assert dm.summary(**crit)["marked_faces"] == int(ref.marked(f, **crit).sum())


def test_a_clean_noisy_part_of_known_rows_marks_no_face_at_four_sigma(maps):
    """The same on rows whose condition the CPU suite checks too (tests/test_deviation_map_cpu.py): 9 rows per face and
    frame of N(0, 0.5), 16 frames."""
    c = ref.CLEAN
    dm, st = maps("torus1022"), ref.State(c["F"])
    for k in range(c["frames"]):
        ids, d = ref.noisy_rows(k)
        dm.add(ids, d, gate=3.0)
        st.add(ids, d, 3.0)
    same_faces(dm.faces(), st.faces())
    assert not ref.marked(st.faces(), z=c["z"]).any()                       # the input's condition (checked on the CPU too)
    got = dm.regions(0.0, z=c["z"])
    assert got["n_regions"] == 0 and (got["labels"] == -1).all() and dm.summary(z=c["z"])["marked_faces"] == 0
    same_regions(dm.regions(0.0, z=1.0), ref.regions(model("torus1022"), st, z=1.0))
