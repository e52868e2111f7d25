"""The coverage map's restatement (tests/_coverage_ref.py) against known answers, the exports and the
Python argument errors: everything here runs without a GPU."""
import os
import re

import numpy as np
import pytest

import _coverage_ref as ref
import _defect_map_ref as dref
from pedp_hip import coverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("create", "destroy", "add", "clear", "faces", "stats", "summary", "regions")
QUAD_TRIS = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)


def quad(z, half=10.0, tilt=0.0):
    """A square of side 2 half centred on the optical axis at depth z, turned by `tilt` about the x axis through its
    centre."""
    c, s = np.cos(tilt), np.sin(tilt)
    p = np.array([[-half, -half], [half, -half], [half, half], [-half, half]])
    return np.stack([p[:, 0], c * p[:, 1], z + s * p[:, 1]], axis=1), QUAD_TRIS


def one_view(rec, K, W, H, **kw):
    t, ids = ref.host_cast(rec, ref.pixel_dirs(K, W, H))
    return ref.State(len(rec[0])).add(rec, K, W, H, t, ids, **kw), t, ids


def test_the_package_and_the_restatement_name_the_same_classes():
    assert coverage.CLASSES == ref.CLASSES and np.float32(coverage.Z_MIN) == ref.Z_MIN
    for name in ("MASKED", "MISS", "NO_DEPTH", "OCCLUDED", "BEHIND", "GRAZING", "SEEN"):
        assert getattr(coverage, name) == getattr(ref, name) == ref.CLASSES.index(name.lower())
    assert np.array_equal(coverage.pixel_rays6(ref.intrinsics(50.0, 40.0, 3.0, 2.0), 7, 5), ref.rays6(ref.intrinsics(50.0, 40.0, 3.0, 2.0), 7, 5))


def test_a_fronto_parallel_quad():
    K, W, H, z = ref.intrinsics(50.0, 40.0, 3.0, 2.0), 7, 5, 4.0
    st, t, ids = one_view(ref.records64(*quad(z)), K, W, H)
    c = st.last
    centre = 2 * W + 3
    assert (c["status"] == ref.SEEN).all() and t[centre] == z
    assert c["cos"][centre] == 1.0 and c["footprint"][centre] == z * z / (50.0 * 40.0)
    d = ref.pixel_dirs(K, W, H)
    assert np.allclose(c["cos"], d[:, 2], rtol=0, atol=1e-15) and np.allclose(c["z_hit"], z, rtol=1e-7)
    assert st.pixels.sum() == W * H and list(st.views) == [1, 1] and st.best_cos.max() == 1.0
    # z^2 / (fx fy) all over a fronto-parallel plane: d_z and the cosine cancel (t_hit is rounded to float32)
    assert np.abs(c["footprint"] - z * z / 2000.0).max() < 1e-8 and np.abs(st.min_footprint - z * z / 2000.0).max() < 1e-8
    assert st.stats()["seen"] == W * H and st.stats()["views"] == 1


def test_the_quad_turned_sixty_degrees():
    K, W, H = ref.intrinsics(50.0, 50.0, 3.0, 2.0), 7, 5
    st, t, ids = one_view(ref.records64(*quad(4.0, tilt=np.deg2rad(60.0))), K, W, H)
    centre = 2 * W + 3
    assert st.last["status"][centre] == ref.SEEN
    assert abs(st.last["cos"][centre] - 0.5) <= 1e-12
    assert abs(st.last["footprint"][centre] - 16.0 / (2500.0 * 0.5)) <= 1e-12


def test_every_class_on_a_4_by_3_frame():
    K, W, H, z = ref.intrinsics(8.0, 8.0, 1.0, 1.0), 4, 3, 2.0
    rec = ref.records64(*quad(z))
    d = ref.pixel_dirs(K, W, H)
    t, ids = ref.host_cast(rec, d)
    assert np.isfinite(t).all()
    z_hit = t.astype(np.float64) * d[:, 2]
    depth = z_hit.astype(np.float32)                     # agrees within float32 rounding, far inside the tolerance
    mask = np.ones(W * H, np.uint8)
    centre = 1 * W + 1                                   # the principal pixel: d = (0, 0, 1), z_hit = 2 exactly
    assert z_hit[centre] == 2.0
    depth[centre] = 2.5                                  # a difference of exactly depth_tol
    depth[0] = np.nan
    depth[1] = 0.0005
    depth[2] = np.inf
    depth[3] = 1.0                                       # something a metre in front
    depth[4] = 3.0                                       # the sensor looked through
    mask[6] = 0
    ids = ids.copy()
    ids[7] = dref.MISS
    ids[8] = 2                                           # an id beyond F
    t = t.copy()
    t[9] = np.inf
    min_cos = float(np.sort(d[:, 2])[0]) + 1e-9          # the corner pixel 11 (with 3, which is OCCLUDED) has the lowest cosine
    st = ref.State(2).add(rec, K, W, H, t, ids, depth=depth, mask=mask, depth_tol=0.5, min_cos=min_cos)
    want = [ref.NO_DEPTH, ref.NO_DEPTH, ref.NO_DEPTH, ref.OCCLUDED, ref.BEHIND, ref.SEEN, ref.MASKED, ref.MISS, ref.MISS, ref.MISS,
            ref.SEEN, ref.GRAZING]
    assert list(st.last["status"]) == want and st.last["status"][centre] == ref.SEEN
    assert st.stats() == {"views": 1, "masked": 1, "miss": 3, "no_depth": 3, "occluded": 1, "behind": 1, "grazing": 1, "seen": 2}
    assert st.pixels.sum() == 2 and st.blocked.sum() == 1
    depth[centre] = 1.5                                  # exactly -depth_tol is SEEN as well
    assert ref.classify(rec, K, W, H, t, ids, depth=depth, depth_tol=0.5)["status"][centre] == ref.SEEN
    depth[centre] = np.nextafter(np.float32(2.5), np.float32(3.0))
    assert ref.classify(rec, K, W, H, t, ids, depth=depth, depth_tol=0.5)["status"][centre] == ref.BEHIND
    # the mask comes first, then the miss: a masked miss with a bad depth is MASKED
    mask[7] = 0
    depth[7] = np.nan
    assert ref.classify(rec, K, W, H, t, ids, depth=depth, mask=mask, depth_tol=0.5)["status"][7] == ref.MASKED


def axis_views():
    """The six rotations that turn each side of the cube towards the camera, with the cube moved down the optical axis."""
    rx = lambda k: np.array([[1, 0, 0], [0, np.cos(k * np.pi / 2).round(), -np.sin(k * np.pi / 2).round()],  # noqa: E731
                             [0, np.sin(k * np.pi / 2).round(), np.cos(k * np.pi / 2).round()]])
    ry = lambda k: np.array([[np.cos(k * np.pi / 2).round(), 0, np.sin(k * np.pi / 2).round()], [0, 1, 0],  # noqa: E731
                             [-np.sin(k * np.pi / 2).round(), 0, np.cos(k * np.pi / 2).round()]])
    return [rx(0), rx(1), rx(2), rx(3), ry(1), ry(3)]


def posed_cube(R):
    v, t = dref.cube()
    return ((v - 0.5) @ R.T + [0.0, 0.0, 3.5]).astype(np.float32), t


def test_the_cube_seen_along_an_axis():
    K, W, H = ref.intrinsics(40.0, 40.0, 7.5, 7.5), 16, 16
    model = dref.Model(*dref.cube())
    v, tris = posed_cube(np.eye(3))
    st, t, ids = one_view(ref.records(v, tris), K, W, H)
    assert set(np.unique(ids[np.isfinite(t)])) == {8, 9}              # the side z = 0 faces the camera
    assert list(np.nonzero(st.covered())[0]) == [8, 9]
    s = st.summary(model)
    assert s["covered_faces"] == 2 and s["covered_area"] == 1.0 and s["total_area"] == 6.0
    left = ref.regions(model, st)
    assert left["n_regions"] == 1 and left["n_faces"][0] == 10 and left["area"][0] == 5.0 and left["hits"][0] == 0
    assert left["peak"][0] == 0.0 and left["max_frames"][0] == 0 and left["first_face"][0] == 0
    seen = ref.regions(model, st, covered=True)
    assert seen["n_regions"] == 1 and seen["n_faces"][0] == 2 and seen["area"][0] == 1.0
    assert seen["hits"][0] == st.pixels.sum() > 0 and seen["max_frames"][0] == 1 and 0.99 < seen["peak"][0] <= 1.0
    assert ref.regions(model, st, covered=True, min_views=2)["n_regions"] == 0
    assert ref.regions(model, st, min_cos=1.5)["n_faces"][0] == 12      # nothing is covered at an impossible angle


def test_six_axis_views_cover_the_cube():
    K, W, H = ref.intrinsics(40.0, 40.0, 7.5, 7.5), 16, 16
    model = dref.Model(*dref.cube())
    st = ref.State(12)
    fractions = []
    for R in axis_views():
        v, tris = posed_cube(R)
        rec = ref.records(v, tris)
        t, ids = ref.host_cast(rec, ref.pixel_dirs(K, W, H))
        st.add(rec, K, W, H, t, ids)
        fractions.append(st.summary(model)["fraction"])
    assert fractions == [k / 6 for k in range(1, 6)] + [1.0]
    assert st.summary(model)["fraction"] == 1.0 and (st.views == 1).all() and st.n_views == 6
    assert ref.regions(model, st)["n_regions"] == 0 and ref.regions(model, st, covered=True)["n_faces"][0] == 12


def test_exports_in_the_header_the_bindings_the_library_and_compat():
    header = open(os.path.join(ROOT, "include", "pedp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    from pedp_hip import _lib, compat, coverage
    import pedp_hip

    lib = _lib.load()
    for name in EXPORTS:
        assert re.search(rf"\bint pedp_coverage_{name}\s*\(", code), name
        assert f"pedp_coverage_{name}" in _lib.PROTOTYPES
        assert hasattr(lib, f"pedp_coverage_{name}")
    for struct, binding in (("pedp_coverage_view", _lib.CoverageView), ("pedp_coverage_criteria", _lib.CoverageCriteria),
                            ("pedp_coverage_totals", _lib.CoverageTotals)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", code, flags=re.S).group(1)
        names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [n for n, _ in binding._fields_], struct
    assert compat.CoverageMap is coverage.CoverageMap is pedp_hip.CoverageMap and "CoverageMap" in compat.__all__
    assert "DESIGN.md s4.20" in header
    assert lib.pedp_coverage_create(None, None) == -1       # a null map is refused before anything else is looked at


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from pedp_hip import _lib
    from pedp_hip.coverage import CoverageMap

    def no_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_call)
    monkeypatch.setattr(_lib, "default_context", no_call)
    E = _lib.PedpError
    ctx, other = object(), object()
    cov = object.__new__(CoverageMap)
    cov.ctx, cov.F, cov._cameras = ctx, 12, {}

    def mesh(F=12, c=ctx):
        m = object.__new__(_lib.Mesh)
        m.ctx, m.F = c, F
        return m

    K = ref.intrinsics(40.0, 40.0, 1.5, 1.0)
    t, ids = np.zeros((3, 4), np.float32), np.zeros((3, 4), np.uint32)
    depth, mask = np.ones((3, 4), np.float32), np.ones((3, 4), np.uint8)
    bad = [
        ("faces", dict(mesh=mesh(F=11))),                                        # the mesh's F is not the map's
        ("another context", dict(mesh=mesh(c=other))),
        ("_lib.Mesh", dict(mesh=object())),
        ("depth_tol", dict(depth=depth)),                                        # no default
        ("depth_tol", dict(depth=depth, depth_tol=-1.0)),
        ("depth_tol", dict(depth=depth, depth_tol=float("nan"))),
        ("min_cos", dict(min_cos=-0.1)),
        ("min_cos", dict(min_cos=1.5)),
        ("min_cos", dict(min_cos=float("nan"))),
        ("depth_scale", dict(depth_scale=float("inf"))),
        ("3 x 3", dict(K=np.eye(4))),
        ("focal", dict(K=ref.intrinsics(0.0, 40.0, 1.5, 1.0))),
        ("H x W", dict(t_hit=np.zeros(12, np.float32))),
        ("t_hit must be float32", dict(t_hit=np.zeros((3, 4)))),
        ("primitive_ids must be H x W", dict(ids=np.zeros((4, 3), np.uint32))),
        ("uint32 or int32", dict(ids=np.zeros((3, 4), np.int64))),
        ("depth must be float32", dict(depth=np.ones((3, 4)), depth_tol=1.0)),
        ("depth must be H x W", dict(depth=np.ones((3, 5), np.float32), depth_tol=1.0)),
        ("mask must be uint8 or bool", dict(mask=np.ones((3, 4), np.int32))),
        ("mask must be H x W", dict(mask=np.ones((2, 4), np.uint8))),
        ("array or a tensor", dict(ids=[[0] * 4] * 3)),
    ]
    for what, kw in bad:
        kw = dict(kw)
        args = (kw.pop("mesh", mesh()), kw.pop("K", K), kw.pop("t_hit", t), kw.pop("ids", ids))
        with pytest.raises(E, match=what):
            cov.add_cast(*args, **kw)
    for what, kw in (("shape", dict(shape=(3,))), ("shape", dict(shape=(0, 4))), ("shape", dict(shape=(3.0, 4))),
                     ("depth_tol", dict(depth=depth)), ("depth must be H x W", dict(shape=(4, 3), depth=depth, depth_tol=1.0)),
                     ("min_cos", dict(min_cos=2.0)), ("faces", dict(mesh=mesh(F=3)))):
        kw = dict(kw)
        with pytest.raises(E, match=what):
            cov.add_view(kw.pop("mesh", mesh()), K, kw.pop("shape", (3, 4)), **kw)
    for fn in (cov.covered, cov.summary, cov.regions):
        for kw in (dict(min_views=1.0), dict(min_pixels=True), dict(min_cos="a"), dict(max_footprint=float("nan")),
                   dict(min_views=2 ** 31), dict(min_pixels=2 ** 63), dict(min_pixels=-2 ** 63 - 1)):
            with pytest.raises(E):
                fn(**kw)
    for grow in (-1, 65, 1.0, True):
        with pytest.raises(E, match="grow"):
            cov.regions(grow=grow)
    with pytest.raises(E, match="by must be"):
        cov.face_colors(by="hits")
    with pytest.raises(E, match="another context"):
        dm = object.__new__(__import__("pedp_hip").DefectMap)
        dm.ctx = ctx
        CoverageMap(dm, ctx=other)
