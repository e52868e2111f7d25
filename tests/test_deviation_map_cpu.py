"""The deviation map's restatement (tests/_deviation_map_ref.py) against known answers, the exports and
the Python argument errors: everything here runs without a GPU."""
import math
import os
import re

import numpy as np
import pytest

import _defect_map_ref as dref
import _deviation_map_ref as ref
from pedp_hip import deviation_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("create", "destroy", "clear", "add", "add_points", "faces", "stats", "summary", "regions")
Q = 2.0 ** -20


def one_face(d, gate=ref.MAX_GATE, F=1):
    d = np.asarray(d, dtype=np.float64)
    st = ref.State(F).add(np.zeros(len(d), np.uint32), d, gate)
    return st, {k: v[0] for k, v in st.faces().items()}


def test_plus_one_and_minus_one():
    st, f = one_face([1.0, -1.0])
    assert (f["n"], f["frames"], f["s1"]) == (2, 1, 0) and (f["s2_hi"], f["s2_lo"]) == (0, 2 * 2 ** 40)
    assert (f["mean"], f["std"], f["min"], f["max"]) == (0.0, 1.0, -1.0, 1.0)


@pytest.mark.parametrize("d", [0.0, 3 * Q, -12345 * Q, 0.5, -1024.0, 1024.0])
@pytest.mark.parametrize("k", [1, 2, 7, 1000])
def test_equal_rows_have_their_value_as_mean_and_no_spread(d, k):
    _, f = one_face([d] * k)
    assert f["n"] == k and f["mean"] == d and f["std"] == 0.0 and f["min"] == f["max"] == d


def test_ties_round_to_even():
    k = np.array([0, 1, 2, 3, -1, -2, -3, 2 ** 29, -(2 ** 29) - 1], dtype=np.int64)
    q = ref.quantise((k + 0.5) * Q)
    assert np.array_equal(q, np.where(k % 2 == 0, k, k + 1))
    assert np.array_equal(ref.quantise([0.49999 * Q, 0.50001 * Q, -0.50001 * Q]), [0, 1, -1])


def test_the_gate_is_inclusive_and_counts_what_it_drops():
    gate = 0.75
    d = [gate, -gate, np.nextafter(gate, np.inf), -np.nextafter(gate, np.inf), np.inf, -np.inf, np.nan, 0.1]
    ids = np.zeros(len(d), np.uint32)
    ids[-1] = 5                                       # no such face
    st = ref.State(1).add(ids, d, gate)
    assert st.stats() == {"observations": 1, "rows_taken": 2, "rows_ignored": 2, "rows_gated": 4, "rows_backfacing": 0}
    f = st.faces()
    assert f["n"][0] == 2 and f["min"][0] == -gate and f["max"][0] == gate and f["mean"][0] == 0.0
    st0 = ref.State(1).add([0, 0, 0], [0.0, -0.0, np.nextafter(0.0, 1.0)], 0.0)       # gate 0 takes +-0 alone
    assert st0.rows_taken == 2 and st0.rows_gated == 1


def test_minus_zero_is_zero():
    _, f = one_face([-0.0, -0.0])
    assert f["s1"] == 0 and f["s2_lo"] == 0 and f["std"] == 0.0
    for k in ("mean", "min", "max"):
        assert f[k] == 0.0 and not np.signbit(f[k]), k      # q is an integer: there is one zero


def test_an_empty_observation_counts_and_an_empty_face_reads_nan():
    st = ref.State(3).add(np.zeros(0, np.uint32), np.zeros(0))
    st.add([1], [0.25])
    f = st.faces()
    assert st.observations == 2 and list(f["n"]) == [0, 1, 0] and list(f["frames"]) == [0, 1, 0]
    for k in ("mean", "std", "min", "max"):
        assert np.isnan(f[k][[0, 2]]).all() and not np.isnan(f[k][1]), k


def test_the_sum_of_squares_crosses_two_to_the_64():
    d = np.full(4097, 1000.0)
    st, f = one_face(d)
    assert st.s2[0] == 4097 * (1000 * 2 ** 20) ** 2 > 2 ** 64 and f["s2_hi"] >= 1
    assert (int(f["s2_hi"]) << 64) + int(f["s2_lo"]) == st.s2[0]
    assert f["mean"] == 1000.0 and f["std"] == 0.0
    d[::2] = -1000.0                                  # 2049 below, 2048 above
    st, f = one_face(d)
    n, s1 = 4097, -1000 * 2 ** 20
    assert f["s1"] == s1 and f["mean"] == (float(s1) / n) * Q
    assert f["std"] == math.sqrt((float(n * st.s2[0] - s1 * s1) / (float(n) * float(n))) * 2.0 ** -40)
    assert abs(f["std"] - 1000.0 * math.sqrt(1.0 - 1.0 / n ** 2)) <= 1e-12 * 1000.0


def test_float_of_int_rounds_a_128_bit_integer_to_nearest_even():
    assert float(2 ** 100 + 2 ** 47) == 2.0 ** 100                      # the tie goes to the even neighbour
    assert float(2 ** 100 + 2 ** 47 + 1) == 2.0 ** 100 + 2.0 ** 48      # a sticky bit breaks it
    assert float(2 ** 100 + 3 * 2 ** 47) == 2.0 ** 100 + 2.0 ** 49


def test_order_does_not_matter_and_a_split_changes_only_the_frames():
    rng = np.random.default_rng(7)
    ids = rng.integers(0, 6, 500).astype(np.uint32)
    d = rng.normal(0.0, 0.5, 500)
    d[::17] = np.nan
    ids[::23] = dref.MISS
    a = ref.State(5).add(ids, d, 1.0).faces()
    p = rng.permutation(500)
    b = ref.State(5).add(ids[p], d[p], 1.0).faces()
    two = ref.State(5).add(ids[:250], d[:250], 1.0).add(ids[250:], d[250:], 1.0)
    c = two.faces()
    for k in ref.FACE_KEYS:
        assert dref.same_bits(a[k], b[k]), k
        if k != "frames":
            assert dref.same_bits(a[k], c[k]), k
    assert (a["frames"] == 1).all() and (c["frames"] == 2).all() and two.observations == 2


def test_the_volume_of_a_lifted_cube_face():
    model = dref.Model(*dref.cube())
    lift = 0.125
    ids = np.repeat(np.arange(12, dtype=np.uint32), 9)
    d = np.where(ids < 2, lift, 0.0)                  # the face x = 0 (two triangles of area 1/2)
    st = ref.State(12).add(ids, d)
    r = ref.regions(model, st, threshold=0.05, sign=+1)
    assert r["n_regions"] == 1 and r["n_faces"][0] == 2 and r["first_face"][0] == 0 and r["hits"][0] == 18
    assert r["area"][0] == r["measured_area"][0] == 1.0 and r["volume"][0] == 1.0 * lift
    assert r["min_mean"][0] == r["max_mean"][0] == r["peak"][0] == lift
    assert ref.regions(model, st, threshold=0.05, sign=-1)["n_regions"] == 0
    grown = ref.regions(model, st, threshold=0.05, grow=1)                  # the neighbours are measured and flat
    assert grown["n_faces"][0] > 2 and grown["volume"][0] == lift and grown["measured_area"][0] == grown["area"][0]
    s = ref.summary(model, st, threshold=0.05)
    assert s["measured_faces"] == 12 and s["marked_faces"] == 2 and s["marked_area"] == 1.0 and s["total_area"] == 6.0
    assert s["s1"] == lift and s["max_abs_mean"] == lift and s["max_face"] == 0


def test_marking_by_sign_significance_and_samples():
    faces = {"n": np.array([0, 1, 4, 4, 100, 100], np.int64), "frames": np.array([0, 1, 1, 2, 3, 3], np.int32),
             "mean": np.array([np.nan, 0.5, -0.5, 0.5, 0.1, 0.1]), "std": np.array([np.nan, 0.0, 1.0, 0.2, 0.5, 0.1])}
    m = lambda **kw: list(ref.marked(faces, **kw).astype(int))    # noqa: E731
    assert m(threshold=0.3) == [0, 1, 1, 1, 0, 0]
    assert m(threshold=0.3, sign=+1) == [0, 1, 0, 1, 0, 0]
    assert m(threshold=0.3, sign=-1) == [0, 0, 1, 0, 0, 0]
    assert m(threshold=0.5) == [0, 0, 0, 0, 0, 0]                 # strictly above
    assert m(threshold=0.3, min_samples=4) == [0, 0, 1, 1, 0, 0]
    assert m(threshold=0.3, min_frames=2) == [0, 0, 0, 1, 0, 0]
    # |mean| sqrt(n) > z std: 0.5 > 0, 1 > 3? no, 1 > 0.6, 1 > 1.5? no, 1 > 0.3
    assert m(threshold=0.05, z=3.0) == [0, 1, 0, 1, 0, 1]
    assert m(threshold=-1.0, min_samples=0) == [0, 1, 1, 1, 1, 1]      # a face without rows is never marked


def test_the_clean_part_marks_nothing_at_four_sigma_where_a_peak_marks_more_with_every_frame():
    """A condition on the input of test_deviation_map_gpu.py's clean-part test (the seed of _deviation_map_ref.CLEAN), and
    the reason for the map: the mean's significance stays put while a peak over frames keeps growing."""
    c = ref.CLEAN
    st, peaks = ref.State(c["F"]), []
    peak = np.zeros(c["F"])
    for k in range(c["frames"]):
        ids, d = ref.noisy_rows(k)
        st.add(ids, d, 3.0)
        np.maximum.at(peak, ids, np.abs(d))
        peaks.append(int((peak > 3.0 * c["sigma"]).sum()))
    f = st.faces()
    assert (f["n"] >= c["frames"] * c["per_face"] - 5).all() and st.rows_gated < 20
    assert not ref.marked(f, z=c["z"]).any() and ref.marked(f, z=1.0).any()
    assert np.abs(f["mean"]).max() < 4.0 * c["sigma"] / np.sqrt(f["n"].min())
    assert peaks[0] < peaks[3] < peaks[15] and peaks[15] > c["F"] // 10


def test_exports_in_the_header_the_bindings_the_library_and_compat():
    header = open(os.path.join(ROOT, "include", "pedp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    from pedp_hip import _lib, compat
    import pedp_hip

    lib = _lib.load()
    for name in EXPORTS:
        assert re.search(rf"\bint pedp_deviation_map_{name}\s*\(", code), name
        assert f"pedp_deviation_map_{name}" in _lib.PROTOTYPES
        assert hasattr(lib, f"pedp_deviation_map_{name}")
    for struct, binding in (("pedp_deviation_criteria", _lib.DeviationCriteria), ("pedp_deviation_totals", _lib.DeviationTotals)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", code, flags=re.S).group(1)
        names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [n for n, _ in binding._fields_], struct
    row = re.search(r"typedef struct pedp_deviation_region \{(.*?)\} pedp_deviation_region;", code, flags=re.S).group(1)
    extra = [n for decl in row.split(";")[1:] for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert list(deviation_map.DEVIATION_REGION_DTYPE.names) == list(deviation_map.REGION_DTYPE.names) + extra
    assert compat.DeviationMap is deviation_map.DeviationMap is pedp_hip.DeviationMap and "DeviationMap" in compat.__all__
    assert "DESIGN.md s4.23" in header and deviation_map.MAX_GATE == ref.MAX_GATE and deviation_map.Q == ref.Q
    assert lib.pedp_deviation_map_create(None, None) == -1     # a null map is refused before anything else is looked at


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from pedp_hip import _lib
    from pedp_hip.deviation_map import DeviationMap

    def no_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_call)
    monkeypatch.setattr(_lib, "default_context", no_call)
    E = _lib.PedpError
    ctx, other = object(), object()
    dm = object.__new__(DeviationMap)
    dm.ctx, dm.F, dm._owns_map = ctx, 12, False

    def handle(cls, c=ctx, F=12):
        h = object.__new__(cls)
        h.ctx, h.F = c, F
        return h

    ids, d = np.zeros(4, np.uint32), np.zeros(4)
    for what, a, kw in (("array or a tensor", ([0] * 4, d), {}), ("1-D of one length", (ids, np.zeros(5)), {}),
                        ("1-D of one length", (ids.reshape(2, 2), d.reshape(2, 2)), {}), ("uint32, int32 or int64", (d, d), {}),
                        ("float32 or float64", (ids, ids), {}), ("gate must be a number in 0 ... 1024", (ids, d), dict(gate=-1.0)),
                        ("got 1025", (ids, d), dict(gate=1025)), ("got nan", (ids, d), dict(gate=float("nan"))),
                        ("got None", (ids, d), dict(gate=None))):
        with pytest.raises(E, match="DeviationMap.add: .*" + what):
            dm.add(*a, **kw)
    mesh, solid, pts = handle(_lib.Mesh), handle(_lib.Solid), np.zeros((5, 3))
    for what, a, kw in (("mesh must be a _lib.Mesh, got object", (object(), pts, solid), {}),
                        ("solid must be a Solid, got NoneType", (mesh, pts, None), {}),
                        ("the mesh belongs to another context", (handle(_lib.Mesh, other), pts, solid), {}),
                        ("the solid belongs to another context", (mesh, pts, handle(_lib.Solid, other)), {}),
                        ("the mesh has 11 faces, the map 12", (handle(_lib.Mesh, F=11), pts, solid), {}),
                        ("points must be N x 3", (mesh, np.zeros((5, 2)), solid), {}), ("points must be N x 3", (mesh, [[0, 0, 0]], solid), {}),
                        ("float32 or float64, got int32", (mesh, np.zeros((5, 3), np.int32), solid), {}),
                        ("gate", (mesh, pts, solid), dict(gate=2000.0)), ("origin must be 3 finite", (mesh, pts, solid), dict(origin=(0, 0))),
                        ("origin must be 3 finite", (mesh, pts, solid), dict(origin=(0.0, np.inf, 0.0)))):
        with pytest.raises(E, match="DeviationMap.add_points: .*" + what):
            dm.add_points(*a, **kw)
    for what, kw in (("sign must be -1", dict(sign=2)), ("sign must be -1", dict(sign=1.0)), ("threshold must be a number", dict(threshold="1")),
                     ("z must be a number, got nan", dict(z=float("nan"))), ("min_samples must be an int64", dict(min_samples=1.5)),
                     ("min_frames must be an int32", dict(min_frames=2 ** 31))):
        with pytest.raises(E, match="DeviationMap.regions: " + what):
            dm.regions(**dict(dict(threshold=0.1), **kw))
        with pytest.raises(E, match="DeviationMap.summary: " + what):
            dm.summary(**kw)
    with pytest.raises(E, match="grow must be an integer in 0 ... 64, got 65"):
        dm.regions(0.1, grow=65)
    for limit in (0.0, -1.0, None, float("nan")):
        with pytest.raises(E, match="face_colors: limit must be a positive number"):
            dm.face_colors(limit)
    dm._h = None
    for call in (lambda: dm.add(ids, d), lambda: dm.add_points(mesh, pts, solid), dm.clear, dm.faces, dm.stats, dm.summary,
                 lambda: dm.regions(0.1)):
        with pytest.raises(E, match="the deviation map is closed"):
            call()
    dm._h, dm.defect_map = 1, type("Closed", (), {"_h": None})()
    for call in (lambda: dm.add(ids, d), dm.clear, dm.faces, lambda: dm.regions(0.1)):
        with pytest.raises(E, match="the defect map under the deviation map is closed"):
            call()
    dm._h = None                                      # nothing for __del__ to destroy
