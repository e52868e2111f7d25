"""The defect map's restatement (tests/_defect_map_ref.py) against known answers, the exports and the Python argument
errors: everything here runs without a GPU."""
import os
import re

import numpy as np
import pytest

import _defect_map_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("create", "destroy", "size", "add", "clear", "faces", "stats", "regions")


def marked(model, faces, value=1.0, frames=1):
    st = ref.State(model.F)
    for _ in range(frames):
        st.add(np.asarray(faces), np.full(len(faces), value))
    return st


def test_unit_cube():
    m = ref.Model(*ref.cube())
    assert m.F == 12 and all(len(n) == 3 for n in m.neighbours)
    assert m.area.sum() == 6.0 and (m.area == 0.5).all()
    everything = ref.regions(m, marked(m, np.arange(12)))
    assert everything["n_regions"] == 1 and (everything["labels"] == 0).all()
    assert everything["area"][0] == 6.0 and everything["n_faces"][0] == 12 and everything["hits"][0] == 12
    assert np.allclose(everything["centroid"][0], 0.5, atol=1e-15)
    assert np.array_equal(everything["lo"][0], [0, 0, 0]) and np.array_equal(everything["hi"][0], [1, 1, 1])
    opposite = ref.regions(m, marked(m, [0, 1, 2, 3], value=0.75, frames=2), min_frames=2)   # the sides x = 0 and x = 1
    assert opposite["n_regions"] == 2
    assert list(opposite["labels"]) == [0, 0, 1, 1] + [-1] * 8
    assert list(opposite["first_face"]) == [0, 2] and list(opposite["n_faces"]) == [2, 2] and list(opposite["max_frames"]) == [2, 2]
    assert list(opposite["area"]) == [1.0, 1.0] and list(opposite["peak"]) == [0.75, 0.75] and list(opposite["hits"]) == [4, 4]
    assert np.allclose(opposite["centroid"], [[0.0, 0.5, 0.5], [1.0, 0.5, 0.5]], atol=1e-15)
    assert ref.regions(m, marked(m, [0, 1, 2, 3], frames=1), min_frames=2)["n_regions"] == 0
    assert ref.regions(m, marked(m, [0, 1, 2, 3], value=0.5))["n_regions"] == 0               # strictly above the threshold
    grown = ref.regions(m, marked(m, [0]), grow=1)
    assert grown["n_regions"] == 1 and grown["n_faces"][0] == 4 and grown["n_seed_faces"][0] == 1


def test_the_weld_holds_an_unwelded_cube_together():
    v, t = ref.unwelded(*ref.cube())
    assert len(v) == 36
    m = ref.Model(v, t)
    assert all(len(n) == 3 for n in m.neighbours)
    welded = ref.Model(*ref.cube())
    assert all(np.array_equal(a, b) for a, b in zip(m.neighbours, welded.neighbours))
    assert (m.w <= np.arange(36)).all() and len(np.unique(m.w)) == 8


def test_the_weld_on_signed_zeros_and_nan():
    v = np.array([[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [np.nan, 1.0, 2.0], [np.nan, 1.0, 2.0], [0.0, 1.0, 2.0], [3.0, 1.0, 2.0]])
    assert list(ref.weld(v)) == [0, 0, 2, 3, 0, 5]


def test_a_strip_between_two_rails():
    """2 x N vertices, 2 N - 2 triangles in a path: the marked ends are two regions, N / 2 rounds of growth join them and
    one round fewer does not."""
    N = 6
    m = ref.Model(*ref.strip(2 * N - 2))
    assert m.F == 10 and [len(n) for n in m.neighbours] == [1] + [2] * 8 + [1]
    ends = marked(m, [0, 1, 8, 9])
    two = ref.regions(m, ends)
    assert two["n_regions"] == 2 and list(two["first_face"]) == [0, 8]
    assert ref.regions(m, ends, grow=N // 2 - 1)["n_regions"] == 2
    one = ref.regions(m, ends, grow=N // 2)
    assert one["n_regions"] == 1 and one["n_faces"][0] == 10 and one["n_seed_faces"][0] == 4


def test_the_key_orders_like_the_values():
    x = np.array([-np.inf, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, np.inf])
    k = ref.key_of(x)
    assert (np.diff(k.astype(object)) > 0).all() and (k > 0).all()
    assert ref.same_bits(ref.value_of(k), x)
    st = ref.State(1).add([0, 0], [-0.0, 0.0])
    assert ref.same_bits(st.peak, np.array([0.0]))
    st = ref.State(2).add([0, 1, 5, ref.MISS, 1], [-2.0, np.nan, 1.0, 1.0, -0.0])
    assert list(st.hits) == [1, 1] and list(st.frames) == [1, 1] and ref.same_bits(st.peak, np.array([-2.0, -0.0]))
    assert st.stats() == {"observations": 1, "rows_added": 2, "rows_ignored": 3}


def test_fin_and_oddities():
    m = ref.Model(*ref.fin())
    assert [list(n) for n in m.neighbours] == [[1, 2], [0, 2], [0, 1]]
    m = ref.Model(*ref.oddities())
    assert m.area[16] == 0.0 and m.area[17] == 0.0 and np.isnan(m.area[18])
    assert list(m.neighbours[19]) == [20] and list(m.neighbours[17]) == [16]
    flat = ref.regions(m, marked(m, [16, 17]))
    assert flat["n_regions"] == 1 and flat["area"][0] == 0.0 and np.isnan(flat["centroid"][0]).all()


def test_exports_in_the_header_the_bindings_and_compat():
    header = open(os.path.join(ROOT, "include", "pedp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    from pedp_hip import _lib, compat, defect_map
    import pedp_hip

    for name in EXPORTS:
        assert re.search(rf"\bint pedp_defect_map_{name}\s*\(", code), name
        assert f"pedp_defect_map_{name}" in _lib.PROTOTYPES
    fields = re.search(r"typedef struct pedp_defect_region \{(.*?)\} pedp_defect_region;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[3\])?\s*[,;]", fields)
    assert names == ["first_face", "n_faces", "n_seed_faces", "max_frames", "hits", "area", "centroid", "moment", "peak", "lo", "hi"]
    assert list(defect_map.REGION_DTYPE.names) == names and defect_map.REGION_DTYPE.itemsize == 136
    assert compat.DefectMap is defect_map.DefectMap is pedp_hip.DefectMap and "DefectMap" in compat.__all__
    assert "DESIGN.md s4.17" in header


def test_argument_errors_come_before_any_launch():
    """None of these reaches the library: they raise without a context."""
    from pedp_hip import _lib
    from pedp_hip.defect_map import DefectMap, _check_region_args, _check_rows

    v, t = ref.cube()

    class Holder:
        vertices, triangles = v, t

    bad_models = [("hold .vertices", object()), ("V x 3", (v[:, :2], t)), ("V x 3", (v.astype(np.int32), t)),
                  ("F x 3", (v, t.reshape(-1, 2))), ("F x 3", (v, t.astype(np.float64))), ("indices", (v, t.astype(np.int64) - 1)),
                  ("indices", (v, t + np.uint32(1)))]
    for what, model in bad_models:
        with pytest.raises(_lib.PedpError, match=what):
            DefectMap(model)
    Holder.triangles = t + np.uint32(5)
    with pytest.raises(_lib.PedpError, match="indices"):
        DefectMap(Holder())
    ids, x = np.zeros(4, np.uint32), np.zeros(4)
    _check_rows(ids, x)
    _check_rows(ids.astype(np.int64), x.astype(np.float32))
    for what, a, b in (("array or a tensor", [0, 1], x), ("1-D", ids.reshape(2, 2), x.reshape(2, 2)), ("one length", ids, x[:3]),
                       ("uint32, int32 or int64", ids.astype(np.int16), x), ("uint32, int32 or int64", ids.astype(np.float64), x),
                       ("float32 or float64", ids, x.astype(np.float16)), ("float32 or float64", ids, ids)):
        with pytest.raises(_lib.PedpError, match=what):
            _check_rows(a, b)
    _check_region_args(1, 0)
    _check_region_args(np.int32(2), 64)
    for mf, g in ((1, -1), (1, 65), (1, 1.0), (1.5, 0), (1, True)):
        with pytest.raises(_lib.PedpError):
            _check_region_args(mf, g)
