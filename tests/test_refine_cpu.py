"""tests/_refine_ref.py, the numpy restatement of pedp_mesh_refine's contract, pinned on its own: the four templates on
one triangle against arrays written by hand, the vectorised form against the plain loops, and on closed meshes what the
contract promises (no long edge left, a conforming closed oriented surface of the same area and volume, parent ids)."""
import numpy as np
import pytest

import _refine_ref as R

CASES = R.single_triangle_cases()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("form", [R.refine, R.refine_loop], ids=["vectorised", "loop"])
def test_single_triangle_templates(case, form):
    name, v, t, max_edge, want_v, want_t = case
    got_v, got_t, pf, rounds = form(v, t, max_edge)
    assert same_bits(got_v, want_v), (name, got_v)
    assert same_bits(got_t, want_t), (name, got_t)
    assert same_bits(pf, np.zeros(len(want_t), np.int32))
    assert rounds == (0 if name == "none" else 1)


def test_cases_cover_every_set_of_long_edges():
    seen = set()
    for name, v, t, max_edge, _, _ in CASES:
        p = v[t[0].astype(np.int64)]
        seen.add(tuple(bool(x) for x in R.len2(p, p[R.NXT]) > max_edge * max_edge))
    assert len(seen) == 8


def test_tie_takes_the_first_diagonal():
    name, v, t, max_edge, _, want_t = next(c for c in CASES if c[0] == "two-tie-short2")
    m0, m1 = 0.5 * (v[0] + v[1]), 0.5 * (v[1] + v[2])
    assert R.len2(m0, v[2]) == R.len2(m1, v[0])
    assert (want_t[1] == (0, 3, 2)).all()


MESHES = {"tetrahedron": R.tetrahedron(), "cube": R.cube(), "icosphere1": R.icosphere(1),
          "cube-split": R.split_vertices(*R.cube(), faces=[0, 5, 10])}


@pytest.mark.parametrize("name,max_edge", [("tetrahedron", 5.0), ("tetrahedron", 1.0), ("tetrahedron", 0.3), ("cube", 1.0),
                                           ("cube", 0.6), ("cube", 0.11), ("icosphere1", 0.5), ("icosphere1", 0.17),
                                           ("cube-split", 0.3)])
def test_closed_meshes_keep_what_the_contract_promises(name, max_edge):
    v0, t0 = MESHES[name]
    v, t, pf, rounds = R.refine(v0, t0, max_edge)
    assert R.longest_edge(v, t) <= max_edge
    assert same_bits(v[:len(v0)], v0)
    assert R.edge_pairing(v0, t0) == (0, 0)
    assert R.edge_pairing(v, t) == (0, 0)                      # every welded edge: two faces, opposite directions
    area0, area = R.face_areas(v0, t0), R.face_areas(v, t)
    per_parent = np.add.reduceat(area, np.flatnonzero(np.r_[True, pf[1:] != pf[:-1]]))
    assert np.allclose(per_parent, area0, rtol=1e-12, atol=0.0)
    assert abs(R.signed_volume(v, t) - R.signed_volume(v0, t0)) <= 1e-12 * abs(R.signed_volume(v0, t0))
    assert (np.diff(pf) >= 0).all() and same_bits(np.unique(pf), np.arange(len(t0), dtype=np.int32))
    ulps = R.plane_distance_ulps(v0, t0, v, t, pf)
    print(f"{name} max_edge {max_edge}: {len(t)} faces, {rounds} rounds, plane distance {ulps:.3f} ulp")
    assert ulps <= 4.0
    if len(t) <= 600:
        for a, b in zip(R.refine_loop(v0, t0, max_edge), (v, t, pf, rounds)):
            assert same_bits(np.asarray(a), np.asarray(b))


def test_vectorised_and_loop_agree_on_odd_meshes():
    rng = np.random.default_rng(5)
    v = rng.uniform(-1.0, 1.0, (9, 3))
    v[7] = v[2]                                                # a duplicated vertex
    t = np.array([[0, 1, 2], [7, 1, 3], [4, 5, 6], [2, 7, 8], [3, 3, 5], [6, 5, 4], [0, 2, 1]], np.uint32)
    for max_edge in (0.9, 0.45, 0.2):
        for a, b in zip(R.refine_loop(v, t, max_edge), R.refine(v, t, max_edge)):
            assert same_bits(np.asarray(a), np.asarray(b))


def test_bad_arguments():
    v, t = R.cube()
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            R.refine(v, t, bad)
    with pytest.raises(ValueError):
        R.refine(v, np.array([[0, 1, 8]], np.uint32), 1.0)
    w = v.copy()
    w[3, 1] = np.nan
    with pytest.raises(ValueError):
        R.refine(w, t, 1.0)
    n = len(R.refine(v, t, 0.3)[1])
    with pytest.raises(ValueError):
        R.refine(v, t, 0.3, max_faces=n - 1)
    assert len(R.refine(v, t, 0.3, max_faces=n)[1]) == n


def test_refine_mesh_checks_its_arguments_before_the_device():
    from pedp_hip import PedpError
    from pedp_hip.mesh_refine import RefinedMesh, refine_mesh

    v, t = R.cube()
    for mesh in (v, (v[:, :2], t), (v, t[:, :2]), (v.astype(np.int32), t), (v, t.astype(np.float64)), (v, -t.astype(np.int64) - 1)):
        with pytest.raises(PedpError, match="refine_mesh:"):
            refine_mesh(mesh, 0.5)
    with pytest.raises(PedpError, match="refine_mesh: max_edge"):
        refine_mesh((v, t), "fine")
    fine = RefinedMesh(None, None, v, t, np.arange(12, dtype=np.int32), 12, 0, 2.0)     # what a 0-round call returns
    with pytest.raises(PedpError, match="how must be"):
        fine.reduce_to_parent(np.zeros(12), "mean")
    with pytest.raises(PedpError, match="values must have shape"):
        fine.reduce_to_parent(np.zeros(11), "max")
    ids = np.array([0, 11, 12, 0xFFFFFFFF], np.uint32)
    assert fine.parent_of(ids).tolist() == [0, 11, -1, -1] and fine.parent_of(ids.view(np.int32)).tolist() == [0, 11, -1, -1]


def test_edge_for_camera():
    from pedp_hip import PedpError
    from pedp_hip.geometry import PinholeCameraIntrinsic
    from pedp_hip.mesh_refine import edge_for_camera

    assert edge_for_camera(PinholeCameraIntrinsic(640, 480, 400.0, 800.0, 320.0, 240.0), 2.0, pixels=1.0) == 2.0 / 400.0
    for bad in ((np.eye(4), 1.0), (np.eye(3), 0.0), (np.eye(3), np.inf), (np.zeros((3, 3)), 1.0)):
        with pytest.raises(PedpError, match="edge_for_camera:"):
            edge_for_camera(*bad)

    K = np.array([[600.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    assert edge_for_camera(K, 0.5) == 2.0 * 0.5 / 500.0
    assert edge_for_camera(K, 0.5, pixels=3.0) == 3.0 * 0.5 / 500.0
