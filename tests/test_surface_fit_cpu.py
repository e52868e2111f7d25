"""CPU tests (no GPU) of the surface fit's numpy restatement (tests/_surface_fit_ref.py), which is the yardstick of the
GPU tests and has to be right on its own: 2,000 points on the triangles of the 50 x 40 torus, moved by a known rigid
motion of 2.7 degrees and 1.1 units, clean and with a dent (the points within 0.35 rad of azimuth 1.0 lifted 3 units)."""
import math

import numpy as np
import pytest

import _closest_ref as ref
import _surface_fit_ref as sf


def test_the_interface_is_exported():
    import pedp_hip
    from pedp_hip import _lib, compat, surface_fit

    for name in ("fit_to_surface", "refit_pose", "fit_frame_to_surface"):
        assert callable(getattr(surface_fit, name)) and getattr(compat, name) is getattr(surface_fit, name)
        assert name in compat.__all__
    assert "pedp_fit_to_surface" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["pedp_fit_to_surface"][1]) == 15
    assert "surface_fit.py" in pedp_hip.__doc__
    T = sf.MOTION
    pose = sf.rigid([0.1, 0.2, 0.3], [4.0, 5.0, 6.0])
    assert np.allclose(surface_fit.refit_pose(pose, T), np.linalg.inv(T) @ pose, rtol=0, atol=1e-15)
    with pytest.raises(_lib.PedpError, match="scale"):
        surface_fit.fit_to_surface(None, np.zeros((4, 3)), loss="tukey")
    with pytest.raises(_lib.PedpError, match="loss"):
        surface_fit.fit_to_surface(None, np.zeros((4, 3)), loss="cauchy")


def test_the_restated_search_has_the_bits_of_closest_ref():
    verts, tris, pts, _ = sf.torus_case(True)
    c, d, f = sf.closest(ref.records(verts, tris), pts[:256])
    want = ref.closest_ref(verts, tris, pts[:256])
    assert ref.same_bits({"points": c, "distances": d, "primitive_ids": f}, want, ("points", "distances", "primitive_ids")) is None
    sverts, stris, spts = sf.soup_case()
    c, d, f = sf.closest(ref.records(sverts, stris), spts[:256])
    want = ref.closest_ref(sverts, stris, spts[:256])
    assert ref.same_bits({"points": c, "distances": d, "primitive_ids": f}, want, ("points", "distances", "primitive_ids")) is None


def test_the_motion_is_the_one_quoted():
    rot, _ = sf.pose_errors(sf.MOTION, np.eye(4))
    assert abs(rot - 2.7) < 1e-9 and abs(np.linalg.norm(sf.MOTION[:3, 3]) - 1.1) < 1e-12
    _, _, pts, _ = sf.torus_case(True)
    _, _, clean, _ = sf.torus_case(False)
    lifted = np.linalg.norm(pts - clean, axis=1)
    assert 0.08 < (lifted > 0).mean() < 0.14 and np.allclose(lifted[lifted > 0], 3.0, rtol=0, atol=1e-9)


def test_clean_fit_recovers_the_motion():
    r = sf.torus_fit("clean")
    start = r["trace"][0, 1]
    assert start > 1.0 and r["iterations"] <= 10 and not r["singular"]
    assert r["rmse"] < 1e-6 * start
    assert r["fitness"] == 1.0 and r["K"] == 2000
    rot, tr = sf.pose_errors(r["T"], sf.MOTION)
    assert rot < 1e-5 and tr < 1e-8
    # every pass but the last moved the pose; the trace holds T as each pass found it
    assert np.array_equal(r["trace"][0, 3:].reshape(4, 4), np.eye(4)) and np.array_equal(r["trace"][-1, 3:].reshape(4, 4), r["T"])


def test_dent_pulls_l2_and_not_tukey():
    l2, huber, tukey = (sf.pose_errors(sf.torus_fit(k)["T"], sf.MOTION) for k in ("dent_l2", "dent_huber", "dent_tukey"))
    print(f"rotation / translation errors: l2 {l2}, huber {huber}, tukey {tukey}")
    assert l2[0] > 0.01 and l2[1] > 0.01                     # the dent does pull the plain least-squares pose
    for k in (0, 1):
        assert tukey[k] <= l2[k] / 10.0
        assert tukey[k] <= huber[k] <= l2[k]
    for name in ("dent_l2", "dent_huber", "dent_tukey"):
        r = sf.torus_fit(name)
        assert r["fitness"] == 1.0 and r["K"] == 2000 and not r["singular"]      # gate 10: the dent's points stay inliers


def test_summation_order_moves_the_fit_by_rounding_alone():
    """The floor the GPU test's bound is 100 times of: the fit with its sums forwards against the fit with them reversed."""
    worst_T = worst_rmse = 0.0
    for fwd, rev in [(sf.torus_fit(k), sf.torus_fit(k, True)) for k in sf.CASES] + [(sf.soup_fit(), sf.soup_fit(True))]:
        assert fwd["iterations"] == rev["iterations"] and np.array_equal(fwd["trace"][:, 2], rev["trace"][:, 2])
        worst_T = max(worst_T, np.abs(fwd["T"] - rev["T"]).max())
        worst_rmse = max(worst_rmse, abs(fwd["rmse"] - rev["rmse"]))
    print(f"forwards against reversed: T {worst_T:.3g}, rmse {worst_rmse:.3g}")
    assert worst_T <= sf.FLOOR_T and worst_rmse <= sf.FLOOR_RMSE


def test_weights():
    scale, gate = 1.5, 10.0
    below, above = np.nextafter(scale, 0.0), np.nextafter(scale, 2.0 * scale)
    d = np.array([0.0, below, scale, above, gate])
    assert np.array_equal(sf.weight("l2", None, d), np.ones(5))
    h = sf.weight("huber", scale, d)
    assert h[0] == 1.0 and h[1] == 1.0 and h[2] == 1.0 and h[3] == scale / above < 1.0 and h[4] == scale / gate
    t = sf.weight("tukey", scale, d)
    assert t[0] == 1.0 and 0.0 < t[1] < 1e-30 and t[2] == 0.0 and t[3] == 0.0 and t[4] == 0.0
    assert sf.weight("tukey", scale, np.array([0.75]))[0] == (1.0 - 0.25) ** 2
    # the gate is a test on the row, not on the weight: a row at the gate takes part, one beyond it adds nothing
    verts, tris = sf.soup(1, 1)
    a, ab, ac, _ = recs = ref.records(verts, tris)
    nrm = np.cross(ab[0], ac[0])
    nrm /= np.linalg.norm(nrm)
    cen = a[0] + (ab[0] + ac[0]) / 3.0
    pts = np.stack([cen + 2.0 * nrm, cen + 4.0 * nrm, a[0], np.full(3, np.nan)])      # (a vertex: d = 0 exactly)
    dist = sf.closest(recs, pts[:3])[1]
    terms, rows, finite = sf.row_terms(recs, pts, np.eye(4), "huber", 1.0, dist[0])
    assert rows.tolist() == [0, 2] and finite == 3
    assert terms[0, 28] == 1.0 and terms[0, 29] == 1.0 / dist[0] and terms[0, 27] == dist[0] * dist[0]
    assert terms[1, 27] == 0.0 and terms[1, 29] == 1.0                      # d = 0: the face's normal, residual 0
    assert abs(abs(terms[1, 20]) - nrm[2] ** 2) < 1e-12                     # [20] = n_z n_z
    with pytest.raises(ValueError):
        sf.weight("cauchy", 1.0, d)


def test_ldlt_and_update_restate_the_device_routines():
    rng = np.random.default_rng(0)
    B = rng.normal(size=(40, 6))
    A, b = B.T @ B, rng.normal(size=6)
    x, ok = sf.solve6_ldlt(A, b)
    assert ok and np.abs(A @ x - b).max() < 1e-12
    x, ok = sf.solve6_ldlt(np.zeros((6, 6)), b)
    assert ok and np.array_equal(x, np.zeros(6))             # no pivot: the component is dropped, as on the device
    T = sf.vec6_to_T([0.01, -0.02, 0.03, 1.0, 2.0, 3.0])
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), rtol=0, atol=1e-15) and T[:3, 3].tolist() == [1.0, 2.0, 3.0]
    assert math.isclose(T[1, 0], math.sin(0.03) * math.cos(-0.02))
