"""tests/_sample_ref.py, the numpy restatement of the surface sampler's contract, pinned on its own: the
generator's known answers, the slice property, the distribution over faces, the thinning's two forms and guarantees, the
count form.  And what the Python layer refuses before it reaches the device."""
import numpy as np
import pytest
from scipy.stats import chi2

import _sample_ref as S


def hex4(words):
    return " ".join(f"{int(w[0]):08x}" for w in words)


def test_philox_known_answers():
    assert hex4(S.philox(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert hex4(S.philox(ones, ones, ones, ones, ones, ones)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    # Random123's third vector: the digits of pi as counter and key
    assert hex4(S.philox(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_a_slice_is_a_slice_of_one_sequence():
    v, t = S.cube()
    vn = S.vertex_normals(v, t)
    whole = S.sample(v, t, 150, seed=7, normals=S.NORMALS_VERTEX, vertex_normals=vn)
    part = S.sample(v, t, 50, seed=7, first=100, normals=S.NORMALS_VERTEX, vertex_normals=vn)
    for name in ("points", "face_ids", "barycentric", "normals", "z"):
        assert np.array_equal(part[name], whole[name][100:150]), name
    other = S.sample(v, t, 50, seed=8, first=100)
    assert not np.array_equal(other["points"], part["points"])


def test_counter_carries_into_the_high_word():
    k = S.sample_numbers(2 ** 32 - 2, 4)
    assert [int(x) for x in k] == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    assert [int(x) for x in S.sample_numbers(2 ** 64 - 1, 2)] == [2 ** 64 - 1, 0]
    x = S.draw(k, 0, 3)
    assert hex4([w[2:3] for w in x]) == hex4(S.philox(0, 1, 0, 0, 3, 0))


def test_face_table():
    v, t = S.with_dead_faces()
    area, amax, w, c, total, a_sum = S.face_table(v, t)
    assert amax == 0.5 and list(w) == [2 ** 32, 0, 2 ** 32, 0] and total == 2 ** 33
    assert area[1] == 0.0 and area[3] == 2.0 ** -35
    assert a_sum == (0.5 + 0.0 + 0.5) + 2.0 ** -35
    s = S.sample(v, t, 4000, seed=2)
    assert set(np.unique(s["face_ids"])) == {0, 2}
    v, t = S.two_triangles_1_3()
    assert list(S.face_table(v, t)[2]) == [(2 ** 32) // 3, 2 ** 32]


@pytest.mark.parametrize("seed", range(5))
def test_faces_are_drawn_by_area(seed):
    v, t = S.cube()
    n = 60000
    got = np.bincount(S.sample(v, t, n, seed=seed)["face_ids"], minlength=len(t))
    want = n * S.face_table(v, t)[0] / 6.0
    stat = float(((got - want) ** 2 / want).sum())
    p = float(chi2.sf(stat, len(t) - 1))
    print(f"seed {seed}: chi-square {stat:.2f}, p = {p:.3f}")
    assert p > 1e-3


def test_points_lie_in_their_faces():
    v, t = S.icosphere(1)
    s = S.sample(v, t, 500, seed=1, normals=S.NORMALS_TRIANGLE)
    b = s["barycentric"]
    assert (b >= 0).all() and np.abs(b.sum(axis=1) - 1.0).max() <= 2 ** -52
    tri = v[t.astype(np.int64)[s["face_ids"]]]
    assert np.array_equal(s["points"], (b[:, :1] * tri[:, 0] + b[:, 1:2] * tri[:, 1]) + b[:, 2:] * tri[:, 2])
    assert np.abs(np.linalg.norm(s["normals"], axis=1) - 1.0).max() < 1e-15
    assert (np.einsum("ij,ij->i", s["normals"], s["points"]) > 0).all()       # outward on a sphere about the origin


def guarantees(p, kept, r):
    """on the output alone, by the full distance matrix"""
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    kk = d2[np.ix_(kept, kept)]
    np.fill_diagonal(kk, np.inf)
    assert not (kk < r * r).any()                      # no two kept points are closer than r
    assert (d2[:, kept] < r * r).any(axis=1).all()     # every point is closer than r to a kept one (itself, if kept)


def test_greedy_equals_rounds_and_keeps_both_guarantees():
    v, t = S.cube()
    s = S.sample(v, t, 2000, seed=0)
    p, key = s["points"], S.keys(s["z"])
    kept = S.thin(p, key, 0.1)
    by_rounds, rounds = S.thin_rounds(p, key, 0.1)
    print(f"kept {kept.sum()} of 2000 in {rounds} rounds")
    assert np.array_equal(kept, by_rounds) and 2 <= rounds <= 32
    guarantees(p, np.flatnonzero(kept), 0.1)
    # a given cloud's keys are a hash of (index, seed): raster order does not make the chain long
    q = np.stack([np.arange(500) * 0.06, np.zeros(500), np.zeros(500)], axis=1)
    a, rounds = S.thin_rounds(q, S.cloud_keys(500, 0), 0.1)
    assert np.array_equal(a, S.thin(q, S.cloud_keys(500, 0), 0.1)) and rounds <= 16
    guarantees(q, np.flatnonzero(a), 0.1)


def test_thinning_edges():
    p = np.array([[0, 0, 0], [3, 4, 0]], np.float64)
    key = S.cloud_keys(2, 0)
    assert S.thin(p, key, 5.0).all()                                     # strict: a distance of exactly r is no conflict
    assert S.thin(p, key, np.nextafter(5.0, np.inf)).sum() == 1
    assert S.thin(p, key, 0.0).all() and S.thin(np.zeros((0, 3)), key[:0], 1.0).shape == (0,)
    same = np.ones((300, 3))
    key = S.cloud_keys(300, 5)
    assert list(np.flatnonzero(S.thin(same, key, 1e-3))) == [int(np.argmin(key))]


@pytest.mark.parametrize("n", [100, 500])
def test_count_form_returns_n_points_no_closer_than_r(n):
    v, t = S.cube()
    d = S.sample_disk(v, t, n, seed=0)
    assert len(d["index"]) == n == len(d["points"]) and d["drawn"] == 5 * n and (np.diff(d["index"]) > 0).all()
    p = d["points"]
    dist = np.linalg.norm(p[:, None] - p[None], axis=2)
    np.fill_diagonal(dist, np.inf)
    print(f"N = {n}: r* = {d['spacing']!r} = {d['spacing'] / np.sqrt(6.0 / n):.4f} sqrt(A / N), minimum distance {dist.min():.6f}")
    assert 0.0 < d["spacing"] <= dist.min()
    assert 0.5 * np.sqrt(6.0 / n) < d["spacing"] < 2.0 * np.sqrt(6.0 / n)


def test_python_layer_names_the_bad_argument():
    from pedp_hip import PedpError, mesh_sample
    from pedp_hip.geometry import TriangleMesh

    v, t = S.cube()
    mesh = TriangleMesh(v, t)
    for call, word in [(lambda: mesh.sample_points_uniformly(0), "number_of_points"),
                       (lambda: mesh.sample_points_poisson_disk(0), "number_of_points"),
                       (lambda: mesh.sample_points_poisson_disk(-3), "number_of_points"),
                       (lambda: mesh.sample_points_poisson_disk(), "number_of_points or spacing"),
                       (lambda: mesh.sample_points_poisson_disk(10, spacing=0.1), "number_of_points or spacing"),
                       (lambda: mesh.sample_points_poisson_disk(10, init_factor=0), "init_factor"),
                       (lambda: mesh.sample_points_poisson_disk(spacing=-0.1), "spacing"),
                       (lambda: mesh.sample_points_poisson_disk(spacing=float("nan")), "spacing"),
                       (lambda: mesh_sample.thin_to_spacing(np.zeros((4, 3)), -1.0), "spacing"),
                       (lambda: mesh_sample.thin_to_spacing(np.zeros((4, 3)), float("nan")), "spacing"),
                       (lambda: mesh_sample.thin_to_spacing(np.zeros((4, 2)), 1.0), "points")]:
        with pytest.raises(PedpError, match=word):
            call()
    import pedp_hip
    from pedp_hip import compat

    for name in ("sample_points_uniformly", "sample_points_poisson_disk", "thin_to_spacing", "mesh_to_pcd"):
        assert getattr(compat, name) is getattr(mesh_sample, name) is getattr(pedp_hip, name) and name in compat.__all__
