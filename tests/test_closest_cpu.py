"""CPU tests of the closest-point feature (no GPU): the numpy restatement of the contract (tests/_closest_ref.py) on
analytic cases and against a barycentric grid search, the skipped records, the Python functions' argument validation,
the compat exports and the heat map's gating arithmetic."""
import numpy as np
import pytest

import _closest_ref as ref

# a = (0, 0, 0), b = (1, 0, 0), c = (0, 1, 0): every expected value below is exact in binary
TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
TRI_T = np.array([[0, 1, 2]], np.uint32)
# rule, query, (v, w), closest point, squared distance
REGIONS = [
    (1, (-1.0, -1.0, 1.0), (0.0, 0.0), (0.0, 0.0, 0.0), 3.0),
    (2, (2.0, -0.5, 0.0), (1.0, 0.0), (1.0, 0.0, 0.0), 1.25),
    (3, (0.25, -1.0, 0.0), (0.25, 0.0), (0.25, 0.0, 0.0), 1.0),
    (4, (-0.5, 2.0, 0.0), (0.0, 1.0), (0.0, 1.0, 0.0), 1.25),
    (5, (-1.0, 0.25, 0.0), (0.0, 0.25), (0.0, 0.25, 0.0), 1.0),
    (6, (1.0, 1.0, 0.0), (0.5, 0.5), (0.5, 0.5, 0.0), 0.5),
    (7, (0.25, 0.25, 2.0), (0.25, 0.25), (0.25, 0.25, 0.0), 4.0),
]


@pytest.mark.parametrize("rule, p, vw, c, d2", REGIONS, ids=[f"rule{r[0]}" for r in REGIONS])
def test_one_analytic_query_per_region(rule, p, vw, c, d2):
    a, ab, ac, skip = ref.records(TRI_V, TRI_T)
    assert not skip[0]
    assert ref.region(np.array(p), a[0], ab[0], ac[0]) == rule
    out = ref.closest_ref(TRI_V, TRI_T, np.array([p]))
    assert tuple(out["primitive_uvs"][0]) == vw
    assert tuple(out["points"][0]) == c
    assert out["distances"][0] == np.sqrt(d2)
    assert out["primitive_ids"][0] == 0
    assert out["sides"][0] == (1 if p[2] > 0 else 0)        # the normal ab x ac is +z


def test_side_is_the_face_normals_side():
    out = ref.closest_ref(TRI_V, TRI_T, np.array([[0.25, 0.25, 2.0], [0.25, 0.25, -2.0], [0.25, 0.25, 0.0]]))
    assert out["sides"].tolist() == [1, -1, 0]
    flipped = ref.closest_ref(TRI_V, np.array([[0, 2, 1]], np.uint32), np.array([[0.25, 0.25, 2.0]]))
    assert flipped["sides"].tolist() == [-1]


def test_restatement_against_a_barycentric_grid_search():
    """29 random triangles x 300 points: never above the minimum over a 41 x 41 barycentric grid, and below it by no more
    than the grid's resolution (a grid point lies within (|ab| + |ac|) / 40 of any point of the triangle)."""
    rng = np.random.default_rng(7)
    g = np.arange(41) / 40.0
    V, W = np.meshgrid(g, g, indexing="ij")
    keep = V + W <= 1.0 + 1e-12
    V, W = V[keep], W[keep]
    for _ in range(29):
        verts = (rng.normal(0.0, 10.0, (1, 3)) + rng.normal(0.0, rng.uniform(0.5, 20.0), (3, 3))).astype(np.float32)
        a, ab, ac, skip = ref.records(verts, TRI_T)
        assert not skip[0]
        pts = rng.normal(0.0, 10.0, (1, 3)) + rng.normal(0.0, 25.0, (300, 3))
        out = ref.closest_ref(verts, TRI_T, pts)
        grid = a[0] + V[:, None] * ab[0] + W[:, None] * ac[0]
        dmin = np.sqrt(((pts[:, None, :] - grid[None]) ** 2).sum(-1)).min(axis=1)
        res = (np.linalg.norm(ab[0]) + np.linalg.norm(ac[0])) / 40.0
        assert (out["distances"] <= dmin * (1 + 1e-12)).all()
        assert (out["distances"] >= dmin - res).all()
        # the closest point is the triangle's point the barycentrics name, and the distance is to it
        v, w = out["primitive_uvs"][:, 0], out["primitive_uvs"][:, 1]
        assert (v >= 0).all() and (w >= 0).all() and (v + w <= 1 + 1e-12).all()
        assert np.allclose(out["points"], a[0] + v[:, None] * ab[0] + w[:, None] * ac[0], rtol=0, atol=1e-12)
        assert np.allclose(np.linalg.norm(pts - out["points"], axis=1), out["distances"], rtol=1e-14, atol=0)


def test_degenerate_triangles_are_skipped():
    verts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0],          # collinear: m = 0
                      [5, 5, 5], [5, 5, 5], [6, 5, 5],          # a repeated vertex
                      [0, 0, 10], [1, 0, 10], [0, 1, 10]], np.float32)
    tris = np.arange(9, dtype=np.uint32).reshape(3, 3)
    assert ref.records(verts, tris)[3].tolist() == [True, True, False]
    out = ref.closest_ref(verts, tris, np.array([[0.5, 0.0, 0.1], [5.0, 5.0, 5.0]]))
    assert out["primitive_ids"].tolist() == [2, 2] and out["unskipped"] == 1
    assert abs(out["distances"][0] - 9.9) < 1e-12 and out["distances"][1] > 5.0
    none = ref.closest_ref(verts, tris[:2], np.array([[0.5, 0.0, 0.1], [np.nan, 0.0, 0.0]]))
    assert none["primitive_ids"].tolist() == [0xFFFFFFFF] * 2 and none["sides"].tolist() == [0, 0]
    assert none["distances"][0] == np.inf and np.isnan(none["distances"][1])
    assert np.isnan(none["points"]).all() and np.isnan(none["primitive_uvs"]).all()


def test_ties_go_to_the_lowest_index():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    tris = np.array([[1, 3, 2], [0, 1, 2]], np.uint32)                      # they share the edge (1, 2)
    out = ref.closest_ref(verts, tris, np.array([[0.5, 0.5, 1.0], [1.0, 0.0, -1.0]]))
    assert out["primitive_ids"].tolist() == [0, 0] and out["distances"].tolist() == [1.0, 1.0]


def test_argument_errors_name_the_function():
    from pedp_hip import _lib, surface_distance as sd

    class Holder:
        vertices = np.zeros((3, 3))
        triangles = np.array([[0, 1, 2]])

    pts = np.zeros((4, 3))
    for fn, name in ((sd.closest_points, "closest_points"), (sd.compute_distance, "compute_distance")):
        with pytest.raises(_lib.PedpError, match=name + ": points must be ... x 3"):
            fn(Holder(), np.zeros((4, 2)))
        with pytest.raises(_lib.PedpError, match=name + ": points must be ... x 3"):
            fn(Holder(), [[0.0, 0.0, 0.0]])
        with pytest.raises(_lib.PedpError, match=name + ": points must be float32 or float64"):
            fn(Holder(), np.zeros((4, 3), np.int32))
        with pytest.raises(_lib.PedpError, match=name + ": mesh must be"):
            fn(object(), pts)
    with pytest.raises(_lib.PedpError, match="align_to_mesh: defect_points must be N x 3"):
        sd.align_to_mesh(np.zeros((4, 2)), Holder())
    assert [len(x) for x in sd.align_to_mesh([], Holder())] == [0, 0]
    depth, K = np.ones((4, 5), np.float32), np.eye(3)
    with pytest.raises(_lib.PedpError, match="deviation_heatmap: depth must be H x W"):
        sd.deviation_heatmap(np.ones((2, 4, 5), np.float32), K, Holder(), 1.0, 5.0)
    with pytest.raises(_lib.PedpError, match="deviation_heatmap: saturation must be positive"):
        sd.deviation_heatmap(depth, K, Holder(), 0.0, 5.0)
    with pytest.raises(_lib.PedpError, match="deviation_heatmap: mask must be 4 x 5"):
        sd.deviation_heatmap(depth, K, Holder(), 1.0, 5.0, mask=np.ones((5, 4), bool))
    with pytest.raises(TypeError):
        sd.deviation_heatmap(depth, K, Holder())                 # saturation and gate have no defaults


def test_compat_exports():
    from pedp_hip import compat, surface_distance

    for name in ("closest_points", "compute_distance", "align_to_mesh", "deviation_heatmap"):
        assert name in compat.__all__ and getattr(compat, name) is getattr(surface_distance, name)
    assert compat.align_to_surface.__module__.endswith("ray_projection")


def test_deviation_heatmap_gating_on_given_distances(monkeypatch):
    from pedp_hip import depth_filters, surface_distance as sd

    depth = np.array([[0.5, 0.5, 0.5, 0.5], [0.0005, 0.0, np.nan, 0.5], [0.5, 0.5, 0.5, 0.5]], np.float32)
    dist = np.array([[0.0, 1.0, 2.0, 4.0], [1.0, 1.0, 1.0, np.nan], [5.0, 5.000001, 8.0, 0.5]])
    mask = np.ones((3, 4), bool)
    mask[2, 3] = False
    want = np.array([[0.0, 0.5, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    heat = sd.heat_from_distances(depth, dist, 2.0, 5.0, mask)
    assert heat.dtype == np.float64 and np.array_equal(heat, want)
    unmasked = sd.heat_from_distances(depth, dist, 2.0, 5.0)
    assert unmasked[2, 3] == 0.25 and np.array_equal(np.delete(unmasked.ravel(), 11), np.delete(want.ravel(), 11))
    # the whole function with the two device calls replaced: the points it asks about are float64(xyz) * unit
    seen = {}

    def fake_xyz(d, K):
        return np.stack([d, 2 * d, 3 * d], axis=-1).astype(np.float32)

    def fake_distance(mesh, pts, ctx=None):
        seen["pts"] = pts
        return dist

    monkeypatch.setattr(depth_filters, "depth2xyzmap", fake_xyz)
    monkeypatch.setattr(sd, "compute_distance", fake_distance)
    heat = sd.deviation_heatmap(depth, np.eye(3), "mesh", 2.0, 5.0, mask=mask)
    assert np.array_equal(heat, want)
    assert seen["pts"].dtype == np.float64 and seen["pts"].shape == (3, 4, 3)
    assert np.array_equal(seen["pts"][0, 0], np.float64(np.float32(0.5)) * np.array([1.0, 2.0, 3.0]) * 1000.0)
    import torch

    t = sd.deviation_heatmap(torch.from_numpy(depth), np.eye(3), "mesh", 2.0, 5.0, mask=torch.from_numpy(mask))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and np.array_equal(t.numpy(), want)
