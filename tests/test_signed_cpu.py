"""CPU tests (no GPU) of the signed-distance contract: the numpy restatement's sign is the inside /
outside that the generalised winding number gives, on every fixture mesh and with no point left out; the face-normal sign
(`sides`) is not; the package's functions exist and refuse to compute without a GPU."""
import numpy as np
import pytest

import _signed_ref as sref


@pytest.mark.parametrize("name", sorted(sref.MESHES))
def test_the_fixture_is_a_closed_outward_mesh(name):
    v32, tris, _ = sref.fixture(name)
    topo = sref.topology(v32, tris)
    assert topo["closed"] == 1 and topo["orientation"] == 1 and topo["degenerate_faces"] == 0
    assert topo["edges"] * 2 == 3 * len(tris)
    if name == "stl_cube":
        assert topo["V"] == 36 and topo["welded_vertices"] == 8


@pytest.mark.parametrize("name", sorted(sref.MESHES))
def test_the_restatement_agrees_with_the_winding_number_everywhere(name):
    _, _, pts, ref, wn = sref.reference(name)
    off = np.minimum(np.abs(wn), np.abs(wn - 1.0))
    print(f"{name}: winding numbers within {off.max():.3g} of 0 or 1, smallest distance {ref['distances'].min():.3g}, "
          f"features {np.bincount(ref['features'], minlength=3)[:3]}")
    assert off.max() <= 1e-9
    inside = wn > 0.5
    assert len(pts) == sref.N_QUERIES and 20 < inside.sum() < sref.N_QUERIES - 20
    assert np.array_equal(ref["signed_distances"] < 0, inside)
    assert np.array_equal(ref["occupancy"].astype(bool), inside)
    assert np.array_equal(np.abs(ref["signed_distances"]), ref["distances"])
    assert (np.abs(np.linalg.norm(ref["normals"], axis=1) - 1.0) < 1e-12).all()


@pytest.mark.parametrize("name", ["wedge", "pyramid"])
def test_the_face_normal_sign_is_wrong_somewhere_on_a_sharp_part(name):
    """`sides` < 0 as "inside" disagrees with the yardstick: these fixtures tell the shortcut from the real thing."""
    _, _, _, ref, wn = sref.reference(name)
    wrong = (ref["sides"] < 0) != (wn > 0.5)
    print(f"{name}: the face-normal sign disagrees with the winding number on {int(wrong.sum())} of {len(wn)} points")
    assert wrong.sum() >= 10
    assert (ref["features"][wrong] != sref.FACE).all()            # never where the closest point is inside a face


def test_every_feature_class_occurs():
    for name in ("cube", "wedge", "torus_12x8"):
        feats = sref.reference(name)[3]["features"]
        assert set(np.unique(feats)) == {sref.FACE, sref.EDGE, sref.VERTEX}


def test_topology_counts_of_broken_meshes():
    v, t = sref.cube()
    topo = sref.topology(v, t[:-1])
    assert topo["boundary_edges"] == 3 and topo["closed"] == 0
    flipped = t.copy()
    flipped[5] = flipped[5][::-1]
    assert sref.topology(v, flipped)["flipped_edges"] == 3
    fin = np.concatenate([t, [[t[0, 0], t[0, 1], 8]]]).astype(np.uint32)
    topo = sref.topology(np.concatenate([v, [[0.5, -1.0, 0.5]]]), fin)
    assert topo["nonmanifold_edges"] == 1 and topo["boundary_edges"] == 2
    topo = sref.topology(v, t[:, ::-1])
    assert topo["closed"] == 1 and topo["orientation"] == -1 and abs(topo["volume"] + 1.0) < 1e-12


def test_the_functions_exist_and_refuse_without_a_gpu():
    import torch

    from pedp_hip import _lib, compat, surface_distance as sd

    for name in ("Solid", "compute_signed_distance", "compute_occupancy", "signed_closest_points", "signed_deviation",
                 "split_deviation"):
        assert callable(getattr(sd, name)) and getattr(compat, name) is getattr(sd, name) and name in compat.__all__
    assert {"pedp_solid_create", "pedp_solid_destroy", "pedp_solid_get_info", "pedp_signed_distance"} <= set(_lib.PROTOTYPES)
    v, t = sref.cube()

    class Holder:
        vertices, triangles = v, t

    pts = np.zeros((4, 3))
    # what needs no device: the arguments' checks, and the split of given signed distances
    with pytest.raises(_lib.PedpError, match="compute_signed_distance: points must be ... x 3"):
        sd.compute_signed_distance(Holder(), np.zeros((4, 2)))
    with pytest.raises(_lib.PedpError, match="compute_occupancy: points must be float32 or float64"):
        sd.compute_occupancy(Holder(), np.zeros((4, 3), np.int32))
    with pytest.raises(_lib.PedpError, match="Solid: mesh must hold"):
        sd.Solid("mesh")
    with pytest.raises(_lib.PedpError, match="signed_deviation: depth must be H x W"):
        sd.signed_deviation(np.ones((2, 4, 5), np.float32), np.eye(3), Holder(), None)
    with pytest.raises(_lib.PedpError, match="split_deviation: saturation must be positive"):
        sd.split_deviation(np.zeros((2, 2)), 0.0, 1.0)
    s = np.array([[0.5, -0.25, np.nan], [3.0, -6.0, 0.0]])
    excess, missing = sd.split_deviation(s, 2.0, 5.0)
    assert np.array_equal(excess, [[0.25, 0.0, 0.0], [1.0, 0.0, 0.0]]) and np.array_equal(missing, [[0.0, 0.125, 0.0], [0.0, 0.0, 0.0]])
    te, tm = sd.split_deviation(torch.from_numpy(s), 2.0, 5.0)
    assert np.array_equal(te.numpy(), excess) and np.array_equal(tm.numpy(), missing)
    if torch.cuda.is_available():
        return
    for call in (lambda: sd.Solid(Holder()), lambda: sd.compute_signed_distance(Holder(), pts), lambda: sd.compute_occupancy(Holder(), pts),
                 lambda: sd.signed_closest_points(Holder(), pts)):
        with pytest.raises(_lib.PedpError):
            call()
