"""All-hits queries without a GPU: the reference helper on known answers, its first entries against the oracle's cast,
and RaycastingScene's argument checks, which come before the device is touched."""
import numpy as np
import pytest

from _all_hits_ref import all_hits, patched, same_bits

# a unit square in z = 1, split along the diagonal (0,0)-(1,1); every coordinate exact in float32
SQUARE_V = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float32)
SQUARE_T = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def _down(x, y, z=0.0, dz=1.0):
    return [x, y, z, 0.0, 0.0, dz]


def test_helper_on_known_answers(oracle):
    rays = np.array([_down(0.75, 0.25),            # inside triangle 0
                     _down(0.5, 0.5),              # on the shared diagonal: both triangles (edges are inclusive)
                     _down(2.0, 2.0),              # beside the square
                     _down(0.25, 0.75, 1.0),       # origin on the surface: t = 0 counts
                     _down(0.25, 0.75, 2.0),       # behind the origin
                     _down(0.0, 0.0),              # the corner both triangles share
                     _down(0.25, 0.75, 0.0, 2.0),  # unnormalised direction: t in units of it
                     _down(0.25, 0.75, 0.0, 0.0),  # no direction
                     [0.25, 0.75, 0.0, np.nan, 0.0, 1.0]], np.float32)
    h = all_hits(oracle, SQUARE_V, SQUARE_T, rays)
    assert h.counts.tolist() == [1, 2, 0, 1, 0, 2, 1, 0, 0]
    assert h.ray_splits.tolist() == [0, 1, 3, 3, 4, 4, 6, 7, 7, 7]
    assert h.ray_ids.tolist() == [0, 1, 1, 3, 5, 5, 6]
    assert h.primitive_ids.tolist() == [0, 0, 1, 1, 0, 1, 1]        # equal t: by triangle index
    assert h.t_hit.tolist() == [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.5]
    assert h.occluded().tolist() == [True, True, False, True, False, True, True, False, False]
    assert h.occluded(1.0, 1.0).tolist() == [True, True, False, False, False, True, False, False, False]    # both ends inclusive
    assert not h.occluded(np.nextafter(np.float32(1), np.float32(2)), 5.0).any()
    assert h.occluded(0.0, np.nextafter(np.float32(1), np.float32(0))).tolist() == [False] * 3 + [True] + [False] * 2 + [True] + [False] * 2
    assert not h.occluded(np.nan, 2.0).any() and not h.occluded(0.0, np.nan).any()
    # rows(): a sub-list, renumbered; patched(): the same list from a base with other rows
    sub = h.rows([1, 5, 6])
    assert sub.counts.tolist() == [2, 2, 1] and sub.ray_ids.tolist() == [0, 0, 1, 1, 2]
    moved = rays.copy()
    moved[2] = rays[1]
    moved[0] = rays[4]
    p, q = patched(oracle, SQUARE_V, SQUARE_T, h, moved, [0, 2]), all_hits(oracle, SQUARE_V, SQUARE_T, moved)
    for name in ("ray_ids", "t_hit", "primitive_ids", "primitive_uvs", "ray_splits", "counts"):
        assert same_bits(getattr(p, name), getattr(q, name)), name


def test_first_entry_is_the_oracles_cast(oracle):
    from pedp_hip import synth

    f = synth.Frame("tiny")
    rays = f.rays6[::3].copy()
    rays[5, 3:] *= 3.0
    rays[6, :3] = f.verts_posed.mean(axis=0)         # an origin inside the part's bounding box
    h = all_hits(oracle, f.verts_posed, f.tris, rays)
    cast = oracle.raycast(f.verts_posed, f.tris, rays)
    hit = h.counts > 0
    assert hit.any() and (h.counts > 1).any() and not hit.all()
    assert (hit == np.isfinite(cast["t_hit"])).all()
    first = h.ray_splits[:-1][hit]
    assert same_bits(h.t_hit[first], cast["t_hit"][hit])
    assert same_bits(h.primitive_ids[first], cast["primitive_ids"][hit])
    assert same_bits(h.primitive_uvs[first], cast["primitive_uvs"][hit])
    assert (np.diff(h.t_hit.view(np.uint32).astype(np.int64))[np.diff(h.ray_ids) == 0] >= 0).all()   # ascending within a ray


def test_scene_checks_arguments_before_the_device():
    """Nothing here may need the library's context: a machine without a GPU raises on creating one."""
    from pedp_hip import PedpError, compat, raycasting_scene

    assert compat.RaycastingScene is raycasting_scene.RaycastingScene and "RaycastingScene" in compat.__all__
    scene = raycasting_scene.RaycastingScene()
    with pytest.raises(PedpError, match="empty"):
        scene.count_intersections(np.zeros((4, 6), np.float32))
    with pytest.raises(PedpError, match="V x 3"):
        scene.add_triangles(np.zeros((4, 2)), SQUARE_T)
    with pytest.raises(PedpError, match="indices"):
        scene.add_triangles(SQUARE_V, SQUARE_T + 3)
    with pytest.raises(PedpError, match="no triangles"):
        scene.add_triangles(SQUARE_V, np.zeros((0, 3), np.uint32))
    bad = SQUARE_V.copy()
    bad[2, 1] = np.nan
    with pytest.raises(PedpError, match="finite"):
        scene.add_triangles(bad, SQUARE_T)
    assert scene.add_triangles(SQUARE_V, SQUARE_T) == 0
    with pytest.raises(NotImplementedError):
        scene.add_triangles(SQUARE_V, SQUARE_T)
    for query in (scene.cast_rays, scene.count_intersections, scene.list_intersections, scene.test_occlusions):
        with pytest.raises(PedpError, match="x 6"):
            query(np.zeros((4, 5), np.float32))
        with pytest.raises(PedpError, match="x 6"):
            query(np.float32(np.nan))                      # a scalar NaN where rays belong: no shape to speak of
        with pytest.raises(PedpError, match="x 6"):
            query([[0.0] * 6])                             # a list is neither an array nor a tensor
        with pytest.raises(PedpError, match="floating"):
            query(np.zeros((4, 6), np.int32))
    rays = np.zeros((2, 3, 6), np.float32)
    for lo, hi in (("near", 1.0), (0.0, None), ([0.0, 1.0], 2.0), (0.0, np.zeros(3))):
        with pytest.raises(PedpError, match="real number"):
            scene.test_occlusions(rays, lo, hi)
    for query in (scene.compute_closest_points, scene.compute_distance, scene.compute_signed_distance, scene.compute_occupancy):
        with pytest.raises(PedpError, match="x 3"):
            query(np.zeros((4, 6)))
