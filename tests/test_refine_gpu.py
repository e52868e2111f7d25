"""refine_mesh (pedp_mesh_refine) on the device against tests/_refine_ref.py's numpy restatement: every
comparison of vertices, triangles, parent_face and rounds is bit equality.  Then what the feature is for: the refined
model under the solid, the ray caster and the defect map."""
import ctypes as C

import numpy as np
import pytest

import _refine_ref as R

pytestmark = pytest.mark.gpu

CASES = R.single_triangle_cases()
MISS = 0xFFFFFFFF


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def refine(ctx, v, t, max_edge, **kw):
    from pedp_hip.mesh_refine import refine_mesh

    return refine_mesh((v, t), max_edge, ctx=ctx, **kw)


def assert_is_ref(got, ref):
    v, t, pf, rounds = ref
    assert same_bits(got.vertices, v)
    assert same_bits(got.triangles, t)
    assert same_bits(got.parent_face, pf)
    assert got.rounds == rounds


def check(ctx, v, t, max_edge):
    got, ref = refine(ctx, v, t, max_edge), R.refine(v, t, max_edge)
    assert_is_ref(got, ref)
    assert got.n_parent_faces == len(t) and got.max_edge == max_edge
    return got


@pytest.fixture(scope="module")
def cube_fine(ctx):
    """The unit cube at max_edge 0.05: 12,288 faces after 5 rounds."""
    v, t = R.cube()
    return v, t, check(ctx, v, t, 0.05)


@pytest.fixture(scope="module")
def sphere_fine(ctx):
    """The 320-face icosphere at max_edge 0.1."""
    v, t = R.icosphere(2)
    return v, t, check(ctx, v, t, 0.1)


# ---------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_single_triangles(ctx, case):
    name, v, t, max_edge, want_v, want_t = case
    got = check(ctx, v, t, max_edge)
    assert same_bits(got.vertices, want_v) and same_bits(got.triangles, want_t)


@pytest.mark.parametrize("duplicated", [False, True], ids=["shared", "duplicated"])
def test_shared_edge_gets_one_midpoint_per_split(ctx, duplicated):
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]], np.float64)
    t = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)            # the edge (1, 2) in opposite index order
    if duplicated:
        v, t = R.split_vertices(v, t, faces=[1])               # face 1 has its own copies of vertices 1 and 2
    got = check(ctx, v, t, 0.4)
    assert got.rounds >= 3
    new = got.vertices[len(v):]
    assert len(np.unique(new, axis=0)) == len(new)             # no midpoint was made twice
    on_edge = np.flatnonzero(got.vertices[:, 0] + got.vertices[:, 1] == 2.0)
    on_edge = on_edge[on_edge >= len(v)]
    assert len(on_edge) >= 7
    side = [np.unique(got.triangles[got.parent_face == f]) for f in (0, 1)]
    assert np.isin(on_edge, side[0]).all() and np.isin(on_edge, side[1]).all()   # both sides refer to each of them
    assert R.edge_pairing(got.vertices, got.triangles)[1] == 0


def test_sliver(ctx):
    L = 1.0
    h = np.sqrt(L * L - (L / 200) ** 2)
    v = np.array([[-L / 200, 0, 0], [0, h, 0], [L / 200, 0, 0]], np.float64)     # sides L, L, L / 100
    got = check(ctx, v, np.array([[0, 1, 2]], np.uint32), L / 8)
    assert R.longest_edge(got.vertices, got.triangles) <= L / 8
    check(ctx, v, np.array([[0, 1, 2]], np.uint32), L / 150)


def test_degenerate_faces_are_copied_through(ctx):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],             # 0 1 2: a face that splits
                  [0.3, 0.3, 0], [0.3, 0.3, 0], [0.3, 0.3, 0],  # 3 4 5: one position, a face of zero area
                  [1, 0, 0], [1, 0.125, 0],                    # 6: a copy of vertex 1; 7 near it
                  [0, 0, 1], [2, 0, 1], [4, 0, 1]], np.float64)  # 8 9 10: collinear, zero area, long edges
    t = np.array([[0, 1, 2], [3, 4, 5], [1, 6, 7], [5, 3, 3]], np.uint32)
    got = check(ctx, v, t, 0.25)
    assert got.rounds >= 2
    for f in (1, 2, 3):
        kids = np.flatnonzero(got.parent_face == f)
        assert len(kids) == 1 and same_bits(got.triangles[kids[0]], t[f])
    # a zero-area face whose edges are long is split like any other, by the same rules
    check(ctx, v, np.vstack([t, [[8, 9, 10]]]).astype(np.uint32), 0.25)


def test_multi_round_cube(ctx):
    v, t = R.cube()
    got = check(ctx, v, t, 0.2)
    assert got.rounds >= 3 and R.longest_edge(got.vertices, got.triangles) <= 0.2
    assert same_bits(got.vertices[:8], v)
    assert (np.diff(got.parent_face) >= 0).all()


def test_large_output(ctx):
    v, t = R.icosphere(3)
    assert len(t) == 1280
    got = check(ctx, v, t, 0.02)                               # the last round mixes all four templates
    assert 70_000 <= len(got.triangles) <= 200_000
    assert R.longest_edge(got.vertices, got.triangles) <= 0.02
    assert R.edge_pairing(got.vertices, got.triangles) == (0, 0)


def test_no_op(ctx):
    v, t = R.cube()
    for max_edge in (np.sqrt(2.0), 1.5, 1e150):                # at the longest edge (the diagonal), and above it
        got = check(ctx, v, t, max_edge)
        assert got.rounds == 0 and same_bits(got.vertices, v) and same_bits(got.triangles, t)
        assert same_bits(got.parent_face, np.arange(12, dtype=np.int32))


def test_device_tensors_give_the_same_bits(ctx):
    import torch

    from pedp_hip.mesh_refine import refine_mesh

    v, t = R.icosphere(1)
    host = check(ctx, v, t, 0.13)
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t.astype(np.int64)).cuda()
    for tri in (dt, dt.to(torch.int32)):
        dev = refine_mesh((dv, tri), 0.13)
        assert dev.vertices.is_cuda and dev.triangles.is_cuda and dev.parent_face.is_cuda
        assert same_bits(dev.vertices.cpu().numpy(), host.vertices)
        assert same_bits(dev.triangles.cpu().numpy().view(np.uint32), host.triangles)
        assert same_bits(dev.parent_face.cpu().numpy(), host.parent_face)
        assert dev.rounds == host.rounds
    x = np.random.default_rng(2).normal(size=len(host.triangles))
    on_dev = dev.reduce_to_parent(torch.from_numpy(x).cuda(), "sum")
    assert on_dev.is_cuda and same_bits(on_dev.cpu().numpy(), host.reduce_to_parent(x, "sum"))


def test_history_independence(ctx):
    from pedp_hip import DefectMap, _lib

    v, t = R.icosphere(2)
    ref = R.refine(v, t, 0.06)
    first = refine(ctx, v, t, 0.06)
    DefectMap(R.cube(), ctx=ctx).close()                       # an unrelated call: it sorts in the context's pooled buffers
    refine(ctx, *R.cube(), 0.3)
    second = refine(ctx, v, t, 0.06)
    fresh_ctx = _lib.Context(0)
    try:
        third = refine(fresh_ctx, v, t, 0.06)
        for got in (first, second, third):
            assert_is_ref(got, ref)
        third.close()
    finally:
        fresh_ctx.close()


def test_bad_arguments(ctx):
    from pedp_hip import PedpError, _lib

    v, t = R.cube()
    bad_t = t.copy()
    bad_t[7, 2] = 8
    with pytest.raises(PedpError, match="status -1"):
        refine(ctx, v, bad_t, 0.5)
    bad_v = v.copy()
    bad_v[5, 1] = np.nan
    with pytest.raises(PedpError, match="status -1"):
        refine(ctx, bad_v, t, 0.5)
    for max_edge in (0.0, -1.0, np.inf):
        with pytest.raises(PedpError, match="status -1"):
            refine(ctx, v, t, max_edge)
    final = len(R.refine(v, t, 0.3)[1])
    assert len(refine(ctx, v, t, 0.3, max_faces=final).triangles) == final
    with pytest.raises(PedpError, match=f"status -1.*reaches {final} faces"):
        refine(ctx, v, t, 0.3, max_faces=final - 1)
    h, reached = C.c_void_p(), C.c_int64()
    rc = _lib.load().pedp_mesh_refine(ctx._h, _lib._ptr(v), 8, _lib._ptr(t), 12, _lib.HOST, 0.3, final - 1, C.byref(h), C.byref(reached))
    assert rc == -1 and not h and reached.value == final


# ---------------------------------------------------------------- downstream
def test_solid_stays_closed_and_oriented(ctx, cube_fine, sphere_fine):
    from pedp_hip.compat import Solid

    for v, t, fine in (cube_fine, sphere_fine):
        before, after = Solid((v, t), ctx).info, Solid(fine, ctx).info
        assert before["closed"] == 1 and after["closed"] == 1
        assert after["orientation"] == before["orientation"] == 1
        for k in ("boundary_edges", "nonmanifold_edges", "flipped_edges", "degenerate_faces"):
            assert after[k] == before[k] == 0
        assert abs(after["volume"] - before["volume"]) <= 1e-12 * before["volume"]


def test_parent_ids_under_a_cast(ctx, cube_fine, sphere_fine):
    from pedp_hip.compat import RaycastingScene

    for v, t, fine in (cube_fine, sphere_fine):
        p = fine.vertices[fine.triangles.astype(np.int64)]
        centroid = p.mean(axis=1)
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        n /= np.linalg.norm(n, axis=1)[:, None]                # outward: the ray starts outside the convex body
        rays = np.hstack([centroid + n, -n]).astype(np.float32)
        coarse, refined = RaycastingScene(ctx), RaycastingScene(ctx)
        coarse.add_triangles((v, t))
        refined.add_triangles(fine)
        prim_original = coarse.cast_rays(rays)["primitive_ids"]
        prim_refined = refined.cast_rays(rays)["primitive_ids"]
        assert (prim_original != MISS).all() and (prim_refined != MISS).all()
        assert same_bits(prim_refined, np.arange(len(rays), dtype=np.uint32))
        assert same_bits(fine.parent_face[prim_refined.astype(np.int64)], prim_original.astype(np.int32))
        assert same_bits(fine.parent_of(prim_refined), prim_original.astype(np.int32))
    assert same_bits(fine.parent_of(np.array([MISS, 0], np.uint32)), np.array([-1, fine.parent_face[0]], np.int32))


@pytest.mark.parametrize("how", ["max", "min", "sum"])
def test_reduce_to_parent(ctx, cube_fine, sphere_fine, how):
    for _, t, fine in (cube_fine, sphere_fine):
        x = np.random.default_rng(11).normal(size=len(fine.triangles))
        starts = np.flatnonzero(np.r_[True, fine.parent_face[1:] != fine.parent_face[:-1]])
        assert len(starts) == len(t)
        if how == "sum":                                       # one after the other, in ascending child order
            want = np.empty(len(t))
            for f, (a, b) in enumerate(zip(starts, np.r_[starts[1:], len(x)])):
                acc = x[a]
                for y in x[a + 1:b]:
                    acc = acc + y
                want[f] = acc
        else:
            want = (np.maximum if how == "max" else np.minimum).reduceat(x, starts)
        assert same_bits(fine.reduce_to_parent(x, how), want)


def test_localisation(ctx, cube_fine):
    """A small defect on one side of the cube: half a side on the CAD model, the disc's own size on the refined one."""
    from pedp_hip import DefectMap
    from pedp_hip.compat import RaycastingScene

    v, t, fine = cube_fine
    h, r, f = 0.05, 0.2, 600.0
    assert fine.max_edge == h
    # one camera at (0.5, 0.5, 3) looking down -z, square-on to the side z = 1 (CAD faces 10 and 11)
    u, w = np.meshgrid(np.arange(-200, 201), np.arange(-200, 201))
    d = np.stack([u.ravel() / f, w.ravel() / f, -np.ones(u.size)], axis=1)
    hit_xy = 0.5 + 2.0 * d[:, :2]
    d = d[np.hypot(hit_xy[:, 0] - 0.5, hit_xy[:, 1] - 0.5) <= r]
    rays = np.hstack([np.tile([0.5, 0.5, 3.0], (len(d), 1)), d]).astype(np.float32)
    area = {}
    for name, mesh in (("cad", (v, t)), ("refined", fine)):
        scene = RaycastingScene(ctx)
        scene.add_triangles(mesh)
        ids = scene.cast_rays(rays)["primitive_ids"]
        assert (ids != MISS).all()
        dmap = DefectMap(mesh, ctx=ctx)
        dmap.add(ids, np.ones(len(ids)))
        reg = dmap.regions(threshold=0.5)
        area[name] = reg["area"]
        if name == "refined":
            peak = dmap.faces()["peak"]
        dmap.close()
    assert len(area["cad"]) == 1 and area["cad"][0] >= 0.5
    # every marked face meets the disc and no edge exceeds h; the faces wholly inside the disc hold pixels (spacing 1 / 300)
    p = fine.vertices[fine.triangles.astype(np.int64)]
    inside = (p[:, :, 2] == 1.0).all(axis=1) & (np.hypot(p[:, :, 0] - 0.5, p[:, :, 1] - 0.5) <= r).all(axis=1)
    lower = R.face_areas(fine.vertices, fine.triangles)[inside].sum()
    print(f"refined region areas {area['refined']}, bounds {lower} ... {np.pi * (r + h) ** 2}")
    assert len(area["refined"]) == 1                          # the marked faces hang together across edges
    assert 0.05 < lower <= area["refined"][0] <= np.pi * (r + h) ** 2 < 0.2
    per_cad = fine.reduce_to_parent(peak, "max")
    assert same_bits(np.flatnonzero(per_cad > 0.5), np.array([10, 11]))
