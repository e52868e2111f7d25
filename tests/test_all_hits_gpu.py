"""count_intersections / test_occlusions / list_intersections on the device against the oracle's list
(tests/_all_hits_ref.py).  Every comparison is bit equality."""
import ctypes as C

import numpy as np
import pytest

from _all_hits_ref import all_hits, assert_list, patched, same_bits

pytestmark = pytest.mark.gpu

GRID, EXHAUSTIVE = 4, 1      # pedp_intersections_last_path


@pytest.fixture(scope="module")
def parity(oracle):
    """The parity frame (4,000 triangles, 23,040 rays of one origin) and its reference, computed once and left alone."""
    from pedp_hip import synth

    f = synth.Frame("parity")
    ref = all_hits(oracle, f.verts_posed, f.tris, f.rays6)
    assert ref.counts.max() >= 4 and (ref.counts == 2).any() and (ref.counts == 0).any()
    return {"f": f, "rays": f.rays6, "ref": ref}


@pytest.fixture()
def own():
    """A context of the test's own: the path choice and the status words are per context."""
    from pedp_hip import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def _check_three(mesh, rays, ref, what, bounds=((0.0, np.inf),)):
    """the three queries of `rays` (an array or a RaySet) against the reference list"""
    assert same_bits(mesh.count_intersections(rays), ref.counts), f"{what}: counts"
    for lo, hi in bounds:
        assert same_bits(mesh.test_occlusions(rays, lo, hi), ref.occluded(lo, hi)), f"{what}: occlusion in [{lo}, {hi}]"
    assert_list(mesh.list_intersections(rays), ref, what)


def _configured(ctx, variant):
    from pedp_hip import _lib

    class _Scope:
        def __enter__(self):
            _lib.raycast_configure(ctx, 0, variant)

        def __exit__(self, *exc):
            _lib.raycast_configure(ctx, 0, 0)

    return _Scope()


# ---------------------------------------------------------------- 1. the parity frame, every path
def test_parity_frame_per_call_rayset_and_exhaustive(own, parity):
    from pedp_hip import _lib

    f, rays, ref = parity["f"], parity["rays"], parity["ref"]
    mesh = _lib.Mesh(own, f.verts_posed, f.tris)
    mid = float(np.median(ref.t_hit))
    bounds = ((0.0, np.inf), (mid, np.inf), (0.0, mid))
    for query in (lambda r: mesh.count_intersections(r), lambda r: mesh.test_occlusions(r), lambda r: mesh.list_intersections(r)):
        query(rays)
        assert _lib.intersections_last_path(own) == (GRID, 0)
    _check_three(mesh, rays, ref, "per call, grid", bounds)
    assert _lib.intersections_last_path(own) == (GRID, 0)
    rs = _lib.RaySet(own, rays)
    _check_three(mesh, rs, ref, "ray set, grid", bounds)
    assert _lib.intersections_last_path(own) == (GRID, 0)
    for variant in (5, 2):
        with _configured(own, variant):
            _check_three(mesh, rays, ref, f"per call, variant {variant}", bounds)
            assert _lib.intersections_last_path(own) == (EXHAUSTIVE, 0)
            _check_three(mesh, rs, ref, f"ray set, variant {variant}", bounds)
            assert _lib.intersections_last_path(own) == (EXHAUSTIVE, 0)
    rs.close()


# ---------------------------------------------------------------- 2. ragged counts, general origins
@pytest.fixture(scope="module")
def ragged(oracle):
    from pedp_hip import synth

    f = synth.Frame("tiny")
    rng = np.random.default_rng(11)
    n = 1000
    cast = oracle.raycast(f.verts_posed, f.tris, f.rays6)
    hit = np.flatnonzero(np.isfinite(cast["t_hit"]))
    centre = f.verts_posed.mean(axis=0)
    rays = np.empty((n, 6), np.float32)
    pick = rng.choice(hit, n)
    # a third from the camera with directions of any length, a third from just inside the surface (inside the tube: an
    # odd number of walls on the way out), a third from outside towards the part
    rays[:] = f.rays6[pick]
    rays[:, 3:] *= rng.uniform(0.01, 50.0, (n, 1)).astype(np.float32)
    inside = np.arange(n) % 3 == 1
    rays[inside, :3] = f.rays6[pick[inside], 3:] * (cast["t_hit"][pick[inside]] * 1.02 + 0.05)[:, None]
    rays[inside, 3:] = rng.normal(0, 1, (int(inside.sum()), 3))
    outside = np.arange(n) % 3 == 2
    rays[outside, :3] = centre + rng.normal(0, 1, (int(outside.sum()), 3)) * 400.0
    rays[outside, 3:] = (centre + rng.normal(0, 30.0, (int(outside.sum()), 3)) - rays[outside, :3]) * rng.uniform(0.1, 3.0, (int(outside.sum()), 1))
    rays[3, 3:] = 0.0
    rays[7, 4] = np.nan
    rays[11, 3] = np.inf
    rays[40, 3:] = -0.0
    rays[41, 3:] = np.nan
    ref = all_hits(oracle, f.verts_posed, f.tris, rays)
    assert (ref.counts[inside] % 2 == 1).sum() > 50 and (ref.counts[outside] > 0).any()
    assert ref.counts[[3, 7, 40, 41]].tolist() == [0, 0, 0, 0]
    return {"f": f, "rays": rays, "ref": ref}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_ragged_counts_general_origins(ctx, ragged, n):
    """N = 0 gives empty results (only a ray SET cannot be empty: test_errors)."""
    from pedp_hip import _lib

    f, rays, ref = ragged["f"], ragged["rays"][:n], ragged["ref"].rows(np.arange(n))
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    mid = float(np.median(ragged["ref"].t_hit))
    _check_three(mesh, rays, ref, f"N = {n}", ((0.0, np.inf), (mid, 2 * mid)))
    if n:
        assert _lib.intersections_last_path(ctx) == (EXHAUSTIVE, 0)
        with _configured(ctx, 4):     # the grid asked to hold rays of many origins: handed over in the same call
            _check_three(mesh, rays, ref, f"N = {n}, grid configured", ((0.0, np.inf), (mid, 2 * mid)))
            assert _lib.intersections_last_path(ctx)[0] == GRID
    mesh.close()


# ---------------------------------------------------------------- 3. what the grid hands over
def test_grid_hands_over_and_leaves_nothing_behind(own, oracle, parity):
    """The cases of test_ray_gpu.py::test_grid_sweep_hands_over_what_it_cannot_answer.  The crowded one makes the grid give
    up AFTER its kernels have counted: what they added must not survive the completion."""
    from pedp_hip import _lib

    f = parity["f"]
    n = 20000
    base = f.rays6[:: max(1, f.n_rays // n)][:n].copy()
    assert same_bits(base, parity["rays"][:n])
    base_ref = parity["ref"].rows(np.arange(n))
    mesh = _lib.Mesh(own, f.verts_posed, f.tris)
    mid = float(np.median(base_ref.t_hit))

    def check(rays, changed, status, what):
        ref = patched(oracle, f.verts_posed, f.tris, base_ref, rays, changed) if len(changed) else base_ref
        with _configured(own, 4):
            for name, query in (("count", lambda: same_bits(mesh.count_intersections(rays), ref.counts)),
                                ("occlusion", lambda: same_bits(mesh.test_occlusions(rays, mid, np.inf), ref.occluded(mid, np.inf))),
                                ("list", lambda: assert_list(mesh.list_intersections(rays), ref, what) is None)):
                assert query(), f"{what}: {name}"
                assert _lib.intersections_last_path(own) == (GRID, status), f"{what}: {name}"
        return ref

    check(base, [], 0, "base")
    mixed = base.copy(); mixed[77, 1] += 0.5
    check(mixed, [77], 1, "moved origin")
    back = base.copy(); back[5, 3:] = -back[5, 3:]
    check(back, [5], 2, "reversed direction")
    inf = base.copy(); inf[9, 3] = np.inf
    check(inf, [9], 2, "infinite direction")
    hit = int(np.flatnonzero(base_ref.counts > 0)[0])
    crowd = base.copy(); crowd[100:400] = crowd[hit]
    crowd_ref = check(crowd, np.arange(100, 400), 4, "crowded cell that triangles visit")
    assert (crowd_ref.counts[100:400] == base_ref.counts[hit]).all()
    assert base_ref.counts[0] == 0
    lonely = base.copy(); lonely[100:400] = lonely[0]
    check(lonely, np.arange(100, 400), 0, "crowded cell nothing visits")
    odd = base.copy(); odd[:40, 3:] = 0.0; odd[40:60, 3:] = np.nan
    check(odd, np.arange(60), 0, "rays without direction")
    # a ray set builds its grid without a triangle in sight: the crowd shows in the walk, the completion is the same
    rs = _lib.RaySet(own, crowd)
    _check_three(mesh, rs, crowd_ref, "crowded ray set", ((mid, np.inf),))
    rs.close()


# ---------------------------------------------------------------- 4. known answers on exact coordinates
CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
CUBE_T = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]], np.uint32)


def _known_cases():
    tri_v = np.array([[0, 0, 2], [4, 0, 2], [0, 4, 2]], np.float32)
    tri_t = np.array([[0, 1, 2]], np.uint32)
    tri_rays = np.array([[1, 1, 0, 0, 0, 1], [2, 2, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1], [3, 3, 0, 0, 0, 1], [1, 1, 2, 0, 0, 1],
                         [1, 1, 3, 0, 0, 1], [1, 1, 0, 0, 0, 4], [0, 2, 4, 0, 0, -0.5]], np.float32)
    cube_rays = np.array([[0.25, 0.625, -1, 0, 0, 1],      # through two faces, off their diagonals
                          [0.5, 0.5, -1, 0, 0, 1],         # through the centre of two faces: on whichever diagonal splits them
                          [0.25, 0.25, -1, 0, 0, 1], [0.25, 0.75, -1, 0, 0, 1],   # on one or the other diagonal
                          [-1, -1, -1, 1, 1, 1],           # through two opposite vertices
                          [-1, 0, 0, 1, 0, 0],             # along an edge
                          [0.25, 0.625, 0, 0, 0, 1],       # an origin on the surface: t = 0 counts
                          [0.25, 0.625, 0.5, 0, 0, 1],     # from inside
                          [0.25, 0.625, 2, 0, 0, 1]], np.float32)
    return [("triangle", tri_v, tri_t, tri_rays), ("cube", CUBE_V, CUBE_T, cube_rays)]


@pytest.mark.parametrize("case", _known_cases(), ids=lambda c: c[0])
def test_known_answers_and_inclusive_bounds(ctx, oracle, case):
    from pedp_hip import _lib

    name, v, t, rays = case
    ref = all_hits(oracle, v, t, rays)
    if name == "triangle":
        assert ref.counts.tolist() == [1, 1, 1, 0, 1, 0, 1, 1] and ref.t_hit.tolist() == [2.0, 2.0, 2.0, 0.0, 0.5, 4.0]
    else:
        assert ref.counts[0] == 2 and ref.counts[1] == 4 and ref.counts[4] >= 6 and ref.counts[7] == 1 and ref.counts[8] == 0
        assert ref.t_hit[ref.ray_splits[6]] == 0.0 and ref.counts[6] == 2
    mesh = _lib.Mesh(ctx, v, t)
    ts = np.unique(ref.t_hit)
    up, down = np.nextafter(ts, np.float32(np.inf)), np.nextafter(ts, np.float32(-np.inf))
    bounds = [(0.0, np.inf), (np.nan, 1.0), (0.0, np.nan)]
    for k in range(len(ts)):
        bounds += [(ts[k], ts[k]), (up[k], np.inf), (0.0, down[k]) if ts[k] > 0 else (-1.0, -0.0), (ts[k], np.inf), (-np.inf, ts[k])]
    for variant in (0, 4):
        with _configured(ctx, variant):
            _check_three(mesh, rays, ref, f"{name}, variant {variant}", bounds)
    # the bounds' ends spelled out on a ray with one hit: its t is in range, its neighbours on either side are not
    one = int(np.flatnonzero(ref.counts == 1)[0])
    t1 = ref.t_hit[ref.ray_splits[one]]
    assert mesh.test_occlusions(rays, t1, t1)[one]
    assert not mesh.test_occlusions(rays, np.nextafter(t1, np.float32(np.inf)), np.inf)[one]
    assert not mesh.test_occlusions(rays, -1.0, np.nextafter(t1, np.float32(-np.inf)))[one]
    mesh.close()


# ---------------------------------------------------------------- 5. long segments
def test_long_segments_are_ordered(ctx, oracle):
    """300 stacked quads (600 triangles) and a fan of 64 triangles around one vertex: segments of hundreds of entries, many
    of them with equal t (the diagonals, the fan's vertex), ordered by t and then by triangle."""
    from pedp_hip import _lib

    verts, tris = [], []
    for k in range(300):
        z = 1.0 + k
        b = len(verts)
        verts += [[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]]
        tris += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    apex = len(verts)
    verts.append([10, 10, 1])
    ring = [[10 + x, 10 - 8, 1] for x in range(-8, 8)] + [[10 + 8, 10 + y, 1] for y in range(-8, 8)] + \
           [[10 - x, 10 + 8, 1] for x in range(-8, 8)] + [[10 - 8, 10 - y, 1] for y in range(-8, 8)]
    first = len(verts)
    verts += ring
    tris += [[apex, first + k, first + (k + 1) % 64] for k in range(64)]
    v, t = np.array(verts, np.float32), np.array(tris, np.uint32)
    assert len(t) == 664
    step = 2.0 ** -12
    par = np.zeros((64, 6), np.float32)                       # parallel rays: many origins
    par[:, 0] = 0.125 + (np.arange(64) % 8) * 0.09375
    par[:, 1] = 0.125 + (np.arange(64) // 8) * 0.09375         # (k % 8 == k // 8: on the quads' diagonal)
    par[:, 5] = 1.0
    par[60, :3] = [10, 10, 0]                                 # the fan's shared vertex
    par[61, :3] = [10, 10, 1]                                 # ... from the vertex itself
    par[62, :3] = [12, 11, -3]
    fanned = np.zeros((64, 6), np.float32)                    # one origin above the stack's centre
    fanned[:, :3] = [0.5, 0.5, 0.0]
    fanned[:, 3] = ((np.arange(64) % 8) - 4) * step
    fanned[:, 4] = ((np.arange(64) // 8) - 4) * step
    fanned[:, 5] = 1.0
    fanned[63, 3:] = [9.5, 9.5, 1.0]                          # from there through the fan's vertex
    mesh = _lib.Mesh(ctx, v, t)
    for what, rays in (("parallel", par), ("one origin", fanned)):
        ref = all_hits(oracle, v, t, rays)
        assert ref.counts.max() == 600 and (ref.counts == 300).any() and (ref.counts == 64).any(), what
        for variant in (0, 4):
            with _configured(ctx, variant):
                _check_three(mesh, rays, ref, f"{what}, variant {variant}", ((150.0, 150.5), (301.0, np.inf)))
    mesh.close()


# ---------------------------------------------------------------- 6. consistency among the queries and with the cast
def test_queries_agree_with_each_other_and_with_cast_rays(ctx, parity):
    from pedp_hip import _lib

    f, rays = parity["f"], parity["rays"]
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    lst, counts, cast = mesh.list_intersections(rays), mesh.count_intersections(rays), mesh.cast_rays(rays)
    splits = lst["ray_splits"]
    assert same_bits(counts, np.diff(splits).astype(np.int32))
    hit = counts > 0
    assert same_bits(hit, np.isfinite(cast["t_hit"])) and same_bits(hit, mesh.test_occlusions(rays))
    first = splits[:-1][hit]
    assert same_bits(lst["t_hit"][first], cast["t_hit"][hit])
    assert same_bits(lst["primitive_ids"][first], cast["primitive_ids"][hit])
    assert same_bits(lst["primitive_uvs"][first], cast["primitive_uvs"][hit])
    assert same_bits(lst["ray_ids"], np.repeat(np.arange(len(rays)), counts))
    ts = np.unique(lst["t_hit"])
    q = ts[[len(ts) // 5, len(ts) // 2, (4 * len(ts)) // 5]]
    between = (q[:-1].astype(np.float64) + q[1:]) / 2
    for lo, hi in ((q[0], q[1]), (q[1], q[1]), (q[1], q[2]), (between[0], between[1]), (between[0], q[2]), (q[2], q[0])):
        lo32, hi32 = np.float32(lo), np.float32(hi)
        inside = (lo32 <= lst["t_hit"]) & (lst["t_hit"] <= hi32)
        want = np.bincount(lst["ray_ids"][inside], minlength=len(rays)) > 0
        assert same_bits(mesh.test_occlusions(rays, lo, hi), want), (lo, hi)
    mesh.close()


# ---------------------------------------------------------------- 7. capacity
def test_capacity_too_small_reports_total_and_python_retries(ctx, ragged):
    from pedp_hip import _lib

    f, rays, ref = ragged["f"], ragged["rays"], ragged["ref"]
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    m, n = len(ref.t_hit), len(rays)
    assert m > 100
    lib = _lib.load()
    for cap in (0, 1, m - 1, m):
        splits = np.full(n + 1, -7, np.int64)
        ids, t = np.full(m + 8, -7, np.int64), np.full(m + 8, -7.0, np.float32)
        prim, uv = np.full(m + 8, 7, np.uint32), np.full((m + 8, 2), -7.0, np.float32)
        total = C.c_int64(-1)
        rc = lib.pedp_list_intersections(ctx._h, mesh._h, _lib._ptr(rays), n, _lib.HOST, cap, _lib._ptr(splits), _lib._ptr(ids),
                                         _lib._ptr(t), _lib._ptr(prim), _lib._ptr(uv), C.byref(total))
        assert total.value == m and same_bits(splits, ref.ray_splits), cap
        if cap < m:
            assert rc != 0
            assert (ids == -7).all() and (t == -7.0).all() and (prim == 7).all() and (uv == -7.0).all(), cap
        else:
            assert rc == 0
            assert same_bits(t[:m], ref.t_hit) and (t[m:] == -7.0).all() and (ids[m:] == -7).all() and (prim[m:] == 7).all()
    mesh._list_cap = 1
    assert_list(mesh.list_intersections(rays), ref, "retried")
    assert mesh._list_cap > m
    assert_list(mesh.list_intersections(rays), ref, "with room kept")
    mesh.close()


# ---------------------------------------------------------------- 8. a posable mesh answers for its pose
def test_posable_mesh_answers_for_the_new_pose(ctx, oracle):
    from pedp_hip import _lib, synth

    f = synth.Frame("tiny")
    mesh = _lib.Mesh(ctx, f.verts, f.tris, posable=True)
    rays = f.rays6[::2]
    seen = []
    for T in (f.T_gt, f.T_start, f.T_gt):
        mesh.set_pose(T)
        ref = all_hits(oracle, oracle.pose_vertices(T, f.verts), f.tris, rays)
        assert ref.counts.max() >= 2
        _check_three(mesh, rays, ref, "posed")
        seen.append(ref.counts)
    assert not same_bits(seen[0], seen[1])
    mesh.close()


# ---------------------------------------------------------------- 9. queries and casts on one context, one ray set
def test_interleaved_with_casts_nothing_changes(own, parity):
    from pedp_hip import _lib

    f, rays, ref = parity["f"], parity["rays"], parity["ref"]
    mesh = _lib.Mesh(own, f.verts_posed, f.tris)
    rs = _lib.RaySet(own, rays)

    def same_cast(a, b):
        return all(same_bits(a[k], b[k]) for k in ("t_hit", "primitive_ids", "primitive_uvs"))

    cast0, cast_rs0 = mesh.cast_rays(rays), mesh.cast_rayset(rs)
    assert same_cast(cast0, cast_rs0) and _lib.raycast_last_variant(own) == (4, 0)
    mid = float(np.median(ref.t_hit))
    for r in (rays, rs, rs, rays):
        assert same_bits(mesh.count_intersections(r), ref.counts)
        assert same_cast(mesh.cast_rayset(rs), cast0) and rs.last_variant() == (4, 0)
        assert same_bits(mesh.count_intersections(r), ref.counts)
        assert same_bits(mesh.test_occlusions(r, mid, np.inf), ref.occluded(mid, np.inf))
        assert same_cast(mesh.cast_rays(rays), cast0) and _lib.raycast_last_variant(own) == (4, 0)
        assert same_bits(mesh.test_occlusions(r, mid, np.inf), ref.occluded(mid, np.inf))
        assert_list(mesh.list_intersections(r), ref, "interleaved")
        assert same_cast(mesh.cast_rayset(rs), cast0) and same_cast(mesh.cast_rays(rays), cast0)
        assert_list(mesh.list_intersections(r), ref, "interleaved, again")
        assert _lib.intersections_last_path(own) == (GRID, 0)
    assert rs.last_variant() == (4, 0) and _lib.raycast_last_variant(own) == (4, 0)
    rs.close()


def test_crowded_count_leaves_the_casts_choice_alone(own, oracle, parity):
    """After a count the grid gave up on, the next cast of that ray count still tries the grid first, as on a fresh context:
    the queries have status words and an avoid-list of their own."""
    from pedp_hip import _lib

    f = parity["f"]
    n = 20000
    base_ref = parity["ref"].rows(np.arange(n))
    crowd = parity["rays"][:n].copy()
    crowd[100:400] = crowd[int(np.flatnonzero(base_ref.counts > 0)[0])]
    ref = patched(oracle, f.verts_posed, f.tris, base_ref, crowd, np.arange(100, 400))
    mesh = _lib.Mesh(own, f.verts_posed, f.tris)
    assert same_bits(mesh.count_intersections(crowd), ref.counts)
    assert _lib.intersections_last_path(own) == (GRID, 4)
    cast = mesh.cast_rays(crowd)
    assert _lib.raycast_last_variant(own) == (4, 4)
    hit = ref.counts > 0
    assert same_bits(cast["t_hit"][hit], ref.t_hit[ref.ray_splits[:-1][hit]])
    # the queries' own choice: that ray count goes to the exhaustive path from now on, other counts to the grid
    assert same_bits(mesh.count_intersections(crowd), ref.counts)
    assert _lib.intersections_last_path(own) == (EXHAUSTIVE, 0)
    assert same_bits(mesh.count_intersections(crowd[:18000]), ref.counts[:18000])
    assert _lib.intersections_last_path(own) == (GRID, 4)
    mesh.close()


# ---------------------------------------------------------------- 10. errors
def test_errors(ctx, own):
    from pedp_hip import PedpError, _lib

    rays = np.zeros((4, 6), np.float32)
    rays[:, 5] = 1.0
    empty = _lib.Mesh(ctx, np.zeros((3, 3), np.float32), np.zeros((0, 3), np.uint32))
    for query in (empty.count_intersections, empty.test_occlusions, empty.list_intersections):
        with pytest.raises(PedpError, match="no triangles"):
            query(rays)
    with pytest.raises(PedpError):
        _lib.RaySet(ctx, np.zeros((0, 6), np.float32))                 # a ray set cannot be empty
    mesh = _lib.Mesh(ctx, CUBE_V, CUBE_T)
    foreign = _lib.RaySet(own, rays)
    for query in (mesh.count_intersections, mesh.test_occlusions, mesh.list_intersections):
        with pytest.raises(PedpError, match="another context"):
            query(foreign)
    lib = _lib.load()
    out = np.zeros(4, np.int32)
    assert lib.pedp_count_intersections(ctx._h, mesh._h, _lib._ptr(rays), 4, 7, _lib._ptr(out)) != 0          # bad mem flag
    assert lib.pedp_count_intersections(ctx._h, mesh._h, None, 4, _lib.HOST, _lib._ptr(out)) != 0             # null rays
    assert lib.pedp_count_intersections(ctx._h, mesh._h, _lib._ptr(rays), 4, _lib.HOST, None) != 0            # null output
    assert lib.pedp_count_intersections(ctx._h, mesh._h, _lib._ptr(rays), -1, _lib.HOST, _lib._ptr(out)) != 0
    assert lib.pedp_count_intersections(ctx._h, None, _lib._ptr(rays), 4, _lib.HOST, _lib._ptr(out)) != 0
    assert lib.pedp_test_occlusions(ctx._h, mesh._h, _lib._ptr(rays), 4, _lib.HOST, C.c_float(0), C.c_float(1), None) != 0
    total = C.c_int64()
    assert lib.pedp_list_intersections(ctx._h, mesh._h, _lib._ptr(rays), 4, _lib.HOST, -1, _lib._ptr(np.zeros(5, np.int64)), None,
                                       None, None, None, C.byref(total)) != 0
    assert lib.pedp_list_intersections(ctx._h, mesh._h, _lib._ptr(rays), 4, _lib.HOST, 8, None, None, None, None, None,
                                       C.byref(total)) != 0
    fresh = _lib.Context(0)
    with pytest.raises(PedpError, match="no all-hits query"):
        _lib.intersections_last_path(fresh)
    fresh.close()
    foreign.close()
    mesh.close()
    empty.close()


# ---------------------------------------------------------------- the public scene
def test_raycasting_scene_numpy_and_tensors(oracle):
    """RaycastingScene over arrays and CUDA tensors of shape (..., 6): the leading shape comes back, the list runs over the
    rays in row-major order, and the five older queries are what surface_distance and the cast give."""
    torch = pytest.importorskip("torch")
    from pedp_hip import surface_distance as sd, synth
    from pedp_hip.raycasting_scene import RaycastingScene

    f = synth.Frame("tiny")
    ref = all_hits(oracle, f.verts_posed, f.tris, f.rays6)
    cast = oracle.raycast(f.verts_posed, f.tris, f.rays6)
    lead = (f.height, f.width)
    mid = float(np.median(ref.t_hit))
    for to in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
        scene = RaycastingScene()
        assert scene.add_triangles(f.verts_posed, f.tris) == 0
        with pytest.raises(NotImplementedError):
            scene.add_triangles(f.verts_posed, f.tris)
        rays = to(f.rays6.reshape(lead + (6,)))
        host = (lambda x: x.cpu().numpy()) if torch.is_tensor(rays) else (lambda x: x)
        counts, occ, hits, lst = scene.count_intersections(rays), scene.test_occlusions(rays, mid, np.inf), scene.cast_rays(rays), \
            scene.list_intersections(rays)
        assert type(counts) is type(rays) and tuple(counts.shape) == lead and tuple(occ.shape) == lead
        assert same_bits(host(counts).reshape(-1), ref.counts)
        assert same_bits(host(occ).reshape(-1), ref.occluded(mid, np.inf))
        assert_list({k: host(v) for k, v in lst.items()}, ref, "scene")
        assert tuple(hits["primitive_uvs"].shape) == lead + (2,)
        for k in ("t_hit", "primitive_ids", "primitive_uvs"):
            assert same_bits(host(hits[k]).reshape(cast[k].shape), cast[k]), k
        assert same_bits(host(hits["geometry_ids"]).reshape(-1) == 0, np.isfinite(cast["t_hit"]))
        pts = to(np.random.default_rng(3).normal(0, 60, (5, 7, 3)) + f.verts_posed.mean(axis=0))
        assert same_bits(host(scene.compute_distance(pts)), host(sd.compute_distance(scene._mesh, pts)))
        assert same_bits(host(scene.compute_closest_points(pts)["points"]), host(sd.closest_points(scene._mesh, pts)["points"]))
        signed, inside = host(scene.compute_signed_distance(pts)), host(scene.compute_occupancy(pts))
        assert signed.shape == (5, 7) and same_bits(np.abs(signed), host(scene.compute_distance(pts)))
        assert same_bits(inside.astype(bool), signed < 0)


