"""The coverage map on the device (csrc/pedp_coverage.hip) against its restatement
(tests/_coverage_ref.py): bit for bit, except the floating-point area sums, which are held to s4.17's bound of any
summation order (n_faces 2^-52 relative to math.fsum) and to repeatability."""
import ctypes as C
import functools

import numpy as np
import pytest

import _coverage_ref as ref
import _defect_map_ref as dref
from pedp_hip import coverage  # noqa: F401  (without the feature every test here fails at import)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
FRAMES = [(1, 1), (63, 1), (64, 1), (65, 1), (16, 16), (257, 1), (241, 17)]      # (W, H): 1 ... 4097 pixels
QUAD = (np.array([[-10.0, -10.0, 4.0], [10.0, -10.0, 4.0], [10.0, 10.0, 4.0], [-10.0, 10.0, 4.0]]),
        np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))


def rot_x(a):
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


def rot_y(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def tilted_quad():
    v, t = QUAD
    return (v - [0.0, 0.0, 4.0]) @ rot_x(np.deg2rad(60.0)).T * [1.0, 0.2, 0.2] + [0.0, 0.0, 4.0], t


MESHES = {
    "quad": lambda: QUAD,
    "tilted_quad": tilted_quad,
    "torus1022": lambda: dref.torus(73, 7),
    "torus2044": lambda: dref.torus(73, 14),
    "torus32000": lambda: dref.torus(200, 80),
    "two_tori": lambda: dref.two_tori(50, 40),
}
# model -> camera: rotation and translation; the tori a long way off, so that most faces of the small one are under a pixel
POSES = {
    "quad": [(np.eye(3), [0.0, 0.0, 0.0])],
    "tilted_quad": [(np.eye(3), [0.0, 0.0, 0.0])],
    "torus1022": [(rot_x(0.6), [0.0, 0.0, 1500.0])],
    "torus2044": [(rot_x(0.6), [0.0, 0.0, 1500.0])],
    "torus32000": [(rot_x(0.6), [3.0, -2.0, 200.0]), (rot_x(-0.9) @ rot_y(0.4), [-5.0, 4.0, 230.0]), (rot_x(2.4), [0.0, 0.0, 180.0])],
    "two_tori": [(rot_x(0.5), [-100.0, 0.0, 600.0]), (rot_x(-1.0), [-100.0, 10.0, 650.0]), (rot_x(2.6) @ rot_y(0.2), [-90.0, 0.0, 560.0])],
}


@functools.lru_cache(maxsize=None)
def model(name):
    return dref.Model(*MESHES[name]())


@functools.lru_cache(maxsize=None)
def posed(name, k=0):
    """float32 vertices of pose k, as a mesh handle takes them, and the records the kernel reads."""
    R, t = POSES[name][k]
    v = np.ascontiguousarray((model(name).verts @ R.T + np.asarray(t)).astype(np.float32))
    return v, ref.records(v, model(name).tris)


def camera(W, H, f):
    return ref.intrinsics(f, f, (W - 1) / 2, (H - 1) / 2)


FOCAL = {"torus32000": 120.0, "two_tori": 100.0}
_maps, _meshes, _casts = {}, {}, {}


@pytest.fixture
def world(ctx):
    """name -> the (cleared) CoverageMap of that model on the session's context, and mesh handles / casts built once."""
    from pedp_hip import CoverageMap, _lib

    class World:
        def cov(self, name):
            if name not in _maps:
                m = model(name)
                _maps[name] = CoverageMap((m.verts, m.tris), ctx)
            _maps[name].clear()
            return _maps[name]

        def mesh(self, name, k=0):
            if (name, k) not in _meshes:
                _meshes[name, k] = _lib.Mesh(ctx, posed(name, k)[0], model(name).tris)
            return _meshes[name, k]

        def cast(self, name, k, K, W, H):
            """t_hit H x W float32, primitive_ids H x W uint32 of the camera's rays against pose k."""
            key = (name, k, K.tobytes(), W, H)
            if key not in _casts:
                hit = self.mesh(name, k).cast_rays(ref.rays6(K, W, H), want_uv=False)
                _casts[key] = (hit["t_hit"].reshape(H, W), hit["primitive_ids"].reshape(H, W))
            return _casts[key]

    return World()


def same_faces(got, want):
    for k in ref.FACE_KEYS:
        assert got[k].dtype == want[k].dtype and dref.same_bits(got[k], want[k]), k


def same_regions(got, want):
    assert got["n_regions"] == want["n_regions"]
    assert np.array_equal(got["labels"], want["labels"])
    for k in dref.INT_COLUMNS:
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    for k in dref.BIT_COLUMNS:
        assert dref.same_bits(got[k], want[k]), k
    n = want["n_faces"].astype(np.float64)
    assert (np.abs(got["area"] - want["area"]) <= n * EPS * want["area"]).all(), "area beyond n_faces 2^-52 of fsum"
    assert (np.abs(got["moment"] - want["moment"]) <= n[:, None] * EPS * want["abs_moment"]).all(), "moment beyond n_faces 2^-52"
    assert np.array_equal(got["centroid"], got["moment"] / got["area"][:, None])


def same_summary(got, want, F):
    assert got["covered_faces"] == want["covered_faces"] and got["faces"] == want["faces"] == F
    for k in ("covered_area", "total_area"):
        assert abs(got[k] - want[k]) <= F * EPS * want[k], k
    assert got["fraction"] == got["covered_area"] / got["total_area"]


def same_table_bits(a, b):
    from pedp_hip.defect_map import REGION_DTYPE

    assert a["n_regions"] == b["n_regions"] and np.array_equal(a["labels"], b["labels"])
    for k in REGION_DTYPE.names:
        assert dref.same_bits(a[k], b[k]), k


# ------------------------------------------------------------------ sizes where the lane, wave and block logic can go wrong
def poked(t, ids, F, seed):
    """The cast with rows that take no part put inside the runs: ids >= F, the miss id, NaN and infinite t."""
    t, ids = t.copy().reshape(-1), ids.copy().reshape(-1)
    n = len(t)
    if n >= 63:
        rng = np.random.default_rng(seed)
        where = rng.choice(n, 4 * (n // 16), replace=False).reshape(4, -1)
        ids[where[0]] = rng.integers(F, 2 ** 32 - 1, where.shape[1])
        ids[where[1]] = dref.MISS
        t[where[2]] = np.nan
        t[where[3]] = rng.choice([np.inf, -np.inf], where.shape[1])
    return t, ids


@pytest.mark.parametrize("name", ["quad", "torus1022", "torus2044"])
@pytest.mark.parametrize("W,H", FRAMES)
def test_frame_sizes(world, name, W, H):
    """The two-triangle quad fills every frame: runs cross the wave and block boundaries and every atomic is contended.
    The 1022-face torus(73, 7) and torus(73, 14) are a long way off: most faces are under a pixel, so there are next to no
    runs."""
    m, cov, mesh = model(name), world.cov(name), world.mesh(name)
    K = camera(W, H, 300.0)
    rec = posed(name)[1]
    t0, ids0 = world.cast(name, 0, K, W, H)
    if name == "quad":
        assert np.isfinite(t0).all()
    elif W * H > 4000:
        hit = ids0[np.isfinite(t0)]
        assert len(hit) > 100 and len(np.unique(hit)) > 0.5 * len(hit)
    st = ref.State(m.F)
    for view, (t, ids) in enumerate([(t0.reshape(-1), ids0.reshape(-1)), poked(t0, ids0, m.F, W)]):
        status = cov.add_cast(mesh, K, t.reshape(H, W), ids.reshape(H, W), want_status=True)
        st.add(rec, K, W, H, t, ids)
        assert status.dtype == np.uint8 and np.array_equal(status.reshape(-1), st.last["status"])
        same_faces(cov.faces(), st.faces())
        assert cov.stats() == st.stats() and st.stats()["views"] == view + 1
    if name == "quad":
        assert st.pixels.sum() >= W * H and (st.views == 2).any()


def test_a_64_by_48_frame_over_the_fine_torus(world):
    name, (W, H) = "torus32000", (64, 48)
    m, cov, K = model(name), world.cov(name), camera(64, 48, FOCAL[name])
    st = ref.State(m.F)
    for k in range(3):
        t, ids = world.cast(name, k, K, W, H)
        assert 300 < np.isfinite(t).sum() <= W * H
        cov.add_cast(world.mesh(name, k), K, t, ids)
        st.add(posed(name, k)[1], K, W, H, t, ids)
    same_faces(cov.faces(), st.faces())
    assert cov.stats() == st.stats() and (st.views >= 2).any()


# ------------------------------------------------------------------ classes
def depth_image(z_hit, W, H):
    """The restatement's z_hit as a sensor would report it in metres (float32), with patches moved nearer and farther,
    invalid values, a masked block, and one pixel whose difference IS the tolerance.  Returns depth H x W, mask H x W,
    depth_tol and that pixel."""
    ok = np.isfinite(z_hit).reshape(H, W)
    z = np.where(ok, z_hit.reshape(H, W), 0.0)
    depth = (z / 1000.0).astype(np.float32)
    r, c = H // 2, W // 2
    near, far = (slice(r + 2, r + 6), slice(c - 10, c - 2)), (slice(r + 2, r + 6), slice(c + 6, c + 14))
    bad, masked = (slice(r - 7, r - 5), slice(c - 9, c - 5)), (slice(r - 3, r), slice(5, 25))
    free = ok & (z > 0)
    for region in (near, far, bad, masked):
        free[region] = False
    i = np.flatnonzero(free)[free.sum() // 2]
    depth.reshape(-1)[i] *= np.float32(1.0 + 2.0 ** -9)                       # farther by about 0.2 %
    tol = float(depth.reshape(-1)[i]) * 1000.0 - float(z.reshape(-1)[i])     # the kernel's own expression at that pixel
    assert tol > 0
    depth[near] -= np.float32(3.0 * tol / 1000.0)                             # something in front
    depth[far] += np.float32(3.0 * tol / 1000.0)                              # looked through
    depth[bad] = [[0.0, np.nan, 0.0005, np.inf], [-1.0, -np.inf, 0.0, np.nan]]
    mask = np.ones((H, W), np.uint8)
    mask[masked] = 0
    return depth, mask, tol, i


@pytest.mark.parametrize("min_cos", [0.0, 0.5, 1.0])
def test_classes_on_the_tilted_quad(world, min_cos):
    name, (W, H) = "tilted_quad", (64, 48)
    m, cov, mesh, K = model(name), world.cov(name), world.mesh(name), camera(64, 48, 60.0)
    rec = posed(name)[1]
    t, ids = world.cast(name, 0, K, W, H)
    plain = ref.classify(rec, K, W, H, t, ids)
    depth, mask, tol, exact = depth_image(plain["z_hit"], W, H)
    kw = dict(depth=depth, mask=mask, depth_scale=1000.0, depth_tol=tol, min_cos=min_cos)
    st = ref.State(m.F).add(rec, K, W, H, t, ids, **kw)
    status = cov.add_cast(mesh, K, t, ids, want_status=True, **kw)
    assert np.array_equal(status.reshape(-1), st.last["status"])
    assert cov.stats() == st.stats()
    same_faces(cov.faces(), st.faces())
    s = st.stats()
    assert s["masked"] == 60 and s["no_depth"] == 8 and s["occluded"] >= 12 and s["behind"] >= 12 and s["miss"] > 0
    assert st.last["status"][exact] == (ref.SEEN if st.last["cos"][exact] >= min_cos else ref.GRAZING)
    assert ref.classify(rec, K, W, H, t, ids, **dict(kw, depth_tol=np.nextafter(tol, 0.0)))["status"][exact] == ref.BEHIND
    if min_cos == 0.0:
        assert s["grazing"] == 0 and s["seen"] > 500
    elif min_cos == 0.5:
        assert s["grazing"] > 100 and s["seen"] > 100                # the cosine crosses 0.5 inside the frame
    else:
        assert s["seen"] == 0 and s["grazing"] > 500 and not cov.faces()["pixels"].any()
    assert (cov.faces()["blocked"] > 0).any()


# ------------------------------------------------------------------ the state is a function of the views
def three_views(world, name, K, W, H):
    views = []
    for k in range(3):
        t, ids = world.cast(name, k, K, W, H)
        z = ref.classify(posed(name, k)[1], K, W, H, t, ids)["z_hit"]
        depth, mask, tol, _ = depth_image(z, W, H)
        views.append((k, t, ids, dict(depth=depth, mask=mask, depth_scale=1000.0, depth_tol=tol, min_cos=0.2)))
    return views


def test_order_repetition_and_clear(world):
    name, (W, H) = "torus32000", (64, 48)
    m, cov, K = model(name), world.cov(name), camera(64, 48, FOCAL[name])
    a, b, _ = three_views(world, name, K, W, H)

    def add(v):
        cov.add_cast(world.mesh(name, v[0]), K, v[1], v[2], **v[3])

    add(a)
    add(b)
    ab, stats = cov.faces(), cov.stats()
    want = ref.State(m.F).add(posed(name, 0)[1], K, W, H, a[1], a[2], **a[3]).add(posed(name, 1)[1], K, W, H, b[1], b[2], **b[3])
    same_faces(ab, want.faces())
    assert stats == want.stats() and (ab["blocked"] > 0).any() and (ab["views"] == 2).any()
    cov.clear()
    assert cov.stats() == dict.fromkeys(stats, 0) and not cov.faces()["pixels"].any() and np.isinf(cov.faces()["min_footprint"]).all()
    add(b)
    add(a)
    same_faces(cov.faces(), ab)                                      # the other order: the same bits
    assert cov.stats() == stats
    cov.clear()
    add(a)
    one = cov.faces()
    add(a)
    two = cov.faces()                                                # the same view twice
    assert np.array_equal(two["pixels"], 2 * one["pixels"]) and np.array_equal(two["blocked"], 2 * one["blocked"])
    assert np.array_equal(two["views"], 2 * one["views"]) and set(np.unique(two["views"])) == {0, 2}
    assert dref.same_bits(two["best_cos"], one["best_cos"]) and dref.same_bits(two["min_footprint"], one["min_footprint"])
    cov.clear()
    add(a)
    same_faces(cov.faces(), one)                                     # clear + re-add


def test_the_shared_defect_map_and_the_coverage_do_not_touch_each_other(world):
    name, (W, H) = "torus32000", (64, 48)
    m, cov, K = model(name), world.cov(name), camera(64, 48, FOCAL[name])
    dm = cov.defect_map
    dm.clear()
    rng = np.random.default_rng(4)
    ids, x = rng.integers(0, m.F, 5000).astype(np.uint32), rng.uniform(0.0, 1.0, 5000)
    dm.add(ids, x)

    def same_map(faces, stats, regions):
        """The defect map's own state as it stands: nothing is cleared or added in front of the comparison."""
        now = dm.faces()
        assert all(dref.same_bits(now[k], faces[k]) for k in faces) and dm.stats() == stats
        same_table_bits(dm.regions(0.5, 1, 1), regions)

    faces_before, stats_before, regions_before = dm.faces(), dm.stats(), dm.regions(0.5, 1, 1)
    want = dref.State(m.F).add(ids, x)
    assert all(dref.same_bits(faces_before[k], want.faces()[k]) for k in faces_before) and (faces_before["hits"] > 0).any()
    a, b, _ = three_views(world, name, K, W, H)
    cov.add_cast(world.mesh(name, 0), K, a[1], a[2], **a[3])
    same_map(faces_before, stats_before, regions_before)             # the map's own faces() is untouched by add
    one = cov.faces()
    dm.add(ids[::-1].copy(), x[::-1].copy())                         # an unrelated observation on the shared map
    same_faces(cov.faces(), one)
    faces_two, stats_two, regions_two = dm.faces(), dm.stats(), dm.regions(0.5, 1, 1)
    want.add(ids[::-1], x[::-1])
    assert all(dref.same_bits(faces_two[k], want.faces()[k]) for k in faces_two) and stats_two == want.stats()
    cov.add_cast(world.mesh(name, 1), K, b[1], b[2], **b[3])
    cov.regions(grow=1)
    cov.summary()
    cov.regions(covered=True)
    same_map(faces_two, stats_two, regions_two)                      # nor by a second view, regions or summary
    dm.clear()
    dm.add(ids, x)
    after = dm.faces()
    assert all(dref.same_bits(after[k], faces_before[k]) for k in after)
    same_table_bits(dm.regions(0.5, 1, 1), regions_before)
    dm.clear()


def test_host_memory_device_memory_and_a_side_stream(ctx, world):
    import torch
    from pedp_hip import CoverageMap, DefectMap, _lib

    name, (W, H) = "torus2044", (241, 17)
    m, K = model(name), camera(241, 17, 300.0)
    t, ids = world.cast(name, 0, K, W, H)
    z = ref.classify(posed(name)[1], K, W, H, t, ids)["z_hit"]
    depth, mask, tol, _ = depth_image(z, W, H)
    kw = dict(depth_scale=1000.0, depth_tol=tol, min_cos=0.1)
    cov = world.cov(name)
    host_status = cov.add_cast(world.mesh(name), K, t, ids, depth=depth, mask=mask, want_status=True, **kw)
    host, stats = cov.faces(), cov.stats()
    same_faces(host, ref.State(m.F).add(posed(name)[1], K, W, H, t, ids, depth=depth, mask=mask, **kw).faces())
    cov.clear()
    cuda = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    status = cov.add_cast(world.mesh(name), K, cuda(t), cuda(ids.view(np.int32)), depth=cuda(depth), mask=cuda(mask.astype(bool)),
                          want_status=True, **kw)                    # torch's default stream
    assert status.is_cuda and np.array_equal(status.cpu().numpy(), host_status)
    same_faces(cov.faces(), host)
    assert cov.stats() == stats
    # device outputs of faces
    out = [torch.empty(m.F, dtype=d, device="cuda") for d in (torch.int64, torch.int32, torch.float64, torch.float64, torch.int64)]
    torch.cuda.synchronize()
    assert _lib.load().pedp_coverage_faces(cov._h, _lib.DEVICE, *[C.c_void_p(o.data_ptr()) for o in out]) == 0
    ctx.synchronize()
    same_faces(dict(zip(ref.FACE_KEYS, [o.cpu().numpy() for o in out])), host)
    only = np.empty(m.F, np.int64)                                   # every pointer of faces is nullable
    assert _lib.load().pedp_coverage_faces(cov._h, _lib.HOST, None, None, None, None, _lib._ptr(only)) == 0
    assert np.array_equal(only, host["blocked"])
    # a context on a side stream: the tensors are made and read on that stream
    side = torch.cuda.Stream()
    sctx = _lib.Context(0, stream=side.cuda_stream)
    scov = CoverageMap((m.verts, m.tris), sctx)
    smesh = _lib.Mesh(sctx, posed(name)[0], m.tris)
    with torch.cuda.stream(side):
        status = scov.add_cast(smesh, K, cuda(t), cuda(ids.view(np.int32)), depth=cuda(depth), mask=cuda(mask), want_status=True, **kw)
        on_side = status.cpu().numpy()
    assert np.array_equal(on_side, host_status)
    same_faces(scov.faces(), host)
    with pytest.raises(_lib.PedpError, match="another context"):
        scov.add_cast(world.mesh(name), K, t, ids)
    assert scov.stats()["views"] == 1
    # add_view on the stream the context shares with torch (nothing waits) against the same cast through add_cast
    rays = _lib.RaySet(sctx, ref.rays6(K, W, H))
    hit = smesh.cast_rayset(rays, want_uv=False)
    scov.clear()
    by_cast = scov.add_cast(smesh, K, hit["t_hit"].reshape(H, W), hit["primitive_ids"].reshape(H, W), depth=depth, mask=mask,
                            want_status=True, **kw)
    faces_by_cast = scov.faces()
    scov.clear()
    with torch.cuda.stream(side):
        status = scov.add_view(smesh, K, (H, W), depth=cuda(depth), mask=cuda(mask), want_status=True, **kw)
        scov.add_view(smesh, K, (H, W), depth=cuda(depth), mask=cuda(mask), **kw)      # the camera's buffers a second time
        by_view = status.cpu().numpy()
    assert np.array_equal(by_view, by_cast) and (by_cast == ref.SEEN).any()
    twice = scov.faces()
    assert np.array_equal(twice["pixels"], 2 * faces_by_cast["pixels"]) and np.array_equal(twice["views"], 2 * faces_by_cast["views"])
    assert dref.same_bits(twice["best_cos"], faces_by_cast["best_cos"]) and len(scov._cameras) == 1
    rays.close()
    # the coverage map closes the defect map it made, and refuses every call once the map under it is closed
    made = scov.defect_map
    scov.close()
    assert not made._h
    with pytest.raises(_lib.PedpError, match="closed"):
        scov.faces()
    shared_map = DefectMap((m.verts, m.tris), sctx)
    over = CoverageMap(shared_map)
    assert over.defect_map is shared_map and over.summary()["covered_faces"] == 0
    shared_map.close()
    for call in (over.faces, over.summary, over.regions, over.stats, over.clear, lambda: over.add_cast(smesh, K, t, ids),
                 lambda: over.add_view(smesh, K, (H, W))):
        with pytest.raises(_lib.PedpError, match="defect map under the coverage map is closed"):
            call()
    over.close()
    with pytest.raises(_lib.PedpError, match="the defect map is closed"):
        CoverageMap(shared_map)
    smesh.close()
    sctx.close()


# ------------------------------------------------------------------ end to end
def test_add_view_equals_cast_rayset_and_add_cast(ctx):
    import torch
    from pedp_hip import CoverageMap, _lib, synth
    from pedp_hip.coverage import pixel_rays6

    verts, tris, _ = synth.bumpy_torus(40, 16)
    W, H = 64, 48
    K = camera(W, H, 60.0)
    nudge = np.eye(4)
    nudge[:3, :3] = synth.axis_angle([0.0, 1.0, 0.0], np.deg2rad(25.0))
    nudge[:3, 3] = [4.0, -3.0, 20.0]
    poses = [synth.gt_pose(), nudge @ synth.gt_pose()]
    m = dref.Model(verts.astype(np.float64), tris)
    mesh = _lib.Mesh(ctx, verts.astype(np.float64), tris, posable=True)
    cov, other = CoverageMap((m.verts, m.tris), ctx), CoverageMap((m.verts, m.tris), ctx)
    assert np.array_equal(pixel_rays6(K, W, H), ref.rays6(K, W, H))
    rays = _lib.RaySet(ctx, ref.rays6(K, W, H))
    st = ref.State(m.F)
    for i, T in enumerate(poses):
        mesh.set_pose(T)
        rec = ref.records(mesh.posed_vertices(T).astype(np.float32), tris)
        hit = mesh.cast_rayset(rays, want_uv=False)
        t, ids = hit["t_hit"].reshape(H, W), hit["primitive_ids"].reshape(H, W)
        z = ref.classify(rec, K, W, H, t, ids)["z_hit"].reshape(H, W)
        depth = (np.where(np.isfinite(z), z, 0.0) / 1000.0).astype(np.float32)
        ys, xs = np.nonzero(np.isfinite(z))
        cy, cx = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])           # a pixel on the surface, half way down the hits
        depth[cy - 2:cy + 2, cx - 2:cx + 2] += np.float32(0.004)     # a dent: 4 mm behind the model's surface
        depth[cy + 4:cy + 9, cx - 6:cx] -= np.float32(0.030)         # a fixture 30 mm in front of it
        kw = dict(depth=depth, depth_scale=1000.0, depth_tol=1.5, min_cos=0.15)
        d = torch.from_numpy(depth).cuda() if i else depth           # a depth image on the host, then one on the device
        status = cov.add_view(mesh, K, (H, W), want_status=True, **dict(kw, depth=d))
        want_status = other.add_cast(mesh, K, t, ids, want_status=True, **kw)
        st.add(rec, K, W, H, t, ids, **kw)
        assert status.is_cuda and np.array_equal(status.cpu().numpy(), want_status)
        assert np.array_equal(want_status.reshape(-1), st.last["status"])
        assert len(cov._cameras) == 1                                # the second view casts the first one's RaySet
    s = st.stats()
    assert s["views"] == 2 and s["behind"] > 0 and s["occluded"] > 0 and s["seen"] > 300
    same_faces(cov.faces(), st.faces())
    same_faces(other.faces(), st.faces())
    assert cov.stats() == other.stats() == s
    same_summary(cov.summary(min_cos=0.5), st.summary(m, min_cos=0.5), m.F)
    same_regions(cov.regions(grow=1, min_cos=0.5), ref.regions(m, st, grow=1, min_cos=0.5))
    assert np.array_equal(cov.covered(min_views=2), st.covered(min_views=2)) and st.covered(min_views=2).any()
    for by in ("views", "best_cos", "min_footprint"):
        colors = cov.face_colors(by=by)
        assert colors.shape == (m.F, 3) and (colors[st.pixels == 0] == 0.5).all() and (colors[st.pixels > 0] != 0.5).any()
    small = _lib.Mesh(ctx, verts[:30], tris[:4] % 30)
    with pytest.raises(_lib.PedpError, match="faces"):
        cov.add_view(small, K, (H, W))
    for h in (small, mesh, rays, other, cov):
        h.close()


# ------------------------------------------------------------------ summary and regions
@pytest.mark.parametrize("name", ["torus32000", "two_tori"])
def test_summary_and_regions(world, name):
    W, H = 64, 48
    m, cov, K = model(name), world.cov(name), camera(64, 48, FOCAL[name])
    st = ref.State(m.F)
    for k, t, ids, kw in three_views(world, name, K, W, H):
        cov.add_cast(world.mesh(name, k), K, t, ids, **kw)
        st.add(posed(name, k)[1], K, W, H, t, ids, **kw)
        if k == 1:
            continue                                                 # after one view and after three
        same_faces(cov.faces(), st.faces())
        for criteria in ({}, dict(min_views=2, min_cos=0.5) if k else dict(min_pixels=2, max_footprint=40.0)):
            assert np.array_equal(cov.covered(**criteria), st.covered(**criteria))
            same_summary(cov.summary(**criteria), st.summary(m, **criteria), m.F)
            for covered in (False, True):
                for grow in (0, 1):
                    got, want = cov.regions(covered, grow, **criteria), ref.regions(m, st, covered, grow, **criteria)
                    assert want["n_regions"] >= 1 or criteria
                    same_regions(got, want)
        assert 0 < st.covered().sum() < m.F
    a, b = cov.regions(grow=1), cov.regions(grow=1)                  # the same bits on every call
    same_table_bits(a, b)
    assert cov.summary() == cov.summary()
    cov.regions(True, 0, min_views=2)
    same_table_bits(cov.regions(grow=1), a)


def test_more_regions_than_room(world):
    from pedp_hip import _lib
    from pedp_hip.defect_map import REGION_DTYPE

    name, (W, H) = "two_tori", (64, 48)
    m, cov, K = model(name), world.cov(name), camera(64, 48, FOCAL[name])
    want = cov.regions()                                             # nothing seen: each torus is one uncovered region
    assert want["n_regions"] == 2 and list(want["n_faces"]) == [m.F // 2, m.F // 2] and not want["hits"].any()
    assert cov.regions(covered=True)["n_regions"] == 0
    with pytest.raises(_lib.PedpError, match="2 regions, room for 1"):
        cov.regions(capacity=1)
    table = np.full(1, 7, dtype=np.uint8).repeat(REGION_DTYPE.itemsize).view(REGION_DTYPE)
    before = table.tobytes()
    labels, n = np.empty(m.F, np.int32), C.c_int64()
    lib = _lib.load()
    rc = lib.pedp_coverage_regions(cov._h, None, 0, 0, _lib.HOST, _lib._ptr(labels), 1, _lib._ptr(table), C.byref(n))
    assert rc == -1 and n.value == 2 and table.tobytes() == before
    assert (labels[:m.F // 2] == 0).all() and (labels[m.F // 2:] == 1).all()
    rc = lib.pedp_coverage_regions(cov._h, None, 0, 65, _lib.HOST, None, 0, None, C.byref(n))
    assert rc == -1 and b"grow" in lib.pedp_last_error()
    t, ids = world.cast(name, 0, K, W, H)
    cov.add_cast(world.mesh(name, 0), K, t, ids)
    many = cov.regions(covered=True)                                 # far more than the first guess of 1024? retried with room
    assert many["n_regions"] == ref.regions(m, ref.State(m.F).add(posed(name, 0)[1], K, W, H, t, ids), covered=True)["n_regions"]


def test_the_c_abi_refuses_what_the_contract_names(ctx, world):
    from pedp_hip import _lib

    name, (W, H) = "quad", (16, 16)
    cov, mesh, K = world.cov(name), world.mesh(name), camera(16, 16, 300.0)
    t, ids = world.cast(name, 0, K, W, H)
    depth = np.full((H, W), 4.0, np.float32)
    lib = _lib.load()
    cam = _lib.Pinhole(300.0, 300.0, 7.5, 7.5, W, H)

    def add(mesh_h=mesh._h, prm=None, d=None):
        return lib.pedp_coverage_add(cov._h, mesh_h, C.byref(cam), _lib._ptr(t), _lib._ptr(ids), _lib._ptr(d),
                                     None, C.byref(prm) if prm is not None else None, _lib.HOST, None)

    assert add() == 0
    assert add(prm=_lib.CoverageView(1.0, 0.5, 0.0, 0.001), d=depth) == 0
    assert add(d=depth) == -1 and b"depth_tol" in lib.pedp_last_error()
    assert add(prm=_lib.CoverageView(1.0, -0.5, 0.0, 0.001), d=depth) == -1
    assert add(prm=_lib.CoverageView(1.0, float("nan"), 0.0, 0.001), d=depth) == -1
    assert add(prm=_lib.CoverageView(1.0, -0.5, 0.0, 0.001)) == 0            # without depth the tolerance is not looked at
    assert add(prm=_lib.CoverageView(1.0, 0.5, 1.5, 0.001)) == -1 and b"min_cos" in lib.pedp_last_error()
    assert add(prm=_lib.CoverageView(1.0, 0.5, -0.1, 0.001)) == -1
    assert add(mesh_h=world.mesh("torus2044")._h) == -1 and b"faces" in lib.pedp_last_error()
    octx = _lib.Context(0)
    omesh = _lib.Mesh(octx, posed(name)[0], model(name).tris)
    assert add(mesh_h=omesh._h) == -1 and b"context" in lib.pedp_last_error()
    omesh.close()
    octx.close()
    assert cov.stats()["views"] == 3 and cov.stats()["seen"] == 3 * W * H


# ------------------------------------------------------------------ pending registration and history
def tiny_view(ctx):
    """A coverage map, the posed mesh and one cast view of synth's tiny frame on `ctx`."""
    from pedp_hip import CoverageMap, _lib, synth

    f = synth.Frame("tiny")
    W, H = f.width, f.height
    K = ref.intrinsics(f.f, f.f, f.cx, f.cy)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    hit = mesh.cast_rays(ref.rays6(K, W, H), want_uv=False)
    t, ids = hit["t_hit"].reshape(H, W), hit["primitive_ids"].reshape(H, W)
    rec = ref.records(f.verts_posed, f.tris)
    z = ref.classify(rec, K, W, H, t, ids)["z_hit"].reshape(H, W)
    depth = (np.where(np.isfinite(z), z, 0.0) / 1000.0).astype(np.float32)
    depth[10:14, 20:26] -= np.float32(0.02)
    kw = dict(depth=depth, depth_scale=1000.0, depth_tol=2.0, min_cos=0.1)
    cov = CoverageMap((f.verts.astype(np.float64), f.tris), ctx)
    want = ref.State(cov.F).add(rec, K, W, H, t, ids, **kw)
    return f, cov, mesh, K, t, ids, kw, want


def test_device_add_while_a_registration_is_pending(ctx):
    """pedp_coverage_add with PEDP_DEVICE only enqueues and has no workspace: a pending registration's result is
    unchanged.  The calls that wait on the stream are refused."""
    import torch
    from pedp_hip import _lib

    f, cov, mesh, K, t, ids, kw, want = tiny_view(ctx)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    icp = dict(max_iteration=6, relative_fitness=-1, relative_rmse=-1)
    one = _lib.icp(ctx, src, tgt, 10.0, f.icp_init(), want_corr=True, **icp)
    d_t, d_ids, d_depth = torch.from_numpy(t).cuda(), torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(kw["depth"]).cuda()
    torch.cuda.synchronize()
    lib = _lib.load()
    cam = _lib.Pinhole(K[0, 0], K[1, 1], K[0, 2], K[1, 2], f.width, f.height)
    prm = _lib.CoverageView(kw["depth_scale"], kw["depth_tol"], kw["min_cos"], 0.001)
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    _lib.icp_begin(ctx, src, tgt, 10.0, f.icp_init(), **icp)
    try:
        assert lib.pedp_coverage_add(cov._h, mesh._h, C.byref(cam), vp(d_t), vp(d_ids), vp(d_depth), None, C.byref(prm), _lib.DEVICE,
                                     None) == 0
        n, totals, classes = C.c_int64(), _lib.CoverageTotals(), (C.c_int64 * 7)()
        assert lib.pedp_coverage_add(cov._h, mesh._h, C.byref(cam), _lib._ptr(t), _lib._ptr(ids), _lib._ptr(kw["depth"]), None,
                                     C.byref(prm), _lib.HOST, None) == -1
        assert lib.pedp_coverage_regions(cov._h, None, 0, 0, _lib.HOST, None, 0, None, C.byref(n)) == -1
        assert lib.pedp_coverage_summary(cov._h, None, C.byref(totals)) == -1
        assert lib.pedp_coverage_stats(cov._h, C.byref(n), classes) == -1
        assert lib.pedp_coverage_stats(cov._h, C.byref(n), None) == 0 and n.value == 1
    finally:
        two = _lib.icp_end(ctx, want_corr=True)
    assert np.array_equal(one["T"], two["T"]) and np.array_equal(one["corr"], two["corr"])
    assert one["fitness"] == two["fitness"] and one["inlier_rmse"] == two["inlier_rmse"]
    same_faces(cov.faces(), want.faces())
    assert cov.stats() == want.stats() and want.stats()["views"] == 1 and want.stats()["occluded"] > 0
    cov.close()
    cov.defect_map.close()


def test_a_context_with_a_history_gives_the_same_bits(ctx):
    from pedp_hip import _lib

    f, cov, mesh, K, t, ids, kw, want = tiny_view(ctx)
    cov.add_cast(mesh, K, t, ids, **kw)
    fresh, fresh_regions, fresh_summary = cov.faces(), cov.regions(grow=1), cov.summary()
    same_faces(fresh, want.faces())
    used = _lib.Context(0)
    umesh = _lib.Mesh(used, f.verts_posed, f.tris)
    scene = f.scene(umesh.cast_rays(f.rays6, want_uv=False)["t_hit"])                      # a cast
    _lib.icp(used, _lib.Cloud(used, scene), _lib.Cloud(used, f.model_points, f.normals), 10.0, f.icp_init(), max_iteration=6,
             relative_fitness=-1, relative_rmse=-1)                                         # a registration
    umesh.closest_points(scene[:500])                                                       # a closest-point query
    _, ucov, umesh2, _, _, _, _, _ = tiny_view(used)
    ucov.add_cast(umesh2, K, t, ids, **kw)
    same_faces(ucov.faces(), fresh)
    same_table_bits(ucov.regions(grow=1), fresh_regions)
    assert ucov.summary() == fresh_summary
    for h in (ucov, ucov.defect_map, umesh, umesh2, cov, cov.defect_map, mesh):
        h.close()
    used.close()
