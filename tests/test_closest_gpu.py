"""GPU tests of pedp_closest_points and the functions over it: every output bit for bit against the numpy restatement
(tests/_closest_ref.py), in every mode (exhaustive and both culled kernels), at the cluster and super-cluster boundaries."""
import ctypes as C

import numpy as np
import pytest

import _closest_ref as ref

pytestmark = pytest.mark.gpu

# triangle counts around one cluster (16), one super-cluster (1024) and the parity torus; the batch size that goes with each
F_CASES = {1: 3072, 15: 257, 16: 65, 17: 64, 1023: 63, 1024: 129, 1025: 3072, 4000: 257}
N_CASES = (1, 63, 64, 65, 257, 3072)


def torus(W, H):
    from pedp_hip import synth

    v, t, _ = synth.bumpy_torus(W, H)
    return v, t


def soup(F, seed):
    """F random triangles of 1 .. 12 mm in a 100 mm box, the second one degenerate (a repeated vertex)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-50.0, 50.0, (F, 1, 3))
    verts = (centre + rng.normal(0.0, rng.uniform(1.0, 12.0, (F, 1, 1)), (F, 3, 3))).reshape(-1, 3).astype(np.float32)
    if F > 2:
        verts[5] = verts[4]
    return verts, np.arange(3 * F, dtype=np.uint32).reshape(F, 3)


def queries(verts, tris, n, seed):
    """n points in turn on vertices, on edge midpoints, at centroids, 0.5 off and 200 off the faces, and scattered."""
    rng = np.random.default_rng(seed)
    v = verts.astype(np.float64)
    f = rng.integers(0, len(tris), n)
    a, b, c = v[tris[f, 0]], v[tris[f, 1]], v[tris[f, 2]]
    nrm = np.cross(b - a, c - a)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    cen = (a + b + c) / 3.0
    sign = rng.choice([-1.0, 1.0], (n, 1))
    kinds = [a, c, 0.5 * (a + b), 0.5 * (b + c), cen, cen + 0.5 * sign * nrm, cen + 200.0 * sign * nrm,
             rng.uniform(-120.0, 120.0, (n, 3))]
    pick = np.arange(n) % len(kinds)
    return np.ascontiguousarray(np.stack(kinds)[pick, np.arange(n)])


@pytest.fixture
def modes(ctx):
    """Runs a query in every mode -- 0 culled (the kernel chosen by N), 1 exhaustive, 2 and 3 culled with the
    lane-per-point and the wave-per-point kernel -- and leaves the context in the default one.  Returns [(outputs, pairs)]."""
    from pedp_hip import _lib

    def run(mesh, pts, want=ref.KEYS):
        out = []
        for mode in (0, 1, 2, 3):
            _lib.closest_configure(ctx, mode)
            out.append((mesh.closest_points(pts, want), _lib.closest_last_stats(ctx)))
        _lib.closest_configure(ctx, 0)
        return out

    yield run
    _lib.closest_configure(ctx, 0)


def check_both(modes, mesh, verts, tris, pts):
    want = ref.closest_ref(verts, tris, pts)
    runs = modes(mesh, pts)
    for name, (out, _) in zip(("culled", "exhaustive", "culled, a lane per point", "culled, a wave per point"), runs):
        assert ref.same_bits(out, want) is None, f"{name}: {ref.same_bits(out, want)}"
    finite = int(np.isfinite(pts).all(axis=1).sum())
    pairs_e = runs[1][1]
    assert pairs_e == finite * want["unskipped"]
    pairs_c = max(runs[k][1] for k in (0, 2, 3))
    assert pairs_c <= pairs_e
    return want, pairs_c, pairs_e


@pytest.mark.parametrize("F", sorted(F_CASES))
@pytest.mark.parametrize("kind", ["torus", "soup"])
def test_every_output_matches_the_restatement(ctx, modes, F, kind):
    from pedp_hip import _lib

    if kind == "torus":
        verts, tris = torus(50, 40)
        tris = np.ascontiguousarray(tris[:F])
    else:
        verts, tris = soup(F, F)
    pts = queries(verts, tris, F_CASES[F], 100 + F)
    want, _, _ = check_both(modes, _lib.Mesh(ctx, verts, tris), verts, tris, pts)
    assert (want["primitive_ids"] != ref.NONE).all()


@pytest.mark.parametrize("N", N_CASES)
def test_batch_sizes(ctx, modes, N):
    from pedp_hip import _lib

    verts, tris = soup(1025, 3)
    check_both(modes, _lib.Mesh(ctx, verts, tris), verts, tris, queries(verts, tris, N, N))


@pytest.mark.parametrize("N", [16384, 16385])
def test_the_batch_size_at_which_the_culled_kernel_changes(ctx, modes, N):
    """Up to 16384 points the culled search runs a wave per point, above a lane per point (WAVE_POINTS_MAX)."""
    from pedp_hip import _lib

    verts, tris = soup(17, 4)
    check_both(modes, _lib.Mesh(ctx, verts, tris), verts, tris, queries(verts, tris, N, N))


def test_a_point_does_not_depend_on_its_batch(ctx, modes):
    from pedp_hip import _lib

    verts, tris = torus(50, 40)
    mesh = _lib.Mesh(ctx, verts, tris)
    pts = queries(verts, tris, 257, 11)
    full = mesh.closest_points(pts)
    for i in (0, 63, 64, 200, 256):
        alone = mesh.closest_points(pts[i:i + 1])
        assert ref.same_bits(alone, {k: full[k][i:i + 1] for k in ref.KEYS}) is None
    moved = mesh.closest_points(np.concatenate([pts[130:], pts[:130], pts[:70]]))          # other indices, other size
    again = {k: np.concatenate([moved[k][127:257], moved[k][:127]]) for k in ref.KEYS}
    assert ref.same_bits(again, full) is None
    assert ref.same_bits({k: moved[k][257:] for k in ref.KEYS}, {k: full[k][:70] for k in ref.KEYS}) is None


def test_cuda_tensor_on_a_side_stream_and_leading_shape():
    import torch
    from pedp_hip import _lib, surface_distance as sd

    verts, tris = torus(50, 40)
    pts = queries(verts, tris, 240, 12)
    side = torch.cuda.Stream()
    sctx = _lib.Context(0, stream=side.cuda_stream)
    mesh = _lib.Mesh(sctx, verts, tris)
    host = sd.closest_points(mesh, pts.reshape(4, 60, 3))
    assert host["points"].shape == (4, 60, 3) and host["sides"].shape == (4, 60) and host["primitive_uvs"].shape == (4, 60, 2)
    assert ref.same_bits({k: host[k].reshape((240,) + host[k].shape[2:]) for k in ref.KEYS}, ref.closest_ref(verts, tris, pts)) is None
    with torch.cuda.stream(side):
        t = torch.from_numpy(pts.reshape(4, 60, 3)).cuda()
        dev = sd.closest_points(mesh, t)
        dist = sd.compute_distance(mesh, t)
    side.synchronize()
    assert all(v.is_cuda for v in dev.values()) and dev["primitive_ids"].dtype == torch.uint32
    assert ref.same_bits({k: v.cpu().numpy() for k, v in dev.items()}, host) is None
    assert np.array_equal(dist.cpu().numpy(), host["distances"])
    # float32 points widen exactly; a CPU tensor comes back as CPU tensors
    p32 = pts.astype(np.float32)
    cpu = sd.closest_points(mesh, torch.from_numpy(p32))
    assert isinstance(cpu["distances"], torch.Tensor) and not cpu["distances"].is_cuda
    assert ref.same_bits({k: v.numpy() for k, v in cpu.items()}, ref.closest_ref(verts, tris, p32.astype(np.float64))) is None
    # a holder mesh is converted like from_legacy

    class Holder:
        vertices, triangles = verts.astype(np.float64), tris

    assert np.array_equal(sd.compute_distance(Holder(), pts), host["distances"].reshape(-1))
    mesh.close()
    sctx.close()


def test_posable_mesh_as_posed(ctx, modes):
    """pedp_mesh_set_pose casts the float64 posed vertices to float32 and builds the records from them, as a plain mesh
    does from posed_vertices cast to float32: the same records, so the same bits."""
    from pedp_hip import _lib, synth

    verts, tris = torus(50, 40)
    T = synth.gt_pose()
    posable = _lib.Mesh(ctx, verts.astype(np.float64), tris, posable=True)
    posed32 = posable.posed_vertices(T).astype(np.float32)
    pts = queries(posed32, tris, 257, 13)
    before = posable.closest_points(pts)
    posable.set_pose(T)
    plain = _lib.Mesh(ctx, posed32, tris)
    want, _, _ = check_both(modes, posable, posed32, tris, pts)
    assert ref.same_bits(plain.closest_points(pts), want) is None
    assert not np.array_equal(before["distances"], want["distances"])
    posable.set_pose(None)                                                      # the handle's history does not matter
    assert ref.same_bits(posable.closest_points(pts), before) is None


def test_a_permuted_triangle_order_keeps_the_distances(ctx, modes):
    from pedp_hip import _lib

    verts, tris = torus(50, 40)
    pts = queries(verts, tris, 257, 14)
    shuffled = np.ascontiguousarray(tris[np.random.default_rng(5).permutation(len(tris))])
    want = ref.closest_ref(verts, tris, pts)["distances"]
    for (out, _) in modes(_lib.Mesh(ctx, verts, shuffled), pts, ("distances",)):
        assert np.array_equal(out["distances"], want)


def test_non_finite_points_no_triangles_and_no_points(ctx, modes):
    from pedp_hip import _lib

    verts, tris = soup(40, 6)
    mesh = _lib.Mesh(ctx, verts, tris)
    pts = queries(verts, tris, 130, 15)
    pts[[0, 64, 129], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    want, _, _ = check_both(modes, mesh, verts, tris, pts)
    assert np.isnan(want["distances"][[0, 64, 129]]).all() and (want["primitive_ids"][[0, 64, 129]] == ref.NONE).all()
    flat = np.zeros((30, 3), np.float32)
    flat[:, 0] = np.arange(30)                                                  # every triangle collinear
    ftris = np.arange(30, dtype=np.uint32).reshape(10, 3)
    want, pairs_c, pairs_e = check_both(modes, _lib.Mesh(ctx, flat, ftris), flat, ftris, pts[:70])
    assert pairs_c == 0 and pairs_e == 0 and np.isinf(want["distances"][1]) and (want["primitive_ids"] == ref.NONE).all()
    empty = mesh.closest_points(np.zeros((0, 3)))
    assert empty["points"].shape == (0, 3) and empty["sides"].shape == (0,)
    with pytest.raises(_lib.PedpError, match="unknown output"):
        mesh.closest_points(pts, want=("points", "normals"))
    rc = _lib.load().pedp_closest_points(ctx._h, mesh._h, None, (1 << 24) + 1, _lib.HOST, None, None, None, None, None)
    assert rc == -1 and b"at most" in _lib.load().pedp_last_error()           # PEDP_ERR_BAD_ARG


def test_device_call_while_a_registration_is_pending(ctx):
    """The contract: a PEDP_DEVICE call has a workspace of its own and leaves a pending registration's result unchanged;
    the PEDP_HOST form and pedp_closest_last_stats, which wait on the stream, are refused."""
    import torch
    from pedp_hip import _lib, synth

    f = synth.Frame("tiny")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    kw = dict(max_iteration=6, relative_fitness=-1, relative_rmse=-1)
    one = _lib.icp(ctx, src, tgt, 10.0, f.icp_init(), want_corr=True, **kw)
    pts = queries(f.verts_posed, f.tris, 257, 16)
    want = mesh.closest_points(pts)
    d_pts = torch.from_numpy(pts).cuda()
    d_out = torch.empty(257, 3, dtype=torch.float64, device="cuda")
    d_dist = torch.empty(257, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.icp_begin(ctx, src, tgt, 10.0, f.icp_init(), **kw)
    try:
        mesh.closest_points_device(d_pts.data_ptr(), 257, d_out.data_ptr(), d_dist.data_ptr())
        lib = _lib.load()
        host = np.empty(257)
        n = C.c_int64()
        assert lib.pedp_closest_points(ctx._h, mesh._h, _lib._ptr(pts), 257, _lib.HOST, None, _lib._ptr(host), None, None, None) == -1
        assert lib.pedp_closest_last_stats(ctx._h, C.byref(n)) == -1
    finally:
        two = _lib.icp_end(ctx, want_corr=True)
    assert np.array_equal(one["T"], two["T"]) and np.array_equal(one["corr"], two["corr"])
    assert one["fitness"] == two["fitness"] and one["inlier_rmse"] == two["inlier_rmse"]
    ctx.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want["points"]) and np.array_equal(d_dist.cpu().numpy(), want["distances"])


def test_the_cull_does_something(ctx, modes):
    """48 runs of 64 neighbouring points near the 16,000-triangle torus: the culled search evaluates at most a quarter of
    the N F pairs (a static bound from the spheres alone with a per-wave union of candidates gives 0.042 of them on this
    input), and returns the exhaustive search's bits."""
    from pedp_hip import _lib

    verts, tris = torus(100, 80)
    assert len(tris) == 16000
    pts = ref.coherent_queries()
    assert pts.shape == (3072, 3)
    (auto, pairs_a), (exh, pairs_e), (lanes, pairs_l), (waves, pairs_w) = modes(_lib.Mesh(ctx, verts, tris), pts)
    print(f"pairs tested of {3072 * 16000}: a lane per point {pairs_l}, a wave per point {pairs_w}, by N {pairs_a}")
    for culled in (auto, lanes, waves):
        assert ref.same_bits(culled, exh) is None
    assert ref.same_bits({k: exh[k][:256] for k in ref.KEYS}, ref.closest_ref(verts, tris, pts[:256])) is None
    assert pairs_e == 3072 * 16000
    assert (exh["distances"] < 3.0).all()
    assert max(pairs_a, pairs_l, pairs_w) <= 3072 * 16000 // 4


def test_align_to_mesh_and_deviation_heatmap_on_a_dented_frame(ctx):
    """A 64 x 48 depth frame of the posed parity torus with a dent pressed in: at chosen pixels (hit well inside a
    triangle that faces the camera) the measured point is moved along its ray until it lies `dent` behind the triangle's
    plane, where the triangle is still the closest one.  The heat there is min(dent / saturation, 1) to the float32
    resolution of the depth: 4 ulp of the largest depth, in the mesh's units, over the saturation."""
    from pedp_hip import _lib, surface_distance as sd, synth

    f = synth.Frame("parity")
    W, H, foc = 64, 48, 90.0
    K = np.array([[foc, 0.0, 31.5], [0.0, foc, 23.5], [0.0, 0.0, 1.0]])
    dirs = synth.pixel_rays(W, H, foc, 31.5, 23.5)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    hit = mesh.cast_rays(synth.rays6_from_dirs(dirs))
    ok = np.isfinite(hit["t_hit"])
    assert 300 < ok.sum() < W * H - 300
    v = f.verts_posed.astype(np.float64)
    tri = f.tris[np.where(ok, hit["primitive_ids"], 0)]
    nrm = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cosine = np.abs((dirs * nrm).sum(axis=1))
    uv = hit["primitive_uvs"]
    inner = ok & (uv[:, 0] > 0.15) & (uv[:, 1] > 0.15) & (uv[:, 0] + uv[:, 1] < 0.85) & (cosine > 0.7)
    dented = np.nonzero(inner)[0]
    far = np.nonzero(ok & ~inner & (cosine > 0.5))[0][::7]
    assert len(dented) >= 10 and len(far) >= 10
    dent, saturation, gate = 0.5, 1.0, 5.0
    # the hit distance again in float64 (the caster's float32 t is a few ulp off): (a - o) . n / (d . n) with o = 0
    along = np.where(ok, (v[tri[:, 0]] * nrm).sum(axis=1) / (dirs * nrm).sum(axis=1), 0.0)
    assert np.abs(along[ok] - hit["t_hit"][ok]).max() < 1e-2
    along[dented] += dent / cosine[dented]
    along[far] -= 20.0                                    # in front of the surface, beyond the gate (6.5 at the least)
    depth = (along * dirs[:, 2] / 1000.0).astype(np.float32).reshape(H, W)
    heat = sd.deviation_heatmap(depth, K, mesh, saturation, gate)
    assert heat.shape == (H, W) and heat.dtype == np.float64
    tol = 4 * 2.0 ** -24 * float(depth.max()) * 1000.0 / saturation
    flat = heat.reshape(-1)
    assert np.abs(flat[dented] - min(dent / saturation, 1.0)).max() <= tol
    assert (flat[~ok] == 0.0).all() and (flat[far] == 0.0).all()
    rest = ok.copy()
    rest[dented] = rest[far] = False
    assert flat[rest].max() <= tol                                              # measured points on the surface itself
    masked = sd.deviation_heatmap(depth, K, mesh, saturation, gate, mask=np.arange(H * W).reshape(H, W) % 2 == 0)
    assert (masked.reshape(-1)[1::2] == 0.0).all() and np.array_equal(masked.reshape(-1)[::2], flat[::2])
    proj = mesh.project_heatmap(heat, K, threshold=0.1)
    assert proj["n_rays"] == len(dented) and 0 < len(proj["points"]) <= len(dented)
    # the same points through align_to_mesh: onto the triangle's plane, then lifted back to the side they are on
    q = dirs[dented] * along[dented, None]
    lifted, aligned = sd.align_to_mesh(np.hstack([q, np.ones((len(q), 1))]), mesh, offset=0.1)
    a = v[tri[dented, 0]]
    # the record's triangle is a, a + fl32(b - a), a + fl32(c - a): within half a float32 ulp of an edge component per
    # vertex of the plane through a, b, c that `nrm` and `dent` were formed with; 4 ulp of the longest edge component
    edge = max(np.abs(v[f.tris[:, k]] - v[f.tris[:, 0]]).max() for k in (1, 2))
    plane_tol = 4 * 2.0 ** -24 * edge
    assert np.abs(((aligned - a) * nrm[dented]).sum(axis=1)).max() <= plane_tol
    assert np.abs(np.linalg.norm(q - aligned, axis=1) - dent).max() <= plane_tol
    assert np.abs(np.linalg.norm(lifted - aligned, axis=1) - 0.1).max() < 1e-12
    assert (((lifted - aligned) * (q - aligned)).sum(axis=1) > 0).all()
