"""GPU tests of pedp_solid_create / pedp_signed_distance and the functions over them: the sign against
the generalised winding number, |sdist| against compute_distance bit for bit, the feature and the pseudonormal against
the numpy restatement (tests/_signed_ref.py), independence of batch, kernel and history, poses, orientation, broken
meshes, edge inputs and a frame with a dent and a bump."""
import numpy as np
import pytest

import _closest_ref as cref
import _signed_ref as sref

pytestmark = pytest.mark.gpu

KEYS = ("signed_distances", "occupancy", "features", "normals")
# |normal - restatement's|: a fan has at most 64 corners here; each term n angle is a few ulp off (the device's atan2 and
# sqrt against numpy's), the sum of at most 64 of them of length <= pi and the normalisation a few ulp more: about
# 64 * 8 * 2^-53 * pi ~ 2e-13, times 10
NORMAL_TOL = 1e-12


def handles(ctx, verts32, tris, model=None):
    from pedp_hip import _lib

    return _lib.Mesh(ctx, verts32, tris), _lib.Solid(ctx, verts32.astype(np.float64) if model is None else model, tris)


def same_bits(got, want, keys=KEYS):
    return cref.same_bits(got, want, keys)


@pytest.mark.parametrize("name", sorted(sref.MESHES))
def test_signs_features_and_normals_on_every_fixture(ctx, name):
    from pedp_hip import surface_distance as sd

    v32, tris, pts, ref, wn = sref.reference(name)
    mesh, solid = handles(ctx, v32, tris)
    info = solid.info
    assert info["closed"] == 1 and info["orientation"] == 1 and info["F"] == len(tris) and info["edges"] * 2 == 3 * len(tris)
    out = solid.signed_distance(mesh, pts)
    inside = wn > 0.5
    assert np.array_equal(out["occupancy"].astype(bool), inside) and np.array_equal(out["signed_distances"] < 0, inside)
    dist = sd.compute_distance(mesh, pts)
    assert np.array_equal(np.abs(out["signed_distances"]).view(np.uint64), dist.view(np.uint64))
    clear = sref.decided(v32, tris, pts)
    print(f"{name}: {int(inside.sum())} inside, {int((~clear).sum())} ties between two triangles, "
          f"normals within {np.abs(out['normals'] - ref['normals']).max():.3g} of the restatement's")
    assert np.array_equal(out["features"][clear], ref["features"][clear])
    assert np.abs(out["normals"] - ref["normals"]).max() <= NORMAL_TOL
    assert np.array_equal(out["signed_distances"], ref["signed_distances"])
    # the wrappers: the same bits from a holder (the solid built for the call), as one dict with closest_points' entries

    class Holder:
        vertices, triangles = v32.astype(np.float64), tris

    assert np.array_equal(sd.compute_signed_distance(Holder(), pts[:300], ctx=ctx), out["signed_distances"][:300])
    assert np.array_equal(sd.compute_occupancy(mesh, pts[:300], solid), out["occupancy"][:300])
    both = sd.signed_closest_points(mesh, pts[:300], solid)
    assert same_bits(both, {k: out[k][:300] for k in KEYS}) is None
    assert cref.same_bits(both, {k: ref[k][:300] for k in cref.KEYS}) is None
    with pytest.raises(Exception, match="pass solid"):
        sd.compute_signed_distance(mesh, pts[:3])


def test_points_exactly_on_a_face_plane_beyond_a_sharp_edge(ctx):
    """The wedge's first two faces lie in y = 0 exactly.  Points with y = 0 beyond the 20 degree edge (x < 0) and beyond the
    right-angled edge (x > L) are outside, at the distance of the edge.  Two faces tie there to within rounding: where a
    face in y = 0 wins, (p - c) . n is exactly 0 and `sides` says nothing; the edge's pseudonormal decides either way."""
    v32, tris, _ = sref.fixture("wedge")
    mesh, solid = handles(ctx, v32, tris)
    rng = np.random.default_rng(3)
    x = np.concatenate([-rng.uniform(0.01, 0.5, 40), sref.WEDGE_LENGTH + rng.uniform(0.01, 0.5, 40)])
    pts = np.column_stack([x, np.zeros(80), rng.uniform(0.05, 0.95, 80)])
    out = solid.signed_distance(mesh, pts)
    cl = mesh.closest_points(pts)
    gap = np.where(x < 0, -x, x - sref.WEDGE_LENGTH)
    in_plane = cl["primitive_ids"] < 2
    print(f"a face in y = 0 wins on {int(in_plane.sum())} of 80 points; sides there: {np.unique(cl['sides'][in_plane])}")
    assert (cl["sides"][in_plane] == 0).all()
    assert (out["features"] == sref.EDGE).all() and (out["occupancy"] == 0).all() and (out["signed_distances"] > 0).all()
    assert np.abs(out["signed_distances"] - gap).max() <= 1e-12
    inner = np.column_stack([rng.uniform(0.5, 1.9, 40), np.full(40, 1e-3), rng.uniform(0.05, 0.95, 40)])   # just above y = 0
    res = solid.signed_distance(mesh, inner)
    assert (res["occupancy"] == 1).all() and np.abs(res["signed_distances"] + 1e-3).max() <= 1e-12


def test_batch_sizes_kernels_and_repeated_calls_give_the_same_bits(ctx):
    from pedp_hip import _lib

    v32, tris, pts, ref, _ = sref.reference("torus_24x22")
    rng = np.random.default_rng(11)
    big = np.ascontiguousarray(np.concatenate([pts, rng.uniform(pts.min(axis=0), pts.max(axis=0), (16385 - len(pts), 3))]))
    mesh, solid = handles(ctx, v32, tris)
    full = solid.signed_distance(mesh, big)                                     # 16385: a lane per point
    assert np.array_equal(full["signed_distances"][:len(pts)], ref["signed_distances"])
    assert np.array_equal(full["occupancy"][:len(pts)], ref["occupancy"])
    for n in (1, 63, 64, 65, 16384):                                            # a wave per point
        part = solid.signed_distance(mesh, big[:n])
        assert same_bits(part, {k: full[k][:n] for k in KEYS}) is None, n
    tail = solid.signed_distance(mesh, big[-65:])                               # other indices, other neighbours
    assert same_bits(tail, {k: full[k][-65:] for k in KEYS}) is None
    try:
        for mode in (1, 2, 3):
            _lib.closest_configure(ctx, mode)
            assert same_bits(solid.signed_distance(mesh, big[:3000]), {k: full[k][:3000] for k in KEYS}) is None, mode
    finally:
        _lib.closest_configure(ctx, 0)
    assert same_bits(solid.signed_distance(mesh, big), full) is None            # twice in a row


def test_posable_mesh_after_set_pose(ctx):
    from pedp_hip import _lib, synth

    v32, tris, pts, ref, wn = sref.reference("l_prism")
    model = v32.astype(np.float64)
    T = synth.gt_pose()
    T[:3, 3] = [0.3, -1.2, 4.0]
    posable = _lib.Mesh(ctx, model, tris, posable=True)
    solid = _lib.Solid(ctx, model, tris)
    far = ref["distances"] >= 1e-3
    assert far.sum() > 3900
    unposed = solid.signed_distance(posable, pts)
    assert np.array_equal(unposed["occupancy"].astype(bool), wn > 0.5)
    posable.set_pose(T)
    moved = pts @ T[:3, :3].T + T[:3, 3]
    back = (moved - T[:3, 3]) @ T[:3, :3]                                       # the inverse-transformed points
    posed = solid.signed_distance(posable, moved)
    posable.set_pose(None)
    again = solid.signed_distance(posable, back)
    assert np.array_equal(posed["occupancy"][far], again["occupancy"][far])
    assert np.array_equal(posed["occupancy"][far].astype(bool), (wn > 0.5)[far])
    assert np.abs(np.abs(posed["signed_distances"]) - ref["distances"]).max() < 1e-5
    # the posed pseudonormals are the rotated ones
    assert np.abs(posed["normals"][far] - unposed["normals"][far] @ T[:3, :3].T).max() < 1e-5
    # a posable mesh keeps its indices: a solid of the same size built from other triangles is refused
    other = _lib.Solid(ctx, model, np.ascontiguousarray(tris[::-1]))
    assert other.info["closed"] == 1
    with pytest.raises(_lib.PedpError, match="not the ones the solid was built from"):
        other.signed_distance(posable, pts[:5])


def test_reversed_and_unshared_cubes(ctx):
    from pedp_hip import _lib

    v32, tris, pts, ref, wn = sref.reference("cube")
    mesh, solid = handles(ctx, v32, tris)
    out = solid.signed_distance(mesh, pts)
    rev = np.ascontiguousarray(tris[:, ::-1])
    rmesh, rsolid = handles(ctx, v32, rev)
    assert rsolid.info["orientation"] == -1 and rsolid.info["volume"] < 0 and rsolid.info["closed"] == 1
    assert abs(solid.info["volume"] - 1.0) < 1e-12 and abs(rsolid.info["volume"] + 1.0) < 1e-12
    rout = rsolid.signed_distance(rmesh, pts)
    assert np.array_equal(rout["signed_distances"], out["signed_distances"]) and np.array_equal(rout["occupancy"], out["occupancy"])
    assert np.abs(rout["normals"] - out["normals"]).max() <= NORMAL_TOL           # outward either way
    sv, st, _ = sref.fixture("stl_cube")
    smesh, ssolid = handles(ctx, sv, st)
    assert ssolid.info["V"] == 36 and ssolid.info["welded_vertices"] == 8 and ssolid.info["edges"] == 18 and ssolid.info["closed"] == 1
    sout = ssolid.signed_distance(smesh, pts)
    assert np.array_equal(sout["signed_distances"], out["signed_distances"]) and np.array_equal(sout["occupancy"], out["occupancy"])
    assert np.array_equal(sout["occupancy"].astype(bool), wn > 0.5)


def test_open_and_broken_meshes(ctx):
    from pedp_hip import _lib

    v32, tris, pts = sref.fixture("cube")
    model = v32.astype(np.float64)
    mesh, solid = handles(ctx, v32, np.ascontiguousarray(tris[:-1]))
    assert solid.info["boundary_edges"] == 3 and solid.info["closed"] == 0 and solid.info["nonmanifold_edges"] == 0
    with pytest.raises(_lib.PedpError, match="bounds no solid"):
        solid.signed_distance(mesh, pts[:10])
    flipped = tris.copy()
    flipped[5] = flipped[5][::-1]
    info = _lib.Solid(ctx, model, flipped).info
    assert info["flipped_edges"] == 3 and info["boundary_edges"] == 0 and info["closed"] == 0
    fin = np.concatenate([tris, [[tris[0, 0], tris[0, 1], 8]]]).astype(np.uint32)
    info = _lib.Solid(ctx, np.concatenate([model, [[0.5, -1.0, 0.5]]]), fin).info
    assert info["nonmanifold_edges"] == 1 and info["boundary_edges"] == 2 and info["closed"] == 0 and info["edges"] == 20
    want = sref.topology(np.concatenate([model, [[0.5, -1.0, 0.5]]]), fin)
    assert all(info[k] == want[k] for k in ("welded_vertices", "edges", "boundary_edges", "nonmanifold_edges", "flipped_edges",
                                            "degenerate_faces", "closed", "orientation"))
    # a solid of another F, and one of another context
    full_mesh, full_solid = handles(ctx, v32, tris)
    with pytest.raises(_lib.PedpError, match="12 faces, the mesh 11"):
        full_solid.signed_distance(mesh, pts[:10])
    other = _lib.Context(0)
    try:
        foreign = _lib.Solid(other, model, tris)
        out = np.empty(10)
        rc = _lib.load().pedp_signed_distance(ctx._h, full_mesh._h, foreign._h, _lib._ptr(pts), 10, _lib.HOST, _lib._ptr(out), None, None,
                                              None)
        assert rc == -1 and b"another context" in _lib.load().pedp_last_error()
        foreign.close()
    finally:
        other.close()


def test_non_finite_points_no_points_and_no_faces(ctx):
    from pedp_hip import _lib

    v32, tris, pts, ref, _ = sref.reference("tetrahedron")
    mesh, solid = handles(ctx, v32, tris)
    p = pts[:130].copy()
    p[[0, 64, 129], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    out = solid.signed_distance(mesh, p)
    bad = np.zeros(130, bool)
    bad[[0, 64, 129]] = True
    assert np.isnan(out["signed_distances"][bad]).all() and (out["occupancy"][bad] == 0).all() and (out["features"][bad] == 255).all()
    assert np.isnan(out["normals"][bad]).all()
    assert same_bits({k: out[k][~bad] for k in KEYS}, {k: solid.signed_distance(mesh, pts[:130])[k][~bad] for k in KEYS}) is None
    empty = solid.signed_distance(mesh, np.zeros((0, 3)))
    assert empty["signed_distances"].shape == (0,) and empty["normals"].shape == (0, 3)
    only = solid.signed_distance(mesh, p, want=("occupancy",))
    assert list(only) == ["occupancy"] and np.array_equal(only["occupancy"], out["occupancy"])
    rc = _lib.load().pedp_signed_distance(ctx._h, mesh._h, solid._h, None, (1 << 24) + 1, _lib.HOST, None, None, None, None)
    assert rc == -1 and b"at most" in _lib.load().pedp_last_error()
    nv, nt = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
    nmesh, nsolid = handles(ctx, nv, nt)
    assert nsolid.info["F"] == 0 and nsolid.info["closed"] == 0 and nsolid.info["orientation"] == 0
    none = nsolid.signed_distance(nmesh, p)
    assert np.isposinf(none["signed_distances"][~bad]).all() and np.isnan(none["signed_distances"][bad]).all()
    assert (none["occupancy"] == 0).all() and (none["features"] == 255).all() and np.isnan(none["normals"]).all()


def test_a_call_while_a_registration_is_pending_is_refused(ctx):
    """The workspace of a signed query is sized by V and N, so the call may have to wait for the device: refused in
    either memory while a registration owns the stream, and the registration's result is what it would have been."""
    import torch
    from pedp_hip import _lib, surface_distance as sd, synth

    f = synth.Frame("tiny")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    solid = _lib.Solid(ctx, f.verts_posed.astype(np.float64), f.tris)
    assert solid.info["closed"] == 1
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    kw = dict(max_iteration=6, relative_fitness=-1, relative_rmse=-1)
    one = _lib.icp(ctx, src, tgt, 10.0, f.icp_init(), want_corr=True, **kw)
    pts = np.ascontiguousarray(scene[:257])
    want = solid.signed_distance(mesh, pts)
    d_pts = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    _lib.icp_begin(ctx, src, tgt, 10.0, f.icp_init(), **kw)
    try:
        with pytest.raises(_lib.PedpError, match="a registration is pending"):
            sd.compute_signed_distance(mesh, d_pts, solid)
        with pytest.raises(_lib.PedpError, match="a registration is pending"):
            solid.signed_distance(mesh, pts)
        with pytest.raises(_lib.PedpError, match="a registration is pending"):
            _lib.Solid(ctx, f.verts_posed.astype(np.float64), f.tris)
    finally:
        two = _lib.icp_end(ctx, want_corr=True)
    assert np.array_equal(one["T"], two["T"]) and np.array_equal(one["corr"], two["corr"])
    assert same_bits(solid.signed_distance(mesh, pts), want) is None


def test_cuda_tensor_on_a_side_stream_and_leading_shape():
    import torch
    from pedp_hip import _lib, surface_distance as sd

    v32, tris, pts, ref, _ = sref.reference("torus_12x8")
    side = torch.cuda.Stream()
    sctx = _lib.Context(0, stream=side.cuda_stream)
    mesh, solid = handles(sctx, v32, tris)
    host = solid.signed_distance(mesh, pts[:15])
    with torch.cuda.stream(side):
        t = torch.from_numpy(pts[:15].reshape(3, 5, 3)).cuda()
        dev = sd.signed_closest_points(mesh, t, solid)
        occ = sd.compute_occupancy(mesh, t, solid)
        sdist = sd.compute_signed_distance(mesh, t.float(), solid)
    side.synchronize()
    assert all(v.is_cuda for v in dev.values()) and dev["normals"].shape == (3, 5, 3) and dev["points"].shape == (3, 5, 3)
    assert dev["occupancy"].dtype == torch.int8 and dev["features"].dtype == torch.uint8 and dev["signed_distances"].shape == (3, 5)
    assert same_bits({k: dev[k].cpu().numpy().reshape((15,) + host[k].shape[1:]) for k in KEYS}, host) is None
    assert np.array_equal(occ.cpu().numpy().reshape(-1), host["occupancy"])
    assert np.array_equal(sdist.cpu().numpy().reshape(-1) < 0, host["occupancy"].astype(bool))
    cpu = sd.compute_signed_distance(mesh, torch.from_numpy(pts[:15]), solid)
    assert isinstance(cpu, torch.Tensor) and not cpu.is_cuda and np.array_equal(cpu.numpy(), host["signed_distances"])
    solid.close()
    mesh.close()
    sctx.close()


def test_signed_deviation_on_a_frame_with_a_dent_and_a_bump(ctx):
    """test_closest_gpu.py's dented frame with two patches: at every other chosen pixel (hit well inside a triangle that
    faces the camera) the measured point is moved along its ray until it lies `dent` BEHIND the triangle's plane, inside
    the solid; at the others until it lies `dent` in FRONT of it, outside.  Behind the plane the triangle is still the
    closest one, so the signed distance there is -dent to the float32 resolution of the depth; in front of it the point is
    at most `dent` from the surface."""
    from pedp_hip import _lib, surface_distance as sd, synth

    f = synth.Frame("parity")
    W, H, foc = 64, 48, 90.0
    K = np.array([[foc, 0.0, 31.5], [0.0, foc, 23.5], [0.0, 0.0, 1.0]])
    dirs = synth.pixel_rays(W, H, foc, 31.5, 23.5)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    solid = _lib.Solid(ctx, f.verts_posed.astype(np.float64), f.tris)
    assert solid.info["closed"] == 1 and solid.info["orientation"] != 0
    hit = mesh.cast_rays(synth.rays6_from_dirs(dirs))
    ok = np.isfinite(hit["t_hit"])
    v = f.verts_posed.astype(np.float64)
    tri = f.tris[np.where(ok, hit["primitive_ids"], 0)]
    nrm = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cosine = np.abs((dirs * nrm).sum(axis=1))
    uv = hit["primitive_uvs"]
    inner = np.nonzero(ok & (uv[:, 0] > 0.15) & (uv[:, 1] > 0.15) & (uv[:, 0] + uv[:, 1] < 0.85) & (cosine > 0.7))[0]
    dented, bumped = inner[::2], inner[1::2]
    assert len(dented) >= 5 and len(bumped) >= 5
    dent, saturation, gate = 0.5, 1.0, 5.0
    along = np.where(ok, (v[tri[:, 0]] * nrm).sum(axis=1) / (dirs * nrm).sum(axis=1), 0.0)
    along[dented] += dent / cosine[dented]
    along[bumped] -= dent / cosine[bumped]
    depth = (along * dirs[:, 2] / 1000.0).astype(np.float32).reshape(H, W)
    signed = sd.signed_deviation(depth, K, mesh, solid)
    assert signed.shape == (H, W) and signed.dtype == np.float64
    flat = signed.reshape(-1)
    tol = 4 * 2.0 ** -24 * float(depth.max()) * 1000.0
    print(f"dent {flat[dented].min():.6f} ... {flat[dented].max():.6f}, bump {flat[bumped].min():.6f} ... {flat[bumped].max():.6f}")
    assert np.isnan(flat[~ok]).all() and not np.isnan(flat[ok]).any()
    assert np.abs(flat[dented] + dent).max() <= tol
    assert (flat[bumped] > 0).all() and flat[bumped].max() <= dent + tol
    rest = ok.copy()
    rest[inner] = False
    assert np.abs(flat[rest]).max() <= tol                                      # measured points on the surface itself
    excess, missing = sd.split_deviation(signed, saturation, gate)
    assert (excess.reshape(-1)[bumped] > 0).all() and (missing.reshape(-1)[bumped] == 0).all()
    assert (missing.reshape(-1)[dented] > 0).all() and (excess.reshape(-1)[dented] == 0).all()
    assert np.abs(missing.reshape(-1)[dented] - dent / saturation).max() <= tol / saturation
    heat = sd.deviation_heatmap(depth, K, mesh, saturation, gate)
    both = ~np.isnan(signed)
    assert np.array_equal((excess + missing)[both].view(np.uint64), heat[both].view(np.uint64))
    assert ((excess + missing)[~both] == 0).all() and (heat[~both] == 0).all()
    masked = sd.signed_deviation(depth, K, mesh, solid, mask=np.arange(H * W).reshape(H, W) % 2 == 0)
    assert np.isnan(masked.reshape(-1)[1::2]).all() and np.array_equal(masked.reshape(-1)[::2], flat[::2], equal_nan=True)
    # each half is a heat map the projection takes: the bump's rays and the dent's rays, apart
    assert mesh.project_heatmap(excess, K, threshold=0.1)["n_rays"] == int((excess > 0.1).sum()) >= len(bumped) // 2
    assert mesh.project_heatmap(missing, K, threshold=0.1)["n_rays"] == len(dented)
