"""The renderer's contract on the CPU: the numpy restatement (tests/_render_ref.py) against analytic answers, the
projection / bbox2d composition against hand-built matrices, make_mesh_tensors on duck-typed meshes, and the dr shim's
refusals.  The GPU tests then hold the device code bit-equal to the same restatement."""
import types

import numpy as np
import pytest

import _render_ref as ref

f32 = np.float32


def _K(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], dtype=np.float64)


def _render(verts, faces, normals, K, H, W, T=None, **kw):
    from pedp_hip.render import projection_matrix_from_intrinsics

    proj = projection_matrix_from_intrinsics(K, H, W, 0.001, 100).astype(np.float32)
    T = np.eye(4, dtype=np.float32)[None] if T is None else np.asarray(T, np.float32).reshape(-1, 4, 4)
    kw.setdefault("vcolor", np.full((len(verts), 3), 0.5, np.float32))
    return ref.render(verts, faces, normals, T, proj, H, W, kw.pop("out_h", H), kw.pop("out_w", W), **kw)


def _backproject(u, v, z, K):
    return (u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1]


def test_fronto_parallel_quad_covers_its_pixel_rectangle():
    H, W, z0 = 24, 32, 0.75
    K = _K(40.0, 15.0, 11.0)
    c_lo, c_hi, r_lo, r_hi = 5, 21, 3, 17  # quad edges on integer pixel coordinates: pixel centres are 0.5 inside
    (x0, y0), (x1, y1) = _backproject(c_lo, r_lo, z0, K), _backproject(c_hi, r_hi, z0, K)
    verts = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    normals = np.tile(np.array([0, 0, -1], np.float32), (4, 1))
    color, depth, normal, xyz = _render(verts, faces, normals, K, H, W, get_normal=True)
    mask = depth[0] != 0
    want = np.zeros((H, W), bool)
    want[r_lo:r_hi, c_lo:c_hi] = True
    assert np.array_equal(mask, want)
    np.testing.assert_allclose(depth[0][want], z0, rtol=1e-6)
    rr, cc = np.nonzero(want)
    bx, by = _backproject(cc + 0.5, rr + 0.5, z0, K)
    np.testing.assert_allclose(xyz[0][want][:, 0], bx, atol=1e-5)
    np.testing.assert_allclose(xyz[0][want][:, 1], by, atol=1e-5)
    np.testing.assert_allclose(normal[0][want], np.tile([0, 0, -1], (want.sum(), 1)), atol=1e-6)
    assert not normal[0][~want].any() and not color[0][~want].any() and not xyz[0][~want].any()
    np.testing.assert_allclose(color[0][want], 0.5, rtol=1e-6)


def _grid_plane(n, H, W, z0, K, step=1.0, lo=4):
    """(n x n) vertices at pixel centres lo + 0.5 + i * step, both diagonal directions alternating."""
    g = lo + 0.5 + step * np.arange(n)
    uu, vv = np.meshgrid(g, g, indexing="xy")
    x, y = _backproject(uu, vv, z0, K)
    verts = np.stack([x, y, np.full_like(x, z0)], -1).reshape(-1, 3).astype(np.float32)
    faces = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, i * n + j + 1, (i + 1) * n + j + 1, (i + 1) * n + j
            faces += [[a, b, c], [a, c, d]] if (i + j) % 2 else [[a, b, d], [b, c, d]]
    return verts, np.array(faces, np.int32)


def test_plane_of_10k_triangles_is_watertight():
    H = W = 80
    K = _K(70.0, 40.0, 40.0)
    verts, faces = _grid_plane(72, H, W, 0.5, K)
    assert len(faces) >= 10000
    normals = np.tile(np.array([0, 0, -1], np.float32), (len(verts), 1))
    _, depth, _, _ = _render(verts, faces, normals, K, H, W)
    inner = depth[0][5:75, 5:75]  # pixel centres strictly inside the grid: every one lies on or in some triangle
    assert (inner != 0).all(), f"{int((inner == 0).sum())} uncovered pixels inside the plane"


def test_tilted_plane_has_no_holes():
    H = W = 64
    K = _K(60.0, 32.0, 32.0)
    verts, faces = _grid_plane(40, H, W, 0.6, K, step=1.3, lo=5)
    T = np.eye(4)
    a = 0.5
    T[:3, :3] = [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]
    T[:3, 3] = -T[:3, :3] @ np.array([0, 0, 0.6]) + np.array([0, 0, 0.6])  # tilt about the plane's centre line
    normals = np.tile(np.array([0, 0, -1], np.float32), (len(verts), 1))
    _, depth, _, _ = _render(verts, faces, normals, K, H, W, T=T)
    m = depth[0] != 0
    assert m.sum() > 500
    for line in list(m) + list(m.T):  # a convex region: covered pixels of every row and column are one run
        idx = np.nonzero(line)[0]
        if len(idx):
            assert idx[-1] - idx[0] + 1 == len(idx), "hole in the coverage"


def test_projection_and_bbox_composition():
    from pedp_hip.render import glcam_in_cvcam, projection_matrix_from_intrinsics

    K = np.array([[500.0, 0.3, 310.0], [0, 505.0, 245.0], [0, 0, 1]])
    H, W, n, f = 480, 640, 0.001, 100.0
    P = projection_matrix_from_intrinsics(K, H, W, n, f)
    hand = np.array([[2 * 500.0 / 640, -2 * 0.3 / 640, (640 - 2 * 310.0) / 640, 0],
                     [0, 2 * 505.0 / 480, (2 * 245.0 - 480) / 480, 0],
                     [0, 0, -(f + n) / (f - n), -2 * f * n / (f - n)],
                     [0, 0, -1, 0]])
    np.testing.assert_allclose(P, hand, rtol=1e-15, atol=1e-15)
    assert np.array_equal(glcam_in_cvcam, np.diag([1.0, -1.0, -1.0, 1.0]))
    rng = np.random.default_rng(3)
    T = np.eye(4)
    T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    T[:3, 3] = [0.02, -0.01, 0.4]
    bbox = np.array([[200.0, 150.0, 360.0, 310.0]])
    M, win = ref.pose_records(P.astype(np.float32), T.astype(np.float32), bbox, H, W)
    np.testing.assert_allclose(M[0], P @ glcam_in_cvcam @ T, rtol=1e-6, atol=1e-6)
    l, t, r, b = 200.0, H - 150.0, 360.0, H - 310.0
    tf = np.eye(4)
    tf[0, 0], tf[1, 1] = W / (r - l), H / (t - b)
    tf[3, 0], tf[3, 1] = (W - r - l) / (r - l), (H - t - b) / (t - b)
    p = rng.normal(size=(50, 3)) * 0.05
    clip = ref.clip_vertices(p.astype(np.float32), M[0], win[0])
    want = (np.c_[p, np.ones(50)] @ (P @ glcam_in_cvcam @ T).T) @ tf  # the row-vector post-multiply
    np.testing.assert_allclose(clip, want, rtol=1e-5, atol=1e-5)
    # the window maps the crop's corners to the NDC corners
    ndc_l = (W / (r - l)) * (2 * l / W - 1) + (W - r - l) / (r - l)
    ndc_r = (W / (r - l)) * (2 * r / W - 1) + (W - r - l) / (r - l)
    assert abs(ndc_l + 1) < 1e-12 and abs(ndc_r - 1) < 1e-12


def test_restatement_composes_like_the_reference():
    """The fused restatement equals rasterize -> interpolate -> flip over the same clip vertices."""
    H, W = 20, 28
    K = _K(30.0, 13.5, 9.5)
    from pedp_hip import synth

    v, t, nrm = synth.bumpy_torus(12, 10)
    v = (v * 0.001).astype(np.float32)
    T = np.eye(4)
    T[:3, :3] = synth.rot_x(0.7)
    T[:3, 3] = [0, 0, 0.3]
    vc = np.random.default_rng(0).random((len(v), 3)).astype(np.float32)
    color, depth, _, xyz = _render(v, t, nrm, K, H, W, T=T, vcolor=vc)
    from pedp_hip.render import projection_matrix_from_intrinsics

    M, win = ref.pose_records(projection_matrix_from_intrinsics(K, H, W, 0.001, 100).astype(np.float32), T, None, H, W)
    rast = ref.rasterize(ref.clip_vertices(v, M[0], win[0])[None], t, H, W)
    assert (rast[..., 3] > 0).sum() > 50
    col = ref.interpolate(vc, rast, t)
    np.testing.assert_array_equal(color[0], np.clip(col[0], 0, 1)[::-1])
    assert np.array_equal(depth[0] != 0, (rast[0, ..., 3] > 0)[::-1])


def test_make_mesh_tensors_duck_types():
    import torch
    from pedp_hip.compat import make_mesh_tensors
    from pedp_hip.geometry import TriangleMesh

    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    faces = np.array([[0, 1, 2]])
    vn = np.tile([0.0, 0.0, 1.0], (3, 1))
    rgba = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 128]], np.uint8)
    m = types.SimpleNamespace(vertices=verts, faces=faces, vertex_normals=vn, visual=types.SimpleNamespace(vertex_colors=rgba))
    mt = make_mesh_tensors(m, device="cpu")
    assert set(mt) == {"pos", "faces", "vnormals", "vertex_color"}
    assert mt["faces"].dtype == torch.int32 and mt["pos"].dtype == torch.float32
    np.testing.assert_array_equal(mt["vertex_color"].numpy(), rgba[:, :3] / np.float32(255.0))

    img = (np.arange(4 * 6 * 3) % 256).astype(np.uint8).reshape(4, 6, 3)
    uv = np.array([[0.0, 0.0], [1.0, 0.25], [0.5, 1.0]])
    mat = types.SimpleNamespace(image=img)
    m = types.SimpleNamespace(vertices=verts, faces=faces, vertex_normals=vn, visual=types.SimpleNamespace(uv=uv, material=mat))
    mt = make_mesh_tensors(m, device="cpu")
    assert tuple(mt["tex"].shape) == (1, 4, 6, 3)
    np.testing.assert_allclose(mt["uv"].numpy(), np.c_[uv[:, 0], 1 - uv[:, 1]], atol=1e-7)
    assert np.array_equal(mt["uv_idx"].numpy(), faces)
    with pytest.raises(NotImplementedError):
        make_mesh_tensors(m, device="cpu", max_tex_size=5)
    assert "tex" in make_mesh_tensors(m, device="cpu", max_tex_size=6)

    tm = TriangleMesh(verts, faces)
    mt = make_mesh_tensors(tm, device="cpu")
    np.testing.assert_allclose(mt["vertex_color"].numpy(), 128 / 255.0, rtol=1e-6)
    np.testing.assert_allclose(np.abs(mt["vnormals"].numpy()[:, 2]), 1.0, rtol=1e-6)


def test_dr_shim_refuses_what_it_does_not_support():
    import torch
    from pedp_hip.compat import dr, nvdiffrast_render  # noqa: F401

    assert dr.RasterizeCudaContext() is not None and dr.RasterizeCudaContext(device="cuda:0").device == "cuda:0"
    pos = torch.zeros((1, 3, 4))
    tri = torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        dr.rasterize(None, pos, tri, (4, 4), ranges=torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        dr.rasterize(None, pos[0], tri, (4, 4))  # range mode (2-D positions)
    with pytest.raises(NotImplementedError):
        dr.rasterize(None, pos.clone().requires_grad_(True), tri, (4, 4))
    with pytest.raises(NotImplementedError):
        dr.interpolate(torch.zeros((3, 2)), torch.zeros((1, 4, 4, 4)), tri, diff_attrs="all")
    tex, uv = torch.zeros((1, 2, 2, 3)), torch.zeros((1, 4, 4, 2))
    for kw in ({"filter_mode": "nearest"}, {"boundary_mode": "clamp"}, {"mip_level_bias": torch.zeros(1)}, {"uv_da": uv}):
        with pytest.raises(NotImplementedError):
            dr.texture(tex, uv, **kw)
    from pedp_hip import compat

    for name in ("nvdiffrast_render", "make_mesh_tensors", "projection_matrix_from_intrinsics", "glcam_in_cvcam", "dr"):
        assert name in compat.__all__


# ---------------------------------------------------------------- float64 geometry (CPU twin of test_render_geometry_gpu.py)

def _geometry_render(verts, faces, poses, K, H, W, out_h, out_w, bbox=None, textured=False, seed=0):
    """ref.render of an analytic scene: colours (or uv into a ramp texture) and normals affine in the model position."""
    import _render_geometry as geo
    from pedp_hip.render import projection_matrix_from_intrinsics

    cf, nf = geo.affine_field(verts, 0.05, 0.95, seed), geo.normal_field(verts, seed + 1)
    kw, uvf = {"vcolor": geo.vertex_values(verts, cf)}, None
    if textured:
        th, tw = 48, 64
        uvf = geo.affine_field(verts, [1.0 / tw, 1.0 / th], [1 - 1.0 / tw, 1 - 1.0 / th], seed + 2, dims=2)
        kw = {"tex": geo.ramp_texture(th, tw), "uv": geo.vertex_values(verts, uvf)}
    proj = projection_matrix_from_intrinsics(K, H, W, 0.001, 100).astype(np.float32)
    out = ref.render(verts, faces, geo.vertex_values(verts, nf), poses, proj, H, W, out_h, out_w, bbox=bbox, get_normal=True, **kw)
    return out, cf, nf, uvf


@pytest.mark.parametrize("textured,crop", [(False, False), (True, False), (False, True)])
def test_restatement_meets_the_geometry_of_a_grazing_quad(textured, crop):
    """The checks of test_render_geometry_gpu.py against the restatement: perspective-correct attributes on the rays
    through the pixel centres, the covered set of the float64 ray test, and a scene in which the wrong conventions
    miss by far."""
    import _render_geometry as geo

    H, W = 480, 640
    v, f = geo.grazing_quad()
    poses = geo.quad_poses(3, seed=1)
    bbox, oh, ow = None, H, W
    if crop:  # windows around the middle of the quad, wider than tall, at a smaller output size
        bbox = np.array([[200.0, 230.0, 440.0, 400.0], [150.5, 180.25, 500.0, 470.0], [300.0, 160.0, 340.0, 200.0]], np.float32)
        oh, ow = 60, 72
    (color, depth, normal, xyz), cf, nf, uvf = _geometry_render(v, f, poses, geo.K_FRAME, H, W, oh, ow, bbox, textured)
    stats = [geo.check_pose((color[n], depth[n], normal[n], xyz[n]), poses[n], geo.K_FRAME, v, f, cf, nf, uvf, 0.3 if textured else None,
                            None if bbox is None else bbox[n], quad=True) for n in range(len(poses))]
    s = geo.summarize(stats)
    print(s)
    assert s["covered"] > (2000 if crop else 50000)


def test_restatement_meets_the_geometry_of_a_torus():
    import _render_geometry as geo
    from pedp_hip import synth

    v, t, _ = synth.bumpy_torus(40, 30)
    v = (v * 0.001).astype(np.float32)
    H, W = 48, 64
    K = np.array([[70.0, 0, 31.2], [0, 66.0, 24.4], [0, 0, 1]])
    rng = np.random.default_rng(4)
    poses = np.empty((3, 4, 4), np.float32)
    for i in range(3):
        T = np.eye(4)
        T[:3, :3] = synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.pi))
        T[:3, 3] = [rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 0.35]
        poses[i] = T
    bbox = np.array([[10.0, 8.0, 50.0, 44.0], [5.5, 2.25, 60.0, 40.0], [20.0, 10.0, 44.0, 34.0]], np.float32)
    for bb, (oh, ow) in ((None, (H, W)), (bbox, (32, 32))):
        (color, depth, normal, xyz), cf, nf, _ = _geometry_render(v, t, poses, K, H, W, oh, ow, bb)
        stats = [geo.check_pose((color[n], depth[n], normal[n], xyz[n]), poses[n], K, v, t, cf, nf, bbox=None if bb is None else bb[n])
                 for n in range(3)]
        s = geo.summarize(stats)
        assert s["covered"] > 100, s


def test_interpolate_restatement_zero_rule():
    """The kernel's rule: a pixel is zero where its id is not in [1, F] (NaN included) or its triangle names a vertex
    outside [0, V); a fractional id truncates; NaN barycentrics with a valid id propagate."""
    attr = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]], f32)
    tri = np.array([[0, 1, 2], [1, 2, 3], [-1, 1, 2], [0, 4, 2], [3, 2, -4]], np.int32)
    ids = [1.0, 2.0, 2.9, 3.0, 4.0, 5.0, 0.0, 6.0, -1.0, np.nan, 5.5]
    rast = np.zeros((1, 1, len(ids) + 1, 4), f32)
    rast[0, 0, :-1, 0], rast[0, 0, :-1, 1], rast[0, 0, :-1, 3] = 0.25, 0.5, ids
    rast[0, 0, -1] = [np.nan, 0.5, 0.0, 1.0]
    out = ref.interpolate(attr, rast, tri)[0, 0]
    a0 = 0.25 * 1.0 + 0.5 * 2.0 + 0.25 * 4.0
    a1 = 0.25 * 2.0 + 0.5 * 4.0 + 0.25 * 8.0
    np.testing.assert_array_equal(out[:3, 0], [a0, a1, a1])          # 2.9 truncates to triangle 1
    np.testing.assert_array_equal(out[:3, 1], [10 * a0, 10 * a1, 10 * a1])
    assert not out[3:len(ids)].any()                                 # bad vertex indices, bad ids
    assert np.isnan(out[-1]).all()
    batched = ref.interpolate(np.stack([attr, 2 * attr]), np.concatenate([rast, rast]), tri)
    np.testing.assert_array_equal(batched[1], 2 * batched[0])
