"""The renderer on the device (csrc/pedp_render.hip through render.py): bit-equal to the numpy restatement
(tests/_render_ref.py), independent of batching, chunking and the large-triangle path, checked against the ray caster,
equal to the reference's composition over the dr shim, and stream-ordered on torch tensors."""
import numpy as np
import pytest

import _render_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ"


def _torus(config, scale=0.001):
    from pedp_hip import synth

    W_, H_ = synth.CONFIGS[config][:2]
    v, t, n = synth.bumpy_torus(W_, H_)
    return (v * scale).astype(np.float32), t.astype(np.int32), n.astype(np.float32)


def _K(W, H, f=None):
    f = f or 0.8 * W
    return np.array([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]], np.float64)


def _poses(n, seed=0, z=0.35):
    from pedp_hip import synth

    rng = np.random.default_rng(seed)
    out = np.empty((n, 4, 4), np.float32)
    for i in range(n):
        T = np.eye(4)
        T[:3, :3] = synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.pi))
        T[:3, 3] = [rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), z + rng.uniform(-0.05, 0.05)]
        out[i] = T
    return out


def _mesh_tensors(v, t, n, textured=False, seed=1):
    rng = np.random.default_rng(seed)
    mt = {"pos": torch.as_tensor(v, device="cuda"), "faces": torch.as_tensor(t, device="cuda"),
          "vnormals": torch.as_tensor(n, device="cuda")}
    if textured:
        mt["tex"] = torch.as_tensor(rng.random((1, 13, 21, 3), dtype=np.float32), device="cuda")
        mt["uv"] = torch.as_tensor(rng.uniform(-0.3, 1.3, (len(v), 2)).astype(np.float32), device="cuda")
        mt["uv_idx"] = mt["faces"]
    else:
        mt["vertex_color"] = torch.as_tensor(rng.random((len(v), 3), dtype=np.float32), device="cuda")
    return mt


def _crop_boxes(N, H, W, seed=2):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(0.4, 0.6, N) * W, rng.uniform(0.4, 0.6, N) * H], 1)
    s = rng.uniform(0.35, 0.6, N) * min(H, W)
    return np.concatenate([c - s[:, None] / 2, c + s[:, None] / 2], 1).astype(np.float32)


def _render_both(v, t, n, poses, K, H, W, textured=False, bbox=None, output_size=None, use_light=False, get_normal=False,
                 light_color=None, light_dir=np.array([0, 0, 1])):
    from pedp_hip.compat import nvdiffrast_render, projection_matrix_from_intrinsics

    mt = _mesh_tensors(v, t, n, textured)
    oh, ow = (H, W) if output_size is None else output_size
    extra = {}
    bb = None if bbox is None else torch.as_tensor(bbox, device="cuda")
    col, dep, nrm = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(poses, device="cuda"), mesh_tensors=mt,
                                      bbox2d=bb, output_size=output_size, use_light=use_light, get_normal=get_normal,
                                      light_color=light_color, light_dir=light_dir, extra=extra)
    proj = projection_matrix_from_intrinsics(K, H, W, 0.001, 100).astype(np.float32)
    kw = {"tex": mt["tex"][0].cpu().numpy(), "uv": mt["uv"].cpu().numpy()} if textured else {"vcolor": mt["vertex_color"].cpu().numpy()}
    want = ref.render(v, t, n, poses, proj, H, W, oh, ow, bbox=bbox, get_normal=get_normal, use_light=use_light,
                      light_color=light_color, light_dir=light_dir, **kw)
    return (col, dep, nrm, extra["xyz_map"]), want


CASES = [
    # mesh, N, textured, bbox, output_size, use_light, get_normal
    ("tiny", 1, False, False, None, False, False),
    ("tiny", 4, True, True, (24, 40), True, True),
    ("tiny", 17, False, True, (32, 32), True, False),
    ("parity", 1, False, True, (40, 40), True, True),
    ("parity", 4, True, False, (36, 52), False, True),
]


@pytest.mark.parametrize("config,N,textured,crop,output_size,use_light,get_normal", CASES)
def test_render_bit_identical_to_restatement(config, N, textured, crop, output_size, use_light, get_normal):
    v, t, n = _torus(config)
    H, W = 48, 64
    K = _K(W, H)
    bbox = _crop_boxes(N, H, W) if crop else None
    got, want = _render_both(v, t, n, _poses(N, seed=N), K, H, W, textured, bbox, output_size, use_light, get_normal)
    assert (want[1] != 0).sum() > 20 * N
    for g, w, what in zip(got, want, ("color", "depth", "normal", "xyz")):
        if w is None:
            assert g is None
        else:
            _assert_bits(g, w, what)


def test_render_light_color_and_point_light():
    v, t, n = _torus("tiny")
    H, W = 40, 40
    got, want = _render_both(v, t, n, _poses(3, seed=7), _K(W, H), H, W, use_light=True, light_color=[0.9, 0.2, 0.4])
    for g, w, what in zip(got, want, ("color", "depth", "normal", "xyz")):
        _assert_bits(g, w, what)
    got, want = _render_both(v, t, n, _poses(2, seed=8), _K(W, H), H, W, use_light=True, light_dir=None)
    _assert_bits(got[0], want[0], "color (point light)")


def test_render_behind_camera_and_inside_znear():
    """Part of the mesh behind the eye (w <= 0 vertices) and nearer than znear: clipped per pixel, no near-plane clip."""
    v, t, n = _torus("parity")
    poses = _poses(3, seed=11)
    poses[0, 2, 3] = 0.0005        # the centre inside znear, the ring around the eye
    poses[1, 2, 3] = 0.02          # the near half behind the camera
    poses[2, :3, :3] = np.eye(3)
    poses[2, :3, 3] = [0.06, 0.0, 0.0]  # the ring through the eye
    H, W = 36, 44
    got, want = _render_both(v, t, n, poses, _K(W, H, 20.0), H, W, get_normal=True)
    assert (want[1] != 0).any()
    for g, w, what in zip(got, want, ("color", "depth", "normal", "xyz")):
        _assert_bits(g, w, what)


def _quad(N, z=0.3):
    v = np.array([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.tile(np.array([0, 0, -1], np.float32), (4, 1))


def test_large_triangles_screen_filling_quad_512():
    from pedp_hip.compat import dr

    N, S = 64, 512
    v, t, _ = _quad(N)
    rng = np.random.default_rng(5)
    pos = np.concatenate([v * rng.uniform(0.9, 1.1, (N, 1, 3)).astype(np.float32), np.ones((N, 4, 1), np.float32)], 2)
    pos[..., 2] = rng.uniform(-0.5, 0.5, (N, 1))
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), torch.as_tensor(pos, device="cuda"), torch.as_tensor(t, device="cuda"), (S, S))
    torch.cuda.synchronize()
    assert rast.shape == (N, S, S, 4)
    for k in (0, 17, 63):  # the restatement is slow at 512 x 512: three of the poses
        _assert_bits(rast[k], ref.rasterize(pos[k:k + 1], t, S, S)[0], f"rast pose {k}")
    assert (rast[..., 3] > 0).float().mean().item() > 0.8


def test_mixed_big_and_tiny_triangles():
    from pedp_hip.compat import dr

    rng = np.random.default_rng(9)
    N, H, W = 5, 96, 80
    big = rng.uniform(-1.5, 1.5, (40, 3, 2))
    tiny = rng.uniform(-1, 1, (400, 1, 2)) + rng.uniform(-0.02, 0.02, (400, 3, 2))
    xy = np.concatenate([big, tiny]).reshape(-1, 2)
    V = len(xy)
    pos = np.empty((N, V, 4), np.float32)
    for i in range(N):
        w = rng.uniform(0.5, 2.0, V)
        pos[i, :, :2] = xy * w[:, None]
        pos[i, :, 2] = rng.uniform(-0.9, 0.9, V) * w
        pos[i, :, 3] = w
    tri = np.arange(V, dtype=np.int32).reshape(-1, 3)
    rast, _ = dr.rasterize(None, torch.as_tensor(pos, device="cuda"), torch.as_tensor(tri, device="cuda"), (H, W))
    _assert_bits(rast, ref.rasterize(pos, tri, H, W), "rast")


def test_batch_independence_chunks_and_determinism():
    from pedp_hip import render

    v, t, n = _torus("parity")
    H, W = 40, 48
    K = _K(W, H)
    poses = _poses(9, seed=3)
    bbox = _crop_boxes(9, H, W)
    mt = _mesh_tensors(v, t, n, textured=True)

    def run(p, b):
        extra = {}
        out = render.nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(p, device="cuda"), mesh_tensors=mt,
                                       bbox2d=torch.as_tensor(b, device="cuda"), output_size=(32, 32), use_light=True, extra=extra)
        return [x.clone() for x in out] + [extra["xyz_map"].clone()]

    a = run(poses, bbox)
    b = run(poses, bbox)
    for x, y in zip(a, b):
        _assert_bits(x, y, "second run")
    for i in (0, 4, 8):
        one = run(poses[i:i + 1], bbox[i:i + 1])
        for x, y in zip(a, one):
            _assert_bits(x[i:i + 1], y, f"pose {i} alone")
    try:
        render.set_pose_chunk(2)
        c = run(poses, bbox)
    finally:
        render.set_pose_chunk(0)
    for x, y in zip(a, c):
        _assert_bits(x, y, "chunked")


def test_depth_and_ids_agree_with_the_ray_caster():
    """bench_100k torus: rays through the pixel centres (c + 0.5, r + 0.5) hit the triangle the renderer shows."""
    from pedp_hip import _lib
    from pedp_hip.compat import dr, nvdiffrast_render, projection_matrix_from_intrinsics

    v, t, n = _torus("bench_100k")
    H, W = 120, 160
    K = _K(W, H, 150.0)
    poses = _poses(2, seed=21, z=0.3)
    ctx = _lib.Context(0)
    try:
        for k in range(2):
            T = poses[k].astype(np.float64)
            vp = (v.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
            mesh = _lib.Mesh(ctx, vp, t.astype(np.uint32))
            rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            d = np.stack([(cc + 0.5 - K[0, 2]) / K[0, 0], (rr + 0.5 - K[1, 2]) / K[1, 1], np.ones_like(cc, float)], -1).reshape(-1, 3)
            rays = np.concatenate([np.zeros_like(d), d], 1).astype(np.float32)
            hit = mesh.cast_rays(rays, want_uv=False)
            extra = {}
            col, dep, _ = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(poses[k:k + 1], device="cuda"),
                                            mesh_tensors=_mesh_tensors(v, t, n), extra=extra)
            # triangle ids: the shim's rast_out over the same clip vertices (flipped into image rows)
            M, win = ref.pose_records(projection_matrix_from_intrinsics(K, H, W, 0.001, 100).astype(np.float32), poses[k:k + 1],
                                      None, H, W)
            clip = torch.as_tensor(ref.clip_vertices(v, M[0], win[0])[None], device="cuda")
            rast, _ = dr.rasterize(None, clip, torch.as_tensor(t, device="cuda"), (H, W))
            ids = (rast[0, ..., 3].flip(0).cpu().numpy().astype(np.int64) - 1).reshape(-1)
            z_r = dep[0].cpu().numpy().reshape(-1)
            ray_hit = np.isfinite(hit["t_hit"])
            both = ray_hit & (ids >= 0)
            assert both.sum() > 2000
            agree = (hit["primitive_ids"][both].astype(np.int64) == ids[both]).mean()
            assert agree >= 0.999, f"pose {k}: triangle ids agree on {agree:.5f}"
            z_ray = (hit["t_hit"] * d[:, 2])[both]
            same = hit["primitive_ids"][both].astype(np.int64) == ids[both]
            np.testing.assert_allclose(z_r[both][same], z_ray[same], rtol=1e-5)
            # coverage may differ only on the silhouette: such a pixel has a 4-neighbour the other side of it
            diff = (ray_hit != (ids >= 0)).reshape(H, W)
            cov = (ids >= 0).reshape(H, W)
            pad = np.pad(cov, 1, mode="edge")
            edge = (pad[1:-1, 1:-1] != pad[:-2, 1:-1]) | (pad[1:-1, 1:-1] != pad[2:, 1:-1]) | \
                   (pad[1:-1, 1:-1] != pad[1:-1, :-2]) | (pad[1:-1, 1:-1] != pad[1:-1, 2:])
            assert not (diff & ~edge).any(), f"pose {k}: {int((diff & ~edge).sum())} coverage differences off the silhouette"
    finally:
        ctx.close()


def test_fused_equals_reference_composition_over_the_shim():
    """The reference's nvdiffrast_render written in torch over dr.rasterize / interpolate / texture (with flips)."""
    import torch.nn.functional as F
    from pedp_hip.compat import dr, glcam_in_cvcam, nvdiffrast_render, projection_matrix_from_intrinsics

    v, t, n = _torus("parity")
    H, W, N = 48, 64, 6
    K = _K(W, H)
    poses = torch.as_tensor(_poses(N, seed=4), device="cuda")
    bbox = torch.as_tensor(_crop_boxes(N, H, W), device="cuda")
    for textured in (False, True):
        mt = _mesh_tensors(v, t, n, textured)
        extra = {}
        col, dep, nrm = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=poses, mesh_tensors=mt, bbox2d=bbox, output_size=(40, 40),
                                          use_light=True, extra=extra)
        # the composition, step by step
        pos, faces, vn = mt["pos"], mt["faces"], mt["vnormals"]
        proj = torch.as_tensor(projection_matrix_from_intrinsics(K, H, W, 0.001, 100), device="cuda", dtype=torch.float)
        mtx = proj[None] @ (torch.as_tensor(glcam_in_cvcam, device="cuda", dtype=torch.float)[None] @ poses)
        pts_cam = (poses[:, None, :3, :3] @ pos[None, ..., None])[..., 0] + poses[:, None, :3, 3]
        clip_t = (mtx[:, None] @ torch.cat([pos, torch.ones_like(pos[:, :1])], 1)[None, ..., None])[..., 0]
        l, tt, r, b = bbox[:, 0], H - bbox[:, 1], bbox[:, 2], H - bbox[:, 3]
        tf = torch.eye(4, device="cuda").expand(N, 4, 4).contiguous()
        tf[:, 0, 0], tf[:, 1, 1] = W / (r - l), H / (tt - b)
        tf[:, 3, 0], tf[:, 3, 1] = (W - r - l) / (r - l), (H - tt - b) / (tt - b)
        clip_t = clip_t @ tf
        # torch's matmuls round in their own order: the rasterizer is fed the contract's clip vertices (the restatement's,
        # bit-equal to the fused path's), after checking that they are the same transform
        M, win = ref.pose_records(proj.cpu().numpy(), poses.cpu().numpy(), bbox.cpu().numpy(), H, W)
        clip = torch.as_tensor(np.stack([ref.clip_vertices(v, M[i], win[i]) for i in range(N)]), device="cuda")
        assert ((clip - clip_t).abs() <= 1e-5 * (1 + clip_t.abs())).all()
        rast, _ = dr.rasterize(dr.RasterizeCudaContext(), clip, faces, resolution=np.asarray([40, 40]))
        xyz, _ = dr.interpolate(pts_cam, rast, faces)
        if textured:
            texc, _ = dr.interpolate(mt["uv"], rast, mt["uv_idx"])
            color = dr.texture(mt["tex"], texc, filter_mode="linear")
        else:
            color, _ = dr.interpolate(mt["vertex_color"], rast, faces)
        vn_cam = (poses[:, None, :3, :3] @ vn[None, ..., None])[..., 0]
        nmap = torch.flip(F.normalize(dr.interpolate(vn_cam, rast, faces)[0], dim=-1), dims=[1])
        dif = (F.normalize(vn_cam, dim=-1) * F.normalize(-torch.tensor([0.0, 0, 1], device="cuda"), dim=-1)).sum(-1).clip(0, 1)[..., None]
        dmap, _ = dr.interpolate(dif, rast, faces)
        color = (color * 0.8 + dmap * color * 0.5).clip(0, 1) * torch.clamp(rast[..., -1:], 0, 1)
        want = (torch.flip(color, dims=[1]), torch.flip(xyz[..., 2], dims=[1]), nmap, torch.flip(xyz, dims=[1]))
        for g, w, what in zip((col, dep, nrm, extra["xyz_map"]), want, ("color", "depth", "normal", "xyz")):
            err = (g - w).abs().max().item()
            assert err <= 1e-6, f"{what} textured={textured}: max |difference| {err:.3g}"
        assert (rast[..., 3] > 0).sum().item() > 1000


def test_torch_tensors_stay_on_device_and_follow_the_stream():
    from pedp_hip.compat import nvdiffrast_render

    v, t, n = _torus("parity")
    H, W = 48, 64
    K = _K(W, H)
    mt = _mesh_tensors(v, t, n)
    poses = torch.as_tensor(_poses(5, seed=6), device="cuda")
    extra = {}
    base = [x.clone() for x in nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=poses, mesh_tensors=mt, get_normal=True, extra=extra)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        p2 = poses * 1.0  # produced on s: the render must be ordered behind it
        extra2 = {}
        out = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=p2, mesh_tensors=mt, get_normal=True, extra=extra2)
        summed = out[1].sum()  # consumed on s straight away
    s.synchronize()
    for x in list(out) + [extra2["xyz_map"], summed]:
        assert x.is_cuda and x.device == poses.device
    for x, y in zip(out, base):
        _assert_bits(x, y, "on a side stream")
    assert abs(summed.item() - base[1].sum().item()) < 1e-3


def test_shapes_and_dtypes_the_callers_index():
    from pedp_hip.compat import dr, make_mesh_tensors, nvdiffrast_render
    from pedp_hip.geometry import TriangleMesh

    v, t, n = _torus("bench_100k")
    tm = TriangleMesh(v.astype(np.float64), t)
    tm.vertex_normals = n.astype(np.float64)
    mt = make_mesh_tensors(tm)
    assert mt["pos"].is_cuda and mt["faces"].dtype == torch.int32
    N = 252
    poses = torch.as_tensor(_poses(N, seed=12), device="cuda")
    K = _K(640, 480, 600.0)
    bbox = torch.as_tensor(_crop_boxes(N, 480, 640), device="cuda")
    extra = {}
    col, dep, nrm = nvdiffrast_render(K=K, H=480, W=640, ob_in_cams=poses, glctx=dr.RasterizeCudaContext(), mesh_tensors=mt,
                                      bbox2d=bbox, output_size=(160, 160), use_light=True, extra=extra)
    assert col.shape == (N, 160, 160, 3) and dep.shape == (N, 160, 160) and nrm.shape == (N, 160, 160, 3)
    assert extra["xyz_map"].shape == (N, 160, 160, 3)
    for x in (col, dep, nrm, extra["xyz_map"]):
        assert x.is_cuda and x.dtype == torch.float32
    assert (dep > 0).float().mean().item() > 0.05
    col, dep, nrm = nvdiffrast_render(K=K, H=480, W=640, ob_in_cams=poses[:2], mesh_tensors=mt, extra=extra)
    assert nrm is None and col.shape == (2, 480, 640, 3)
    rast, db = dr.rasterize(None, torch.zeros((2, 3, 4), device="cuda"), torch.zeros((1, 3), dtype=torch.int32, device="cuda"), (8, 6))
    assert db is None and rast.shape == (2, 8, 6, 4) and rast.dtype == torch.float32


def test_bad_shapes_and_empty_batches():
    from pedp_hip.compat import dr, nvdiffrast_render

    v, t, n = _torus("tiny")
    mt = _mesh_tensors(v, t, n)
    K = _K(32, 24)
    with pytest.raises(RuntimeError):
        nvdiffrast_render(K=K, H=24, W=32, ob_in_cams=torch.zeros((2, 3, 4), device="cuda"), mesh_tensors=mt)
    with pytest.raises(RuntimeError):
        nvdiffrast_render(K=K, H=24, W=32, ob_in_cams=torch.eye(4, device="cuda")[None], mesh_tensors=mt,
                          bbox2d=torch.zeros((3, 4), device="cuda"))
    with pytest.raises(RuntimeError):
        dr.rasterize(None, torch.zeros((1, 3, 3), device="cuda"), torch.as_tensor(t, device="cuda"), (8, 8))
    with pytest.raises(RuntimeError):
        dr.interpolate(torch.zeros((2, 5, 3), device="cuda"), torch.zeros((1, 4, 4, 4), device="cuda"), torch.as_tensor(t, device="cuda"))
    with pytest.raises(RuntimeError):
        dr.rasterize(None, torch.zeros((1, 3, 4), device="cuda"), torch.as_tensor(t, device="cuda"), (0, 8))
    extra = {}
    col, dep, nrm = nvdiffrast_render(K=K, H=24, W=32, ob_in_cams=torch.zeros((0, 4, 4), device="cuda"), mesh_tensors=mt,
                                      get_normal=True, extra=extra)
    assert col.shape == (0, 24, 32, 3) and dep.shape == (0, 24, 32) and nrm.shape == (0, 24, 32, 3)
    empty = dict(mt, faces=torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    col, dep, nrm = nvdiffrast_render(K=K, H=24, W=32, ob_in_cams=torch.as_tensor(_poses(2), device="cuda"), mesh_tensors=empty,
                                      get_normal=True, extra=extra)
    for x in (col, dep, nrm, extra["xyz_map"]):
        assert x.shape[0] == 2 and not x.any()
    rast, _ = dr.rasterize(None, torch.zeros((2, 3, 4), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), (4, 4))
    assert not rast.any()


def test_host_arrays_work_too():
    from pedp_hip.compat import dr, nvdiffrast_render, projection_matrix_from_intrinsics

    v, t, n = _torus("tiny")
    H, W = 30, 36
    K = _K(W, H)
    poses = _poses(3, seed=2)
    vc = np.random.default_rng(1).random((len(v), 3)).astype(np.float32)
    mt = {"pos": v, "faces": t, "vnormals": n, "vertex_color": vc}
    extra = {}
    col, dep, nrm = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=poses, mesh_tensors=mt, get_normal=True, extra=extra)
    assert isinstance(col, np.ndarray)
    proj = projection_matrix_from_intrinsics(K, H, W, 0.001, 100).astype(np.float32)
    want = ref.render(v, t, n, poses, proj, H, W, H, W, vcolor=vc, get_normal=True)
    for g, w, what in zip((col, dep, nrm, extra["xyz_map"]), want, ("color", "depth", "normal", "xyz")):
        _assert_bits(g, w, what)
    M, win = ref.pose_records(proj, poses, None, H, W)
    clip = np.stack([ref.clip_vertices(v, M[i], win[i]) for i in range(3)])
    rast, _ = dr.rasterize(None, torch.as_tensor(clip), torch.as_tensor(t), (H, W))
    assert isinstance(rast, torch.Tensor) and not rast.is_cuda
    _assert_bits(rast, ref.rasterize(clip, t, H, W), "rast (host)")
    _assert_bits(dr.interpolate(vc, rast.numpy(), t)[0], ref.interpolate(vc, rast.numpy(), t), "interpolate (host)")


# ---------------------------------------------------------------- the big-triangle list's overflow

BIG_CAP = 1 << 20          # big-list entries per chunk (csrc/pedp_render.hip)
KEY_BUDGET = 128 << 20     # key bytes per automatic chunk


def _big_triangles(N, F, S, rng, min_px=10):
    """N x 3F x 4 clip positions (w = 1) of F triangles per pose, each inside the viewport with a projected bounding box
    at least min_px wide and tall and an area of at least 20 px^2: none is culled, every rectangle exceeds 64 px."""
    px = 2.0 / S
    xy = np.empty((N, F, 3, 2))
    todo = np.ones((N, F), bool)
    while todo.any():
        k = int(todo.sum())
        c = rng.uniform(-0.7, 0.7, (k, 1, 2))
        xy[todo] = c + rng.uniform(-0.28, 0.28, (k, 3, 2))
        ext = xy.max(2) - xy.min(2)
        e1, e2 = xy[:, :, 1] - xy[:, :, 0], xy[:, :, 2] - xy[:, :, 0]
        area = 0.5 * np.abs(e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]) / (px * px)
        todo = (ext < min_px * px).any(-1) | (area < 20)
    pos = np.ones((N, F * 3, 4), np.float32)
    pos[..., :2] = xy.reshape(N, F * 3, 2)
    pos[..., 2] = rng.uniform(-0.9, 0.9, (N, F * 3))
    assert (np.abs(pos[..., :2]) <= 0.98).all()
    return pos


def test_big_list_overflow_rasterize():
    """655 poses x 2048 triangles at 160 x 160, one automatic chunk: 1,341,440 big rectangles for a list of 2^20, so
    292,864 lanes cover their own rectangles.  Which lanes overflow depends on the order of the atomics; the result
    must not."""
    from pedp_hip import render
    from pedp_hip.compat import dr

    N, F, S = 655, 2048, 160
    assert KEY_BUDGET // (8 * S * S) == N                      # one chunk
    assert N * F == 1_341_440 and N * F - BIG_CAP == 292_864   # entries past the list's end
    assert 8 * F < BIG_CAP                                      # chunks of 8 poses: 16,384 entries, no overflow
    pos = _big_triangles(N, F, S, np.random.default_rng(31))
    tri = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    pos_t, tri_t = torch.as_tensor(pos, device="cuda"), torch.as_tensor(tri, device="cuda")
    a, _ = dr.rasterize(None, pos_t, tri_t, (S, S))
    b, _ = dr.rasterize(None, pos_t, tri_t, (S, S))
    _assert_bits(b, a, "second run")
    del b
    try:
        render.set_pose_chunk(8)
        c, _ = dr.rasterize(None, pos_t, tri_t, (S, S))
    finally:
        render.set_pose_chunk(0)
    _assert_bits(c, a, "chunks of 8 poses")
    del c
    for k in (0, 1, 327, 653, 654):
        _assert_bits(a[k], ref.rasterize(pos[k:k + 1], tri, S, S)[0], f"pose {k} against the restatement")
    assert (a[..., 3] > 0).float().mean().item() > 0.7


def test_big_list_overflow_fused_render():
    """The fused path's overflow: 2048 large triangles at 655 perturbed poses, 160 x 160."""
    from pedp_hip import render, synth
    from pedp_hip.compat import nvdiffrast_render, projection_matrix_from_intrinsics

    N, F, S = 655, 2048, 160
    rng = np.random.default_rng(32)
    K = np.array([[200.0, 0, 79.5], [0, 200.0, 79.5], [0, 0, 1]])
    c = np.concatenate([rng.uniform(-0.12, 0.12, (F, 1, 2)), rng.uniform(0.45, 0.55, (F, 1, 1))], 2)
    off = rng.uniform(0.035, 0.06, (F, 3, 2)) * np.array([[[-1, -1], [1, -0.2], [-0.3, 1]]])
    v = (c + np.concatenate([off, rng.uniform(-0.02, 0.02, (F, 3, 1))], 2)).reshape(-1, 3).astype(np.float32)
    t = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    n = np.tile(np.array([0, 0, -1], np.float32), (3 * F, 1))
    poses = np.empty((N, 4, 4), np.float32)
    for i in range(N):
        T = np.eye(4)
        T[:3, :3] = synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.deg2rad(2)))
        T[:3, 3] = rng.uniform(-0.005, 0.005, 3)
        poses[i] = T
    # the overflow is reached: more than 2^20 (pose, triangle) rectangles of at least 10 x 10 px, inside the image
    cam = np.einsum("nij,vj->nvi", poses[:, :3, :3].astype(np.float64), v.astype(np.float64)) + poses[:, None, :3, 3]
    uv = (cam[..., :2] / cam[..., 2:]) * 200.0 + 79.5
    uv = uv.reshape(N, F, 3, 2)
    ext = uv.max(2) - uv.min(2)
    big = ((ext >= 10).all(-1) & (uv.min((2, 3)) >= 0) & (uv.max((2, 3)) <= S)).sum()
    assert big > BIG_CAP + 100_000, f"only {big} big rectangles"
    mt = _mesh_tensors(v, t, n)
    pt = torch.as_tensor(poses, device="cuda")

    def run():
        extra = {}
        out = nvdiffrast_render(K=K, H=S, W=S, ob_in_cams=pt, mesh_tensors=mt, use_light=True, get_normal=True, extra=extra)
        return list(out) + [extra["xyz_map"]]

    a = run()
    for x, y, what in zip(a, run(), ("color", "depth", "normal", "xyz")):
        _assert_bits(y, x, f"{what}, second run")
    try:
        render.set_pose_chunk(8)
        c8 = run()
    finally:
        render.set_pose_chunk(0)
    for x, y, what in zip(a, c8, ("color", "depth", "normal", "xyz")):
        _assert_bits(y, x, f"{what}, chunks of 8 poses")
    del c8
    proj = projection_matrix_from_intrinsics(K, S, S, 0.001, 100).astype(np.float32)
    for k in (0, 654):
        want = ref.render(v, t, n, poses[k:k + 1], proj, S, S, S, S, vcolor=mt["vertex_color"].cpu().numpy(), get_normal=True,
                          use_light=True)
        for x, w, what in zip(a, want, ("color", "depth", "normal", "xyz")):
            _assert_bits(x[k:k + 1], w, f"{what}, pose {k} against the restatement")
    assert (a[1] > 0).float().mean().item() > 0.5


# ---------------------------------------------------------------- dr.texture and dr.interpolate, bit for bit

f32 = np.float32


def _guard_u(n):
    """float32 u at which the sampler's x = u n - 0.5 is exactly 1e8 (sampled as zeros) and the one just below it."""
    n32 = f32(n)

    def x(u):
        return f32(f32(u) * n32) - f32(0.5)

    u = f32(f32(1e8) / n32)
    while x(u) >= f32(1e8):
        u = np.nextafter(u, f32(0))
    while x(u) < f32(1e8):
        u = np.nextafter(u, f32(np.inf))
    return u, np.nextafter(u, f32(0))


def _texture_case(N, th, tw, C, per_image, rng):
    tex = rng.random((N if per_image else 1, th, tw, C), dtype=np.float32) + f32(0.5)   # no zero texel
    H, W = 6, 40
    uv = rng.uniform(-2.5, 3.5, (N, H, W, 2)).astype(np.float32)
    j = np.arange(tw + 1)
    i = np.arange(th + 1)
    row_u = np.concatenate([(j[:tw] + 0.5) / tw, j / tw, [0.0, 1.0, -1.0 / tw, -0.25, 1.25, 2.0, -3.0]]).astype(np.float32)
    row_v = np.concatenate([(i[:th] + 0.5) / th, i / th, [0.0, 1.0, -1.0 / th, -0.25, 1.25, 2.0, -3.0]]).astype(np.float32)
    k = min(W, len(row_u))
    uv[:, 0, :k, 0] = row_u[:k]                        # texel centres and edges, 0 and 1, wrap in u
    k = min(W, len(row_v))
    uv[:, 1, :k, 1] = row_v[:k]                        # ... and in v
    at_u, below_u = _guard_u(tw)
    at_v, below_v = _guard_u(th)
    special = [(np.nan, 0.3), (0.3, np.nan), (np.inf, 0.3), (0.3, -np.inf), (-np.inf, np.inf), (at_u, 0.3), (-at_u, 0.3),
               (0.3, at_v), (below_u, 0.3), (0.3, below_v), (-below_u, -below_v)]
    uv[:, 2, :len(special)] = np.array(special, np.float32)
    zero = np.zeros((H, W), bool)
    zero[2, :8] = True                                  # NaN, inf and |x| >= 1e8: zeros
    return tex, uv, zero


@pytest.mark.parametrize("C", [1, 2, 3, 4, 16])
@pytest.mark.parametrize("per_image", [False, True])
def test_texture_bit_equal_to_restatement(C, per_image):
    from pedp_hip.compat import dr

    rng = np.random.default_rng(C * 2 + per_image)
    N = 3
    for th, tw in ((1, 1), (1, 7), (5, 1), (13, 21)):
        tex, uv, zero = _texture_case(N, th, tw, C, per_image, rng)
        want = ref.texture(tex, uv)
        assert not want[:, zero].any() and want[:, ~zero].all(), "the case does not separate zeros from samples"
        got = dr.texture(torch.as_tensor(tex, device="cuda"), torch.as_tensor(uv, device="cuda"), filter_mode="linear")
        assert got.is_cuda and tuple(got.shape) == (N, 6, 40, C)
        _assert_bits(got, want, f"{th} x {tw}, device")
        _assert_bits(dr.texture(tex, uv), want, f"{th} x {tw}, host")
        for dt in (np.float64, np.float16):  # other dtypes: the result of their float32 conversion
            tx, u = tex.astype(dt), uv.astype(dt)
            w2 = ref.texture(tx.astype(np.float32), u.astype(np.float32))
            _assert_bits(dr.texture(torch.as_tensor(tx, device="cuda"), torch.as_tensor(u, device="cuda")), w2, f"{dt.__name__} device")
            _assert_bits(dr.texture(tx, u), w2, f"{dt.__name__} host")


def test_texture_refuses_bad_channel_and_texture_counts():
    from pedp_hip import _lib
    from pedp_hip.compat import dr

    uv = torch.zeros((3, 4, 4, 2), device="cuda")
    with pytest.raises(_lib.PedpError):
        dr.texture(torch.zeros((1, 2, 2, 17), device="cuda"), uv)
    with pytest.raises(_lib.PedpError):
        dr.texture(torch.zeros((2, 2, 2, 3), device="cuda"), uv)
    assert tuple(dr.texture(torch.zeros((3, 2, 2, 16), device="cuda"), uv).shape) == (3, 4, 4, 16)


@pytest.mark.parametrize("A", [1, 2, 3, 7])
@pytest.mark.parametrize("per_image", [False, True])
def test_interpolate_bit_equal_to_restatement(A, per_image):
    """rast from dr.rasterize, then edited: ids 0, F + 1, 2.5 (triangle 1), negative and NaN, NaN barycentrics with a
    valid id, and triangles that name a vertex outside [0, V)."""
    from pedp_hip.compat import dr, projection_matrix_from_intrinsics

    v, t, _ = _torus("tiny")
    N, H, W = 3, 24, 32
    F, V = len(t), len(v)
    K = _K(W, H)
    M, win = ref.pose_records(projection_matrix_from_intrinsics(K, H, W, 0.001, 100).astype(np.float32), _poses(N, seed=40), None,
                              H, W)
    clip = np.stack([ref.clip_vertices(v, M[i], win[i]) for i in range(N)])
    rast, _ = dr.rasterize(None, torch.as_tensor(clip, device="cuda"), torch.as_tensor(t, device="cuda"), (H, W))
    rast = rast.cpu().numpy()
    assert (rast[..., 3] > 0).sum() > 200
    tri = t.copy()
    tri[5] = [-1, 1, 2]              # a negative vertex index
    tri[6] = [0, V, 2]               # one past the last vertex
    tri[7] = [3, 4, 2 ** 31 - 1]
    # (id, barycentrics, expected): 0 zeros, 1 a value, nan NaN
    edits = [(0.0, "", 0), (F + 1.0, "", 0), (2.5, "", 1), (-1.0, "", 0), (-0.5, "", 0), (np.nan, "", 0), (2.0, "u", np.nan),
             (4.0, "v", np.nan), (6.0, "", 0), (7.0, "", 0), (8.0, "", 0), (float(F), "", 1), (F + 0.5, "", 0), (3.999, "", 1)]
    where = []
    for k, (rid, bad, _) in enumerate(edits):
        at = (k % N, 2 + k // 4, 3 + 5 * (k % 4))
        where.append(at)
        rast[at][:2] = [np.nan if bad == "u" else 0.25, np.nan if bad == "v" else 0.5]
        rast[at][3] = rid
    rng = np.random.default_rng(A)
    attr = rng.normal(size=((N, V, A) if per_image else (V, A))).astype(np.float32)
    want = ref.interpolate(attr, rast, tri)
    for at, (rid, _, exp) in zip(where, edits):
        val = want[at]
        ok = np.isnan(val).all() if exp is np.nan else (not val.any() if exp == 0 else np.isfinite(val).all() and val.any())
        assert ok, f"the restatement at id {rid}: {val}"
    got = dr.interpolate(torch.as_tensor(attr, device="cuda"), torch.as_tensor(rast, device="cuda"), torch.as_tensor(tri, device="cuda"))[0]
    assert got.is_cuda and tuple(got.shape) == (N, H, W, A)
    _assert_bits(got, want, "device")
    _assert_bits(dr.interpolate(attr, rast, tri)[0], want, "host")
