"""The renderer against float64 geometry at the refiner's sizes (tests/_render_geometry.py): every covered pixel's xyz
on the ray through its pixel centre (with and without bbox2d), colour and normal equal to affine fields of the model
position, a ramp texture sampled back to its uv, the covered set of a grazing quad equal to the float64 ray test, and
background zero in every map.  The same checks measure two wrong conventions at the same pixels and require them to
fail by far.  Every batch is also bit-equal to itself rendered one pose per chunk."""
import numpy as np
import pytest

import _render_geometry as geo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEY_BUDGET = 128 << 20   # bytes of per-pixel keys per automatic chunk (csrc/pedp_render.hip)


def _mesh_tensors(verts, faces, seed, textured=False):
    cf, nf = geo.affine_field(verts, 0.05, 0.95, seed), geo.normal_field(verts, seed + 1)
    mt = {"pos": torch.as_tensor(verts, device="cuda"), "faces": torch.as_tensor(faces, device="cuda"),
          "vnormals": torch.as_tensor(geo.vertex_values(verts, nf), device="cuda")}
    uvf = None
    if textured:
        th, tw = 48, 64
        uvf = geo.affine_field(verts, [1.0 / tw, 1.0 / th], [1 - 1.0 / tw, 1 - 1.0 / th], seed + 2, dims=2)
        mt["tex"] = torch.as_tensor(geo.ramp_texture(th, tw)[None], device="cuda")
        mt["uv"] = torch.as_tensor(geo.vertex_values(verts, uvf), device="cuda")
        mt["uv_idx"] = mt["faces"]
    else:
        mt["vertex_color"] = torch.as_tensor(geo.vertex_values(verts, cf), device="cuda")
    return mt, cf, nf, uvf


def _render(mt, poses, K, H, W, bbox=None, output_size=None):
    from pedp_hip.compat import nvdiffrast_render

    extra = {}
    bb = None if bbox is None else torch.as_tensor(bbox, device="cuda")
    col, dep, nrm = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(poses, device="cuda"), mesh_tensors=mt, bbox2d=bb,
                                      output_size=output_size, use_light=False, get_normal=True, extra=extra)
    return col, dep, nrm, extra["xyz_map"]


def _render_checked(mt, poses, K, H, W, bbox=None, output_size=None):
    """The batch, after asserting it bit-equal to the same call with one pose per chunk."""
    from pedp_hip import render

    out = _render(mt, poses, K, H, W, bbox, output_size)
    try:
        render.set_pose_chunk(1)
        one = _render(mt, poses, K, H, W, bbox, output_size)
    finally:
        render.set_pose_chunk(0)
    for a, b, what in zip(out, one, ("color", "depth", "normal", "xyz")):
        diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
        assert diff == 0, f"{what}: {diff} values differ from the one-pose-per-chunk render"
    return out


def _check_all(out, poses, K, verts, faces, cf, nf, uvf=None, bbox=None, quad=False):
    stats = []
    for n in range(len(poses)):
        maps = [x[n].cpu().numpy() for x in out]
        try:
            stats.append(geo.check_pose(maps, poses[n], K, verts, faces, cf, nf, uvf, 0.3 if uvf is not None else None,
                                        None if bbox is None else bbox[n], quad=quad))
        except AssertionError as e:
            raise AssertionError(f"pose {n}: {e}") from None
    s = geo.summarize(stats)
    print({k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in s.items()})
    return s


@pytest.mark.parametrize("textured", [False, True])
def test_grazing_quad_full_frames(textured):
    """480 x 640, 120 poses: the automatic chunks hold poses 0-53, 54-107 and 108-119."""
    H, W, N = 480, 640, 120
    assert KEY_BUDGET // (8 * H * W) == 54
    v, f = geo.grazing_quad()
    poses = geo.quad_poses(N, seed=11 + textured)
    mt, cf, nf, uvf = _mesh_tensors(v, f, seed=3, textured=textured)
    out = _render_checked(mt, poses, geo.K_FRAME, H, W)
    s = _check_all(out, poses, geo.K_FRAME, v, f, cf, nf, uvf, quad=True)
    assert s["covered"] > 50000  # the smallest of the poses' covered sets


def _torus():
    from pedp_hip import synth

    v, t, _ = synth.bumpy_torus(250, 200)   # the bench_100k torus, scaled as in test_render_gpu.py
    return (v * 0.001).astype(np.float32), t.astype(np.int32)


def _torus_poses(n, seed, z=0.35):
    from pedp_hip import synth

    rng = np.random.default_rng(seed)
    out = np.empty((n, 4, 4), np.float32)
    for i in range(n):
        T = np.eye(4)
        T[:3, :3] = synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.pi))
        T[:3, 3] = [rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), z + rng.uniform(-0.05, 0.05)]
        out[i] = T
    return out


def test_torus_refiner_crops():
    """252 poses at 160 x 160 through the crop windows' bbox2d (one chunk)."""
    from pedp_hip.crop import _crop_window

    v, t = _torus()
    K = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
    N, S = 252, 160
    poses = _torus_poses(N, seed=5)
    diameter = float(np.linalg.norm(v.max(0) - v.min(0)))
    _, bbox = _crop_window(torch.as_tensor(poses, device="cuda"), K, diameter * 1.4 / 2, S, S, (S - 1, S - 1), True)
    bbox = bbox.cpu().numpy()
    assert np.isfinite(bbox).all() and (bbox[:, 2] > bbox[:, 0]).all() and (bbox[:, 3] > bbox[:, 1]).all()
    mt, cf, nf, _ = _mesh_tensors(v, t, seed=6)
    out = _render_checked(mt, poses, K, 480, 640, bbox=bbox, output_size=(S, S))
    s = _check_all(out, poses, K, v, t, cf, nf, bbox=bbox)
    assert s["covered"] > 2000


def test_torus_full_frames():
    """60 frames at 480 x 640: two automatic chunks (54 + 6)."""
    v, t = _torus()
    K = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
    poses = _torus_poses(60, seed=7)
    mt, cf, nf, _ = _mesh_tensors(v, t, seed=8)
    out = _render_checked(mt, poses, K, 480, 640)
    s = _check_all(out, poses, K, v, t, cf, nf)
    assert s["covered"] > 5000
