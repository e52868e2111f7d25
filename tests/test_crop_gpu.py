"""The crop kernels on the device (csrc/pedp_crop.hip through crop.py): warp_perspective and the crop windows bit-equal
to the numpy contract (tests/_crop_ref.py), the fused refiner and scorer crop batches bit-equal to the unfused
composition of the package's own pieces, determinism, streams and bad shapes."""
import numpy as np
import pytest

import _crop_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H_, W_, CROP = 480, 640, 160
K_ = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ"


def _homographies(n, H, W, h, w, seed):
    """Source pixel -> destination pixel maps that bring most of an H x W source into an h x w output, with
    perspective terms."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 3, 3), np.float32)
    for i in range(n):
        s = rng.uniform(0.6, 1.2) * min(h / H, w / W) * 1.3
        A = np.eye(3)
        A[:2, :2] = s * (np.eye(2) + rng.normal(0, 0.1, (2, 2)))
        A[:2, 2] = [rng.uniform(-0.2, 0.3) * w, rng.uniform(-0.2, 0.3) * h]
        A[2, :2] = rng.normal(0, 0.3 / max(H, W), 2)
        out[i] = A
    return out


def _warp_case(B, C, dtype, layout, H, W, seed):
    rng = np.random.default_rng(seed)
    if dtype == "u8":
        frame = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    else:
        frame = rng.normal(0, 10, (H, W, C)).astype(np.float32)
    t = torch.as_tensor(frame, device="cuda")
    if layout == "expand":          # the reference's rgb.permute(2, 0, 1)[None].expand(B, -1, -1, -1)
        src = t.permute(2, 0, 1)[None].expand(B, -1, -1, -1)
        ref_src = frame.transpose(2, 0, 1)[None]
    else:                            # B images, channel-last storage behind a permuted view
        imgs = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8) if dtype == "u8" else \
            rng.normal(0, 10, (B, H, W, C)).astype(np.float32)
        src = torch.as_tensor(imgs, device="cuda").permute(0, 3, 1, 2)
        ref_src = imgs.transpose(0, 3, 1, 2)
    return src, ref_src


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("C,dtype,layout", [(3, "u8", "expand"), (1, "f32", "expand"), (3, "f32", "channels_last"),
                                            (1, "u8", "channels_last")])
def test_warp_bit_equal_to_contract(mode, align, C, dtype, layout):
    from pedp_hip.compat import warp_perspective

    H, W, h, w = 37, 53, 29, 41       # dsize != source size, odd sizes
    for B in (1, 7):
        src, ref_src = _warp_case(B, C, dtype, layout, H, W, seed=B + C)
        M = _homographies(B, H, W, h, w, seed=B)
        got = warp_perspective(src, torch.as_tensor(M, device="cuda"), (h, w), mode=mode, align_corners=align)
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (B, C, h, w)
        _assert_bits(got, ref.warp(ref_src, M, (h, w), mode, align), f"B={B}")


@pytest.mark.parametrize("B", [252, 600])
def test_warp_crop_sizes(B):
    """The crop step's shapes: 160 x 160 windows of a 480 x 640 uint8 frame (expanded) and of float32 maps."""
    from pedp_hip.compat import warp_perspective

    rng = np.random.default_rng(B)
    frame = rng.integers(0, 256, (H_, W_, 3), dtype=np.uint8)
    P = _poses(B, seed=B)
    tf, _ = ref.crop_window(P, K_, np.float32(0.1 * 1.4 / 2), CROP, CROP)
    tft = torch.as_tensor(tf, device="cuda")
    src = torch.as_tensor(frame, device="cuda").permute(2, 0, 1)[None].expand(B, -1, -1, -1)
    sel = rng.choice(B, 12, replace=False)
    for mode in ("bilinear", "nearest"):
        got = warp_perspective(src, tft, (CROP, CROP), mode=mode, align_corners=False)
        want = ref.warp(frame.transpose(2, 0, 1)[None], tf[sel], (CROP, CROP), mode, False)
        _assert_bits(got[torch.as_tensor(sel, device="cuda")], want, mode)


def test_warp_host_memory_and_singular():
    from pedp_hip.compat import warp_perspective

    src, ref_src = _warp_case(3, 3, "f32", "channels_last", 20, 30, seed=1)
    M = _homographies(3, 20, 30, 16, 24, seed=2)
    M[1] = 0                          # singular: zeros
    M[2, 0, 0] = np.nan               # non-finite: zeros
    dev = warp_perspective(src, torch.as_tensor(M, device="cuda"), (16, 24), mode="bilinear", align_corners=False)
    host = warp_perspective(ref_src, M, (16, 24), mode="bilinear", align_corners=False)
    assert isinstance(host, np.ndarray)
    _assert_bits(dev, host, "device vs host")
    _assert_bits(host, ref.warp(ref_src, M, (16, 24), "bilinear", False), "host vs contract")
    assert not host[1:].any()


def _poses(n, seed=0, z=0.5):
    from pedp_hip import synth

    rng = np.random.default_rng(seed)
    out = np.empty((n, 4, 4), np.float32)
    for i in range(n):
        T = np.eye(4)
        T[:3, :3] = synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.pi))
        T[:3, 3] = [rng.uniform(-0.08, 0.08), rng.uniform(-0.06, 0.06), z + rng.uniform(-0.1, 0.1)]
        out[i] = T
    return out


def test_crop_window_equals_restatement():
    from pedp_hip.crop import _crop_window

    B = 600
    P = _poses(B, seed=4)
    radius = 0.1 * 1.4 / 2
    tf, bb = _crop_window(torch.as_tensor(P, device="cuda"), K_, radius, CROP, CROP, (CROP - 1, CROP - 1), True)
    tf_r, bb_r = ref.crop_window(P, K_, np.float32(radius), CROP, CROP, (CROP - 1, CROP - 1))
    # poses whose window edge lies within 1e-3 px of a rounding tie: a different order of the float32 products
    # (an FMA in a GEMM) could move their window; the contract's order is fixed and these are only counted
    t = P[:, :3, 3].astype(np.float64)
    cu = K_[0, 0] * t[:, 0] / t[:, 2] + K_[0, 2]
    rad = K_[0, 0] * radius / t[:, 2]
    frac = np.abs(np.modf(cu - rad)[0] % 1 - 0.5)
    print(f"tie-adjacent poses: {int((frac < 1e-3).sum())} of {B}")
    _assert_bits(tf, tf_r, "tf_to_crops")
    _assert_bits(bb, bb_r, "bbox2d")
    from pedp_hip.compat import compute_crop_window_tf_batch

    tf2 = compute_crop_window_tf_batch(poses=torch.as_tensor(P, device="cuda"), K=K_, crop_ratio=1.4, out_size=(CROP, CROP),
                                       method="box_3d", mesh_diameter=0.1)
    _assert_bits(tf2, tf_r, "compute_crop_window_tf_batch")

    # Utils.py:577-621 restated in torch on the device with K in float32: the same windows and scales (the scale is
    # `out_size[0] / (right - left)`, a number over a tensor) except where a GEMM's products move a tie-adjacent edge
    Pt = torch.as_tensor(P, device="cuda")
    Kt = torch.as_tensor(K_.astype(np.float32), device="cuda")
    r = radius
    offsets = torch.tensor([0, 0, 0, r, 0, 0, -r, 0, 0, 0, r, 0, 0, -r, 0], device="cuda", dtype=torch.float32).reshape(-1, 3)
    pts = Pt[:, :3, 3].reshape(-1, 1, 3) + offsets.reshape(1, -1, 3)
    projected = (Kt @ pts.reshape(-1, 3).T).T
    uvs = (projected[:, :2] / projected[:, 2:3]).reshape(B, -1, 2)
    center = uvs[:, 0]
    rd = torch.abs(uvs - center.reshape(-1, 1, 2)).reshape(B, -1).max(axis=-1)[0].reshape(-1)
    edges = torch.stack([center[:, 0] - rd, center[:, 0] + rd, center[:, 1] - rd, center[:, 1] + rd], 1)
    left, right, top, bottom = edges.round().unbind(1)
    t0 = torch.eye(3, device="cuda")[None].expand(B, -1, -1).contiguous()
    t0[:, 0, 2], t0[:, 1, 2] = -left, -top
    n0 = torch.eye(3, device="cuda")[None].expand(B, -1, -1).contiguous()
    n0[:, 0, 0], n0[:, 1, 1] = CROP / (right - left), CROP / (bottom - top)
    tf_t = (n0 @ t0).cpu().numpy()
    tie = (torch.abs(edges - edges.floor() - 0.5) < 1e-3).any(1).cpu().numpy()
    differ = (tf_t.reshape(B, 9).view(np.uint32) != tf_r.reshape(B, 9).view(np.uint32)).any(1)
    assert not (differ & ~tie).any(), f"{int((differ & ~tie).sum())} windows differ from torch's away from a tie"
    print(f"windows differing from torch's: {int(differ.sum())}, all tie-adjacent")


# ---------------------------------------------------------------- fused crop batches

def _scene():
    """A torus in a 480 x 640 frame: rgb (uint8), depth and xyz / normal maps from one render of the true pose."""
    from pedp_hip import synth
    from pedp_hip.compat import depth2xyzmap_batch, make_mesh_tensors, nvdiffrast_render  # noqa: F401

    v, t, n = synth.bumpy_torus(60, 40)
    v = (v * 0.0008).astype(np.float32)
    rng = np.random.default_rng(0)
    mt = {"pos": torch.as_tensor(v, device="cuda"), "faces": torch.as_tensor(t.astype(np.int32), device="cuda"),
          "vnormals": torch.as_tensor(n.astype(np.float32), device="cuda"),
          "vertex_color": torch.as_tensor(rng.random((len(v), 3), dtype=np.float32), device="cuda")}
    diameter = float(np.linalg.norm(v.max(0) - v.min(0)))
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.01, -0.01, 0.5]
    extra = {}
    color, depth, normal = nvdiffrast_render(K=K_, H=H_, W=W_, ob_in_cams=torch.as_tensor(T[None], device="cuda"),
                                             get_normal=True, mesh_tensors=mt, extra=extra)
    rgb = (color[0] * 255).clamp(0, 255).to(torch.uint8).cpu().numpy()
    depth = depth[0] + torch.as_tensor(rng.normal(0, 0.002, (H_, W_)).astype(np.float32), device="cuda") * (depth[0] > 0)
    xyz = depth2xyzmap_batch(depth[None], K_.astype(np.float32)[None], zfar=np.inf)[0]
    return mt, diameter, rgb, depth, xyz, normal[0], T


def _hypotheses(B, T, seed):
    from pedp_hip import synth

    rng = np.random.default_rng(seed)
    out = np.repeat(T[None], B, 0).astype(np.float32)
    for i in range(B):
        out[i, :3, :3] = synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.pi)).astype(np.float32)
        out[i, :3, 3] += rng.normal(0, 0.01, 3).astype(np.float32)
    return out


def _transform(xyz, poseA, normalize, z_invalid, diameter):
    """transform_batch's xyz arithmetic, restated in torch (h5_dataset.py:79-116, :137-180)."""
    B = len(xyz)
    invalid = xyz[:, 2:3] < z_invalid
    out = xyz - poseA[:, :3, 3].reshape(B, 3, 1, 1)
    if normalize:
        radius = torch.ones(B, dtype=torch.float32, device="cuda") * diameter / 2
        out = out * (1 / radius.reshape(B, 1, 1, 1))
        invalid = invalid.expand(B, 3, -1, -1) | (torch.abs(out) >= 2)
        out[invalid] = 0
    return out


def _unfused(variant, poses, scene, normalize, use_normal):
    """The reference's crop-batch composition on the package's own pieces (crop windows, renderer, warp_perspective,
    depth2xyzmap_batch) and a torch restatement of transform_batch."""
    from pedp_hip.compat import depth2xyzmap_batch, nvdiffrast_render, warp_perspective
    from pedp_hip.crop import _crop_window

    mt, diameter, rgb, depth, xyz, normal, _ = scene
    B = len(poses)
    poseA = torch.as_tensor(poses, device="cuda")
    tf, bbox = _crop_window(poseA, K_, diameter * 1.4 / 2, CROP, CROP, (CROP - 1, CROP - 1), True)
    extra = {}
    rgb_r, depth_r, normal_r = nvdiffrast_render(K=K_, H=H_, W=W_, ob_in_cams=poseA, get_normal=use_normal, mesh_tensors=mt,
                                                 output_size=(CROP, CROP), bbox2d=bbox, use_light=True, extra=extra)
    ds = (CROP, CROP)
    out = {"rgbAs": (rgb_r.permute(0, 3, 1, 2) * 255) / 255.0}
    rgbt = torch.as_tensor(rgb, dtype=torch.float, device="cuda").permute(2, 0, 1)[None].expand(B, -1, -1, -1)
    out["rgbBs"] = warp_perspective(rgbt, tf, dsize=ds, mode="bilinear", align_corners=False) / 255.0
    z_inv = 0.1 if variant == 1 else 0.001
    out["xyz_mapAs"] = _transform(extra["xyz_map"].permute(0, 3, 1, 2), poseA, normalize, z_inv, diameter)
    if variant == 0:
        xB = warp_perspective(xyz.permute(2, 0, 1)[None].expand(B, -1, -1, -1), tf, dsize=ds, mode="nearest", align_corners=False)
        if use_normal:
            out["normalAs"] = warp_perspective(normal_r.permute(0, 3, 1, 2), tf, dsize=ds, mode="nearest", align_corners=False)
            out["normalBs"] = warp_perspective(normal.permute(2, 0, 1)[None].expand(B, -1, -1, -1), tf, dsize=ds, mode="nearest",
                                               align_corners=False)
    else:
        dB = warp_perspective(depth[None, None].expand(B, -1, -1, -1), tf, dsize=ds, mode="nearest", align_corners=False)
        out["depthBs"], out["depthAs"] = dB, depth_r[..., None].permute(0, 3, 1, 2)
        c2o = torch.as_tensor(ref.crop_to_ori(tf.cpu().numpy()), device="cuda")
        d_ori = warp_perspective(dB, c2o, dsize=(H_, W_), mode="nearest", align_corners=False)
        Ks = np.repeat(K_.astype(np.float32)[None], B, 0)
        x_ori = depth2xyzmap_batch(d_ori[:, 0], Ks, zfar=np.inf).permute(0, 3, 1, 2)
        xB = warp_perspective(x_ori, tf, dsize=ds, mode="nearest", align_corners=False)
    out["xyz_mapBs"] = _transform(xB, poseA, normalize, z_inv, diameter)
    out["tf_to_crops"] = tf
    return out


class _Cfg(dict):
    pass


class _Dataset:
    def __init__(self, normalize):
        self.cfg = {"normalize_xyz": normalize}


@pytest.fixture(scope="module")
def scene():
    return _scene()


def _fused(variant, poses, scene, normalize, use_normal, **kw):
    from pedp_hip.compat import make_crop_data_batch, make_score_crop_data_batch

    mt, diameter, rgb, depth, xyz, normal, _ = scene
    cfg = _Cfg(input_resize=(CROP, CROP), use_normal=use_normal)
    poses_t = torch.as_tensor(poses, device="cuda")
    if variant == 0:
        return make_crop_data_batch((CROP, CROP), poses_t, None, torch.as_tensor(rgb, dtype=torch.float, device="cuda"), depth,
                                    K_, 1.4, xyz, normal_map=normal, mesh_diameter=diameter, cfg=cfg, mesh_tensors=mt,
                                    dataset=_Dataset(normalize), **kw)
    return make_score_crop_data_batch((CROP, CROP), poses_t, None, rgb, depth.cpu().numpy(), K_, 1.4, mesh_diameter=diameter,
                                      mesh_tensors=mt, dataset=_Dataset(normalize), cfg=cfg, **kw)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("use_normal", [False, True])
def test_refiner_batch_equals_unfused(scene, normalize, use_normal):
    poses = _hypotheses(64, scene[-1], seed=1)
    got = _fused(0, poses, scene, normalize, use_normal)
    want = _unfused(0, poses, scene, normalize, use_normal)
    for k, v in want.items():
        _assert_bits(getattr(got, k), v, k)
    assert got.depthAs is None and got.depthBs is None
    if not use_normal:
        assert got.normalAs is None and got.normalBs is None
    assert float(got.xyz_mapBs.abs().sum()) > 0 and float(got.rgbBs.sum()) > 0
    assert tuple(got.Ks.shape) == (1, 3, 3) and tuple(got.mesh_diameters.shape) == (64,)


@pytest.mark.parametrize("normalize", [True, False])
def test_scorer_batch_equals_unfused_round_trip(scene, normalize):
    poses = _hypotheses(8, scene[-1], seed=2)
    got = _fused(1, poses, scene, normalize, False)
    want = _unfused(1, poses, scene, normalize, False)
    for k, v in want.items():
        _assert_bits(getattr(got, k), v, k)
    assert tuple(got.Ks.shape) == (8, 3, 3)
    valid = (got.xyz_mapBs != 0).any(1)
    assert int(valid.sum()) > 1000, "the round trip left too few valid pixels to test"


def test_batches_are_deterministic_and_take_the_callers_class(scene):
    class Holder:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    poses = _hypotheses(252, scene[-1], seed=3)
    a = _fused(1, poses, scene, True, False)
    b = _fused(1, poses, scene, True, False, batch_cls=Holder)
    assert isinstance(b, Holder)
    for k in ("rgbAs", "rgbBs", "depthBs", "xyz_mapAs", "xyz_mapBs", "tf_to_crops"):
        _assert_bits(getattr(a, k), getattr(b, k), k)
    # what predict_pose_refine.py:212 does with it
    assert tuple(a.tf_to_crops[0:4].inverse().shape) == (4, 3, 3)


def test_batches_run_on_the_callers_stream_without_a_host_wait(scene):
    """On a side stream, the calls return while the stream is still busy with work their inputs depend on, and their
    results are those of the default stream: they were enqueued on the caller's stream, not run on another one with a
    host wait around them."""
    from pedp_hip.compat import make_crop_data_batch, warp_perspective

    mt, diameter, rgb, depth, xyz, normal, T = scene
    poses = torch.as_tensor(_hypotheses(32, T, seed=4), device="cuda")
    rgb_t = torch.as_tensor(rgb, device="cuda")
    cfg = _Cfg(input_resize=(CROP, CROP), use_normal=True)
    src = torch.rand(2, 3, 50, 60, device="cuda")
    M = torch.as_tensor(_homographies(2, 50, 60, 40, 40, 9), device="cuda")

    def crop(p):
        return make_crop_data_batch((CROP, CROP), p, None, rgb_t, depth, K_, 1.4, xyz, normal_map=normal,
                                    mesh_diameter=diameter, cfg=cfg, mesh_tensors=mt, dataset=_Dataset(True))

    base, base_w = crop(poses), warp_perspective(src, M, (40, 40))
    a = torch.randn(4096, 4096, device="cuda")
    c = torch.empty_like(a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        crop(poses), warp_perspective(src, M, (40, 40))  # this stream's context and workspaces
        s.synchronize()
        for _ in range(150):                             # about 0.1 s of work ahead of the inputs
            torch.matmul(a, a, out=c)
        ready = torch.isfinite(c[0, 0])
        p2, src2 = torch.where(ready, poses, poses), torch.where(ready, src, src)  # exact copies, written after it
        got = crop(p2)
        got_w = warp_perspective(src2, M, (40, 40))
        pending = not s.query()
    s.synchronize()
    assert pending, "the calls waited on the host for the caller's stream"
    for k in ("rgbAs", "rgbBs", "xyz_mapAs", "xyz_mapBs", "normalAs", "normalBs", "tf_to_crops"):
        _assert_bits(getattr(got, k), getattr(base, k), k)
    _assert_bits(got_w, base_w, "warp on a side stream")


def test_bad_shapes_raise(scene):
    from pedp_hip import _lib
    from pedp_hip.compat import make_crop_data_batch, warp_perspective

    src = torch.zeros(2, 3, 10, 10, device="cuda")
    eye = torch.eye(3, device="cuda")[None]
    with pytest.raises(_lib.PedpError):
        warp_perspective(src[0], eye, (4, 4))                       # not N x C x H x W
    with pytest.raises(_lib.PedpError):
        warp_perspective(src, eye.expand(3, 3, 3), (4, 4))          # 2 images, 3 matrices
    with pytest.raises(_lib.PedpError):
        warp_perspective(src, torch.zeros(2, 2, 3, device="cuda"), (4, 4))
    with pytest.raises(_lib.PedpError):
        warp_perspective(src, eye.expand(2, 3, 3), (0, 4))
    mt, diameter, rgb, depth, xyz, normal, T = scene
    cfg = _Cfg(input_resize=(CROP, CROP), use_normal=False)
    P = torch.as_tensor(T[None], device="cuda")
    with pytest.raises(NotImplementedError):
        make_crop_data_batch((CROP, 128), P, None, rgb, depth, K_, 1.4, xyz, mesh_diameter=diameter, cfg=cfg, mesh_tensors=mt)
    with pytest.raises(_lib.PedpError):
        make_crop_data_batch((CROP, CROP), P, None, rgb[..., :2], depth, K_, 1.4, xyz, mesh_diameter=diameter, cfg=cfg,
                             mesh_tensors=mt)
    with pytest.raises(_lib.PedpError):
        make_crop_data_batch((CROP, CROP), P, None, rgb, depth, K_, 1.4, xyz[:100], mesh_diameter=diameter, cfg=cfg,
                             mesh_tensors=mt)


# ---------------------------------------------------------------- degenerate hypotheses

def _assert_bits_nan(got, want, what):
    """Bit equality where both are numbers; a NaN where the other is a NaN (of any payload)."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    gn, wn = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    assert np.array_equal(gn, wn), f"{what}: NaN at {int((gn != wn).sum())} differing places"
    bad = (g != w) & ~gn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ"


# kind -> the translation it gets (the rotation stays the hypothesis')
DEGENERATE = {
    "z_zero": [0.01, -0.01, 0.0],
    "z_negative": [0.01, -0.01, -0.3],
    "z_tiny": [0.01, -0.01, 1e-30],
    "x_nan": [np.nan, -0.01, 0.5],
    "x_inf": [np.inf, -0.01, 0.5],
    "x_minus_inf": [-np.inf, -0.01, 0.5],
    "z_nan": [0.01, -0.01, np.nan],
    "x_overflow": [1e37, -0.01, 0.5],                         # u overflows to inf, v stays finite: the radius is NaN
    "off_frame": [50 * W_ * 0.5 / K_[0, 0], -0.01, 0.5],      # the centre 50 frame widths right of the image
    "sub_pixel": [0.3, 0.3, 1e4],                              # radius << 0.5 px: right == left after rounding
}
# the crop window is not finite: tf_to_crops holds NaN, the maps are "singular" and the render's bbox2d is NaN
NONFINITE = ("z_zero", "x_nan", "x_inf", "x_minus_inf", "z_nan", "x_overflow", "sub_pixel")


def _mixed_batch(T):
    poses = _hypotheses(64, T, seed=21)
    slots = {k: 3 + 6 * i for i, k in enumerate(DEGENERATE)}
    for k, s in slots.items():
        poses[s, :3, 3] = DEGENERATE[k]
    return poses, slots


def test_degenerate_crop_windows(scene):
    from pedp_hip.compat import compute_crop_window_tf_batch
    from pedp_hip.crop import _crop_window

    mt, diameter, rgb, depth, xyz, normal, T = scene
    poses, slots = _mixed_batch(T)
    r = diameter * 1.4 / 2
    tf_r, bb_r = ref.crop_window(poses, K_, np.float32(r), CROP, CROP, (CROP - 1, CROP - 1))
    for k in NONFINITE:
        assert np.isnan(tf_r[slots[k]]).any() and np.isnan(bb_r[slots[k]]).all(), k
    # torch.max's NaN: without it the finite v extent would give x_overflow a finite second row
    assert np.isnan(tf_r[slots["x_overflow"], 1]).all()
    for k in ("z_negative", "z_tiny", "off_frame"):
        assert np.isfinite(tf_r[slots[k]]).all(), k
    pt = torch.as_tensor(poses, device="cuda")
    tf, bb = _crop_window(pt, K_, r, CROP, CROP, (CROP - 1, CROP - 1), True)
    _assert_bits_nan(tf, tf_r, "tf_to_crops")
    _assert_bits_nan(bb, bb_r, "bbox2d")
    tf2 = compute_crop_window_tf_batch(poses=pt, K=K_, crop_ratio=1.4, out_size=(CROP, CROP), method="box_3d", mesh_diameter=diameter)
    _assert_bits_nan(tf2, tf_r, "compute_crop_window_tf_batch")
    tfh, bbh = _crop_window(poses, K_, r, CROP, CROP, (CROP - 1, CROP - 1), True)
    _assert_bits_nan(tfh, tf_r, "tf_to_crops (host)")
    _assert_bits_nan(bbh, bb_r, "bbox2d (host)")
    # every window under half a pixel: mesh_diameter is one number per batch, so a call of its own
    healthy = np.delete(poses, list(slots.values()), 0)
    tiny = 1e-4
    tf_r, bb_r = ref.crop_window(healthy, K_, np.float32(tiny * 1.4 / 2), CROP, CROP, (CROP - 1, CROP - 1))
    assert np.isnan(tf_r).any((1, 2)).mean() > 0.5, "too few windows collapsed to right == left"
    tf, bb = _crop_window(torch.as_tensor(healthy, device="cuda"), K_, tiny * 1.4 / 2, CROP, CROP, (CROP - 1, CROP - 1), True)
    _assert_bits_nan(tf, tf_r, "sub-pixel tf_to_crops")
    _assert_bits_nan(bb, bb_r, "sub-pixel bbox2d")
    tf2 = compute_crop_window_tf_batch(poses=torch.as_tensor(healthy, device="cuda"), K=K_, crop_ratio=1.4, out_size=(CROP, CROP),
                                       method="box_3d", mesh_diameter=tiny)
    _assert_bits_nan(tf2, tf_r, "sub-pixel compute_crop_window_tf_batch")


def _field(batch, k):
    v = getattr(batch, k) if not isinstance(batch, dict) else batch.get(k)
    return None if v is None else v.detach().cpu().numpy()


def _contract_of_degenerate(got, slots, poses, variant, normalize, use_normal):
    """What the contract gives each kind.  transform_batch of an empty pixel (xyz 0) fails the z test: 0 under
    normalize_xyz, else 0 - t per channel."""
    empty_xyz = {k: (np.zeros((3, CROP, CROP), np.float32) if normalize else
                     np.broadcast_to((np.float32(0) - poses[s, :3, 3])[:, None, None], (3, CROP, CROP)))
                 for k, s in slots.items()}
    a_side = ["rgbAs"] + (["normalAs"] if use_normal else []) + (["depthAs"] if variant == 1 else [])
    b_side = ["rgbBs"] + (["normalBs"] if use_normal else []) + (["depthBs"] if variant == 1 else [])
    for k, s in slots.items():
        empty_a = k in NONFINITE or k == "z_negative"   # no window, or the mesh behind the camera: nothing rendered
        empty_b = k in NONFINITE or k in ("z_tiny", "off_frame")  # no window, or a window that samples off the frame
        for f in (a_side if empty_a else []) + (b_side if empty_b else []):
            assert not _field(got, f)[s].any(), f"{k}: {f} not all zero"
        if empty_a:
            _assert_bits_nan(_field(got, "xyz_mapAs")[s], empty_xyz[k], f"{k}: xyz_mapAs")
        if empty_b:
            _assert_bits_nan(_field(got, "xyz_mapBs")[s], empty_xyz[k], f"{k}: xyz_mapBs")
    s = slots["off_frame"]
    assert _field(got, "rgbAs")[s].any(), "off_frame: the render inside its own window is empty"
    s = slots["z_negative"]
    assert _field(got, "rgbBs")[s].any(), "z_negative: the mirrored window samples nothing"


@pytest.mark.parametrize("variant,normalize,use_normal", [(0, True, True), (0, False, True), (1, True, False), (1, False, False)])
def test_degenerate_hypotheses_through_the_crop_batch(scene, variant, normalize, use_normal):
    poses, slots = _mixed_batch(scene[-1])
    got = _fused(variant, poses, scene, normalize, use_normal)
    want = _unfused(variant, poses, scene, normalize, use_normal)
    for k, v in want.items():
        _assert_bits_nan(getattr(got, k), v, k)
    _contract_of_degenerate(got, slots, poses, variant, normalize, use_normal)
    # no cross-talk: the healthy hypotheses equal a batch of only them
    healthy = np.setdiff1d(np.arange(len(poses)), list(slots.values()))
    alone = _fused(variant, poses[healthy], scene, normalize, use_normal)
    for k in ("rgbAs", "rgbBs", "xyz_mapAs", "xyz_mapBs", "normalAs", "normalBs", "depthAs", "depthBs", "tf_to_crops"):
        a, b = _field(got, k), _field(alone, k)
        assert (a is None) == (b is None), k
        if a is not None:
            _assert_bits(a[healthy], b, f"{k}, healthy hypotheses alone")
            assert np.isfinite(b).all(), f"{k}: a healthy hypothesis has a non-finite value"
