"""The pose kernels on the device (csrc/pedp_pose.hip through pose.py) and the packed crop batch (pedp_crop_batch_packed
through crop.py): bit equality with the numpy contract (tests/_pose_ref.py) and with numpy's norm maximum, the torch
composition within float32 tolerance, host memory, streams and bad shapes."""
import numpy as np
import pytest

import _pose_ref as ref

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


def _poses(B, rng):
    P = np.zeros((B, 4, 4), np.float32)
    P[:, :3, :3] = ref.so3_exp(rng.normal(size=(B, 3)).astype(np.float32))
    P[:, :3, 3] = rng.normal(0, 0.1, (B, 3)) + [0, 0, 0.6]
    P[:, 3, 3] = 1
    return P


def _outputs(B, width, rng):
    """Network outputs with saturated tanh (|o| > 10), exact zeros, ordinary values, and whole rows small enough that
    the rotation's squared norm falls below the 1e-4 clamp (|x| around 1e-3 and 5e-3 after tanh and rot_normalizer)."""
    o = rng.normal(0, 1.5, (B, width)).astype(np.float32)
    k = rng.choice(B * width, size=max(1, B * width // 8), replace=False)
    o.reshape(-1)[k[: len(k) // 2]] = rng.choice([-1, 1], len(k) // 2) * rng.uniform(10, 40, len(k) // 2)
    o.reshape(-1)[k[len(k) // 2:]] = 0
    rows = rng.permutation(B)[: max(1, B // 6)]
    for j, i in enumerate(rows):
        o[i] = rng.normal(0, (2e-3, 1e-2)[j % 2], width)
    return o


def _assert_bits_nan(got, want, what):
    """Bit equality where both are numbers; a NaN where the other is a NaN (of any payload)."""
    g, w = _bits(got), _bits(want)
    gn, wn = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    assert np.array_equal(gn, wn), f"{what}: NaN at {int((gn != wn).sum())} differing places"
    bad = (g != w) & ~gn
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ"


BRANCHES = [
    dict(trans_rep="tracknet", rot_rep="axis_angle", normalize_xyz=False, trans_normalizer=0.02, rot_normalizer=0.3),
    dict(trans_rep="tracknet", rot_rep="axis_angle", normalize_xyz=False, trans_normalizer=[0.02, 0.03, 0.05],
         rot_normalizer=0.3490658503988659),
    dict(trans_rep="tracknet", rot_rep="axis_angle", normalize_xyz=True, rot_normalizer=0.3, mesh_diameter=0.1834),
    dict(trans_rep="raw", rot_rep="axis_angle", normalize_xyz=False, rot_normalizer=0.5),
    dict(trans_rep="raw", rot_rep="6d", normalize_xyz=True, mesh_diameter=0.25),
    dict(trans_rep="tracknet", rot_rep="6d", normalize_xyz=False, trans_normalizer=[0.02, 0.03, 0.05]),
]


@pytest.mark.parametrize("branch", range(len(BRANCHES)))
def test_pose_update_bit_equal_to_contract(branch):
    from pedp_hip.pose import pose_update

    cfg = BRANCHES[branch]
    width = 6 if cfg["rot_rep"] == "6d" else 3
    for B in (1, 7, 252, 1025):
        rng = np.random.default_rng(B + 100 * branch)
        P, t, r = _poses(B, rng), _outputs(B, 3, rng), _outputs(B, width, rng)
        want, wtd, wrd = ref.pose_update(t, r, P, **cfg)
        dev = [torch.as_tensor(x, device="cuda") for x in (t, r, P)]
        got, td, rd = pose_update(*dev, want_deltas=True, **cfg)
        assert got.is_cuda and tuple(got.shape) == (B, 4, 4)
        _assert_bits(got, want, f"poses B={B}")
        _assert_bits(td, wtd, f"trans_delta B={B}")
        _assert_bits(rd, wrd, f"rot_mat_delta B={B}")
        host, _, _ = pose_update(t, r, P, **cfg)                 # host memory
        assert isinstance(host, np.ndarray)
        _assert_bits(host, want, f"host B={B}")


def test_pose_update_clamp_and_non_finite_values():
    """theta is clamped to 0.01 below |x| = 0.01 (on the GPU as in the contract); NaN and infinities propagate."""
    from pedp_hip.pose import pose_update

    eye = torch.eye(4, device="cuda").expand(3, 4, 4).contiguous()
    x = np.array([[1e-3, 0, 0], [5e-3, 0, 0], [0.02, 0, 0]])
    rot = torch.as_tensor(np.arctanh(x / 0.3).astype(np.float32), device="cuda")
    got, _, rd = pose_update(torch.zeros(3, 3, device="cuda"), rot, eye, trans_normalizer=0.02, rot_normalizer=0.3,
                             want_deltas=True)
    xs = (np.tanh(np.arctanh(x / 0.3).astype(np.float32).astype(np.float64)).astype(np.float32) * np.float32(0.3))[:, 0]
    s = got[:, 1, 2].cpu().numpy().astype(np.float64)                 # Rd[1, 2] = R[2, 1] = (sin t / t) x0 for x = (x0, 0, 0)
    theta = np.maximum(xs.astype(np.float64), 0.01)
    assert np.abs(s - np.sin(theta) / theta * xs).max() < 3e-9        # the clamped form (float32 rounding)
    assert abs(s[0] - np.sin(xs[0])) > 1e-8 and abs(s[1] - np.sin(xs[1])) > 1e-8
    assert abs(s[2] - np.sin(xs[2])) < 3e-9                            # above the clamp: the exact rotation
    _assert_bits(got, ref.pose_update(np.zeros((3, 3), np.float32), rot.cpu().numpy(), eye.cpu().numpy(),
                                      trans_normalizer=0.02, rot_normalizer=0.3)[0], "clamp rows")

    rng = np.random.default_rng(11)
    for cfg in BRANCHES:
        width = 6 if cfg["rot_rep"] == "6d" else 3
        B = 40
        P, t, r = _poses(B, rng), _outputs(B, 3, rng), _outputs(B, width, rng)
        t[0, 1], t[1, 2], r[2, 0], r[3, width - 1], r[4, 1] = np.nan, np.inf, np.nan, np.inf, -np.inf
        P[5, 0, 3], P[6, 1, 1] = np.nan, np.inf
        want, wtd, wrd = ref.pose_update(t, r, P, **cfg)
        got, td, rd = pose_update(*(torch.as_tensor(a, device="cuda") for a in (t, r, P)), want_deltas=True, **cfg)
        _assert_bits_nan(got, want, f"non-finite {cfg}")
        _assert_bits_nan(td, wtd, "trans_delta")
        _assert_bits_nan(rd, wrd, "rot_mat_delta")
        assert np.isnan(want[2]).any() and np.isnan(want[5]).any()


def test_pose_update_refuses_a_wrong_out():
    from pedp_hip import _lib
    from pedp_hip.pose import pose_update

    P = torch.eye(4, device="cuda").expand(6, 4, 4).contiguous()
    t = torch.zeros(6, 3, device="cuda")
    bad = [torch.empty(6, 4, 4, dtype=torch.float16, device="cuda"), torch.empty(6, 4, 4, dtype=torch.bfloat16, device="cuda"),
           torch.empty(6, 4, 4, dtype=torch.float64, device="cuda"), torch.empty(6, 4, 4),            # CPU, CUDA inputs
           torch.empty(6, 4, 8, device="cuda")[:, :, :4], torch.empty(4, 6, 4, device="cuda").transpose(0, 1),
           np.empty((6, 4, 4), np.float32), torch.empty(5, 4, 4, device="cuda")]
    for o in bad:
        with pytest.raises(_lib.PedpError):
            pose_update(t, t, P, trans_normalizer=0.02, out=o)
    with pytest.raises(_lib.PedpError):                                                          # CUDA out, host inputs
        pose_update(t.cpu().numpy(), t.cpu().numpy(), P.cpu().numpy(), out=torch.empty(6, 4, 4, device="cuda"))
    host = torch.empty(6, 4, 4)                                                                  # CPU tensor, host inputs
    got, _, _ = pose_update(t.cpu(), t.cpu(), P.cpu(), out=host)
    assert got is host and torch.equal(host, P.cpu())


def test_zero_outputs_leave_poses_unchanged_and_update_in_place():
    from pedp_hip.pose import pose_update

    rng = np.random.default_rng(5)
    P = torch.as_tensor(_poses(300, rng), device="cuda")
    z = torch.zeros(300, 3, device="cuda")
    got, _, _ = pose_update(z, z, P, trans_normalizer=0.02, rot_normalizer=0.3)
    assert torch.equal(got, P)
    # poses may be poseA itself
    t, r = (torch.as_tensor(_outputs(300, 3, rng), device="cuda") for _ in range(2))
    want, _, _ = pose_update(t, r, P, trans_normalizer=0.02, rot_normalizer=0.3)
    Q = P.clone()
    pose_update(t, r, Q, trans_normalizer=0.02, rot_normalizer=0.3, out=Q)
    _assert_bits(Q, want, "in place")


def _torch_update(t, r, P, cfg):
    """The refiner's update written in torch ops (tanh, pytorch3d's formulas, bmm, the delta composition)."""
    tn = torch.as_tensor(np.asarray(cfg.get("trans_normalizer", 1.0), np.float32).reshape(1, -1), device="cuda")
    if cfg["trans_rep"] == "tracknet" and not cfg["normalize_xyz"]:
        td = torch.tanh(t) * tn
    else:
        td = t.clone()
    if cfg["normalize_xyz"]:
        td = td * (cfg["mesh_diameter"] / 2)
    if cfg["rot_rep"] == "axis_angle":
        x = torch.tanh(r) * cfg["rot_normalizer"]
        th = (x * x).sum(1).clamp(1e-4).sqrt()
        z = torch.zeros_like(x[:, 0])
        K = torch.stack([z, -x[:, 2], x[:, 1], x[:, 2], z, -x[:, 0], -x[:, 1], x[:, 0], z], 1).view(-1, 3, 3)
        R = (th.sin() / th)[:, None, None] * K + ((1 - th.cos()) / th / th)[:, None, None] * torch.bmm(K, K) + \
            torch.eye(3, device="cuda")
    else:
        b1 = torch.nn.functional.normalize(r[:, :3], dim=-1)
        b2 = torch.nn.functional.normalize(r[:, 3:] - (b1 * r[:, 3:]).sum(-1, keepdim=True) * b1, dim=-1)
        R = torch.stack([b1, b2, torch.linalg.cross(b1, b2)], 1)
    out = P.clone()
    out[:, :3, :3] = R.transpose(1, 2) @ P[:, :3, :3]
    out[:, :3, 3] = P[:, :3, 3] + td
    return out


@pytest.mark.parametrize("branch", range(len(BRANCHES)))
def test_pose_update_close_to_torch_composition(branch):
    from pedp_hip.pose import pose_update

    cfg = BRANCHES[branch]
    rng = np.random.default_rng(40 + branch)
    B = 1024
    P = torch.as_tensor(_poses(B, rng), device="cuda")
    t = torch.as_tensor(_outputs(B, 3, rng), device="cuda")
    r = torch.as_tensor(_outputs(B, 6 if cfg["rot_rep"] == "6d" else 3, rng), device="cuda")
    got, _, _ = pose_update(t, r, P, **cfg)
    want = _torch_update(t, r, P, cfg)
    tol = torch.full((B,), 2e-6, device="cuda", dtype=torch.float64)
    if cfg["rot_rep"] == "6d":
        # Gram-Schmidt in float32 loses |a2| / |a2 - (b1.a2) b1| to cancellation when a2 nearly parallels a1: both sides
        # round differently there (torch's norm, its fused sums), so such rows get that factor of the bound
        a = r.double()
        b1 = torch.nn.functional.normalize(a[:, :3], dim=-1)
        res = a[:, 3:] - (b1 * a[:, 3:]).sum(-1, keepdim=True) * b1
        cond = a[:, 3:].norm(dim=-1) / res.norm(dim=-1).clamp_min(1e-300)
        tol = tol * cond.clamp_min(1.0)
        assert int((cond <= 2).sum()) > B // 2
    err = (got[:, :3, :3] - want[:, :3, :3]).abs().amax((1, 2)).double()
    assert bool((err <= tol).all()), f"rotation differs by {float(err.max()):.3g}"
    err = (got[:, :3, 3] - want[:, :3, 3]).abs().amax(1) / want[:, :3, 3].abs().amax(1)   # relative to each translation
    assert float(err.max()) <= 1e-6


def test_pose_update_runs_on_the_callers_stream_without_a_host_wait():
    from pedp_hip.pose import pose_update

    rng = np.random.default_rng(9)
    P = torch.as_tensor(_poses(252, rng), device="cuda")
    t, r = (torch.as_tensor(_outputs(252, 3, rng), device="cuda") for _ in range(2))
    base, _, _ = pose_update(t, r, P, trans_normalizer=0.02, rot_normalizer=0.3)
    a = torch.randn(4096, 4096, device="cuda")
    c = torch.empty_like(a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pose_update(t, r, P, trans_normalizer=0.02, rot_normalizer=0.3)   # this stream's context
        s.synchronize()
        for _ in range(150):
            torch.matmul(a, a, out=c)
        ready = torch.isfinite(c[0, 0])
        P2 = torch.where(ready, P, P)
        got, _, _ = pose_update(t, r, P2, trans_normalizer=0.02, rot_normalizer=0.3)
        pending = not s.query()
    s.synchronize()
    assert pending, "pose_update waited on the host for the caller's stream"
    _assert_bits(got, base, "side stream")


# ---------------------------------------------------------------- pair maximum

def _assert_same_double(got, want, what):
    if np.isnan(want):
        assert np.isnan(got), f"{what}: {got} (want NaN)"
    else:
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), f"{what}: {got!r} != {want!r}"


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 10000])
def test_pair_maximum_bit_equal_to_numpy(n):
    from pedp_hip.pose import max_pair_distance

    rng = np.random.default_rng(n)
    p = rng.normal(0, 0.05, (n, 3)) * [1.0, 0.7, 0.3] + [0.2, -0.1, 0.5]
    want = ref.max_pair_distance(p)
    _assert_same_double(max_pair_distance(p), want, f"host n={n}")
    _assert_same_double(max_pair_distance(torch.as_tensor(p, device="cuda")), want, f"device n={n}")


def test_pair_maximum_edge_cases():
    from pedp_hip import _lib
    from pedp_hip.pose import max_pair_distance

    rng = np.random.default_rng(7)
    assert max_pair_distance(np.array([[1.0, 2.0, 3.0]])) == 0.0
    dup = np.repeat(rng.normal(size=(1, 3)), 300, 0)
    assert max_pair_distance(dup) == 0.0
    p = rng.normal(size=(700, 3))
    p[10], p[400] = p[600], p[3]                                  # duplicates among others
    _assert_same_double(max_pair_distance(p), ref.max_pair_distance(p), "duplicates")
    far = p * 1e-3 + 1e6                                          # large offset, small spread
    _assert_same_double(max_pair_distance(far), ref.max_pair_distance(far), "offset")
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[517, 2] = bad
        assert np.isnan(ref.max_pair_distance(q))
        assert np.isnan(max_pair_distance(q)), f"{bad}"
        assert np.isnan(max_pair_distance(torch.as_tensor(q, device="cuda"))), f"{bad} on the device"
    with pytest.raises(_lib.PedpError):
        max_pair_distance(np.zeros((0, 3)))
    with pytest.raises(_lib.PedpError):
        max_pair_distance(np.zeros((5, 2)))


def test_pose_update_bad_shapes_raise():
    from pedp_hip import _lib
    from pedp_hip.pose import pose_update

    P = torch.eye(4, device="cuda").expand(5, 4, 4).contiguous()
    t = torch.zeros(5, 3, device="cuda")
    with pytest.raises(_lib.PedpError):
        pose_update(t, torch.zeros(5, 3, device="cuda"), P, rot_rep="6d")
    with pytest.raises(_lib.PedpError):
        pose_update(torch.zeros(4, 3, device="cuda"), t, P)
    with pytest.raises(_lib.PedpError):
        pose_update(t, t, P[:, :3])
    with pytest.raises(NotImplementedError):
        pose_update(t, t, P, trans_rep="deepim")


# ---------------------------------------------------------------- packed crop batch

def _scene():
    from pedp_hip import synth
    from pedp_hip.compat import depth2xyzmap_batch, nvdiffrast_render

    v, t, n = synth.bumpy_torus(60, 40)
    v = (v * 0.0008).astype(np.float32)
    rng = np.random.default_rng(0)
    mt = {"pos": torch.as_tensor(v, device="cuda"), "faces": torch.as_tensor(t.astype(np.int32), device="cuda"),
          "vnormals": torch.as_tensor(n.astype(np.float32), device="cuda"),
          "vertex_color": torch.as_tensor(rng.random((len(v), 3), dtype=np.float32), device="cuda")}
    diameter = float(np.linalg.norm(v.max(0) - v.min(0)))
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.01, -0.01, 0.5]
    color, depth, _ = nvdiffrast_render(K=K_, H=H_, W=W_, ob_in_cams=torch.as_tensor(T[None], device="cuda"), mesh_tensors=mt)
    rgb = (color[0] * 255).clamp(0, 255).to(torch.uint8)
    depth = depth[0] + torch.as_tensor(rng.normal(0, 0.002, (H_, W_)).astype(np.float32), device="cuda") * (depth[0] > 0)
    xyz = depth2xyzmap_batch(depth[None], K_.astype(np.float32)[None], zfar=np.inf)[0]
    P = np.repeat(T[None], 252, 0)
    P[:, :3, :3] = ref.so3_exp(rng.normal(size=(252, 3)).astype(np.float32))
    P[:, :3, 3] += rng.normal(0, 0.01, (252, 3))
    return mt, diameter, rgb, depth, xyz, torch.as_tensor(P, device="cuda")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("normalize", [False, True])
def test_packed_crops_equal_concatenated_fields(variant, normalize):
    from pedp_hip.crop import _crop_batch

    mt, diameter, rgb, depth, xyz, P = _scene()
    cfg = {"input_resize": (CROP, CROP), "use_normal": False, "normalize_xyz": normalize}

    def batch(packed):
        return _crop_batch(variant, (CROP, CROP), P, None, rgb, depth, K_, 1.2, xyz if variant == 0 else None, None, diameter,
                           cfg, None, mt, None, None, packed=packed)

    plain, packed = batch(False), batch(True)
    assert tuple(packed.A.shape) == (252, 6, CROP, CROP) and packed.A.is_contiguous() and packed.B.is_contiguous()
    _assert_bits(packed.A, torch.cat([plain.rgbAs, plain.xyz_mapAs], 1), "A")
    _assert_bits(packed.B, torch.cat([plain.rgbBs, plain.xyz_mapBs], 1), "B")
    for k in ("rgbAs", "rgbBs", "xyz_mapAs", "xyz_mapBs", "tf_to_crops"):
        _assert_bits(getattr(packed, k), getattr(plain, k), k)
    if variant == 1:
        _assert_bits(packed.depthBs, plain.depthBs, "depthBs")
    assert float(packed.B[:, 3:].abs().sum()) > 0


def test_packed_crops_from_host_memory():
    """pedp_crop_batch_packed with every array in host memory (staged through the context) equals the device call and
    pedp_crop_batch's host call concatenated."""
    import ctypes as C

    from pedp_hip import _lib
    from pedp_hip.crop import _crop_window, _image, crop_pass
    from pedp_hip.compat import nvdiffrast_render

    mt, diameter, rgb, depth, xyz, P = _scene()
    P = P[:37].contiguous()
    B = int(P.shape[0])
    tf, bbox = _crop_window(P, K_, diameter * 1.2 / 2, CROP, CROP, (CROP - 1, CROP - 1), True)
    extra = {}
    rgb_r, _, _ = nvdiffrast_render(K=K_, H=H_, W=W_, ob_in_cams=P, mesh_tensors=mt, output_size=(CROP, CROP), bbox2d=bbox,
                                    use_light=True, extra=extra)
    dev = crop_pass(0, tf, P, K_, diameter, rgb, rgb_r, extra["xyz_map"], xyz_map=xyz, normalize_xyz=True, packed=True)
    h = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in
         dict(tf=tf, P=P, rgb=rgb, xyz=xyz, rgb_r=rgb_r, xyz_r=extra["xyz_map"]).items()}
    prm = _lib.CropParams()
    prm.variant, prm.normalize_xyz, prm.use_normal, prm.B = 0, 1, 0, B
    prm.H, prm.W, prm.out_h, prm.out_w = H_, W_, CROP, CROP
    prm.K[:] = K_.astype(np.float32).reshape(9).tolist()
    prm.mesh_diameter = float(np.float32(diameter))
    im_rgb, im_xyz = _image(h["rgb"], "HWC"), _image(h["xyz"], "HWC")
    lib, ctx = _lib.load(), _lib.default_context()
    A, Bo = np.full((B, 6, CROP, CROP), np.nan, np.float32), np.full((B, 6, CROP, CROP), np.nan, np.float32)
    _lib.check(lib.pedp_crop_batch_packed(ctx._h, C.byref(prm), _lib._ptr(h["tf"]), _lib._ptr(h["P"]), C.byref(im_rgb),
                                          C.byref(im_xyz), None, None, _lib._ptr(h["rgb_r"]), _lib._ptr(h["xyz_r"]), _lib.HOST,
                                          _lib._ptr(A), _lib._ptr(Bo), None, None), "pedp_crop_batch_packed")
    plain = {k: np.empty((B, 3, CROP, CROP), np.float32) for k in ("rgbA", "rgbB", "xyzA", "xyzB")}
    _lib.check(lib.pedp_crop_batch(ctx._h, C.byref(prm), _lib._ptr(h["tf"]), _lib._ptr(h["P"]), C.byref(im_rgb),
                                   C.byref(im_xyz), None, None, _lib._ptr(h["rgb_r"]), _lib._ptr(h["xyz_r"]), _lib.HOST,
                                   *(_lib._ptr(plain[k]) for k in ("rgbA", "rgbB", "xyzA", "xyzB")), None, None),
               "pedp_crop_batch")
    _assert_bits(A, dev["A"], "A host vs device")
    _assert_bits(Bo, dev["B"], "B host vs device")
    _assert_bits(A, np.concatenate([plain["rgbA"], plain["xyzA"]], 1), "A vs pedp_crop_batch")
    _assert_bits(Bo, np.concatenate([plain["rgbB"], plain["xyzB"]], 1), "B vs pedp_crop_batch")
