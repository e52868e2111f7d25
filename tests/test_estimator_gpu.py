"""The estimator on the device: pedp_mask_depth_stats against numpy (every field equal, the median by bit pattern), the
predictors' loops and register / track_one against the same steps composed by hand from the package's public pieces
(tests/_estimator_ref.py).  Equality is exact everywhere; nothing is compared with the functions under test themselves."""
import numpy as np
import pytest

import _estimator_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K_ = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
SIZES = [(1, 1), (37, 53), (576, 640), (720, 1280)]
FIELDS = ("n_pos", "n_valid", "n_med", "umin", "umax", "vmin", "vmax")


@pytest.fixture(autouse=True)
def _fixed_switches():
    """register calls set_seed, which also sets cudnn's switches: set them up front so that a hand-composed run before the
    first register and one after it pick their convolutions alike."""
    from pedp_hip.estimator import set_seed

    set_seed(0)


# ---------------------------------------------------------------- the statistics kernel

def _depth(h, w, rng, quantised):
    d = rng.uniform(0.3, 1.6, (h, w)).astype(np.float32)
    if quantised:
        d = (np.round(d * 1000) / 1000).astype(np.float32)           # millimetres: a few hundred values, heavy ties
    r = rng.random((h, w))
    d[r < 0.10] = 0
    d[(r >= 0.10) & (r < 0.13)] = -0.4
    d[(r >= 0.13) & (r < 0.15)] = np.nan
    d[(r >= 0.15) & (r < 0.16)] = np.inf
    d[(r >= 0.16) & (r < 0.17)] = 0.0009999
    d[(r >= 0.17) & (r < 0.18)] = 0.001
    return d


def _mask(h, w, rng, kind):
    yy, xx = np.mgrid[:h, :w]
    blob = ((yy - 0.45 * h) ** 2 / max(0.09 * h * h, 1) + (xx - 0.55 * w) ** 2 / max(0.06 * w * w, 1)) <= 1
    blob &= rng.random((h, w)) < 0.9
    if kind == "bool":
        return blob
    if kind == "uint8":
        return (blob * rng.choice(np.array([1, 2, 255], np.uint8), (h, w))).astype(np.uint8)
    m = np.where(blob, rng.uniform(0.1, 2.0, (h, w)), 0).astype(np.float32)
    r = rng.random((h, w))
    m[r < 0.02] = -1.5            # truthy but not positive: enters the median, not the box
    m[(r >= 0.02) & (r < 0.04)] = np.nan
    m[(r >= 0.04) & (r < 0.06)] = -0.0
    return m


def _check(depth, mask, what, device=True, host=True):
    from pedp_hip.estimator import guess_translation, mask_depth_stats

    want = ref.stats(depth, mask)
    center = ref.guess_translation(depth, mask, K_)
    runs = []
    if host:
        runs.append(("host", depth, mask))
    if device:
        runs.append(("device", torch.as_tensor(depth, device="cuda"), torch.as_tensor(mask, device="cuda")))
    for where, d, m in runs:
        got = mask_depth_stats(d, m)
        print(f"{what} [{where}]: got {got} want {want}")
        for k in FIELDS:
            assert got[k] == want[k], f"{what} [{where}] {k}: {got[k]} != {want[k]}"
        assert isinstance(got["median"], np.float32) and ref.same_bits(got["median"], want["median"]), \
            f"{what} [{where}] median: {got['median']!r} != {want['median']!r}"
        assert ref.same_bits(guess_translation(d, m, K_), center), f"{what} [{where}] guess_translation"
    return want


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_statistics_equal_numpy_for_every_field(size):
    h, w = size
    seen = set()
    for j, (quantised, kind) in enumerate([(q, k) for q in (True, False) for k in ("bool", "uint8", "float32")]):
        rng = np.random.default_rng(1000 * h + 10 * w + j)
        d, m = _depth(h, w, rng, quantised), _mask(h, w, rng, kind)
        if h * w == 1:
            d[0, 0], m[0, 0] = (0.5, 1) if j % 2 else (0.0, 1)
        rec = _check(d, m, f"{h}x{w} q={quantised} {kind}")
        seen.add(rec["n_med"] % 2)
        if h * w > 1 and rec["n_med"] > 1:                           # one element fewer: the other parity, same frame
            with np.errstate(invalid="ignore"):
                rows, cols = np.nonzero(m.astype(bool) & (d >= 0.001))
            d2 = d.copy()
            d2[rows[len(rows) // 2], cols[len(rows) // 2]] = 0
            seen.add(_check(d2, m, f"{h}x{w} q={quantised} {kind} minus one", host=False)["n_med"] % 2)
    if h * w > 1:
        assert seen == {0, 1}                                        # odd and even counts both met


def test_few_valid_pixels_on_both_sides_of_registers_gate():
    rng = np.random.default_rng(5)
    h, w = 37, 53
    for n_valid in range(6):
        for kind in ("bool", "float32"):
            d = np.zeros((h, w), np.float32)
            m = np.zeros((h, w), np.float32 if kind == "float32" else bool)
            m[5:20, 7:30] = 1
            d[5:20, 7:30] = rng.choice(np.array([0, -1, np.nan, 0.0005], np.float32), (15, 23))
            flat = rng.choice(15 * 23, n_valid, replace=False)
            d[5 + flat // 23, 7 + flat % 23] = rng.uniform(0.4, 0.9, n_valid).astype(np.float32)
            d[0, 0], d[30, 40] = 0.7, 0.8                            # depth outside the mask counts for nothing
            rec = _check(d, m, f"{n_valid} valid, {kind}")
            assert rec["n_valid"] == n_valid and rec["n_pos"] == 15 * 23


def test_every_pixel_valid_and_extreme_depths():
    rng = np.random.default_rng(6)
    d = rng.uniform(0.2, 3.0, (576, 640)).astype(np.float32)
    rec = _check(d, np.ones(d.shape, np.uint8), "all valid")
    assert rec["n_med"] == d.size and (rec["umin"], rec["umax"], rec["vmin"], rec["vmax"]) == (0, 639, 0, 575)
    _check(np.full((8, 8), 0.625, np.float32), np.ones((8, 8), bool), "one value")
    big = np.full((1, 2), 3e38, np.float32)                          # (a + b) overflows in float32, as numpy's mean does
    assert _check(big, np.ones((1, 2), bool), "overflow")["median"] == np.inf
    d = np.array([[0.001, np.inf, np.inf, 1e-3, 2.5e38, 1.1754944e-38]], np.float32)
    _check(d, np.ones(d.shape, np.uint8), "infinities")
    _check(d[:, :5], np.ones((1, 5), np.uint8), "infinities, odd")
    corners = np.zeros((720, 1280), bool)                            # the box spans the frame from two pixels
    corners[0, 1279] = corners[719, 0] = True
    rec = _check(np.full(corners.shape, 1.25, np.float32), corners, "corners")
    assert (rec["umin"], rec["umax"], rec["vmin"], rec["vmax"]) == (0, 1279, 0, 719)


def test_statistics_on_a_second_stream_and_rerun():
    from pedp_hip.estimator import mask_depth_stats

    rng = np.random.default_rng(7)
    d, m = _depth(576, 640, rng, True), _mask(576, 640, rng, "uint8")
    dd, dm = torch.as_tensor(d, device="cuda"), torch.as_tensor(m, device="cuda")
    first = mask_depth_stats(dd, dm)
    assert all(first[k] == ref.stats(d, m)[k] for k in FIELDS)
    for _ in range(3):
        again = mask_depth_stats(dd, dm)
        assert again == first or (np.isnan(again["median"]) and np.isnan(first["median"]))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d2 = dd * 1.0                                                 # produced on this stream just before the call
        side = mask_depth_stats(d2, dm)
        mixed = mask_depth_stats(d2, m)                               # a host mask with a device frame
    s.synchronize()
    assert side == first and mixed == first
    smaller = mask_depth_stats(dd[:100].contiguous(), dm[:100].contiguous())   # nothing left over from the larger frame
    assert all(smaller[k] == ref.stats(d[:100], m[:100])[k] for k in FIELDS)
    assert ref.same_bits(smaller["median"], ref.stats(d[:100], m[:100])["median"])
    sliced = mask_depth_stats(dd[:, ::2], dm[:, ::2])                  # strided views are gathered first
    assert all(sliced[k] == ref.stats(d[:, ::2], m[:, ::2])[k] for k in FIELDS)


def test_bad_shapes_and_dtypes_are_refused():
    from pedp_hip import _lib
    from pedp_hip.estimator import mask_depth_stats

    d, m = torch.zeros(4, 5, device="cuda"), torch.zeros(4, 5, device="cuda", dtype=torch.uint8)
    for depth, mask in ((d, m[:3]), (d[None], m[None]), (d.double(), m), (d.half(), m), (d, m.int()), (d, m.double()),
                        (d.reshape(-1), m.reshape(-1)), (d[:0], m[:0])):
        with pytest.raises(_lib.PedpError):
            mask_depth_stats(depth, mask)
    lib, ctx = _lib.load(), _lib.default_context()
    rec = _lib.MaskDepthStats()
    import ctypes as C

    a = np.zeros((4, 5), np.float32)
    for args in ((None, _lib._ptr(a), _lib.F32, 4, 5), (_lib._ptr(a), None, _lib.F32, 4, 5), (_lib._ptr(a), _lib._ptr(a), 7, 4, 5),
                 (_lib._ptr(a), _lib._ptr(a), _lib.F32, 0, 5), (_lib._ptr(a), _lib._ptr(a), _lib.F32, 4097, 4096)):
        assert lib.pedp_mask_depth_stats(ctx._h, *args, _lib.HOST, C.byref(rec)) != 0


# ---------------------------------------------------------------- scene for the loops

CROP = 160
H_, W_ = 480, 640


class _Scene:
    def __init__(self):
        from pedp_hip import synth
        from pedp_hip.compat import TriangleMesh, depth2xyzmap_batch, make_mesh_tensors, nvdiffrast_render

        v, t, n = synth.bumpy_torus(60, 40)
        v = v * 0.0008 + np.array([0.03, -0.02, 0.01])               # off-centre: the estimator has to centre it
        self.mesh = TriangleMesh(v, t)
        self.mesh.vertex_normals = np.asarray(n, np.float64)
        self.model_pts, self.model_normals = v, np.asarray(n, np.float64)
        centred = TriangleMesh(v - (v.min(0) + v.max(0)) / 2, t)
        centred.vertex_normals = self.mesh.vertex_normals
        self.mt = make_mesh_tensors(centred)
        self.diameter = float(np.linalg.norm(v.max(0) - v.min(0)))
        rng = np.random.default_rng(0)
        self.frames = []
        for shift in ((0.01, -0.01, 0.5), (0.015, -0.005, 0.52), (-0.03, 0.02, 0.6)):
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = synth.rot_x(0.4)[:3, :3] @ synth.rot_z(0.3 + shift[0] * 10)[:3, :3]
            T[:3, 3] = shift
            color, depth, _ = nvdiffrast_render(K=K_, H=H_, W=W_, ob_in_cams=torch.as_tensor(T[None], device="cuda"),
                                                mesh_tensors=self.mt)
            rgb = (color[0] * 255).clamp(0, 255).to(torch.uint8).cpu().numpy()
            d = depth[0].cpu().numpy()
            mask = d > 0
            d = (d + rng.normal(0, 0.002, d.shape).astype(np.float32) * mask + 1.2 * ~mask).astype(np.float32)
            self.frames.append((rgb, d, mask, T))
        rgb, d, _, T = self.frames[0]
        self.rgb, self.depth = rgb, torch.as_tensor(d, device="cuda")
        self.xyz = depth2xyzmap_batch(self.depth[None], K_.astype(np.float32)[None], zfar=np.inf)[0]
        self.T = T

    def poses(self, B, seed=1):
        import _pose_ref

        rng = np.random.default_rng(seed)
        P = np.repeat(self.T[None], B, 0)
        P[:, :3, :3] = _pose_ref.so3_exp(rng.normal(size=(B, 3)).astype(np.float32))
        P[:, :3, 3] += rng.normal(0, 0.01, (B, 3)).astype(np.float32)
        return P


@pytest.fixture(scope="module")
def scene():
    return _Scene()


def _cfg(rot_rep="axis_angle", normalize=False):
    return {"input_resize": (CROP, CROP), "trans_normalizer": [0.02, 0.02, 0.05], "rot_normalizer": 0.3490658503988659,
            "rot_rep": rot_rep, "normalize_xyz": normalize, "trans_rep": "tracknet", "crop_ratio": 1.2, "use_normal": False}


def _equal(got, want, what):
    g, w = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.shape} {g.dtype} != {w.shape} {w.dtype}"
    assert ref.same_bits(g, w), f"{what}: {int((g.view(np.uint32) != w.view(np.uint32)).sum())} of {g.size} values differ"


# ---------------------------------------------------------------- refiner

@pytest.mark.parametrize("amp", [True, False], ids=["amp", "fp32"])
@pytest.mark.parametrize("normalize", [False, True], ids=["metres", "normalised"])
@pytest.mark.parametrize("rot_rep", ["axis_angle", "6d"])
def test_refiner_equals_the_hand_composed_loop(scene, rot_rep, normalize, amp):
    from pedp_hip.estimator import PoseRefinePredictor

    cfg = _cfg(rot_rep, normalize)
    net = ref.make_refine_net(6 if rot_rep == "6d" else 3).cuda()
    refiner = PoseRefinePredictor(net, cfg, amp=amp)
    for B, iterations in ((1, (1, 2, 5)), (252, (1, 2, 5)), (1300, (1, 2, 5))):
        P = scene.poses(B)
        for it in iterations:
            want, wtd, wrd = ref.refine_loop(net, cfg, amp, scene.rgb, scene.depth, K_, P, scene.xyz, scene.mt, scene.diameter, it)
            got, vis = refiner.predict(rgb=scene.rgb, depth=scene.depth, K=K_, ob_in_cams=P, xyz_map=scene.xyz,
                                       mesh_tensors=scene.mt, mesh_diameter=scene.diameter, iteration=it)
            assert vis is None and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B, 4, 4)
            _equal(got, want, f"B={B} it={it}")
            _equal(refiner.last_trans_update, wtd, f"last_trans_update B={B} it={it}")
            _equal(refiner.last_rot_update, wrd, f"last_rot_update B={B} it={it}")
            assert tuple(wtd.shape) == (B % 1024 or 1024, 3)          # the last chunk's deltas
        moved = float((got - torch.as_tensor(P, device="cuda")).abs().max())
        assert moved > 1e-4, "the stand-in network moved nothing"
    Pd = torch.as_tensor(P, device="cuda")
    keep = Pd.clone()
    from_tensor, _ = refiner.predict(rgb=scene.rgb, depth=scene.depth, K=K_, ob_in_cams=Pd, xyz_map=scene.xyz,
                                     mesh_tensors=scene.mt, mesh_diameter=scene.diameter, iteration=5)
    _equal(from_tensor, got, "tensor ob_in_cams")
    assert torch.equal(Pd, keep), "predict wrote into the caller's poses"


# ---------------------------------------------------------------- scorer

@pytest.mark.parametrize("amp", [True, False], ids=["amp", "fp32"])
def test_scorer_equals_the_hand_composed_forward(scene, amp):
    from pedp_hip.estimator import ScorePredictor

    cfg = _cfg()
    net = ref.make_score_net().cuda()
    scorer = ScorePredictor(net, cfg, amp=amp)
    for B in (1, 7, 252):
        P = scene.poses(B, seed=4)
        want = ref.score_once(net, cfg, amp, scene.rgb, scene.depth, K_, P, scene.mt, scene.diameter)
        got, vis = scorer.predict(rgb=scene.rgb, depth=scene.depth, K=K_, ob_in_cams=P, mesh_tensors=scene.mt,
                                  mesh_diameter=scene.diameter)
        assert vis is None and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B,)
        _equal(got, want, f"scores B={B}")
        assert float(got.min()) > 50 and (B == 1 or float(got.max() - got.min()) > 0)


# ---------------------------------------------------------------- register and track_one

def _estimator(scene, amp=True):
    from pedp_hip.estimator import FoundationPose, PoseRefinePredictor, ScorePredictor

    cfg = _cfg()
    rn, sn = ref.make_refine_net(3).cuda(), ref.make_score_net().cuda()
    est = FoundationPose(scene.model_pts, scene.model_normals, mesh=scene.mesh, refiner=PoseRefinePredictor(rn, cfg, amp=amp),
                         scorer=ScorePredictor(sn, cfg, amp=amp))
    return est, rn, sn, cfg


def _filtered(depth):
    from pedp_hip.compat import bilateral_filter_depth, erode_depth

    d = torch.as_tensor(depth, device="cuda", dtype=torch.float)
    return bilateral_filter_depth(erode_depth(d, radius=2), radius=2)


def _register_by_hand(est, rn, sn, cfg, rgb, depth, mask, iteration):
    from pedp_hip.compat import depth2xyzmap

    d = _filtered(depth)
    center = ref.guess_translation(d.cpu().numpy(), mask, K_)
    poses = est.rot_grid.clone()
    poses[:, :3, 3] = torch.as_tensor(center, device="cuda", dtype=torch.float).reshape(1, 3)
    xyz = depth2xyzmap(d, K_)
    poses, _, _ = ref.refine_loop(rn, cfg, True, rgb, d, K_, poses, xyz, est.mesh_tensors, est.diameter, iteration)
    scores = ref.score_once(sn, cfg, True, rgb, d, K_, poses, est.mesh_tensors, est.diameter)
    ids = scores.argsort(descending=True, stable=True)
    return poses[ids], scores[ids], ids


def test_estimator_construction(scene):
    est, *_ = _estimator(scene)
    v = scene.model_pts
    assert np.array_equal(est.model_center, (v.min(0) + v.max(0)) / 2)
    assert tuple(est.rot_grid.shape) == (252, 4, 4) and est.rot_grid.is_cuda
    c = v - est.model_center
    assert est.diameter == np.linalg.norm(c[None] - c[:, None], axis=-1).max()   # all 2400 vertices are drawn
    assert est.vox_size == max(est.diameter / 20.0, 0.003) and est.dist_bin == est.vox_size / 2
    assert est.pts.is_cuda and est.pts.dtype == torch.float32 and est.pts.shape == est.normals.shape and len(est.pts) > 50
    assert torch.allclose(est.normals.norm(dim=-1), torch.ones(len(est.normals), device="cuda"), atol=1e-6)
    assert np.array_equal(np.asarray(est.mesh.vertices), c)
    assert np.array_equal(np.asarray(est.mesh_ori.vertices), v) and np.array_equal(np.asarray(scene.mesh.vertices), v)
    tf = est.get_tf_to_centered_mesh().cpu().numpy()
    assert np.array_equal(tf[:3, 3], (-est.model_center).astype(np.float32)) and np.array_equal(tf[:3, :3], np.eye(3))
    assert tuple(est.symmetry_tfs.shape) == (1, 4, 4) and est.pose_last is None
    assert float(est.compute_add_err_to_gt_pose(est.rot_grid).sum()) == -252


def test_register_equals_the_hand_composed_pipeline(scene):
    est, rn, sn, cfg = _estimator(scene)
    rgb, depth, mask, _ = scene.frames[0]
    np.random.seed(0)
    seeded = np.random.get_state()
    np.random.rand(3)
    pose = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=5)
    state = np.random.get_state()
    assert state[0] == seeded[0] and np.array_equal(state[1], seeded[1]) and state[2:] == seeded[2:]
    poses, scores, ids = _register_by_hand(est, rn, sn, cfg, rgb, depth, mask, 5)
    assert isinstance(pose, np.ndarray) and pose.shape == (4, 4) and pose.dtype == np.float32
    assert ref.same_bits(pose, (poses[0] @ est.get_tf_to_centered_mesh()).cpu().numpy())
    _equal(est.poses, poses, "poses")
    _equal(est.scores, scores, "scores")
    assert tuple(est.poses.shape) == (252, 4, 4) and tuple(est.scores.shape) == (252,)
    assert bool((est.scores[:-1] >= est.scores[1:]).all()) and float(est.scores[0] - est.scores[-1]) > 0
    assert int(est.best_id) == int(ids[0]) and torch.equal(est.pose_last, poses[0])
    assert (est.H, est.W) == (H_, W_) and est.glctx is not None
    for mask_kind in (mask.astype(np.uint8), mask.astype(np.float32), torch.as_tensor(mask, device="cuda"),
                      mask.astype(np.int64)):                          # the last one takes the host path
        again = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask_kind, iteration=5)
        assert ref.same_bits(again, pose)
    _equal(est.poses, poses, "poses of the repeated call")
    on_device = est.register(K=K_, rgb=rgb, depth=torch.as_tensor(depth, device="cuda"), ob_mask=mask, iteration=5)
    assert ref.same_bits(on_device, pose)


def test_register_does_not_depend_on_an_earlier_frame(scene):
    est, *_ = _estimator(scene)
    fresh, *_ = _estimator(scene)
    rgb0, depth0, mask0, _ = scene.frames[0]
    rgb2, depth2, mask2, _ = scene.frames[2]
    est.register(K=K_, rgb=rgb0, depth=depth0, ob_mask=mask0, iteration=2)
    after = est.register(K=K_, rgb=rgb2, depth=depth2, ob_mask=mask2, iteration=2)
    alone = fresh.register(K=K_, rgb=rgb2, depth=depth2, ob_mask=mask2, iteration=2)
    assert ref.same_bits(after, alone)
    _equal(est.scores, fresh.scores, "scores")


def test_register_returns_early_below_four_valid_pixels(scene):
    est, *_ = _estimator(scene)
    rgb, depth, mask, _ = scene.frames[0]
    d = _filtered(depth).cpu().numpy()
    keeps = mask & (d >= 0.001)                                       # object pixels that keep their depth through the filters
    rows, cols = np.nonzero(keeps)
    lost_r, lost_c = np.nonzero(mask & ~keeps)                        # ... and those the filters emptied
    for n in (0, 3, 4):
        small = np.zeros_like(mask)
        pick = np.arange(n) * 7 + len(rows) // 2
        small[rows[pick], cols[pick]] = True
        small[lost_r[:5], lost_c[:5]] = True                          # in the mask, but never valid
        n_valid = int(((d >= 0.001) & small).sum())
        assert n_valid == n
        pose = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=small, iteration=1)
        if n_valid < 4:
            want = np.eye(4)
            want[:3, 3] = ref.guess_translation(d, small, K_)
            assert pose.dtype == np.float64 and ref.same_bits(pose, want) and est.pose_last is None
        else:
            assert pose.dtype == np.float32 and est.pose_last is not None
    assert n_valid >= 4, "the four-pixel case never ran the networks"


def test_track_one_chains_through_pose_last(scene):
    from pedp_hip.compat import depth2xyzmap_batch

    est, rn, sn, cfg = _estimator(scene)
    rgb, depth, mask, _ = scene.frames[0]
    with pytest.raises(RuntimeError):
        est.track_one(rgb=rgb, depth=depth, K=K_, iteration=2)
    est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=2)
    last = est.pose_last.clone()
    tf = est.get_tf_to_centered_mesh()
    for k in (1, 0):
        rgb, depth, _, _ = scene.frames[k]
        got = est.track_one(rgb=rgb, depth=depth, K=K_, iteration=2)
        d = _filtered(depth)
        xyz = depth2xyzmap_batch(d[None], K_.astype(np.float32)[None], zfar=np.inf)[0]
        want, _, _ = ref.refine_loop(rn, cfg, True, rgb, d, K_, last.reshape(1, 4, 4), xyz, est.mesh_tensors, est.diameter, 2)
        assert got.shape == (4, 4) and got.dtype == np.float32
        assert ref.same_bits(got, (want @ tf).cpu().numpy().reshape(4, 4))
        assert tuple(est.pose_last.shape) == (1, 4, 4)
        _equal(est.pose_last, want, f"pose_last after frame {k}")
        assert not torch.equal(want.reshape(4, 4), last.reshape(4, 4))
        last = est.pose_last.clone()
