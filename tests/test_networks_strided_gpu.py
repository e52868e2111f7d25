"""The refine and score networks with strided='hip' (the three stride-2 convolutions on conv.conv_stem / conv.conv_strided)
on the cases of tests/golden/g9_networks.npz: the criterion of tests/test_networks_gpu.py unchanged (e <= 2 * e_torch +
10 * e_ref32 and e_torch < d_swap / 4, e_torch the all-torch autocast forward's error against the fixture), which path a
call takes and when the fifteen packed layers are dropped, and register / track_one against the same steps composed by hand.
The fixture, the fill and the helpers are that file's."""
import numpy as np
import pytest

import _estimator_ref as ref
import _net_fill
import test_networks_gpu as base

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLD, PAIRS = base.GOLD, base.PAIRS


@pytest.fixture(autouse=True)
def _reproducible_torch_convolutions():
    """These tests compare bits of forwards in which some convolutions are torch's.  Left to choose, torch's convolution
    library takes kernels on the MI355X that sum with atomics: two identical F.conv2d calls on a 256- or 512-channel layer
    then differ (by up to 0.016 in float16 at 8 x 8).  Asking torch for its deterministic choice makes torch's side of each
    comparison a fixed function of its inputs; the package's kernels are not affected by the flag."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def _net(kind, rot_rep, backend, strided="hip", heads="torch", shift=0):
    from pedp_hip import networks

    cfg = {"use_BN": True, "rot_rep": rot_rep or "axis_angle"}
    cls = networks.RefineNet if kind == "refiner" else networks.ScoreNetMultiPair
    net = cls(cfg, c_in=6, backend=backend, heads=heads, strided=strided)
    keys = [str(k) for k in GOLD[f"{base._tag(kind, rot_rep)}/keys"]]
    if shift:
        keys = keys[shift:] + keys[:shift]
    return _net_fill.fill(net, keys).cuda().eval()


@pytest.mark.parametrize("backend,heads", [("hip", "torch"), ("torch", "torch"), ("hip", "hip")])
@pytest.mark.parametrize("case,rot_rep", PAIRS)
def test_strided_forward_under_autocast_is_as_close_as_torch(case, rot_rep, backend, heads):
    kind = _net_fill.CASES[case][0]
    tag = base._tag(kind, rot_rep)
    net = _net(kind, rot_rep, backend, heads=heads)
    out = base._run(net, case, True)
    assert len(net._packed) == (15 if backend == "hip" else 3) and all(p is not None for p in net._packed.values())
    e = base._errors(out, case, tag)
    e_torch = base._errors(base._run(_net(kind, rot_rep, "torch", strided="torch"), case, True), case, tag)
    again = base._run(net, case, True)
    for name in out:
        e_ref = float(GOLD[f"{case}/{tag}/{name}/e_ref32"])
        d_swap = float(GOLD[f"{case}/{tag}/{name}/d_swap"])
        print(f"{case} {tag} {name} backend={backend} heads={heads}: e_torch {e_torch[name]:.3e}, e {e[name]:.3e}, "
              f"e_ref32 {e_ref:.3e}, d_swap {d_swap:.3e}")
        assert e_torch[name] < d_swap / 4, "the case cannot tell a working network from a broken one"
        assert e[name] <= 2 * e_torch[name] + 10 * e_ref
        assert np.array_equal(again[name], out[name]), "two forwards differ"
    if kind == "scorer":
        want = GOLD[f"{case}/{tag}/score_logit"]
        top = np.sort(want, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 4 * e_torch["score_logit"]
        print(f"{case}: rows with a clear winner {int(clear.sum())} of {len(clear)}")
        assert np.array_equal(out["score_logit"].argmax(1)[clear], want.argmax(1)[clear])


def test_float16_crops_take_the_same_path():
    net = _net("refiner", "axis_angle", "hip")
    A, B = (t.cuda() for t in _net_fill.inputs("refiner_2x48x32", torch.float32))
    outs = []
    for a, b in ((A, B), (A.half(), B.half()), (A, B.half())):         # the kernel's own rounding, torch's, and a mixed pair
        with torch.inference_mode(), torch.autocast("cuda"):
            outs.append({k: v.clone() for k, v in net(a, b).items()})
    assert all(torch.equal(outs[0][k], o[k]) for o in outs[1:] for k in o)


@pytest.mark.parametrize("kind,case", [("refiner", "refiner_3x32x32"), ("scorer", "scorer_4x32x32")])
def test_which_path_a_call_takes(kind, case):
    net, plain = _net(kind, "axis_angle", "hip"), _net(kind, "axis_angle", "torch", strided="torch")
    a, b = base._run(net, case, False), base._run(plain, case, False)  # no autocast: the torch modules, the same bits
    assert not net._packed and all(np.array_equal(a[k], b[k]) for k in a)
    fused = base._run(net, case, True)
    assert len(net._packed) == 15
    today = base._run(_net(kind, "axis_angle", "hip", strided="torch"), case, True)
    assert net.set_strided("torch") is net
    back = base._run(net, case, True)                                  # the block kernels alone: today's fused bits
    assert all(np.array_equal(back[k], today[k]) for k in back)
    net.set_backend("torch")                                           # and nothing of ours: the torch modules
    assert all(np.array_equal(v, w) for v, w in zip(base._run(net, case, True).values(), base._run(plain, case, True).values()))
    net.set_backend("hip").set_strided("hip")
    assert all(np.array_equal(v, w) for v, w in zip(base._run(net, case, True).values(), fused.values()))
    assert len(net._packed) == 15
    only = _net(kind, "axis_angle", "torch")                           # strided alone also takes the fused forward
    base._run(only, case, True)
    assert len(only._packed) == 3
    net.train(), plain.train()                                         # training: the torch modules (dropout seeded alike)
    assert not net._packed
    outs = []
    for m in (net, plain):
        torch.manual_seed(5)
        outs.append(base._run(m, case, True))
    assert all(np.array_equal(outs[0][k], outs[1][k]) for k in outs[0]) and not net._packed
    other = _net(kind, "axis_angle", "hip", shift=1)                   # other weights: the packed ones are rebuilt
    net.eval()                                                         # (the training forwards moved the running statistics)
    net.load_state_dict(other.state_dict())
    assert not net._packed
    moved, want = base._run(net, case, True), base._run(other, case, True)
    assert all(np.array_equal(moved[k], want[k]) for k in moved)
    assert all(np.abs(moved[k] - fused[k]).max() > 1e-2 for k in moved), "the forward ignored the new weights"
    assert len(net._packed) == 15
    net.half()                                                         # .to() drops them too
    assert not net._packed


def test_register_and_track_one_with_the_strided_networks():
    from pedp_hip import synth
    from pedp_hip.compat import TriangleMesh, depth2xyzmap, depth2xyzmap_batch, make_mesh_tensors, nvdiffrast_render
    from pedp_hip.estimator import FoundationPose, PoseRefinePredictor, ScorePredictor, set_seed

    K_, CROP = base.K_, base.CROP
    set_seed(0)
    v, t, n = synth.bumpy_torus(60, 40)
    v = v * 0.0008
    mesh = TriangleMesh(v, t)
    mesh.vertex_normals = np.asarray(n, np.float64)
    frames = []
    rng = np.random.default_rng(0)
    for shift in ((0.01, -0.01, 0.5), (0.015, -0.005, 0.52)):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = synth.rot_x(0.4)[:3, :3] @ synth.rot_z(0.3)[:3, :3]
        T[:3, 3] = shift
        color, depth, _ = nvdiffrast_render(K=K_, H=480, W=640, ob_in_cams=torch.as_tensor(T[None], device="cuda"),
                                            mesh_tensors=make_mesh_tensors(mesh))
        d = depth[0].cpu().numpy()
        mask = d > 0
        d = (d + rng.normal(0, 0.002, d.shape).astype(np.float32) * mask + 1.2 * ~mask).astype(np.float32)
        frames.append(((color[0] * 255).clamp(0, 255).to(torch.uint8).cpu().numpy(), d, mask))
    cfg = {"input_resize": (CROP, CROP), "trans_normalizer": [0.02, 0.02, 0.05], "rot_normalizer": 0.3490658503988659,
           "rot_rep": "axis_angle", "normalize_xyz": True, "trans_rep": "tracknet", "crop_ratio": 1.2, "use_normal": False,
           "use_BN": True, "c_in": 6}
    rn, sn = _net("refiner", "axis_angle", "hip"), _net("scorer", None, "hip")
    est = FoundationPose(v, mesh.vertex_normals, mesh=mesh, refiner=PoseRefinePredictor(rn, cfg), scorer=ScorePredictor(sn, cfg))
    rgb, depth, mask = frames[0]
    pose = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=2)
    assert len(rn._packed) == 15 and len(sn._packed) == 15, "register did not take the strided forward"
    poses_1, scores_1 = est.poses.clone(), est.scores.clone()
    assert pose.shape == (4, 4) and np.isfinite(pose).all() and tuple(est.poses.shape) == (252, 4, 4)
    assert bool(torch.isfinite(est.poses).all()) and bool(torch.isfinite(est.scores).all())
    assert float(est.scores[0] - est.scores[-1]) > 0
    # by hand: the crop batches, the model and pose_update (tests/_estimator_ref.py)
    d = base._filtered(depth)
    start = est.rot_grid.clone()
    start[:, :3, 3] = torch.as_tensor(ref.guess_translation(d.cpu().numpy(), mask, K_), device="cuda", dtype=torch.float).reshape(1, 3)
    by_hand, _, _ = ref.refine_loop(rn, cfg, True, rgb, d, K_, start, depth2xyzmap(d, K_), est.mesh_tensors, est.diameter, 2)
    scores = ref.score_once(sn, cfg, True, rgb, d, K_, by_hand, est.mesh_tensors, est.diameter)
    ids = scores.argsort(descending=True, stable=True)
    assert ref.same_bits(est.poses.cpu().numpy(), by_hand[ids].cpu().numpy())
    assert ref.same_bits(est.scores.cpu().numpy(), scores[ids].cpu().numpy())
    assert ref.same_bits(pose, (by_hand[ids][0] @ est.get_tf_to_centered_mesh()).cpu().numpy())
    last = est.pose_last.clone()
    rgb2, depth2, _ = frames[1]
    tracked = est.track_one(rgb=rgb2, depth=depth2, K=K_, iteration=2)
    d2 = base._filtered(depth2)
    xyz2 = depth2xyzmap_batch(d2[None], K_.astype(np.float32)[None], zfar=np.inf)[0]
    want, _, _ = ref.refine_loop(rn, cfg, True, rgb2, d2, K_, last.reshape(1, 4, 4), xyz2, est.mesh_tensors, est.diameter, 2)
    assert np.isfinite(tracked).all() and ref.same_bits(tracked, (want @ est.get_tf_to_centered_mesh()).cpu().numpy().reshape(4, 4))
    assert not torch.equal(want.reshape(4, 4), last.reshape(4, 4))
    # the same calls again: the same bits
    again = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=2)
    assert ref.same_bits(again, pose) and torch.equal(est.poses, poses_1) and torch.equal(est.scores, scores_1)
    assert ref.same_bits(est.track_one(rgb=rgb2, depth=depth2, K=K_, iteration=2), tracked)
