"""The refine and score networks on the GPU, on the four cases of tests/golden/g9_networks.npz (outputs of the reference's
own definitions in float64): the torch path in float32, the torch and the fused path under float16 autocast, which path a
call takes, and register / track_one around the real architectures against the same steps composed by hand.

Under autocast, with e_torch and e_hip the two backends' errors against the fixture: e_hip <= 2 * e_torch + 10 * e_ref32
(both are float16 pipelines rounding in different places), and e_torch < d_swap / 4 (the case can tell a working network
from one with A and B swapped)."""
import os

import numpy as np
import pytest

import _estimator_ref as ref
import _net_fill

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_networks.npz"))
PAIRS = [(c, r) for c, v in _net_fill.CASES.items() if v[0] == "refiner" for r in _net_fill.ROT_REPS] + \
        [(c, None) for c, v in _net_fill.CASES.items() if v[0] == "scorer"]


def _tag(kind, rot_rep):
    return kind if kind == "scorer" else f"{kind}_{rot_rep}"


def _net(kind, rot_rep, backend, shift=0):
    from pedp_hip import networks

    cfg = {"use_BN": True, "rot_rep": rot_rep or "axis_angle"}
    net = (networks.RefineNet if kind == "refiner" else networks.ScoreNetMultiPair)(cfg, c_in=6, backend=backend)
    keys = [str(k) for k in GOLD[f"{_tag(kind, rot_rep)}/keys"]]
    if shift:                                                          # other weights: the rule with the key list rotated
        keys = keys[shift:] + keys[:shift]
    return _net_fill.fill(net, keys).cuda().eval()


def _run(net, case, amp, dtype=torch.float32):
    kind, _, _, L, _ = _net_fill.CASES[case]
    A, B = (t.cuda() for t in _net_fill.inputs(case, dtype))
    with torch.inference_mode(), torch.autocast("cuda", enabled=amp):
        out = net(A, B) if kind == "refiner" else net(A, B, L=L)
    return {k: v.double().cpu().numpy() for k, v in out.items()}


def _errors(out, case, tag):
    return {k: float(np.abs(v - GOLD[f"{case}/{tag}/{k}"]).max()) for k, v in out.items()}


@pytest.mark.parametrize("case,rot_rep", PAIRS)
def test_torch_backend_in_float32(case, rot_rep):
    kind = _net_fill.CASES[case][0]
    tag = _tag(kind, rot_rep)
    for name, err in _errors(_run(_net(kind, rot_rep, "torch"), case, False), case, tag).items():
        e_ref = float(GOLD[f"{case}/{tag}/{name}/e_ref32"])
        print(f"{case} {tag} {name}: float32 err {err:.3e}, e_ref32 {e_ref:.3e}")
        assert err <= 10 * e_ref


@pytest.mark.parametrize("case,rot_rep", PAIRS)
def test_fused_forward_under_autocast_is_as_close_as_torch(case, rot_rep):
    kind = _net_fill.CASES[case][0]
    tag = _tag(kind, rot_rep)
    hip = _net(kind, rot_rep, "hip")
    out_hip = _run(hip, case, True)
    assert len(hip._packed) == 12 and all(p is not None for p in hip._packed.values()), "a block convolution did not take the kernel"
    e_hip = _errors(out_hip, case, tag)
    e_torch = _errors(_run(_net(kind, rot_rep, "torch"), case, True), case, tag)
    again = _run(hip, case, True)
    for name in out_hip:
        e_ref = float(GOLD[f"{case}/{tag}/{name}/e_ref32"])
        d_swap = float(GOLD[f"{case}/{tag}/{name}/d_swap"])
        print(f"{case} {tag} {name}: e_torch {e_torch[name]:.3e}, e_hip {e_hip[name]:.3e}, e_ref32 {e_ref:.3e}, d_swap {d_swap:.3e}")
        assert e_torch[name] < d_swap / 4, "the case cannot tell a working network from a broken one"
        assert e_hip[name] <= 2 * e_torch[name] + 10 * e_ref
        assert np.array_equal(again[name], out_hip[name]), "two fused forwards differ"
    if kind == "scorer":
        want = GOLD[f"{case}/{tag}/score_logit"]
        top = np.sort(want, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 4 * e_torch["score_logit"]
        print(f"{case}: rows with a clear winner {int(clear.sum())} of {len(clear)}")
        assert np.array_equal(out_hip["score_logit"].argmax(1)[clear], want.argmax(1)[clear])


@pytest.mark.parametrize("kind,case", [("refiner", "refiner_3x32x32"), ("scorer", "scorer_4x32x32")])
def test_which_path_a_call_takes(kind, case):
    hip, plain = _net(kind, "axis_angle", "hip"), _net(kind, "axis_angle", "torch")
    a, b = _run(hip, case, False), _run(plain, case, False)            # no autocast: the torch modules, the same bits
    assert not hip._packed and all(np.array_equal(a[k], b[k]) for k in a)
    fused = _run(hip, case, True)
    assert len(hip._packed) == 12
    from pedp_hip import networks

    auto = _net(kind, "axis_angle", "auto")
    by_table = _run(auto, case, True)                                  # 'auto': the table picks per layer (4 layers per width)
    assert len(auto._packed) == 4 * sum(networks._AUTO[c] == "hip" for c in (128, 256, 512))
    if not auto._packed:
        assert all(np.array_equal(by_table[k], b2) for k, b2 in _run(plain, case, True).items())
    hip.set_backend("torch")
    assert all(np.array_equal(v, w) for v, w in zip(_run(hip, case, True).values(), _run(plain, case, True).values()))
    hip.set_backend("hip")
    hip.train(), plain.train()                                         # training: the torch modules (dropout seeded alike)
    assert not hip._packed
    outs = []
    for net in (hip, plain):
        torch.manual_seed(5)
        outs.append(_run(net, case, True))
    assert all(np.array_equal(outs[0][k], outs[1][k]) for k in outs[0])
    assert not hip._packed
    # other weights: the packed ones are rebuilt
    other = _net(kind, "axis_angle", "hip", shift=1)
    hip.eval()
    hip.load_state_dict(other.state_dict())
    assert not hip._packed
    moved, want = _run(hip, case, True), _run(other, case, True)
    assert all(np.array_equal(moved[k], want[k]) for k in moved)
    assert all(np.abs(moved[k] - fused[k]).max() > 1e-2 for k in moved), "the fused output ignored the new weights"
    assert len(hip._packed) == 12
    hip.half()                                                         # .to() drops them too
    assert not hip._packed


# ---------------------------------------------------------------- register and track_one around the real architectures

K_ = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
CROP = 32


def _filtered(depth):
    from pedp_hip.compat import bilateral_filter_depth, erode_depth

    return bilateral_filter_depth(erode_depth(torch.as_tensor(depth, device="cuda", dtype=torch.float), radius=2), radius=2)


def test_register_and_track_one_with_the_fused_networks():
    from pedp_hip import synth
    from pedp_hip.compat import TriangleMesh, depth2xyzmap, depth2xyzmap_batch, make_mesh_tensors, nvdiffrast_render
    from pedp_hip.estimator import FoundationPose, PoseRefinePredictor, ScorePredictor, set_seed

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
    assert len(rn._packed) == 12 and len(sn._packed) == 12, "register did not take the fused forward"
    poses_1, scores_1 = est.poses.clone(), est.scores.clone()
    assert pose.shape == (4, 4) and np.isfinite(pose).all() and tuple(est.poses.shape) == (252, 4, 4)
    assert bool(torch.isfinite(est.poses).all()) and bool(torch.isfinite(est.scores).all())
    assert float(est.scores[0] - est.scores[-1]) > 0
    # by hand: the crop batches, the model and pose_update (tests/_estimator_ref.py)
    d = _filtered(depth)
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
    d2 = _filtered(depth2)
    xyz2 = depth2xyzmap_batch(d2[None], K_.astype(np.float32)[None], zfar=np.inf)[0]
    want, _, _ = ref.refine_loop(rn, cfg, True, rgb2, d2, K_, last.reshape(1, 4, 4), xyz2, est.mesh_tensors, est.diameter, 2)
    assert np.isfinite(tracked).all() and ref.same_bits(tracked, (want @ est.get_tf_to_centered_mesh()).cpu().numpy().reshape(4, 4))
    assert not torch.equal(want.reshape(4, 4), last.reshape(4, 4))
    # the same calls again: the same bits
    again = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=2)
    assert ref.same_bits(again, pose) and torch.equal(est.poses, poses_1) and torch.equal(est.scores, scores_1)
    assert ref.same_bits(est.track_one(rgb=rgb2, depth=depth2, K=K_, iteration=2), tracked)
