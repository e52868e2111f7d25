"""The refine and score networks with heads='hip' (attention.self_attention in the refiner's encoder layers and the scorer's
two attentions) on the four cases of tests/golden/g9_networks.npz, by the criterion of tests/test_networks_gpu.py: with e and
e_torch the errors of the heads='hip' forward and of the stock forward under float16 autocast against the float64 fixture,
e <= 2 * e_torch + 10 * e_ref32 and e_torch < d_swap / 4; which path a call takes; register / track_one."""
import os

import numpy as np
import pytest

import _net_fill

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_networks.npz"))
PAIRS = [(c, r) for c, v in _net_fill.CASES.items() if v[0] == "refiner" for r in _net_fill.ROT_REPS] + \
        [(c, None) for c, v in _net_fill.CASES.items() if v[0] == "scorer"]
_TORCH = {}


def _tag(kind, rot_rep):
    return kind if kind == "scorer" else f"{kind}_{rot_rep}"


def _net(kind, rot_rep, backend, heads):
    from pedp_hip import networks

    cfg = {"use_BN": True, "rot_rep": rot_rep or "axis_angle"}
    net = (networks.RefineNet if kind == "refiner" else networks.ScoreNetMultiPair)(cfg, c_in=6, backend=backend, heads=heads)
    return _net_fill.fill(net, [str(k) for k in GOLD[f"{_tag(kind, rot_rep)}/keys"]]).cuda().eval()


def _run(net, case, amp):
    kind, _, _, L, _ = _net_fill.CASES[case]
    A, B = (t.cuda() for t in _net_fill.inputs(case, torch.float32))
    with torch.inference_mode(), torch.autocast("cuda", enabled=amp):
        out = net(A, B) if kind == "refiner" else net(A, B, L=L)
    return {k: v.double().cpu().numpy() for k, v in out.items()}


def _errors(out, case, tag):
    return {k: float(np.abs(v - GOLD[f"{case}/{tag}/{k}"]).max()) for k, v in out.items()}


def _torch_errors(case, rot_rep):
    """The stock forward's errors under autocast, once per case."""
    if (case, rot_rep) not in _TORCH:
        kind = _net_fill.CASES[case][0]
        _TORCH[case, rot_rep] = _errors(_run(_net(kind, rot_rep, "torch", "torch"), case, True), case, _tag(kind, rot_rep))
    return _TORCH[case, rot_rep]


def _count_kernel_calls(monkeypatch):
    from pedp_hip import attention

    calls = []
    real = attention.mha_core

    def counted(qkv, *a, **kw):
        calls.append(tuple(qkv.shape))
        return real(qkv, *a, **kw)

    monkeypatch.setattr(attention, "mha_core", counted)
    return calls


@pytest.mark.parametrize("backend", ["torch", "hip"])
@pytest.mark.parametrize("case,rot_rep", PAIRS)
def test_hip_heads_under_autocast_are_as_close_as_torch(case, rot_rep, backend, monkeypatch):
    kind = _net_fill.CASES[case][0]
    tag = _tag(kind, rot_rep)
    calls = _count_kernel_calls(monkeypatch)
    net = _net(kind, rot_rep, backend, "hip")
    out = _run(net, case, True)
    assert len(calls) == 2, "both attentions of a forward go through the kernel"
    assert len(net._packed) == (12 if backend == "hip" else 0)
    e, e_torch = _errors(out, case, tag), _torch_errors(case, rot_rep)
    again = _run(net, case, True)
    for name in out:
        e_ref = float(GOLD[f"{case}/{tag}/{name}/e_ref32"])
        d_swap = float(GOLD[f"{case}/{tag}/{name}/d_swap"])
        print(f"{case} {tag} {name} backend {backend}: e_torch {e_torch[name]:.3e}, e {e[name]:.3e}, e_ref32 {e_ref:.3e}, d_swap {d_swap:.3e}")
        assert e_torch[name] < d_swap / 4, "the case cannot tell a working network from a broken one"
        assert e[name] <= 2 * e_torch[name] + 10 * e_ref
        assert np.array_equal(again[name], out[name]), "two forwards differ"
    if kind == "scorer":
        want = GOLD[f"{case}/{tag}/score_logit"]
        top = np.sort(want, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 4 * e_torch["score_logit"]
        print(f"{case}: rows with a clear winner {int(clear.sum())} of {len(clear)}")
        assert np.array_equal(out["score_logit"].argmax(1)[clear], want.argmax(1)[clear])


@pytest.mark.parametrize("kind,case", [("refiner", "refiner_3x32x32"), ("scorer", "scorer_4x32x32")])
def test_which_path_the_heads_take(kind, case, monkeypatch):
    calls = _count_kernel_calls(monkeypatch)
    hip, plain = _net(kind, "axis_angle", "torch", "hip"), _net(kind, "axis_angle", "torch", "torch")
    a, b = _run(hip, case, False), _run(plain, case, False)             # no autocast: the stock modules, the same bits
    assert not calls and all(np.array_equal(a[k], b[k]) for k in a)
    stock = _run(plain, case, True)
    assert not calls                                                     # heads='torch' never calls the kernel
    fused = _run(hip, case, True)
    assert len(calls) == 2
    hip.set_heads("torch")
    assert all(np.array_equal(v, stock[k]) for k, v in _run(hip, case, True).items()) and len(calls) == 2
    plain.set_heads("hip")
    assert all(np.array_equal(v, fused[k]) for k, v in _run(plain, case, True).items()) and len(calls) == 4
    hip.set_heads("hip")
    hip.train(), plain.set_heads("torch").train()                        # training: the stock modules (dropout seeded alike)
    outs = []
    for net in (hip, plain):
        torch.manual_seed(5)
        outs.append(_run(net, case, True))
    assert len(calls) == 4 and all(np.array_equal(outs[0][k], outs[1][k]) for k in outs[0])
    assert list(hip.state_dict().keys()) == [str(k) for k in GOLD[f"{_tag(kind, 'axis_angle')}/keys"]]


# ---------------------------------------------------------------- register and track_one

K_ = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
CROP = 32


def test_register_and_track_one_with_hip_heads(monkeypatch):
    from pedp_hip import synth
    from pedp_hip.compat import TriangleMesh, make_mesh_tensors, nvdiffrast_render
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
    calls = _count_kernel_calls(monkeypatch)
    rn, sn = _net("refiner", "axis_angle", "hip", "hip"), _net("scorer", None, "hip", "hip")
    est = FoundationPose(v, mesh.vertex_normals, mesh=mesh, refiner=PoseRefinePredictor(rn, cfg), scorer=ScorePredictor(sn, cfg))
    rgb, depth, mask = frames[0]
    pose = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=2)
    assert any(c[1] == 16 for c in calls) and any(c[:2] == (1, 252) for c in calls), "register did not take the kernel in both networks"
    poses_1, scores_1 = est.poses.clone(), est.scores.clone()
    assert pose.shape == (4, 4) and np.isfinite(pose).all() and tuple(est.poses.shape) == (252, 4, 4)
    assert bool(torch.isfinite(est.poses).all()) and bool(torch.isfinite(est.scores).all())
    assert bool((est.scores[:-1] >= est.scores[1:]).all()) and float(est.scores[0] - est.scores[-1]) > 0
    rgb2, depth2, _ = frames[1]
    n_calls = len(calls)
    tracked = est.track_one(rgb=rgb2, depth=depth2, K=K_, iteration=2)
    assert np.isfinite(tracked).all() and len(calls) > n_calls
    again = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=2)
    assert np.array_equal(again, pose) and torch.equal(est.poses, poses_1) and torch.equal(est.scores, scores_1)
    assert np.array_equal(est.track_one(rgb=rgb2, depth=depth2, K=K_, iteration=2), tracked)
