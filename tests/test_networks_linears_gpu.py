"""The refine and score networks with heads='hip', linears='hip' (linear.linear, linear_add_norm and token_pool around
attention.mha_core) on the four cases of tests/golden/g9_networks.npz, by the criterion of tests/test_networks_heads_gpu.py:
with e and e_torch the errors of this forward and of the stock forward under float16 autocast against the float64 fixture,
e <= 2 * e_torch + 10 * e_ref32 and e_torch < d_swap / 4; which path a call takes; the packed weights' life; register /
track_one.

Known miss, left as the criterion stands.  test_hip_linears_under_autocast_are_as_close_as_torch[scorer_4x32x32-None-torch-
torch] depends on which kernels torch's convolution library takes for the encoder on the machine at hand.  Seen on MI355X
machines: e_torch 0.0409 with e 0.0157 (passes), e_torch 0.1407 with e 0.1720 (passes), and e_torch 0.0470 with e 0.1034
against a limit of 0.0945 (fails).  The logits of that case are 32 .. 37.5, where one float16 step of the returned logit is
0.03125; the error against the fixture is the float16 encoder's (0.11 .. 0.14 with the float64 heads evaluated on the same
float16 tokens), and the heads add within one step of it: the stock heads 0.0076, this path 0.0289 from those float64 heads,
i.e. one step in one logit.  On scorer_6x32x48 the same figures are 0.386 for the stock heads and 0.145 for this path.  So
the miss is a float16 step of the output falling on the far side of the encoder's error, not a fault found in the kernels;
the bound is the issue's and is not widened."""
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
# calls of (linear.linear, linear.linear_add_norm, linear.token_pool) in one forward, and packed entries of the heads
CALLS = {"refiner": (4, 4, 2), "scorer": (4, 0, 2)}
HEAD_PACKS = {"refiner": 4, "scorer": 3}


@pytest.fixture(autouse=True)
def _reproducible_torch_convolutions():
    """These tests compare bits of forwards in which some convolutions are torch's, whose library otherwise takes kernels on
    the MI355X that sum with atomics (tests/test_networks_strided_gpu.py).  The flag fixes torch's side of
    each comparison; the package's kernels are not affected by it."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def _tag(kind, rot_rep):
    return kind if kind == "scorer" else f"{kind}_{rot_rep}"


def _net(kind, rot_rep, backend="torch", heads="hip", linears="hip", strided="torch"):
    from pedp_hip import networks

    cfg = {"use_BN": True, "rot_rep": rot_rep or "axis_angle"}
    net = (networks.RefineNet if kind == "refiner" else networks.ScoreNetMultiPair)(cfg, c_in=6, backend=backend, heads=heads,
                                                                                    linears=linears, strided=strided)
    return _net_fill.fill(net, [str(k) for k in GOLD[f"{_tag(kind, rot_rep)}/keys"]]).cuda().eval()


def _run(net, case, amp):
    kind, _, _, L, _ = _net_fill.CASES[case]
    A, B = (t.cuda() for t in _net_fill.inputs(case, torch.float32))
    with torch.inference_mode(), torch.autocast("cuda", enabled=amp):
        out = net(A, B) if kind == "refiner" else net(A, B, L=L)
    return {k: v.double().cpu().numpy() for k, v in out.items()}, {k: v.dtype for k, v in out.items()}


def _errors(out, case, tag):
    return {k: float(np.abs(v - GOLD[f"{case}/{tag}/{k}"]).max()) for k, v in out.items()}


def _stock(case, rot_rep):
    """The stock forward under autocast, once per case: (errors, output dtypes)."""
    if (case, rot_rep) not in _TORCH:
        kind = _net_fill.CASES[case][0]
        out, dtypes = _run(_net(kind, rot_rep, "torch", "torch", "torch"), case, True)
        _TORCH[case, rot_rep] = _errors(out, case, _tag(kind, rot_rep)), dtypes
    return _TORCH[case, rot_rep]


def _count_calls(monkeypatch):
    """Counters of the three kernel wrappers and of the torch ops they replace."""
    import torch.nn.functional as F
    from pedp_hip import linear

    calls = {"linear": 0, "linear_add_norm": 0, "token_pool": 0, "F.linear": 0, "F.layer_norm": 0}

    def counted(real, name):
        def f(*a, **kw):
            calls[name] += 1
            return real(*a, **kw)
        return f

    for name in ("linear", "linear_add_norm", "token_pool"):
        monkeypatch.setattr(linear, name, counted(getattr(linear, name), name))
    monkeypatch.setattr(F, "linear", counted(F.linear, "F.linear"))
    monkeypatch.setattr(F, "layer_norm", counted(F.layer_norm, "F.layer_norm"))
    return calls


def _kernel_calls(calls):
    return (calls["linear"], calls["linear_add_norm"], calls["token_pool"])


@pytest.mark.parametrize("backend,strided", [("torch", "torch"), ("hip", "torch"), ("hip", "hip")])
@pytest.mark.parametrize("case,rot_rep", PAIRS)
def test_hip_linears_under_autocast_are_as_close_as_torch(case, rot_rep, backend, strided, monkeypatch):
    kind = _net_fill.CASES[case][0]
    tag = _tag(kind, rot_rep)
    (e_torch, dtypes) = _stock(case, rot_rep)
    calls = _count_calls(monkeypatch)
    net = _net(kind, rot_rep, backend, "hip", "hip", strided)
    out, got_dtypes = _run(net, case, True)
    assert _kernel_calls(calls) == CALLS[kind] and calls["F.linear"] == 0 and calls["F.layer_norm"] == 0
    assert len(net._packed) == HEAD_PACKS[kind] + (12 if backend == "hip" else 0) + (3 if strided == "hip" else 0)
    assert got_dtypes == dtypes, "the outputs' dtypes are the stock autocast forward's"
    e = _errors(out, case, tag)
    again, _ = _run(net, case, True)
    for name in out:
        e_ref = float(GOLD[f"{case}/{tag}/{name}/e_ref32"])
        d_swap = float(GOLD[f"{case}/{tag}/{name}/d_swap"])
        print(f"{case} {tag} {name} backend {backend} strided {strided}: e_torch {e_torch[name]:.3e}, e {e[name]:.3e}, "
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


@pytest.mark.parametrize("kind,case", [("refiner", "refiner_3x32x32"), ("scorer", "scorer_4x32x32")])
def test_which_path_the_linears_take(kind, case, monkeypatch):
    calls = _count_calls(monkeypatch)
    both, heads_only = _net(kind, "axis_angle"), _net(kind, "axis_angle", linears="torch")
    stock, odd = _net(kind, "axis_angle", heads="torch", linears="torch"), _net(kind, "axis_angle", heads="torch", linears="hip")
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)
    # no autocast: the stock modules, the same bits, whatever the switches say
    plain = _run(stock, case, False)[0]
    assert same(_run(both, case, False)[0], plain) and same(_run(odd, case, False)[0], plain) and _kernel_calls(calls) == (0, 0, 0)
    # linears='hip' without heads='hip' is the stock forward; with heads='hip' alone the present heads path
    amp_stock, amp_heads = _run(stock, case, True)[0], _run(heads_only, case, True)[0]
    assert same(_run(odd, case, True)[0], amp_stock) and _kernel_calls(calls) == (0, 0, 0)
    assert calls["F.linear"] > 0 and (calls["F.layer_norm"] > 0) == (kind == "refiner")
    before = dict(calls)
    fused = _run(both, case, True)[0]
    assert _kernel_calls(calls) == CALLS[kind]
    assert calls["F.linear"] == before["F.linear"] and calls["F.layer_norm"] == before["F.layer_norm"]
    both.set_linears("torch")
    assert same(_run(both, case, True)[0], amp_heads) and _kernel_calls(calls) == CALLS[kind]
    heads_only.set_linears("hip")
    assert same(_run(heads_only, case, True)[0], fused) and _kernel_calls(calls) == tuple(2 * c for c in CALLS[kind])
    # training: the stock modules (dropout seeded alike)
    both.set_linears("hip").train(), stock.train()
    outs = []
    for net in (both, stock):
        torch.manual_seed(5)
        outs.append(_run(net, case, True)[0])
    assert same(*outs) and _kernel_calls(calls) == tuple(2 * c for c in CALLS[kind])
    assert list(both.state_dict().keys()) == [str(k) for k in GOLD[f"{_tag(kind, 'axis_angle')}/keys"]]


@pytest.mark.parametrize("kind,case", [("refiner", "refiner_2x48x32"), ("scorer", "scorer_6x32x48")])
def test_packed_linears_follow_the_weights(kind, case):
    net = _net(kind, "axis_angle")
    first = _run(net, case, True)[0]
    assert len(net._packed) == HEAD_PACKS[kind]
    lin = net.trans_head[0].linear1 if kind == "refiner" else net.att.out_proj
    with torch.no_grad():
        lin.weight.mul_(1.5)
    assert all(np.array_equal(v, first[k]) for k, v in _run(net, case, True)[0].items()), "an in-place edit is not seen before drop_packed"
    net.drop_packed()
    assert not net._packed and not net._buffers_tok
    edited = _run(net, case, True)[0]
    name = "trans" if kind == "refiner" else "score_logit"
    assert not np.array_equal(edited[name], first[name]), "drop_packed() did not rebuild the packed weights"
    fresh = _net(kind, "axis_angle")
    state = {k: v.clone() for k, v in fresh.state_dict().items()}
    net.load_state_dict(state)
    assert not net._packed, "load_state_dict keeps stale packs"
    assert all(np.array_equal(v, first[k]) for k, v in _run(net, case, True)[0].items())
    assert len(net._packed) == HEAD_PACKS[kind]
    net.train()
    assert not net._packed
    net.eval().half().float()
    assert not net._packed


def test_token_buffers_are_kept():
    net = _net("refiner", "axis_angle", backend="hip", strided="hip")
    _run(net, "refiner_3x32x32", True)
    (key, buf), = net._buffers_tok.items()
    ptrs = {k: v.data_ptr() for k, v in buf.items()}
    assert set(buf) == {"qkv", "a", "y"} and tuple(buf["qkv"].shape) == (3, 16, 1536)
    _run(net, "refiner_3x32x32", True)
    assert {k: v.data_ptr() for k, v in net._buffers_tok[key].items()} == ptrs, "the token buffers were allocated again"


# ---------------------------------------------------------------- register and track_one

K_ = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
CROP = 32


def test_register_and_track_one_with_hip_linears(monkeypatch):
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
    calls = _count_calls(monkeypatch)
    rn, sn = _net("refiner", "axis_angle", "hip"), _net("scorer", None, "hip")
    est = FoundationPose(v, mesh.vertex_normals, mesh=mesh, refiner=PoseRefinePredictor(rn, cfg), scorer=ScorePredictor(sn, cfg))
    rgb, depth, mask = frames[0]
    pose = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=2)
    assert calls["linear_add_norm"] > 0 and calls["token_pool"] > 0 and calls["F.layer_norm"] == 0, "register did not take the kernels"
    assert rn._buffers_tok and sn._buffers_tok
    poses_1, scores_1 = est.poses.clone(), est.scores.clone()
    assert pose.shape == (4, 4) and np.isfinite(pose).all() and tuple(est.poses.shape) == (252, 4, 4)
    assert bool(torch.isfinite(est.poses).all()) and bool(torch.isfinite(est.scores).all())
    assert bool((est.scores[:-1] >= est.scores[1:]).all()) and float(est.scores[0] - est.scores[-1]) > 0
    rgb2, depth2, _ = frames[1]
    n_calls = calls["linear"]
    tracked = est.track_one(rgb=rgb2, depth=depth2, K=K_, iteration=2)
    assert np.isfinite(tracked).all() and calls["linear"] > n_calls
    again = est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=2)
    assert np.array_equal(again, pose) and torch.equal(est.poses, poses_1) and torch.equal(est.scores, scores_1)
    assert np.array_equal(est.track_one(rgb=rgb2, depth=depth2, K=K_, iteration=2), tracked)
