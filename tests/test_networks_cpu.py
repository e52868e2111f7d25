"""The refine and score networks without a GPU: their state_dict against the reference's (keys, shapes, dtypes, order)
and their float64 / float32 forwards against outputs of the reference's own definitions (tests/golden/g9_networks.npz,
written by tests/golden/make_network_golden.py with the by-name fill of tests/_net_fill.py), and the checkpoint loaders."""
import os

import numpy as np
import pytest

import _net_fill

torch = pytest.importorskip("torch")

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_networks.npz"))
REFINER_CASES = [c for c, v in _net_fill.CASES.items() if v[0] == "refiner"]
SCORER_CASES = [c for c, v in _net_fill.CASES.items() if v[0] == "scorer"]
PAIRS = [(c, r) for c in REFINER_CASES for r in _net_fill.ROT_REPS] + [(c, None) for c in SCORER_CASES]


def build(kind, rot_rep=None, use_bn=True, **kw):
    from pedp_hip import networks

    cfg = {"use_BN": use_bn, "rot_rep": rot_rep or "axis_angle"}
    return (networks.RefineNet if kind == "refiner" else networks.ScoreNetMultiPair)(cfg, c_in=6, **kw)


def tag_of(kind, rot_rep):
    return kind if kind == "scorer" else f"{kind}_{rot_rep}"


def listed(tag):
    return ([str(k) for k in GOLD[f"{tag}/keys"]], [tuple(int(s) for s in str(x).split(",") if s) for x in GOLD[f"{tag}/shapes"]],
            [str(d) for d in GOLD[f"{tag}/dtypes"]])


def filled(kind, rot_rep, dtype):
    net = build(kind, rot_rep).to(dtype).eval()
    return _net_fill.fill(net, listed(tag_of(kind, rot_rep))[0])


def forward(net, case, dtype):
    kind, _, _, L, _ = _net_fill.CASES[case]
    A, B = _net_fill.inputs(case, dtype)
    with torch.no_grad():
        out = net(A, B) if kind == "refiner" else net(A, B, L=L)
        feat = net.encode(A[:1], B[:1]) if kind == "refiner" else None
    return {k: v.double().numpy() for k, v in out.items()}, feat


@pytest.mark.parametrize("kind,rot_rep", [("refiner", "axis_angle"), ("refiner", "6d"), ("scorer", None)])
def test_state_dict_is_the_references(kind, rot_rep):
    keys, shapes, dtypes = listed(tag_of(kind, rot_rep))
    assert len(keys) == (134 if kind == "refiner" else 116)
    sd = build(kind, rot_rep).state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert [str(v.dtype) for v in sd.values()] == dtypes
    n = sum(int(np.prod(s)) if s else 1 for s in shapes)
    assert abs(n - (17.04e6 if kind == "refiner" else 15.99e6)) < 0.01e6

    def is_bn(k):
        return ".bn1." in k or ".bn2." in k or ".net.1." in k

    plain = build(kind, rot_rep, use_bn=False).state_dict()
    want = [(k, s, d) for k, s, d in zip(keys, shapes, dtypes) if not is_bn(k)]
    assert len(want) < len(keys)
    assert [(k, tuple(v.shape), str(v.dtype)) for k, v in plain.items()] == want


def test_cfg_defaults_are_the_reference_predictors():
    from pedp_hip import networks
    from pedp_hip.estimator import Config

    net = networks.RefineNet({"rot_rep": "6d"})
    assert net.encodeA[0].net[0].in_channels == 4 and not any("running_mean" in k for k in net.state_dict())
    assert net.rot_head[1].out_features == 6
    net = networks.ScoreNetMultiPair(Config(c_in=6, use_BN=True))
    assert net.encoderA[0].net[0].in_channels == 6 and any("running_mean" in k for k in net.state_dict())
    with pytest.raises(ValueError):
        networks.RefineNet({"rot_rep": "quaternion"})
    with pytest.raises(ValueError):
        networks.RefineNet({}, backend="triton")


@pytest.mark.parametrize("case,rot_rep", PAIRS)
def test_float64_forward_equals_the_reference(case, rot_rep):
    kind = _net_fill.CASES[case][0]
    assert int(GOLD[f"{case}/seed"]) == _net_fill.CASES[case][4]
    tag = tag_of(kind, rot_rep)
    net = filled(kind, rot_rep, torch.float64)
    out, _ = forward(net, case, torch.float64)
    A, B = _net_fill.inputs(case)
    with torch.no_grad():
        tokens = net.encode(A, B)[0].numpy()                          # (h/8 * w/8) x 512
    want_feat = GOLD[f"{case}/feat"]
    err_feat = np.abs(tokens - want_feat.reshape(512, -1).T).max()
    print(f"{case} {tag}: pair-encoder feature err {err_feat:.3e}")
    assert err_feat <= 1e-9
    for name, got in out.items():
        want = GOLD[f"{case}/{tag}/{name}"]
        err = np.abs(got - want).max()
        print(f"{case} {tag} {name}: err {err:.3e}, |out| {np.abs(want).max():.3g}")
        assert got.shape == want.shape and err <= 1e-9


@pytest.mark.parametrize("case,rot_rep", PAIRS)
def test_float32_forward_stays_within_ten_times_the_references_own_error(case, rot_rep):
    kind = _net_fill.CASES[case][0]
    tag = tag_of(kind, rot_rep)
    net = filled(kind, rot_rep, torch.float32)
    out, _ = forward(net, case, torch.float32)
    for name, got in out.items():
        err = np.abs(got - GOLD[f"{case}/{tag}/{name}"]).max()
        e_ref = float(GOLD[f"{case}/{tag}/{name}/e_ref32"])
        print(f"{case} {tag} {name}: err {err:.3e}, e_ref32 {e_ref:.3e}")
        assert err <= 10 * e_ref


@pytest.mark.parametrize("kind", ["refiner", "scorer"])
def test_loaders_take_a_checkpoint_a_state_dict_and_refuse_a_renamed_key(kind, tmp_path):
    from pedp_hip import networks

    cfg = {"use_BN": True, "rot_rep": "axis_angle", "c_in": 6}
    load = networks.load_refiner if kind == "refiner" else networks.load_scorer
    src = _net_fill.fill(build(kind, "axis_angle"))
    sd = src.state_dict()
    path = str(tmp_path / "model_best.pth")
    torch.save({"model": sd, "epoch": 3}, path)
    bare = str(tmp_path / "bare.pth")
    torch.save(sd, bare)
    for source in (path, bare, sd, {"model": sd}):
        net = load(source, cfg, device="cpu")
        assert not net.training and type(net) is type(src)
        got = net.state_dict()
        assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    renamed = dict(sd)
    key = "encodeA.0.net.0.weight" if kind == "refiner" else "encoderA.0.net.0.weight"
    renamed[key.replace("net.0", "net.conv")] = renamed.pop(key)
    with pytest.raises(RuntimeError):
        load(renamed, cfg, device="cpu")
    from pedp_hip import compat

    assert compat.RefineNet is networks.RefineNet and compat.load_scorer is networks.load_scorer
