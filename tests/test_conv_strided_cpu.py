"""The stride-2 convolutions' host side without a GPU: conv.out_hw and conv.supported_strided, and the networks' `strided`
keyword, which off the GPU changes nothing."""
import pytest

import _net_fill

torch = pytest.importorskip("torch")
F = torch.nn.functional


def _stem(cin=6, cout=64):
    return torch.nn.Conv2d(cin, cout, 7, 2, 3)


def _down(cin, cout):
    return torch.nn.Conv2d(cin, cout, 3, 2, 1)


@pytest.mark.parametrize("conv", [_stem(), _down(64, 128)], ids=["7x7", "3x3"])
def test_out_hw_is_conv2d_s_output_shape(conv):
    from pedp_hip.conv import out_hw

    for h in range(1, 10):
        for w in range(1, 10):
            with torch.no_grad():
                want = tuple(conv(torch.zeros(1, conv.in_channels, h, w)).shape[2:])
            assert out_hw(h, w, conv) == want, (h, w)
    assert out_hw(160, 160, _stem()) == (80, 80) and out_hw(80, 80, _down(64, 128)) == (40, 40)


def test_supported_strided_takes_the_reference_s_three_layers_and_nothing_else():
    from pedp_hip.conv import supported, supported_strided

    for conv in (_stem(), _down(64, 128), _down(256, 512)):
        assert supported_strided(conv) and not supported(conv), conv
    nn = torch.nn
    for conv in (nn.Conv2d(64, 128, 3, 1, 1), nn.Conv2d(64, 128, 3, 3, 1), nn.Conv2d(64, 128, 3, 2, 2, dilation=2),
                 nn.Conv2d(64, 128, 3, 2, 1, groups=2), nn.Conv2d(9, 64, 7, 2, 3), nn.Conv2d(48, 128, 3, 2, 1),
                 nn.Conv2d(6, 64, 7, 1, 3), nn.Conv2d(6, 64, 7, 2, 2), nn.Conv2d(64, 128, 3, 2, 0), nn.Conv2d(6, 48, 7, 2, 3),
                 nn.Conv2d(64, 128, 5, 2, 2)):
        assert not supported_strided(conv), conv


def test_the_strided_keyword_is_checked_and_kept():
    from pedp_hip import networks

    for cls in (networks.RefineNet, networks.ScoreNetMultiPair):
        with pytest.raises(ValueError):
            cls({"use_BN": True}, c_in=6, strided="bogus")
        net = cls({"use_BN": True}, c_in=6)
        assert net.strided == "torch" and net.set_strided("hip") is net and net.strided == "hip"
        with pytest.raises(ValueError):
            net.set_strided("auto")
        assert cls({"use_BN": True}, c_in=6, strided="hip").strided == "hip"


@pytest.mark.parametrize("kind,case", [("refiner", "refiner_3x32x32"), ("scorer", "scorer_4x32x32")])
def test_on_the_cpu_in_float32_strided_hip_is_the_default_forward(kind, case):
    from pedp_hip import networks

    cls = networks.RefineNet if kind == "refiner" else networks.ScoreNetMultiPair
    nets = [cls({"use_BN": True}, c_in=6, backend="torch", strided=s) for s in ("torch", "hip")]
    assert list(nets[0].state_dict()) == list(nets[1].state_dict())
    keys = list(nets[0].state_dict())
    L = _net_fill.CASES[case][3]
    A, B = _net_fill.inputs(case, torch.float32)
    outs = []
    for net in nets:
        _net_fill.fill(net, keys).eval()
        with torch.inference_mode():
            outs.append(net(A, B) if kind == "refiner" else net(A, B, L=L))
        assert not net._packed
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
    assert all(torch.equal(v, w) for v, w in zip(nets[0].state_dict().values(), nets[1].state_dict().values()))
