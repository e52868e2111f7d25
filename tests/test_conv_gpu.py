"""conv.conv3x3 (csrc/pedp_conv.hip) against F.conv2d in float64 on the CPU, on the float16-rounded x, the packed w' read
back, b' and the residual.  Per element, with K = 9 * Cin and y the float64 pre-activation result:

    |y_kernel - y| <= (K + 4) * 2^-24 * (conv(|x|, |w'|) + |b'| + |res|) + 2^-11 * |y| + 2^-24

the float32 accumulation bound for any summation order plus one rounding to float16; ReLU is 1-Lipschitz, so the bound
holds after it unchanged.  One float64 reference per shape serves every variant of that shape.  The tap-map test needs no
bound: one input element is 1, every weight is its own code, and each output element is one product or zero."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
F = torch.nn.functional

SHAPES = [(1, 1, 1, 128), (1, 1, 7, 128), (1, 7, 1, 128), (3, 5, 7, 128), (2, 9, 11, 256), (1, 4, 4, 512), (2, 40, 40, 256),
          (2, 20, 20, 512)]


def _modules(cin, cout, bn, seed):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cin)) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    norm = None
    if bn:
        norm = torch.nn.BatchNorm2d(cout).eval()
        with torch.no_grad():
            norm.weight.copy_(1 + 0.1 * torch.randn(cout, generator=g))
            norm.bias.copy_(0.1 * torch.randn(cout, generator=g))
            norm.running_mean.copy_(0.1 * torch.randn(cout, generator=g))
            norm.running_var.copy_(1 + 0.25 * torch.rand(cout, generator=g))
    return conv.cuda(), (norm.cuda() if bn else None)


@functools.lru_cache(maxsize=None)
def _case(n, h, w, cin, cout, bn):
    """Inputs on the GPU, the packed layer, and the float64 reference pieces on the CPU (channels-last)."""
    from pedp_hip.conv import pack_conv3x3

    seed = 7 * n + 11 * h + 13 * w + cin + 3 * cout + int(bn)
    conv, norm = _modules(cin, cout, bn, seed)
    packed = pack_conv3x3(conv, norm)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((n, h, w, cin), generator=g).half()
    res = torch.randn((n, h, w, cout), generator=g).half()
    w64 = packed.weight_oihw().double().cpu()
    b64 = packed.bias.double().cpu()
    x64 = x.double().permute(0, 3, 1, 2)
    pre = F.conv2d(x64, w64, None, 1, 1).permute(0, 2, 3, 1)
    mag = F.conv2d(x64.abs(), w64.abs(), None, 1, 1).permute(0, 2, 3, 1)
    return {"x": x.cuda(), "res": res.cuda(), "packed": packed, "pre": pre, "mag": mag, "b": b64, "res64": res.double(),
            "conv": conv, "norm": norm}


def _check(got, c, residual, relu, what):
    K = 9 * c["packed"].cin
    y = c["pre"] + c["b"] + (c["res64"] if residual else 0)
    mag = c["mag"] + c["b"].abs() + (c["res64"].abs() if residual else 0)
    bound = (K + 4) * 2.0 ** -24 * mag + 2.0 ** -11 * y.abs() + 2.0 ** -24
    want = y.clamp(min=0) if relu else y
    err = (got.double().cpu() - want).abs()
    used = float((err / bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, largest share of the bound {used:.3f}")
    assert got.dtype == torch.float16 and tuple(got.shape) == tuple(want.shape)
    assert bool(torch.isfinite(got).all()) and used <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements exceed the bound"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_with_batchnorm_folded_stays_within_the_float32_bound(shape):
    from pedp_hip.conv import conv3x3

    n, h, w, c_ = shape
    c = _case(n, h, w, c_, c_, True)
    for relu in (True, False):
        _check(conv3x3(c["x"], c["packed"], relu=relu), c, False, relu, f"{shape} relu={relu}")
        _check(conv3x3(c["x"], c["packed"], residual=c["res"], relu=relu), c, True, relu, f"{shape} residual relu={relu}")
        y = c["res"].clone()
        out = conv3x3(c["x"], c["packed"], residual=y, relu=relu, out=y)          # the residual is the destination
        assert out.data_ptr() == y.data_ptr()
        _check(y, c, True, relu, f"{shape} residual aliasing the output relu={relu}")


NEW_CHANNELS = [(96, 32), (96, 224), (160, 96), (192, 128), (320, 64), (480, 480)]


@pytest.mark.parametrize("pixels", [(3, 5, 7), (2, 9, 11)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cin,cout", NEW_CHANNELS)
def test_channel_counts_beside_the_networks(cin, cout, pixels):
    """Cin = 96, 160 and 480: three, five and fifteen 32-channel steps per tap (conv_kernel<1, 1>); Cin = 192 and 320: an
    odd number of 64-channel steps; Cout = 224 and 480: a partial channel tile behind full ones.  105 pixels are one tile
    straddling three images, 198 are two tiles."""
    from pedp_hip.conv import conv3x3

    c = _case(*pixels, cin, cout, True)
    what = f"{pixels} {cin} -> {cout}"
    for relu in (True, False):
        _check(conv3x3(c["x"], c["packed"], relu=relu), c, False, relu, f"{what} relu={relu}")
        _check(conv3x3(c["x"], c["packed"], residual=c["res"], relu=relu), c, True, relu, f"{what} residual relu={relu}")
        y = c["res"].clone()
        out = conv3x3(c["x"], c["packed"], residual=y, relu=relu, out=y)          # the residual is the destination
        assert out.data_ptr() == y.data_ptr()
        _check(y, c, True, relu, f"{what} residual aliasing the output relu={relu}")


@pytest.mark.parametrize("pixels", [(3, 5, 7), (2, 9, 11)], ids=lambda s: "x".join(map(str, s)))
def test_partial_channel_tile_into_a_destination_with_its_own_stride_and_offset(pixels):
    """96 -> 224 channels: the second channel tile holds 96 of 128; the channels on both sides of the slice stay."""
    from pedp_hip.conv import conv3x3

    c = _case(*pixels, 96, 224, True)
    n, h, w = pixels
    dense = conv3x3(c["x"], c["packed"], residual=c["res"], relu=True)
    _check(dense, c, True, True, f"{pixels} 96 -> 224 dense")
    pattern = (torch.arange(n * h * w * 480, device="cuda") % 251).half().reshape(n, h, w, 480)
    for c0 in (32, 256):
        out = pattern.clone()
        got = conv3x3(c["x"], c["packed"], residual=c["res"], relu=True, out=out, out_c0=c0)
        assert got.data_ptr() == out[..., c0:].data_ptr() and tuple(got.shape) == (n, h, w, 224)
        assert torch.equal(out[..., c0:c0 + 224], dense), f"y_c0 = {c0} differs from the dense call"
        assert torch.equal(out[..., :c0], pattern[..., :c0]) and torch.equal(out[..., c0 + 224:], pattern[..., c0 + 224:]), \
            f"channels outside {c0} .. {c0 + 224} were written"


@pytest.mark.parametrize("cin,cout,as_bits", [(32, 32, False), (96, 160, True)], ids=["32", "96"])
def test_tap_map_is_exact(cin, cout, as_bits):
    """Stride 1 through pack_conv3x3: a 1 at one input element and coded weights give each output element as one product
    or zero, exactly.  32 channels are one 32-channel K step per tap; 96 are three, with the 1 at channels 95 and 48 in the
    third and the second step (6912 codes, as float16 bit patterns): a 32-channel path that left the channel step out
    of its offset would return the codes of channels 31 and 16 there.  160 output channels end in a tile of 32 behind a
    full one.  77 pixels per image: the 231 pixels fill two tiles, the first holds two images' ends."""
    from test_conv_strided_gpu import _coded_layer

    from pedp_hip.conv import conv3x3

    packed, w64 = _coded_layer(cout, cin, 3, as_bits, stride=1)
    n, h, w = 3, 7, 11
    for img, ci, y, x in ((0, 0, 0, 0), (2, cin - 1, 6, 10), (1, 7, 0, 5), (1, cin // 2, 3, 4), (1, 3, 6, 10), (2, 1, 2, 0)):
        src = torch.zeros((n, h, w, cin), dtype=torch.float16)
        src[img, y, x, ci] = 1.0
        want = F.conv2d(src.double().permute(0, 3, 1, 2), w64, None, 1, 1).permute(0, 2, 3, 1)
        got = conv3x3(src.cuda(), packed, relu=False).double().cpu()
        assert int((want != 0).sum()) >= 4 * cout
        assert torch.equal(got, want), f"a 1 at image {img}, channel {ci}, ({y}, {x}): {int((got != want).sum())} elements differ"


def test_the_fold_is_the_float32_fold():
    c = _case(3, 5, 7, 128, 128, True)
    conv, bn, p = c["conv"], c["norm"], c["packed"]
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    w = (conv.weight * s[:, None, None, None]).half()
    b = (conv.bias - bn.running_mean) * s + bn.bias
    assert (p.weight_oihw().float() - w.float()).abs().max() <= 2.0 ** -10 * float(w.abs().max())
    assert torch.allclose(p.bias, b, rtol=1e-6, atol=1e-7)
    assert p.w.dtype == torch.float16 and tuple(p.w.shape) == (128, 9, 128) and p.bias.dtype == torch.float32


@pytest.mark.parametrize("shape", [(3, 5, 7, 128), (1, 4, 4, 512)], ids=lambda s: "x".join(map(str, s)))
def test_plain_conv_without_batchnorm(shape):
    from pedp_hip.conv import conv3x3

    n, h, w, c_ = shape
    c = _case(n, h, w, c_, c_, False)
    assert torch.equal(c["packed"].bias, c["conv"].bias.detach().float())
    assert torch.equal(c["packed"].weight_oihw(), c["conv"].weight.detach().half())
    _check(conv3x3(c["x"], c["packed"], relu=True), c, False, True, f"{shape} plain")
    _check(conv3x3(c["x"], c["packed"], residual=c["res"], relu=False), c, True, False, f"{shape} plain residual identity")


def test_different_channel_counts_in_and_out():
    from pedp_hip.conv import conv3x3

    c = _case(2, 6, 5, 64, 96, True)
    _check(conv3x3(c["x"], c["packed"], relu=True), c, False, True, "64 -> 96")
    _check(conv3x3(c["x"], c["packed"], residual=c["res"], relu=False), c, True, False, "64 -> 96 residual identity")
    c = _case(1, 3, 3, 32, 160, False)                                 # one 32-channel K step; two channel tiles, one partial
    _check(conv3x3(c["x"], c["packed"], relu=False), c, False, False, "32 -> 160")


@pytest.mark.parametrize("shape", [(3, 5, 7, 128), (2, 9, 11, 256)], ids=lambda s: "x".join(map(str, s)))
def test_destination_with_its_own_channel_stride_and_offset(shape):
    from pedp_hip.conv import conv3x3

    n, h, w, c_ = shape
    c = _case(n, h, w, c_, c_, True)
    pattern = (torch.arange(n * h * w * 2 * c_, device="cuda") % 251).half().reshape(n, h, w, 2 * c_)
    for c0 in (0, c_):
        out = pattern.clone()
        got = conv3x3(c["x"], c["packed"], residual=c["res"], relu=True, out=out, out_c0=c0)
        assert got.data_ptr() == out[..., c0:].data_ptr() and tuple(got.shape) == (n, h, w, c_)
        _check(out[..., c0:c0 + c_], c, True, True, f"{shape} y_ld={2 * c_} y_c0={c0}")
        other = slice(c_, 2 * c_) if c0 == 0 else slice(0, c_)
        assert torch.equal(out[..., other], pattern[..., other]), "the other half of the destination was written"
        dense = conv3x3(c["x"], c["packed"], residual=c["res"], relu=True)
        assert torch.equal(out[..., c0:c0 + c_], dense)
    both = pattern.clone()                                            # a residual that is a channel slice of the destination
    both[..., c_:] = c["res"]
    conv3x3(c["x"], c["packed"], residual=both[..., c_:], relu=True, out=both, out_c0=c_)
    assert torch.equal(both[..., c_:], dense) and torch.equal(both[..., :c_], pattern[..., :c_])


def test_a_tile_straddling_two_images_equals_each_image_alone():
    from pedp_hip.conv import conv3x3

    c = _case(2, 9, 11, 256, 256, True)                                # 99 pixels per image: the first tile of 128 holds both
    whole = conv3x3(c["x"], c["packed"], residual=c["res"], relu=True)
    for k in range(2):
        alone = conv3x3(c["x"][k:k + 1], c["packed"], residual=c["res"][k:k + 1], relu=True)
        assert torch.equal(whole[k:k + 1], alone), f"image {k} differs from the image convolved alone"


def test_two_calls_give_identical_bits():
    from pedp_hip.conv import conv3x3

    for shape in ((2, 20, 20, 512), (2, 40, 40, 256)):
        c = _case(*shape, shape[3], True)
        a = conv3x3(c["x"], c["packed"], residual=c["res"], relu=True)
        b = conv3x3(c["x"], c["packed"], residual=c["res"], relu=True)
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        x2 = c["x"] * 1.0                                             # produced on this stream just before the call
        on_side = conv3x3(x2, c["packed"], residual=c["res"], relu=True)
    s.synchronize()
    assert torch.equal(on_side, a)


def test_unsupported_channels_are_bad_arguments():
    from pedp_hip import _lib
    from pedp_hip.conv import conv3x3, pack_conv3x3, supported

    lib, ctx = _lib.load(), _lib.default_context()
    x = torch.zeros((1, 4, 4, 64), dtype=torch.float16, device="cuda")
    wp = torch.zeros((64, 9, 64), dtype=torch.float16, device="cuda")
    b = torch.zeros(64, dtype=torch.float32, device="cuda")
    y = torch.zeros((1, 4, 4, 64), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()

    def call(**kw):
        prm = _lib.Conv3x3Params()
        prm.N, prm.H, prm.W, prm.Cin, prm.Cout, prm.y_ld, prm.y_c0, prm.relu = 1, 4, 4, 64, 64, 64, 0, 1
        for k, v in kw.items():
            setattr(prm, k, v)
        return lib.pedp_conv3x3_f16(ctx._h, C.byref(prm), C.c_void_p(x.data_ptr()), C.c_void_p(wp.data_ptr()),
                                    C.c_void_p(b.data_ptr()), None, C.c_void_p(y.data_ptr()))

    BAD_ARG = -1                                                       # PEDP_ERR_BAD_ARG (include/pedp.h)
    assert call() == 0
    ctx.synchronize()
    for kw in ({"Cin": 48}, {"Cout": 48}, {"Cin": 544}, {"Cin": 0}, {"N": 0}, {"H": 0}, {"y_ld": 32}, {"y_c0": 32}, {"y_c0": -4}):
        assert call(**kw) == BAD_ARG, kw
    conv48 = torch.nn.Conv2d(48, 64, 3, 1, 1).cuda()
    assert not supported(conv48) and not supported(torch.nn.Conv2d(64, 64, 3, 2, 1)) and supported(torch.nn.Conv2d(64, 64, 3, 1, 1))
    with pytest.raises(_lib.PedpError):
        pack_conv3x3(conv48)
    assert lib.pedp_conv3x3_pack(ctx._h, 48, 64, C.c_void_p(x.data_ptr()), None, None, None, None, None, 0.0,
                                 C.c_void_p(wp.data_ptr()), C.c_void_p(b.data_ptr())) == BAD_ARG
    c = _case(3, 5, 7, 128, 128, True)
    for bad in (c["x"].float(), c["x"][..., :64], c["x"].cpu(), c["x"].permute(0, 3, 1, 2)):
        with pytest.raises(_lib.PedpError):
            conv3x3(bad, c["packed"])
    with pytest.raises(_lib.PedpError):
        conv3x3(c["x"], c["packed"], residual=c["res"][:, :, :, :64])
    with pytest.raises(_lib.PedpError):
        conv3x3(c["x"], c["packed"], out=torch.empty((3, 5, 7, 192), dtype=torch.float16, device="cuda"), out_c0=128)
