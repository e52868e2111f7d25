"""conv.conv_stem and conv.conv_strided (csrc/pedp_conv.hip, csrc/conv/stem.h) against F.conv2d in float64 on the CPU, on the
float16-rounded input, the packed w' read back and b'.  Per element, with K the number of K-axis slots summed (9 * Cin, and
392 for the stem) and y the float64 pre-activation result, DESIGN.md s4.12's bound:

    |y_kernel - y| <= (K + 4) * 2^-24 * (conv(|x|, |w'|) + |b'|) + 2^-11 * |y| + 2^-24

the float32 accumulation bound for any summation order plus one rounding to float16; ReLU is 1-Lipschitz, so the bound
holds after it unchanged.  One float64 reference per shape serves every variant of that shape.  The tap-map tests need no
bound: one input element is 1, every weight is its own code, and each output element is one product or zero.

Stride 1 is not the new entry point's: pack_conv refuses such a layer and pedp_conv2d_f16 returns PEDP_ERR_BAD_ARG
(conv3x3 / pedp_conv3x3_f16 is the stride-1 call)."""
import ctypes as C
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
F = torch.nn.functional

STEM_SHAPES = [(1, 1, 1), (1, 7, 7), (2, 5, 9), (3, 13, 17), (3, 32, 32), (2, 48, 32), (2, 160, 160)]
DOWN_SHAPES = [(1, 1, 1, 64, 128), (1, 2, 2, 64, 128), (3, 5, 7, 64, 128), (2, 9, 11, 256, 512), (2, 6, 5, 64, 96),
               (2, 80, 80, 64, 128), (2, 40, 40, 256, 512)]
BAD_ARG = -1                                                           # PEDP_ERR_BAD_ARG (include/pedp.h)


def _ids(s):
    return "x".join(map(str, s))


def _modules(k, cin, cout, bn, seed):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, k, 2, (k - 1) // 2, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (k * k * cin)) ** 0.5)
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


def _reference(x64_nchw, packed):
    """The float64 pieces, channels-last: conv(x, w'), conv(|x|, |w'|), b'."""
    w64 = packed.weight_oihw().double().cpu()
    pre = F.conv2d(x64_nchw, w64, None, 2, packed.pad).permute(0, 2, 3, 1)
    mag = F.conv2d(x64_nchw.abs(), w64.abs(), None, 2, packed.pad).permute(0, 2, 3, 1)
    return {"pre": pre, "mag": mag, "b": packed.bias.double().cpu()}


@functools.lru_cache(maxsize=None)
def _stem_case(n, h, w, bn, cin=6, cout=64):
    """x NCHW float32 and its float16 rounding on the GPU (one reference serves both), the packed layer, the reference."""
    from pedp_hip.conv import pack_conv

    seed = 5 * n + 11 * h + 13 * w + cin + 3 * cout + int(bn)
    conv, norm = _modules(7, cin, cout, bn, seed)
    packed = pack_conv(conv, norm)
    x = torch.randn((n, cin, h, w), generator=torch.Generator().manual_seed(seed + 1))
    c = _reference(x.half().double(), packed)
    c.update({"x32": x.cuda(), "x16": x.half().cuda(), "packed": packed, "conv": conv, "norm": norm, "K": 392})
    return c


@functools.lru_cache(maxsize=None)
def _down_case(n, h, w, cin, cout, bn=True):
    from pedp_hip.conv import pack_conv

    seed = 7 * n + 11 * h + 13 * w + cin + 3 * cout + int(bn)
    conv, norm = _modules(3, cin, cout, bn, seed)
    packed = pack_conv(conv, norm)
    x = torch.randn((n, h, w, cin), generator=torch.Generator().manual_seed(seed + 1)).half()
    c = _reference(x.double().permute(0, 3, 1, 2), packed)
    c.update({"x": x.cuda(), "packed": packed, "conv": conv, "norm": norm, "K": 9 * cin})
    return c


def _check(got, c, relu, what):
    y = c["pre"] + c["b"]
    bound = (c["K"] + 4) * 2.0 ** -24 * (c["mag"] + c["b"].abs()) + 2.0 ** -11 * y.abs() + 2.0 ** -24
    want = y.clamp(min=0) if relu else y
    assert got.dtype == torch.float16 and tuple(got.shape) == tuple(want.shape), (got.dtype, tuple(got.shape), tuple(want.shape))
    err = (got.double().cpu() - want).abs()
    used = float((err / bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, largest share of the bound {used:.3f}")
    assert bool(torch.isfinite(got).all()) and used <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements exceed the bound"


# ---------------------------------------------------------------- the bound

@pytest.mark.parametrize("bn", [True, False], ids=["bn", "plain"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_ids)
def test_stem_stays_within_the_float32_bound(shape, dtype, bn):
    from pedp_hip.conv import conv_stem, out_hw

    c = _stem_case(*shape, bn)
    x = c["x32"] if dtype == "float32" else c["x16"]
    for relu in (True, False):
        y = conv_stem(x, None, c["packed"], relu=relu)
        assert tuple(y.shape[1:3]) == out_hw(shape[1], shape[2], c["conv"])
        _check(y, c, relu, f"stem {shape} {dtype} bn={bn} relu={relu}")


@pytest.mark.parametrize("shape", DOWN_SHAPES, ids=_ids)
def test_strided_3x3_stays_within_the_float32_bound(shape):
    from pedp_hip.conv import conv_strided, out_hw

    c = _down_case(*shape)
    for relu in (True, False):
        y = conv_strided(c["x"], c["packed"], relu=relu)
        assert tuple(y.shape[1:3]) == out_hw(shape[1], shape[2], c["conv"])
        _check(y, c, relu, f"3x3/2 {shape} relu={relu}")


NEW_CHANNELS = [(96, 32), (96, 224), (160, 96), (192, 128), (320, 64), (480, 480)]


@pytest.mark.parametrize("pixels", [(3, 5, 7), (2, 9, 11)], ids=_ids)
@pytest.mark.parametrize("cin,cout", NEW_CHANNELS)
def test_strided_3x3_over_channel_counts_beside_the_networks(cin, cout, pixels):
    """Cin = 96, 160 and 480: three, five and fifteen 32-channel steps per tap (conv_kernel<1, 2>); Cin = 192 and 320: an
    odd number of 64-channel steps; Cout = 224 and 480: a partial channel tile behind full ones."""
    from pedp_hip.conv import conv_strided

    c = _down_case(*pixels, cin, cout)
    for relu in (True, False):
        _check(conv_strided(c["x"], c["packed"], relu=relu), c, relu, f"3x3/2 {pixels} {cin} -> {cout} relu={relu}")


def test_strided_3x3_without_batchnorm_and_the_fold():
    from pedp_hip.conv import conv_strided

    c = _down_case(3, 5, 7, 64, 128, False)
    assert torch.equal(c["packed"].bias, c["conv"].bias.detach().float())
    assert torch.equal(c["packed"].weight_oihw(), c["conv"].weight.detach().half())
    _check(conv_strided(c["x"], c["packed"], relu=True), c, True, "3x3/2 plain")
    c = _down_case(3, 5, 7, 64, 128, True)
    conv, bn, p = c["conv"], c["norm"], c["packed"]
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    w = (conv.weight * s[:, None, None, None]).half()
    assert float((p.weight_oihw().float() - w.float()).abs().max()) <= 2.0 ** -10 * float(w.detach().abs().max())
    assert torch.allclose(p.bias, (conv.bias - bn.running_mean) * s + bn.bias, rtol=1e-6, atol=1e-7)


def test_the_stem_s_packed_form_pads_with_zeros():
    c = _stem_case(2, 5, 9, False)
    p = c["packed"]
    assert p.w.dtype == torch.float16 and tuple(p.w.shape) == (64, 416) and p.bias.dtype == torch.float32
    assert torch.equal(p.weight_oihw(), c["conv"].weight.detach().half())
    assert torch.equal(p.bias, c["conv"].bias.detach().float())
    taps = p.w.reshape(64, 52, 8)
    assert not bool(taps[:, 49:].any()) and not bool(taps[:, :, 6:].any()), "the padding of the packed row is not zero"
    c = _stem_case(2, 5, 9, True)
    conv, bn = c["conv"], c["norm"]
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    w = (conv.weight * s[:, None, None, None]).half()
    assert float((c["packed"].weight_oihw().float() - w.float()).abs().max()) <= 2.0 ** -10 * float(w.detach().abs().max())
    assert torch.allclose(c["packed"].bias, (conv.bias - bn.running_mean) * s + bn.bias, rtol=1e-6, atol=1e-7)


def test_fewer_input_channels_and_more_output_channels_in_the_stem():
    from pedp_hip.conv import conv_stem

    for cin, cout in ((1, 32), (8, 96), (4, 160)):                     # a partial channel tile; two and three tiles
        c = _stem_case(2, 13, 17, True, cin, cout)
        _check(conv_stem(c["x32"], None, c["packed"], relu=False), c, False, f"stem {cin} -> {cout}")


# ---------------------------------------------------------------- A and B from two tensors

@pytest.mark.parametrize("n0,n", [(1, 2), (2, 3)])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_two_inputs_equal_their_concatenation_and_each_alone(n0, n, dtype):
    from pedp_hip.conv import conv_stem

    c = _stem_case(3, 13, 17, True)
    x = (c["x32"] if dtype == "float32" else c["x16"])[:n]
    a, b = x[:n0].clone(), x[n0:].clone()
    whole = conv_stem(x.clone(), None, c["packed"])
    split = conv_stem(a, b, c["packed"])
    assert torch.equal(split, whole), "A and B from two tensors differ from cat([A, B])"
    assert torch.equal(conv_stem(a, None, c["packed"]), whole[:n0]) and torch.equal(conv_stem(b, None, c["packed"]), whole[n0:])
    assert torch.equal(conv_stem(a, b[:0], c["packed"]), whole[:n0])
    _check(split, {k: (v[:n] if k in ("pre", "mag") else v) for k, v in c.items()}, True, f"stem split {n0}/{n} {dtype}")


def test_strided_3x3_tile_straddling_images_equals_each_image_alone():
    from pedp_hip.conv import conv_strided

    c = _down_case(2, 9, 11, 256, 512)                                 # 30 output pixels per image: one tile holds both
    whole = conv_strided(c["x"], c["packed"])
    for k in range(2):
        assert torch.equal(whole[k:k + 1], conv_strided(c["x"][k:k + 1].contiguous(), c["packed"]))


# ---------------------------------------------------------------- the tap map

def _coded_weights(cout, cin, k, as_bits):
    """Cout x Cin x k x k float16, every (co mod 8, ci, ky, kx) its own value: small integers -n .. n without 0, or, where
    there are more codes than integers float16 holds exactly (as_bits), consecutive float16 bit patterns from 1.0 on."""
    co, ci, ky, kx = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(k), torch.arange(k), indexing="ij")
    code = ((ky * k + kx) * cin + ci) * 8 + co % 8
    n = 8 * cin * k * k
    if as_bits:
        assert n < 0x3C00
        return (code + 0x3C00).to(torch.int16).view(torch.float16)
    assert n // 2 + 1 <= 2048
    v = code - n // 2
    return (v + (v >= 0)).to(torch.float16)


def _coded_layer(cout, cin, k, as_bits, stride=2):
    """The packed layer with _coded_weights and no bias (stride 1: conv3x3's form, through pack_conv3x3), and the weights."""
    from pedp_hip.conv import pack_conv, pack_conv3x3

    conv = torch.nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, bias=True)
    w = _coded_weights(cout, cin, k, as_bits)
    with torch.no_grad():
        conv.weight.copy_(w.float())
        conv.bias.zero_()
    packed = (pack_conv if stride == 2 else pack_conv3x3)(conv.cuda())
    assert torch.equal(packed.weight_oihw().cpu(), w) and len(torch.unique(w[:8])) == 8 * cin * k * k
    return packed, w.double()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_stem_tap_map_is_exact(dtype):
    from pedp_hip.conv import conv_stem

    packed, w64 = _coded_layer(64, 6, 7, False)
    n, h, w = 2, 40, 70                                                # 20 x 35 outputs: 3 x 3 tiles of 8 x 16 per image
    for img, ci, y, x in ((0, 0, 0, 0), (1, 5, 39, 69), (1, 2, 0, 33), (0, 3, 16, 33), (1, 4, 17, 32), (0, 1, 23, 0)):
        src = torch.zeros((n, 6, h, w), dtype=getattr(torch, dtype))
        src[img, ci, y, x] = 1.0
        want = F.conv2d(src.double(), w64, None, 2, 3).permute(0, 2, 3, 1)
        got = conv_stem(src[:1].cuda(), src[1:].cuda(), packed, relu=False).double().cpu()
        assert int((want != 0).sum()) >= 64 * 4
        assert torch.equal(got, want), f"a 1 at image {img}, channel {ci}, ({y}, {x}): {int((got != want).sum())} elements differ"


@pytest.mark.parametrize("cin,cout,as_bits", [(32, 32, False), (64, 128, True), (96, 160, True)], ids=["32", "64", "96"])
def test_strided_3x3_tap_map_is_exact(cin, cout, as_bits):
    """32 channels take the kernel's 32-channel K step with integer codes; 64 channels (4608 codes, more than the integers
    float16 holds exactly) take the 64-channel step the networks' layers use, with bit-pattern codes; 96 channels (6912
    codes) take three 32-channel steps per tap, the ones at channels 95 and 48 in the third and the second, and 160 output
    channels end in a tile of 32 behind a full one."""
    from pedp_hip.conv import conv_strided

    packed, w64 = _coded_layer(cout, cin, 3, as_bits)
    n, h, w = 3, 13, 21                                                # 7 x 11 outputs per image: the 231 pixels fill two tiles
    for img, ci, y, x in ((0, 0, 0, 0), (2, cin - 1, 12, 20), (1, 7, 0, 10), (1, cin // 2, 6, 9), (1, 3, 7, 20), (2, 1, 5, 0)):
        src = torch.zeros((n, h, w, cin), dtype=torch.float16)
        src[img, y, x, ci] = 1.0
        want = F.conv2d(src.double().permute(0, 3, 1, 2), w64, None, 2, 1).permute(0, 2, 3, 1)
        got = conv_strided(src.cuda(), packed, relu=False).double().cpu()
        assert int((want != 0).sum()) >= cout
        assert torch.equal(got, want), f"a 1 at image {img}, channel {ci}, ({y}, {x}): {int((got != want).sum())} elements differ"


# ---------------------------------------------------------------- destination, determinism

def test_destination_with_its_own_channel_stride_and_offset():
    from pedp_hip.conv import conv_stem, conv_strided

    c = _stem_case(3, 13, 17, True)
    d = _down_case(3, 5, 7, 64, 128)
    for what, c_, run in (("stem", c, lambda **kw: conv_stem(c["x32"][:2], c["x32"][2:], c["packed"], **kw)),
                          ("3x3/2", d, lambda **kw: conv_strided(d["x"], d["packed"], **kw))):
        dense = run()
        n, oh, ow, cout = dense.shape
        _check(dense, c_, True, what)
        pattern = (torch.arange(n * oh * ow * (2 * cout + 32), device="cuda") % 251).half().reshape(n, oh, ow, 2 * cout + 32)
        for c0 in (0, 32, cout + 32):
            out = pattern.clone()
            got = run(out=out, out_c0=c0)
            assert got.data_ptr() == out[..., c0:].data_ptr() and tuple(got.shape) == tuple(dense.shape)
            assert torch.equal(out[..., c0:c0 + cout], dense), f"{what}: y_c0 = {c0} differs from the dense call"
            assert torch.equal(out[..., :c0], pattern[..., :c0]) and torch.equal(out[..., c0 + cout:], pattern[..., c0 + cout:]), \
                f"{what}: channels outside {c0} .. {c0 + cout} were written"


@pytest.mark.parametrize("pixels", [(3, 5, 7), (2, 9, 11)], ids=_ids)
def test_partial_channel_tile_into_a_destination_with_its_own_stride_and_offset(pixels):
    """96 -> 224 channels: the second channel tile holds 96 of 128; the channels on both sides of the slice stay."""
    from pedp_hip.conv import conv_strided

    c = _down_case(*pixels, 96, 224)
    dense = conv_strided(c["x"], c["packed"], relu=False)
    _check(dense, c, False, f"3x3/2 {pixels} 96 -> 224")
    n, oh, ow, cout = dense.shape
    pattern = (torch.arange(n * oh * ow * (2 * cout + 32), device="cuda") % 251).half().reshape(n, oh, ow, 2 * cout + 32)
    for c0 in (32, cout + 32):
        out = pattern.clone()
        got = conv_strided(c["x"], c["packed"], relu=False, out=out, out_c0=c0)
        assert got.data_ptr() == out[..., c0:].data_ptr()
        assert torch.equal(out[..., c0:c0 + cout], dense), f"y_c0 = {c0} differs from the dense call"
        assert torch.equal(out[..., :c0], pattern[..., :c0]) and torch.equal(out[..., c0 + cout:], pattern[..., c0 + cout:]), \
            f"channels outside {c0} .. {c0 + cout} were written"


def test_two_calls_give_identical_bits():
    from pedp_hip.conv import conv_stem, conv_strided

    c = _stem_case(2, 160, 160, True)
    for x in (c["x32"], c["x16"]):
        assert torch.equal(conv_stem(x[:1], x[1:], c["packed"]), conv_stem(x[:1], x[1:], c["packed"]))
    assert torch.equal(conv_stem(c["x32"], None, c["packed"]), conv_stem(c["x16"], None, c["packed"])), \
        "float32 input is not rounded to float16 to nearest even"
    for shape in ((2, 80, 80, 64, 128), (2, 40, 40, 256, 512)):
        d = _down_case(*shape)
        a = conv_strided(d["x"], d["packed"])
        assert torch.equal(a, conv_strided(d["x"], d["packed"]))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        x2 = d["x"] * 1.0                                              # produced on this stream just before the call
        on_side = conv_strided(x2, d["packed"])
    s.synchronize()
    assert torch.equal(on_side, a)


# ---------------------------------------------------------------- what is refused

def test_stride_1_belongs_to_conv3x3():
    """The choice: the new entry points refuse a stride-1 layer; conv3x3 is its call."""
    from pedp_hip import _lib
    from pedp_hip.conv import conv_strided, pack_conv, pack_conv3x3

    conv = torch.nn.Conv2d(64, 64, 3, 1, 1).cuda()
    with pytest.raises(_lib.PedpError):
        pack_conv(conv)
    x = torch.zeros((1, 4, 4, 64), dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.PedpError):
        conv_strided(x, pack_conv3x3(conv))


def test_bad_arguments_launch_nothing():
    from pedp_hip import _lib
    from pedp_hip.conv import conv_stem, conv_strided, pack_conv

    lib, ctx = _lib.load(), _lib.default_context()
    c, d = _stem_case(2, 5, 9, True), _down_case(3, 5, 7, 64, 128)
    E = _lib.PedpError
    sentinel = torch.full((3, 3, 4, 128), 7.0, dtype=torch.float16, device="cuda")
    out = sentinel.clone()
    with pytest.raises(E):                                             # a residual with stride 2
        conv_strided(d["x"], d["packed"], out=out, residual=out)
    for bad in (d["x"].float(), d["x"][..., :32], d["x"].cpu(), d["x"].permute(0, 2, 1, 3), d["x"][:, :, ::2]):
        with pytest.raises(E):
            conv_strided(bad, d["packed"], out=out if bad.is_cuda else None)
    for shape, dt in (((3, 5, 7, 128), torch.float16), ((3, 3, 4, 96), torch.float16), ((3, 3, 4, 128), torch.float32)):
        with pytest.raises(E):                                         # an `out` of the wrong size (or type)
            conv_strided(d["x"], d["packed"], out=torch.empty(shape, dtype=dt, device="cuda"))
    with pytest.raises(E):
        conv_strided(d["x"], d["packed"], out=out, out_c0=32)
    with pytest.raises(E):
        conv_strided(d["x"], c["packed"])                              # the stem's weights
    assert torch.equal(out, sentinel), "a refused call wrote its destination"

    sent2 = torch.full((2, 3, 5, 64), 7.0, dtype=torch.float16, device="cuda")
    out2 = sent2.clone()
    x = c["x32"]
    with pytest.raises(E):                                             # Cin = 9
        pack_conv(torch.nn.Conv2d(9, 64, 7, 2, 3).cuda())
    with pytest.raises(E):
        conv_stem(torch.zeros((2, 9, 5, 9), device="cuda"), None, c["packed"], out=out2)
    nhwc = x.contiguous(memory_format=torch.channels_last)
    assert not nhwc.is_contiguous()
    for bad in (nhwc, x.permute(0, 2, 3, 1).contiguous(), x[:, :, :, ::2], x.double(), x.cpu()):
        with pytest.raises(E):                                         # NHWC input, non-contiguous input, another dtype
            conv_stem(bad, None, c["packed"], out=out2 if bad.is_cuda else None)
    with pytest.raises(E):
        conv_stem(x[:1], x[1:].half(), c["packed"], out=out2)
    with pytest.raises(E):
        conv_stem(x[:1], x[1:, :, :4].contiguous(), c["packed"], out=out2)
    with pytest.raises(E):
        conv_stem(x, None, d["packed"])
    for wrong in ((2, 5, 9, 64), (3, 3, 5, 64), (2, 3, 5, 32)):
        with pytest.raises(E):
            conv_stem(x, None, c["packed"], out=torch.empty(wrong, dtype=torch.float16, device="cuda"))
    assert torch.equal(out2, sent2), "a refused call wrote its destination"

    # the C entry points themselves
    def call(x_, x2_, p, res=None, y=out2, **kw):
        prm = _lib.Conv2dParams()
        prm.N, prm.H, prm.W, prm.Cin, prm.Cout, prm.KH, prm.KW, prm.stride, prm.pad = 2, 5, 9, 6, 64, 7, 7, 2, 3
        prm.layout, prm.dtype, prm.N0, prm.y_ld, prm.y_c0, prm.relu = _lib.NCHW, _lib.F32, 2, 64, 0, 1
        for k, v in kw.items():
            setattr(prm, k, v)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        return lib.pedp_conv2d_f16(ctx._h, C.byref(prm), ptr(x_), ptr(x2_), ptr(p.w), ptr(p.bias), ptr(res), ptr(y))

    torch.cuda.synchronize()
    for kw in ({"Cin": 9}, {"Cin": 0}, {"Cout": 48}, {"layout": _lib.NHWC}, {"dtype": _lib.U8}, {"stride": 1}, {"stride": 3},
               {"pad": 2}, {"KH": 5}, {"N": 0}, {"H": 0}, {"N0": 1}, {"N0": 3}, {"y_ld": 32}, {"y_c0": 2}, {"y_c0": -4}):
        assert call(x, None, c["packed"], **kw) == BAD_ARG, kw
    assert call(x, None, c["packed"], res=out2) == BAD_ARG
    assert call(x[:1], x[1:], c["packed"], N0=3) == BAD_ARG
    down = dict(N=3, H=5, W=7, Cin=64, Cout=128, KH=3, KW=3, pad=1, layout=_lib.NHWC, dtype=_lib.F16, N0=3, y_ld=128)
    for kw in ({"stride": 1}, {"Cin": 48}, {"layout": _lib.NCHW}, {"dtype": _lib.F32}, {"pad": 0}, {"Cin": 544}):
        assert call(d["x"], None, d["packed"], y=out, **{**down, **kw}) == BAD_ARG, kw
    assert call(d["x"], None, d["packed"], res=out, y=out, **down) == BAD_ARG
    assert call(d["x"], d["x"], d["packed"], y=out, **down) == BAD_ARG
    wp = torch.zeros((64, 416), dtype=torch.float16, device="cuda")
    b = torch.zeros(64, dtype=torch.float32, device="cuda")
    w9 = torch.zeros((64, 9, 7, 7), device="cuda")
    for cin, cout, kh, kw_ in ((9, 64, 7, 7), (6, 48, 7, 7), (6, 64, 5, 5), (6, 64, 3, 3), (6, 64, 7, 3)):
        assert lib.pedp_conv2d_pack(ctx._h, cin, cout, kh, kw_, C.c_void_p(w9.data_ptr()), None, None, None, None, None, 0.0,
                                    C.c_void_p(wp.data_ptr()), C.c_void_p(b.data_ptr())) == BAD_ARG, (cin, cout, kh, kw_)
    ctx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(out2, sent2) and torch.equal(out, sentinel) and not bool(wp.any()), "a refused call wrote its destination"
    assert call(x, None, c["packed"]) == 0 and call(d["x"], None, d["packed"], y=out, **down) == 0
    ctx.synchronize()
    assert torch.equal(out2, conv_stem(x, None, c["packed"])) and torch.equal(out, conv_strided(d["x"], d["packed"]))
