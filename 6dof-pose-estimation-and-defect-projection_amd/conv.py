"""The convolutions of the networks' encoders on libpedp_hip.so (csrc/pedp_conv.hip).

    pack_conv3x3(conv, bn=None)     the Conv2d's weights with the eval-mode BatchNorm2d folded in, as the kernel reads them
    conv3x3(x, packed, ...)         y = act(conv(x, w') + b' [+ residual]) on channels-last float16 CUDA tensors

Stride 1, padding 1, Cin and Cout multiples of 32 up to 512.  The three layers that halve the resolution:

    supported_strided(conv)         3x3 / stride 2 / padding 1 with such channels, or 7x7 / stride 2 / padding 3 with Cin <= 8
    out_hw(h, w, conv)              the output size
    pack_conv(conv, bn=None)        the fold and the packing for either form
    conv_strided(x, packed, ...)    the 3x3 form on channels-last float16
    conv_stem(a, b, packed, ...)    the 7x7 form on one or two NCHW float32 / float16 tensors (`cat([a, b], 0)` is not formed)

All run on the caller's current torch stream with no host wait.  There is no torch fallback here: a shape the kernel does
not take raises.
"""
import ctypes as C

from . import _lib
from ._bridge import launch, ptr


class PackedConv3x3:
    """w: Cout x 9 x Cin float16 (tap = 3 * ky + kx), bias: Cout float32, both with the BatchNorm folded in."""

    def __init__(self, w, bias, cin, cout):
        self.w, self.bias, self.cin, self.cout = w, bias, cin, cout

    def weight_oihw(self):
        """The packed weights as a Cout x Cin x 3 x 3 tensor (float16), as F.conv2d takes them."""
        return self.w.reshape(self.cout, 3, 3, self.cin).permute(0, 3, 1, 2)


def supported(conv):
    """Whether the kernel takes this Conv2d (3x3, stride 1, padding 1, one group, channels multiples of 32 up to 512)."""
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
            and all(32 <= c <= 512 and c % 32 == 0 for c in (conv.in_channels, conv.out_channels)))


def _f32(t):
    import torch

    return None if t is None else t.detach().to(torch.float32).contiguous()


def _pack(who, conv, bn, k):
    """Fold `bn` into `conv` in float32 and pack through `who`'s entry point: the packed weights, the bias, Cin, Cout."""
    import torch

    w = _f32(conv.weight)
    if not w.is_cuda:
        raise _lib.PedpError(f"{who}: the module must be on a GPU")
    dev, cin, cout = w.device, conv.in_channels, conv.out_channels
    b = _f32(conv.bias)
    g = be = mu = var = None
    eps = 0.0
    if bn is not None:
        if bn.running_mean is None or bn.running_var is None:
            raise _lib.PedpError(f"{who}: a BatchNorm2d without running statistics cannot be folded")
        ones = torch.ones(cout, dtype=torch.float32, device=dev)
        g = _f32(bn.weight) if bn.weight is not None else ones
        be = _f32(bn.bias) if bn.bias is not None else torch.zeros_like(ones)
        mu, var, eps = _f32(bn.running_mean), _f32(bn.running_var), float(bn.eps)
    with torch.inference_mode(False):
        wp = torch.empty((cout, 9, cin) if k == 3 else (cout, STEM_K), dtype=torch.float16, device=dev)
        bp = torch.empty((cout,), dtype=torch.float32, device=dev)
    fn_name, dims = ("pedp_conv3x3_pack", (cin, cout)) if who == "pack_conv3x3" else ("pedp_conv2d_pack", (cin, cout, k, k))
    launch(dev, fn_name, lambda lib, hd, mem: getattr(lib, fn_name)(
        hd, *dims, ptr(w), ptr(b), ptr(g), ptr(be), ptr(mu), ptr(var), eps, ptr(wp), ptr(bp)))
    return wp, bp, cin, cout


def pack_conv3x3(conv, bn=None):
    """Fold `bn` (BatchNorm2d in eval mode, or None) into `conv` (Conv2d on a GPU) in float32 and pack (pedp_conv3x3_pack)."""
    if not supported(conv):
        raise _lib.PedpError(f"pack_conv3x3: {conv} is not a stride-1, pad-1 3x3 convolution with channels in 32 .. 512 by 32")
    return PackedConv3x3(*_pack("pack_conv3x3", conv, bn, 3))


def _pixel_stride(t, name):
    """Channel stride of an N x H x W x C view whose pixels lie one after another (a channel slice of a dense buffer)."""
    n, h, w, c = t.shape
    sn, sh, sw, sc = t.stride()
    ld = sw
    ok = (sc == 1 or c == 1) and ld >= c and (sh == w * ld or h == 1) and (sn == h * w * ld or n == 1)
    if not ok:
        raise _lib.PedpError(f"conv3x3: {name} must be a channels-last N x H x W x C tensor or a channel slice of one, "
                             f"got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    return int(ld)


def conv3x3(x_nhwc, packed, residual=None, relu=True, out=None, out_c0=0):
    """x N x H x W x Cin float16, dense -> the N x H x W x Cout result (pedp_conv3x3_f16).  `out`: a dense N x H x W x ld
    float16 buffer whose channels out_c0 .. out_c0 + Cout receive the result (the rest of it is not touched); the returned
    tensor is that slice.  `residual`: N x H x W x Cout float16, dense or a channel slice; it may be the destination."""
    import torch

    x = x_nhwc
    n, h, w, out, y_ld, out_c0 = _operands("conv3x3", x, packed, out, out_c0, 1)
    cin, cout = packed.cin, packed.cout
    prm = _lib.Conv3x3Params()
    prm.N, prm.H, prm.W, prm.Cin, prm.Cout = n, h, w, cin, cout
    prm.y_ld, prm.y_c0, prm.relu = y_ld, out_c0, int(bool(relu))
    if residual is not None:
        if not (residual.is_cuda and residual.dtype == torch.float16 and tuple(residual.shape) == (n, h, w, cout)):
            raise _lib.PedpError(f"conv3x3: residual must be {n} x {h} x {w} x {cout} float16 on the GPU")
        prm.res_ld, prm.res_c0 = _pixel_stride(residual, "residual"), 0
    launch(x.device, "pedp_conv3x3_f16", lambda lib, hd, mem: lib.pedp_conv3x3_f16(
        hd, C.byref(prm), ptr(x), ptr(packed.w), ptr(packed.bias), ptr(residual), ptr(out)))
    return out[..., out_c0:out_c0 + cout]


# ------------------------------------------------------------------ the stride-2 layers

STEM_K = 416    # a packed 7x7 row: 52 taps of 8 channels, the last three taps zero (csrc/conv/stem.h)


class PackedConv:
    """A stride-2 layer as pedp_conv2d_f16 reads it.  3x3: w Cout x 9 x Cin float16; 7x7: w Cout x 416 float16,
    [co][8 * (7 * ky + kx) + ci], zero for ci >= Cin and past tap 48.  bias: Cout float32.  BatchNorm folded into both."""

    def __init__(self, w, bias, cin, cout, k, stride, pad):
        self.w, self.bias, self.cin, self.cout, self.k, self.stride, self.pad = w, bias, cin, cout, k, stride, pad

    def weight_oihw(self):
        """The packed weights as a Cout x Cin x k x k tensor (float16), as F.conv2d takes them."""
        if self.k == 3:
            return self.w.reshape(self.cout, 3, 3, self.cin).permute(0, 3, 1, 2)
        return self.w[:, :49 * 8].reshape(self.cout, 7, 7, 8)[..., :self.cin].permute(0, 3, 1, 2)


def supported_strided(conv):
    """Whether pedp_conv2d_f16 takes this Conv2d: 3x3, stride 2, padding 1 with channels multiples of 32 up to 512, or
    7x7, stride 2, padding 3 with at most 8 input channels and such output channels; one group, no dilation."""
    if not (tuple(conv.stride) == (2, 2) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and conv.padding_mode == "zeros" and 32 <= conv.out_channels <= 512 and conv.out_channels % 32 == 0):
        return False
    if tuple(conv.kernel_size) == (3, 3):
        return tuple(conv.padding) == (1, 1) and 32 <= conv.in_channels <= 512 and conv.in_channels % 32 == 0
    return tuple(conv.kernel_size) == (7, 7) and tuple(conv.padding) == (3, 3) and 1 <= conv.in_channels <= 8


def out_hw(h, w, conv):
    """Height and width of `conv`'s output on an h x w input: (h + 2 * pad - dilation * (k - 1) - 1) // stride + 1."""
    def one(n, i):
        return (n + 2 * conv.padding[i] - conv.dilation[i] * (conv.kernel_size[i] - 1) - 1) // conv.stride[i] + 1
    return one(int(h), 0), one(int(w), 1)


def pack_conv(conv, bn=None):
    """pack_conv3x3 for a stride-2 layer (pedp_conv2d_pack): `bn` (BatchNorm2d in eval mode, or None) folded into `conv`
    (Conv2d on a GPU) in float32."""
    if not supported_strided(conv):
        raise _lib.PedpError(f"pack_conv: {conv} is neither a 3x3 / stride 2 / padding 1 convolution with channels in "
                             "32 .. 512 by 32 nor a 7x7 / stride 2 / padding 3 one with at most 8 input channels")
    k = int(conv.kernel_size[0])
    return PackedConv(*_pack("pack_conv", conv, bn, k), k, 2, (k - 1) // 2)


def _destination(who, out, out_c0, n, oh, ow, cout, dev):
    import torch

    if out is None:
        out, out_c0 = torch.empty((n, oh, ow, cout), dtype=torch.float16, device=dev), 0
    if not (out.is_cuda and out.dtype == torch.float16 and out.dim() == 4 and out.is_contiguous()
            and tuple(out.shape[:3]) == (n, oh, ow)):
        raise _lib.PedpError(f"{who}: out must be a contiguous {n} x {oh} x {ow} x ld float16 CUDA tensor")
    y_ld, out_c0 = int(out.shape[3]), int(out_c0)
    if out_c0 < 0 or out_c0 + cout > y_ld:
        raise _lib.PedpError(f"{who}: channels {out_c0} .. {out_c0 + cout} do not fit a destination of {y_ld}")
    return out, y_ld, out_c0


def _operands(who, x, packed, out, out_c0, stride):
    """conv3x3's and conv_strided's check of x, of its channel count and of the destination of a stride-`stride` layer on
    it: (n, h, w, out, y_ld, out_c0)."""
    import torch

    if not (x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 and x.is_contiguous()):
        raise _lib.PedpError(f"{who}: x must be a contiguous N x H x W x Cin float16 CUDA tensor")
    n, h, w, cin = (int(v) for v in x.shape)
    if cin != packed.cin:
        raise _lib.PedpError(f"{who}: x has {cin} channels, the weights take {packed.cin}")
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    return (n, h, w, *_destination(who, out, out_c0, n, oh, ow, packed.cout, x.device))


def _conv2d(who, prm, packed, x, x2, residual, out):
    prm.Cin, prm.Cout, prm.KH, prm.KW, prm.stride, prm.pad = packed.cin, packed.cout, packed.k, packed.k, packed.stride, packed.pad
    launch(out.device, "pedp_conv2d_f16", lambda lib, hd, mem: lib.pedp_conv2d_f16(
        hd, C.byref(prm), ptr(x), ptr(x2), ptr(packed.w), ptr(packed.bias), ptr(residual), ptr(out)))


def conv_strided(x_nhwc, packed, relu=True, out=None, out_c0=0, residual=None):
    """x N x H x W x Cin float16, dense -> the N x OH x OW x Cout result of a packed 3x3 stride-2 layer (pedp_conv2d_f16);
    `out` and `out_c0` as in conv3x3.  The stride-2 layers add no residual: one is refused, like a stride-1 layer (that is
    conv3x3's)."""
    x = x_nhwc
    if not (isinstance(packed, PackedConv) and packed.k == 3):
        raise _lib.PedpError("conv_strided: the weights must come from pack_conv on a 3x3 stride-2 layer")
    n, h, w, out, y_ld, out_c0 = _operands("conv_strided", x, packed, out, out_c0, 2)
    prm = _lib.Conv2dParams()
    prm.N, prm.H, prm.W, prm.layout, prm.dtype, prm.N0 = n, h, w, _lib.NHWC, _lib.F16, n
    prm.y_ld, prm.y_c0, prm.relu = y_ld, out_c0, int(bool(relu))
    _conv2d("conv_strided", prm, packed, x, None, residual, out)
    return out[..., out_c0:out_c0 + packed.cout]


def conv_stem(a, b, packed, relu=True, out=None, out_c0=0):
    """a Na x Cin x H x W and b Nb x Cin x H x W (or None), contiguous NCHW CUDA tensors of one dtype, float32 or float16 ->
    the (Na + Nb) x OH x OW x Cout channels-last float16 result of a packed 7x7 stride-2 layer on `cat([a, b], 0)`, which
    is not formed (pedp_conv2d_f16).  float32 input is rounded to float16 as autocast's cast does."""
    import torch

    if not (isinstance(packed, PackedConv) and packed.k == 7):
        raise _lib.PedpError("conv_stem: the weights must come from pack_conv on a 7x7 stride-2 layer")
    for t in (a,) if b is None else (a, b):
        if not (t.is_cuda and t.dim() == 4 and t.is_contiguous() and t.dtype in (torch.float32, torch.float16)
                and t.dtype == a.dtype and t.device == a.device and tuple(t.shape[1:]) == tuple(a.shape[1:])):
            raise _lib.PedpError("conv_stem: a and b must be contiguous N x Cin x H x W float32 or float16 CUDA tensors of "
                                 "one dtype and image shape")
    na, cin, h, w = (int(v) for v in a.shape)
    n = na + (0 if b is None else int(b.shape[0]))
    if cin != packed.cin:
        raise _lib.PedpError(f"conv_stem: the input has {cin} channels, the weights take {packed.cin}")
    if b is not None and int(b.shape[0]) == 0:
        b = None
    if na == 0:
        raise _lib.PedpError("conv_stem: a is empty")
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out, y_ld, out_c0 = _destination("conv_stem", out, out_c0, n, oh, ow, packed.cout, a.device)
    prm = _lib.Conv2dParams()
    prm.N, prm.H, prm.W, prm.layout, prm.N0 = n, h, w, _lib.NCHW, na
    prm.dtype = _lib.F32 if a.dtype == torch.float32 else _lib.F16
    prm.y_ld, prm.y_c0, prm.relu = y_ld, out_c0, int(bool(relu))
    _conv2d("conv_stem", prm, packed, a, b, None, out)
    return out[..., out_c0:out_c0 + packed.cout]
