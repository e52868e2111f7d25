"""The 3x3 convolution of the networks' residual blocks on libpedp_hip.so (csrc/pedp_conv.hip).

    pack_conv3x3(conv, bn=None)     the Conv2d's weights with the eval-mode BatchNorm2d folded in, as the kernel reads them
    conv3x3(x, packed, ...)         y = act(conv(x, w') + b' [+ residual]) on channels-last float16 CUDA tensors

Stride 1, padding 1, Cin and Cout multiples of 32 up to 512.  Both run on the caller's current torch stream with no host
wait.  There is no torch fallback here: a shape the kernel does not take raises.
"""
import ctypes as C

from . import _lib
from .crop import _launch


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


def pack_conv3x3(conv, bn=None):
    """Fold `bn` (BatchNorm2d in eval mode, or None) into `conv` (Conv2d on a GPU) in float32 and pack (pedp_conv3x3_pack)."""
    import torch

    if not supported(conv):
        raise _lib.PedpError(f"pack_conv3x3: {conv} is not a stride-1, pad-1 3x3 convolution with channels in 32 .. 512 by 32")
    w = _f32(conv.weight)
    if not w.is_cuda:
        raise _lib.PedpError("pack_conv3x3: the module must be on a GPU")
    dev, cin, cout = w.device, conv.in_channels, conv.out_channels
    b = _f32(conv.bias)
    g = be = mu = var = None
    eps = 0.0
    if bn is not None:
        if bn.running_mean is None or bn.running_var is None:
            raise _lib.PedpError("pack_conv3x3: a BatchNorm2d without running statistics cannot be folded")
        ones = torch.ones(cout, dtype=torch.float32, device=dev)
        g = _f32(bn.weight) if bn.weight is not None else ones
        be = _f32(bn.bias) if bn.bias is not None else torch.zeros_like(ones)
        mu, var, eps = _f32(bn.running_mean), _f32(bn.running_var), float(bn.eps)
    with torch.inference_mode(False):
        wp = torch.empty((cout, 9, cin), dtype=torch.float16, device=dev)
        bp = torch.empty((cout,), dtype=torch.float32, device=dev)

    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    _launch(dev, "pedp_conv3x3_pack", lambda lib, hd, mem: lib.pedp_conv3x3_pack(
        hd, cin, cout, p(w), p(b), p(g), p(be), p(mu), p(var), eps, p(wp), p(bp)))
    return PackedConv3x3(wp, bp, cin, cout)


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
    if not (x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 and x.is_contiguous()):
        raise _lib.PedpError("conv3x3: x must be a contiguous N x H x W x Cin float16 CUDA tensor")
    n, h, w, cin = (int(v) for v in x.shape)
    if cin != packed.cin:
        raise _lib.PedpError(f"conv3x3: x has {cin} channels, the weights take {packed.cin}")
    cout = packed.cout
    if out is None:
        out, out_c0 = torch.empty((n, h, w, cout), dtype=torch.float16, device=x.device), 0
    if not (out.is_cuda and out.dtype == torch.float16 and out.dim() == 4 and out.is_contiguous()
            and tuple(out.shape[:3]) == (n, h, w)):
        raise _lib.PedpError(f"conv3x3: out must be a contiguous {n} x {h} x {w} x ld float16 CUDA tensor")
    y_ld, out_c0 = int(out.shape[3]), int(out_c0)
    if out_c0 < 0 or out_c0 + cout > y_ld:
        raise _lib.PedpError(f"conv3x3: channels {out_c0} .. {out_c0 + cout} do not fit a destination of {y_ld}")
    prm = _lib.Conv3x3Params()
    prm.N, prm.H, prm.W, prm.Cin, prm.Cout = n, h, w, cin, cout
    prm.y_ld, prm.y_c0, prm.relu = y_ld, out_c0, int(bool(relu))
    r_ptr = None
    if residual is not None:
        if not (residual.is_cuda and residual.dtype == torch.float16 and tuple(residual.shape) == (n, h, w, cout)):
            raise _lib.PedpError(f"conv3x3: residual must be {n} x {h} x {w} x {cout} float16 on the GPU")
        prm.res_ld, prm.res_c0 = _pixel_stride(residual, "residual"), 0
        r_ptr = C.c_void_p(residual.data_ptr())
    _launch(x.device, "pedp_conv3x3_f16", lambda lib, hd, mem: lib.pedp_conv3x3_f16(
        hd, C.byref(prm), C.c_void_p(x.data_ptr()), C.c_void_p(packed.w.data_ptr()), C.c_void_p(packed.bias.data_ptr()),
        r_ptr, C.c_void_p(out.data_ptr())))
    return out[..., out_c0:out_c0 + cout]
