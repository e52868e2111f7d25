"""The attention core of the networks' heads on libpedp_hip.so (csrc/pedp_attn.hip).

    mha_core(qkv, num_heads, ...)   softmax(scale * q k^T) v per (batch, head) on the packed in-projection output
    attention(q, k, v, ...)         the same on three B x S x E tensors (row-strided views are read in place)
    self_attention(mha, x)          an nn.MultiheadAttention's self-attention: F.linear, mha_core, out_proj
    encoder_layer(layer, x)         a post-norm relu nn.TransformerEncoderLayer with its attention through self_attention
    mha_reference(q, k, v, scale)   the formula in plain torch at the inputs' dtype (any device; the tests' reference)

Head dimension 128 and float16 CUDA tensors only; no mask, no dropout (eval).  The kernel runs on the caller's current
torch stream with no host wait and never forms the S x S weights.  There is no torch fallback here: a shape, dtype or
device the kernel does not take raises.
"""
import ctypes as C
import math

from . import _lib
from ._bridge import launch, ptr

HEAD_DIM = 128


def _rows(t, name, e):
    """Row stride (elements) of a B x S x E view whose rows lie at one stride and whose channels are contiguous."""
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16 and t.dim() == 3):
        raise _lib.PedpError(f"attention: {name} must be a B x S x E float16 CUDA tensor")
    b, s, c = (int(v) for v in t.shape)
    sb, ss, sc = (int(v) for v in t.stride())
    if c != e or not ((sc == 1 or c == 1) and ss >= c and (sb == s * ss or b == 1)):
        raise _lib.PedpError(f"attention: {name} must be B x S x {e} with contiguous channels and one row stride, got shape "
                             f"{tuple(t.shape)} with strides {tuple(t.stride())}")
    return ss


def attention(q, k, v, num_heads, scale=None, out=None):
    """q, k, v: B x S x E float16 CUDA tensors (E = num_heads * 128), dense or views with a larger row stride -> the B x S x E
    result (pedp_mha_f16).  `out`: a B x S x E float16 destination of the same kind that overlaps no input."""
    import torch

    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        raise _lib.PedpError("attention: q must be a B x S x E float16 CUDA tensor")
    b, s, e = (int(x) for x in q.shape)
    h = int(num_heads)
    if h < 1 or e != h * HEAD_DIM:
        raise _lib.PedpError(f"attention: E = {e} with {h} heads is a head dimension of {e / max(h, 1):g}; only {HEAD_DIM} is built")
    if tuple(k.shape) != (b, s, e) or tuple(v.shape) != (b, s, e):
        raise _lib.PedpError(f"attention: k and v must have q's shape {(b, s, e)}")
    if len({q.device, k.device, v.device}) != 1:
        raise _lib.PedpError("attention: q, k and v must be on one device")
    prm = _lib.MhaParams()
    prm.B, prm.S, prm.H, prm.D = b, s, h, HEAD_DIM
    prm.q_ld, prm.k_ld, prm.v_ld = _rows(q, "q", e), _rows(k, "k", e), _rows(v, "v", e)
    if out is None:
        out = torch.empty((b, s, e), dtype=torch.float16, device=q.device)
    elif tuple(out.shape) != (b, s, e) or out.device != q.device:
        raise _lib.PedpError(f"attention: out must be {(b, s, e)} on {q.device}")
    prm.o_ld = _rows(out, "out", e)
    prm.scale = 1.0 / math.sqrt(HEAD_DIM) if scale is None else float(scale)
    launch(q.device, "pedp_mha_f16", lambda lib, hd, mem: lib.pedp_mha_f16(hd, C.byref(prm), ptr(q), ptr(k), ptr(v), ptr(out)))
    return out


def mha_core(qkv, num_heads, scale=None, out=None):
    """qkv: B x S x 3E float16 CUDA tensor, the in-projection's output (q | k | v along the channels, head h of each at
    channel h * 128) -> B x S x E.  The three operands are read in place.  scale: 1 / sqrt(128) when None."""
    import torch

    if not (isinstance(qkv, torch.Tensor) and qkv.dim() == 3 and qkv.shape[2] % 3 == 0):
        raise _lib.PedpError("mha_core: qkv must be a B x S x 3E float16 CUDA tensor")
    e = int(qkv.shape[2]) // 3
    return attention(qkv[..., :e], qkv[..., e:2 * e], qkv[..., 2 * e:], num_heads, scale, out)


def _check_mha(mha, who):
    """The nn.MultiheadAttention the heads' kernels stand in for: anything else is refused in `who`'s name."""
    if (not mha.batch_first or not mha._qkv_same_embed_dim or mha.bias_k is not None or mha.add_zero_attn
            or mha.in_proj_weight is None):
        raise _lib.PedpError(f"{who}: the module must be batch_first with one embed dim and no bias_k / zero attention")
    if mha.training and mha.dropout > 0:
        raise _lib.PedpError(f"{who}: dropout is not built")


def _check_post_norm_relu(layer, who):
    if layer.norm_first or getattr(layer, "activation_relu_or_gelu", 1) != 1:
        raise _lib.PedpError(f"{who}: only the post-norm relu layer is decomposed")


def self_attention(mha, x):
    """`mha(x, x, x, need_weights=False)[0]` of an nn.MultiheadAttention (batch_first, one embed dim for q, k, v, no bias_k /
    zero-attention, eval) on x: B x S x E on a GPU.  The two projections are torch's GEMMs in float16; between them runs
    mha_core."""
    import torch
    import torch.nn.functional as F

    _check_mha(mha, "self_attention")
    if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16:
        cast = lambda t: t                       # autocast makes (and caches) the float16 weights itself
    else:
        cast = lambda t: None if t is None else t.half()
    qkv = F.linear(cast(x), cast(mha.in_proj_weight), cast(mha.in_proj_bias))
    o = mha_core(qkv, mha.num_heads)
    return F.linear(o, cast(mha.out_proj.weight), cast(mha.out_proj.bias))


def encoder_layer(layer, x, attn=self_attention):
    """An nn.TransformerEncoderLayer with torch's defaults (post-norm, relu) in eval mode, decomposed:
    norm1(x + attn(layer.self_attn, x)), then norm2(y + linear2(relu(linear1(y)))).  `attn`: self_attention, or a stand-in
    with its signature."""
    import torch

    _check_post_norm_relu(layer, "encoder_layer")
    y = layer.norm1(x + attn(layer.self_attn, x).to(x.dtype))
    return layer.norm2(y + layer.linear2(torch.relu(layer.linear1(y))).to(y.dtype))


def mha_reference(q, k, v, scale, num_heads=None):
    """softmax(scale * q k^T) v in plain torch at the inputs' dtype.  q, k, v: ... x S x D, or with `num_heads` B x S x E
    split into heads of E / num_heads channels and merged again."""
    import torch

    if num_heads is not None:
        b, s, e = q.shape
        q, k, v = (t.reshape(b, s, num_heads, e // num_heads).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    o = p @ v
    return o if num_heads is None else o.transpose(1, 2).reshape(b, s, e)
