"""The linear layers of the networks' heads on libpedp_hip.so (csrc/pedp_linear.hip).

    pack_linear(linear)                           an nn.Linear's float16 weight and float32 bias, made once
    linear(x, packed, relu=False, pos=, period=)  F.linear (and relu) on ... x K float16 rows, the position table added on the way in
    linear_add_norm(x, packed, residual, norm)    norm(residual + F.linear(x)) of a post-norm encoder layer, one launch
    token_pool(x, groups, packed=None, out=None)  the mean over each group's tokens, and a small Linear of it
    self_attention_fused(mha, x, packs, pos=)     in-projection, attention.mha_core, out-projection: three launches
    attention_pooled_fused(mha, x, packs, pos=)   the same followed by the mean over the tokens, the mean taken first
    encoder_layer_fused(layer, x, packs, pos, period)   a post-norm relu nn.TransformerEncoderLayer in five launches
    encoder_layer_formula / pooled_linear_formula       the same decompositions in plain torch (any device and dtype)

float16 CUDA tensors only.  The kernels run on the caller's current torch stream with no host wait.  There is no torch
fallback here: a shape, dtype or device the kernels do not take raises.
"""
import ctypes as C

from . import _lib
from ._bridge import launch, ptr
from .attention import _check_mha, _check_post_norm_relu, mha_core

LN_N = 512
POOL_E = 512


class PackedLinear:
    """weight: N x K float16, bias: N float32 or None, both contiguous on the module's device."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias
        self.n, self.k = (int(v) for v in weight.shape)


def pack_linear(linear, weight=None, bias=None):
    """The packed form of an nn.Linear (or of a weight / bias pair, e.g. an attention's in-projection)."""
    import torch

    if weight is None:
        weight, bias = linear.weight, linear.bias
    with torch.no_grad():
        w = weight.detach().to(torch.float16).contiguous().clone()
        b = None if bias is None else bias.detach().to(torch.float32).contiguous().clone()
    if w.dim() != 2:
        raise _lib.PedpError("pack_linear: the weight must be N x K")
    return PackedLinear(w, b)


def pack_f32(linear):
    """token_pool's form of a small nn.Linear: float32 weight and bias."""
    import torch

    with torch.no_grad():
        w = linear.weight.detach().to(torch.float32).contiguous().clone()
        b = None if linear.bias is None else linear.bias.detach().to(torch.float32).contiguous().clone()
    return PackedLinear(w, b)


def _rows2d(t, name, c):
    """(rows, row stride) of a ... x c float16 CUDA tensor whose rows lie at one stride with contiguous channels."""
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float16 and t.dim() >= 2):
        raise _lib.PedpError(f"linear: {name} must be a ... x {c} float16 CUDA tensor")
    shape, stride = [int(v) for v in t.shape], [int(v) for v in t.stride()]
    if shape[-1] != c or (stride[-1] != 1 and c != 1):
        raise _lib.PedpError(f"linear: {name} must have {c} contiguous channels, got shape {tuple(shape)}, strides {tuple(stride)}")
    ld, rows = stride[-2], shape[-2]
    for n, s in zip(reversed(shape[:-2]), reversed(stride[:-2])):      # the leading axes must continue the rows
        if n != 1 and s != rows * ld:
            raise _lib.PedpError(f"linear: {name}'s rows must lie at one stride, got shape {tuple(shape)}, strides {tuple(stride)}")
        rows *= n
    if rows == 1:
        ld = max(ld, c)
    return rows, ld


def _table(pos, period, cols, who):
    import torch

    if pos is None:
        if period is not None:
            raise _lib.PedpError(f"{who}: a period without a position table")
        return None, 0, 0
    if period is None:
        raise _lib.PedpError(f"{who}: a position table needs its period")
    if not (isinstance(pos, torch.Tensor) and pos.is_cuda and pos.dtype == torch.float32 and pos.is_contiguous()):
        raise _lib.PedpError(f"{who}: pos must be a contiguous float32 CUDA tensor")
    if pos.dim() == 3 and pos.shape[0] == 1:
        pos = pos[0]
    if pos.dim() != 2 or int(pos.shape[1]) != cols:
        raise _lib.PedpError(f"{who}: pos must be rows x {cols}, got {tuple(pos.shape)}")
    return pos, int(pos.shape[0]), int(period)


def _run(who, x, packed, epilogue, res, pos, period, norm, out, pos_on_x):
    import torch

    if not isinstance(packed, PackedLinear) or packed.weight.dtype != torch.float16:
        raise _lib.PedpError(f"{who}: `packed` must come from pack_linear")
    m, x_ld = _rows2d(x, "x", packed.k)
    n = packed.n
    if packed.weight.device != x.device:
        raise _lib.PedpError(f"{who}: x is on {x.device}, the weights on {packed.weight.device}")
    if out is None:
        out = torch.empty((*x.shape[:-1], n), dtype=torch.float16, device=x.device)
    elif out.device != x.device:
        raise _lib.PedpError(f"{who}: out must be on {x.device}")
    mo, y_ld = _rows2d(out, "out", n)
    if mo != m:
        raise _lib.PedpError(f"{who}: out has {mo} rows for x's {m}")
    prm = _lib.LinearParams()
    prm.M, prm.N, prm.K, prm.x_ld, prm.y_ld, prm.epilogue = m, n, packed.k, x_ld, y_ld, epilogue
    gamma = beta = None
    if epilogue == _lib.LINEAR_ADD_LN:
        mr, prm.res_ld = _rows2d(res, "residual", n)
        if mr != m or res.device != x.device:
            raise _lib.PedpError(f"{who}: residual must have x's {m} rows on {x.device}")
        if tuple(norm.normalized_shape) != (n,) or norm.weight is None:
            raise _lib.PedpError(f"{who}: norm must be an affine LayerNorm over the {n} channels")
        gamma = norm.weight.detach()
        beta = None if norm.bias is None else norm.bias.detach()
        for name, p in (("weight", gamma), ("bias", beta)):
            if p is not None and not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise _lib.PedpError(f"{who}: the norm's {name} must be a contiguous float32 CUDA tensor")
        prm.eps = float(norm.eps)
        pos, prm.pos_rows, prm.pos_period = _table(pos, period, n, who)
        prm.pos_a = int(bool(pos_on_x)) if pos is not None else 0
    else:
        pos, prm.pos_rows, prm.pos_period = _table(pos, period, packed.k, who)
    launch(x.device, "pedp_linear_f16", lambda lib, hd, mem: lib.pedp_linear_f16(
        hd, C.byref(prm), ptr(x), ptr(packed.weight), ptr(packed.bias), ptr(res), ptr(pos), ptr(gamma), ptr(beta), ptr(out)))
    return out


def linear(x, packed, relu=False, pos=None, period=None, out=None):
    """F.linear(x, W, b), with relu=True relu of it: x ... x K float16 (dense or a view with a larger row stride) -> ... x N
    float16 (pedp_linear_f16).  pos (rows x K float32) with `period` S: row r of x is taken as half(x[r] + pos[r % S])."""
    return _run("linear", x, packed, _lib.LINEAR_RELU if relu else _lib.LINEAR_PLAIN, None, pos, period, None, out, True)


def linear_add_norm(x, packed, residual, norm, pos=None, period=None, out=None, pos_on_x=True):
    """norm(residual + F.linear(x, W, b)) over rows of N = 512, `norm` an affine nn.LayerNorm.  pos (rows x 512 float32) with
    `period` S is added in float32 to residual row r as pos[r % S], and with pos_on_x (the default) to x's row as in
    `linear`; an out-projection, whose x is the attention's output, passes pos_on_x=False.  out may be `residual` itself."""
    return _run("linear_add_norm", x, packed, _lib.LINEAR_ADD_LN, residual, pos, period, norm, out, pos_on_x)


def token_pool(x, groups, packed=None, out=None):
    """x: ... x 512 float16 rows in `groups` groups of consecutive rows -> groups x 512 float16, each group's float32 mean; with
    `packed` (pack_f32 of an nn.Linear(512, n <= 8)) groups x n: the Linear of the mean, which is the mean of the Linear.
    out: a contiguous float16 destination of that shape."""
    import torch

    rows, x_ld = _rows2d(x, "x", POOL_E)
    groups = int(groups)
    if groups < 1 or rows % groups:
        raise _lib.PedpError(f"token_pool: {rows} rows do not split into {groups} groups")
    prm = _lib.TokenPoolParams()
    prm.B, prm.S, prm.E, prm.x_ld = groups, rows // groups, POOL_E, x_ld
    w = b = None
    if packed is not None:
        if not isinstance(packed, PackedLinear) or packed.weight.dtype != torch.float32 or packed.k != POOL_E:
            raise _lib.PedpError("token_pool: `packed` must come from pack_f32 of a Linear(512, n)")
        if packed.weight.device != x.device:
            raise _lib.PedpError(f"token_pool: x is on {x.device}, the weights on {packed.weight.device}")
        w, b, prm.n_out = packed.weight, packed.bias, packed.n
    shape = (groups, prm.n_out if w is not None else POOL_E)
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=x.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float16 and out.device == x.device and tuple(out.shape) == shape
              and out.is_contiguous()):
        raise _lib.PedpError(f"token_pool: out must be a contiguous {shape} float16 tensor on {x.device}")
    launch(x.device, "pedp_token_pool_f16", lambda lib, hd, mem: lib.pedp_token_pool_f16(
        hd, C.byref(prm), ptr(x), ptr(w), ptr(b), ptr(out)))
    return out


# ---------------------------------------------------------------- the heads' modules over the three kernels

def pack_attention(mha):
    """{'in': ..., 'out': ...}: the packed projections of an nn.MultiheadAttention."""
    _check_mha(mha, "pack_attention")
    return {"in": pack_linear(None, mha.in_proj_weight, mha.in_proj_bias), "out": pack_linear(mha.out_proj)}


def pack_encoder_layer(layer):
    """The packed linears of an nn.TransformerEncoderLayer: the attention's two and the feed-forward's two."""
    return {**pack_attention(layer.self_attn), "linear1": pack_linear(layer.linear1), "linear2": pack_linear(layer.linear2)}


def self_attention_fused(mha, x, packs, pos=None, period=None, qkv=None, attn=None, out=None):
    """`mha(x + pos, x + pos, x + pos, need_weights=False)[0]` on x: B x S x E float16: in-projection with the table, mha_core,
    out-projection.  qkv (B x S x 3E), attn and out (B x S x E): destinations to reuse."""
    _check_mha(mha, "self_attention_fused")
    qkv = linear(x, packs["in"], pos=pos, period=period, out=qkv)
    o = mha_core(qkv, mha.num_heads, out=attn)
    return linear(o, packs["out"], out=out)


def attention_pooled_fused(mha, x, packs, pos=None, period=None, qkv=None, attn=None):
    """`mha(x + pos, ...)[0].mean(1)` on x: B x S x E float16 -> B x E: in-projection with the table, mha_core, the mean over
    the tokens, and the out-projection of the B means -- the mean and a Linear commute, so the out-projection runs on B rows
    instead of B * S and no per-token result is rounded to float16 before the mean."""
    _check_mha(mha, "attention_pooled_fused")
    qkv = linear(x, packs["in"], pos=pos, period=period, out=qkv)
    o = mha_core(qkv, mha.num_heads, out=attn)
    return linear(token_pool(o, len(x)), packs["out"])


def encoder_layer_fused(layer, x, packs, pos=None, period=None, qkv=None, attn=None, out=None):
    """`layer(x + pos)` of an nn.TransformerEncoderLayer with torch's defaults (post-norm, relu, eval) on the raw tokens
    x: B x S x 512 float16, in five launches: in-projection with the table, mha_core, out-projection + add + norm1 (the table
    added to the residual), linear1 + relu (into `attn`), linear2 + add + norm2 (in place).  Returns `out`."""
    _check_post_norm_relu(layer, "encoder_layer_fused")
    _check_mha(layer.self_attn, "encoder_layer_fused")
    qkv = linear(x, packs["in"], pos=pos, period=period, out=qkv)
    o = mha_core(qkv, layer.self_attn.num_heads, out=attn)
    y = linear_add_norm(o, packs["out"], x, layer.norm1, pos=pos, period=period, out=out, pos_on_x=False)
    h = linear(y, packs["linear1"], relu=True, out=o if packs["linear1"].n == o.shape[-1] else None)
    return linear_add_norm(h, packs["linear2"], y, layer.norm2, out=y)


def encoder_layer_formula(layer, x, pos, attn):
    """encoder_layer_fused's arithmetic in plain torch at x's dtype; attn(mha, x): the attention with its two projections."""
    import torch
    import torch.nn.functional as F

    xp = x + pos
    y = layer.norm1(xp + attn(layer.self_attn, xp))
    return layer.norm2(y + F.linear(torch.relu(F.linear(y, layer.linear1.weight, layer.linear1.bias)), layer.linear2.weight,
                                    layer.linear2.bias))


def pooled_linear_formula(lin, x):
    """token_pool's arithmetic in plain torch: the Linear of the mean over axis 1."""
    import torch.nn.functional as F

    return F.linear(x.mean(dim=1), lin.weight, lin.bias)
