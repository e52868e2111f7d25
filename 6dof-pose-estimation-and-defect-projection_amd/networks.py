"""FoundationPose's refine and score networks, with their residual blocks on this package's 3x3 convolution kernel.

    RefineNet(cfg, c_in)            learning/models/refine_network.py:26-93      -> {'trans': B x 3, 'rot': B x 3 or B x 6}
    ScoreNetMultiPair(cfg, c_in)    learning/models/score_network.py:27-90       -> {'score_logit': B/L x L}
    load_refiner / load_scorer      the checkpoint loading of predict_pose_refine.py:109-120 and predict_score.py:131-141

The modules are written here after the reference's architecture (network_modules.py); what they share with it is the
contract: `state_dict()` has the reference's keys, shapes, dtypes and order, so a published checkpoint loads with
strict=True.  Weights stay the user's file.

Two forwards.  In eval mode on a GPU under float16 autocast (how the predictors call a network with
amp=True) and with backend 'hip' or 'auto', the twelve stride-1 3x3 convolutions of the residual blocks run through
conv.conv3x3 on channels-last float16 buffers kept per batch size, BatchNorm folded into packed weights that are built
on first use and dropped by load_state_dict, .to() and .train().  Everything else (the stride-2 convolutions unless
strided='hip', the heads unless heads='hip'), and every other case (training, CPU, float32 / float64, backend 'torch'), is plain torch.  Weights changed in
place after the first fused forward are not seen: call `drop_packed()`.

The heads.  With heads='hip', under the same conditions (eval, GPU, float16 autocast), the attention of
the refiner's two encoder layers and of the scorer's `att` and `att_cross` runs through attention.self_attention: torch's
two projection GEMMs around the fused kernel, and no S x S weights are formed.  The default is heads='torch', the stock
modules; in every other case they run whatever `heads` says.

The heads' linear layers.  With linears='hip' together with heads='hip', under the same conditions, the
projections, the feed-forward, both LayerNorms, the position table's add and the final mean and Linear run through
linear.linear, linear.linear_add_norm and linear.token_pool on kept float16 buffers: a refiner head is six launches, and
neither F.linear nor F.layer_norm is called from the heads.  The packed float16 weights live with the packed
convolutions.  The default is linears='torch'.

The stride-2 layers.  With strided='hip', under the same conditions, the three convolutions that halve
the resolution run through conv.conv_stem and conv.conv_strided: the 7x7 stem reads A and B as they arrive (no cat, no
NCHW intermediate, no conversion pass) and the forward is channels-last float16 on kept buffers from the crops to the
tokens, whatever `backend` says about the block convolutions.  The tokens `encode` returns are then a view of a kept
buffer, valid until the next forward of the same batch size.  The default is strided='torch'.
"""
import math

import torch
import torch.nn as nn

from . import attention as _attn
from . import conv as _conv
from . import linear as _lin

_BACKENDS = ("auto", "hip", "torch")
_HEADS = ("torch", "hip")
_STRIDED = ("torch", "hip")
_LINEARS = ("torch", "hip")

# backend 'auto': which path a block convolution of this many channels takes -- the kernel where tools/networks_time.py
# finds it not slower than F.conv2d on the same channels-last float16 tensors, torch otherwise.
# NOT MEASURED YET: no figures exist for either side, so every shape stays on torch until profiles/networks_time.json
# holds the pairs (kernel ms, torch ms) to quote here.
_AUTO = {
    128: "torch",   # 504 images of 40 x 40: unmeasured
    256: "torch",   # 252 images of 40 x 40: unmeasured
    512: "torch",   # 252 images of 20 x 20: unmeasured
}


def _get(cfg, key, default):
    if cfg is None:
        return default
    try:
        v = cfg[key]
    except (KeyError, TypeError, AttributeError, IndexError):
        v = getattr(cfg, key, None)
    return default if v is None else v


class _ConvNormReLU(nn.Module):
    """Convolution, optional BatchNorm2d, ReLU as one `net` (keys net.0.*, net.1.*)."""

    def __init__(self, c_in, c_out, kernel_size, stride, norm):
        super().__init__()
        layers = [nn.Conv2d(c_in, c_out, kernel_size, stride, (kernel_size - 1) // 2, bias=True)]
        if norm:
            layers.append(nn.BatchNorm2d(c_out))
        layers.append(nn.ReLU(inplace=True))
        self.net = nn.Sequential(*layers)

    def forward(self, x):
        return self.net(x)


class _BasicBlock(nn.Module):
    """ResNet basic block without downsampling: relu(bn2(conv2(relu(bn1(conv1(x))))) + x), the convolutions with bias."""

    def __init__(self, planes, norm):
        super().__init__()
        self.conv1 = nn.Conv2d(planes, planes, 3, 1, 1, bias=True)
        if norm:
            self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=True)
        if norm:
            self.bn2 = nn.BatchNorm2d(planes)
        self.norm = bool(norm)

    def forward(self, x):
        out = self.conv1(x)
        if self.norm:
            out = self.bn1(out)
        out = self.relu(out)
        out = self.conv2(out)
        if self.norm:
            out = self.bn2(out)
        out += x
        return self.relu(out)

    def pairs(self):
        return ((self.conv1, self.bn1 if self.norm else None), (self.conv2, self.bn2 if self.norm else None))


class _PositionTable(nn.Module):
    """Sinusoidal position table 1 x max_len x d_model (float32 arithmetic), added to the tokens."""

    def __init__(self, d_model, max_len):
        super().__init__()
        pos = torch.arange(0, max_len).float().unsqueeze(1)
        freq = (torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model)).exp()[None]
        pe = torch.zeros(max_len, d_model).float()
        pe[:, 0::2] = torch.sin(pos * freq)
        pe[:, 1::2] = torch.cos(pos * freq)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x):
        return x + self.pe[:, :x.size(1)]


def _shared_encoder(c_in, norm):
    return nn.Sequential(_ConvNormReLU(c_in, 64, 7, 2, norm), _ConvNormReLU(64, 128, 3, 2, norm), _BasicBlock(128, norm),
                         _BasicBlock(128, norm))


def _pair_encoder(norm):
    return nn.Sequential(_BasicBlock(256, norm), _BasicBlock(256, norm), _ConvNormReLU(256, 512, 3, 2, norm),
                         _BasicBlock(512, norm), _BasicBlock(512, norm))


def _pack_block(conv, bn):
    """A block convolution's packed form; None: a layer the kernel does not take, kept on torch."""
    return _conv.pack_conv3x3(conv, bn) if _conv.supported(conv) else None


def _fp16_autocast():
    return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16


class _PairNet(nn.Module):
    """What both networks share: the two encoders' forward, in torch or fused, and the packed weights' life cycle.
    Subclasses set `_enc_names` to their (shared encoder, pair encoder) attribute names."""

    _enc_names = ("", "")

    def _init_backend(self, backend, heads="torch", strided="torch", linears="torch"):
        # id(conv) -> PackedConv3x3 | PackedConv | None (None: a block layer the kernel does not take, kept on torch);
        # id(a head's module) -> its packed linears (linear.pack_*)
        self._packed = {}
        self._buffers_nhwc = {}
        self._buffers_tok = {}
        self.set_backend(backend)
        self.set_heads(heads)
        self.set_strided(strided)
        self.set_linears(linears)

    def _set(self, name, value, allowed):
        if value not in allowed:
            raise ValueError(f"{name} must be one of {allowed}, got {value!r}")
        setattr(self, name, value)
        return self

    def set_backend(self, backend):
        """'hip': every block convolution through the kernel; 'torch': none; 'auto': per layer by the measured table."""
        return self._set("backend", backend, _BACKENDS)

    def set_heads(self, heads):
        """'hip': the heads' attention through attention.self_attention (eval, GPU, float16 autocast); 'torch': the stock
        modules."""
        return self._set("heads", heads, _HEADS)

    def set_strided(self, strided):
        """'hip': the three stride-2 convolutions through conv.conv_stem / conv.conv_strided (eval, GPU, float16
        autocast); 'torch': the stock modules."""
        return self._set("strided", strided, _STRIDED)

    def set_linears(self, linears):
        """'hip': with heads='hip', the heads' linear layers, LayerNorms and means through linear.linear, linear_add_norm
        and token_pool (eval, GPU, float16 autocast); 'torch': the stock modules."""
        return self._set("linears", linears, _LINEARS)

    def _heads_fused(self, x):
        return self.heads == "hip" and not self.training and x.is_cuda and _fp16_autocast()

    def _linears_fused(self, x):
        return self.linears == "hip" and self._heads_fused(x)

    def drop_packed(self):
        self._packed = {}
        self._buffers_nhwc = {}
        self._buffers_tok = {}

    def _memo(self, module, pack, *args):
        """self._packed's entry of `module`, made by pack(module, *args) on first use."""
        key = id(module)
        if key not in self._packed:
            self._packed[key] = pack(module, *args)
        return self._packed[key]

    @staticmethod
    def _kept(cache, key, make):
        """cache[key], allocated by make() outside inference mode on first use.  A tracker alternates between a few
        batch sizes; do not hoard more: at four keys the cache is cleared."""
        buf = cache.get(key)
        if buf is None:
            if len(cache) >= 4:
                cache.clear()
            with torch.inference_mode(False):
                buf = cache[key] = make()
        return buf

    def _tokens(self, tok, names=("qkv", "a", "y")):
        """The tokens of `encode` as contiguous float16 and the kept buffers `names` of the heads at this batch and length:
        'qkv' bs x S x 1536, 'a' and 'y' bs x S x 512."""
        bs, s, e = (int(v) for v in tok.shape)
        buf = self._kept(self._buffers_tok, (tok.device, bs, s), lambda: {
            n: torch.empty((bs, s, 3 * e if n == "qkv" else e), dtype=torch.float16, device=tok.device) for n in names})
        if tok.dtype != torch.float16 or not tok.is_contiguous():      # the torch encoder's channels-first result
            if "tok" not in buf:
                with torch.inference_mode(False):
                    buf["tok"] = torch.empty((bs, s, e), dtype=torch.float16, device=tok.device)
            buf["tok"].copy_(tok)
            tok = buf["tok"]
        return tok, buf

    def train(self, mode=True):
        self.drop_packed()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self.drop_packed()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.drop_packed()
        return super().load_state_dict(*args, **kwargs)

    # ------------------------------------------------------------ the encoders
    def _encoders(self):
        return getattr(self, self._enc_names[0]), getattr(self, self._enc_names[1])

    def _uses_kernel(self, channels):
        return self.backend == "hip" or (self.backend == "auto" and _AUTO.get(channels, "torch") == "hip")

    def _fused(self, A):
        return ((self.strided == "hip" or any(self._uses_kernel(c) for c in (128, 256, 512))) and not self.training
                and A.is_cuda and _fp16_autocast())

    def encode(self, A, B):
        """The pair encoder's output as tokens, bs x (h/8 * w/8) x 512, before the position table."""
        if self._fused(A):
            return self._encode_fused(A, B)
        bs = len(A)
        enc_a, enc_ab = self._encoders()
        x = enc_a(torch.cat([A, B], dim=0))
        ab = enc_ab(torch.cat((x[:bs], x[bs:]), 1).contiguous())
        return ab.reshape(bs, ab.shape[1], -1).permute(0, 2, 1)

    def _pack(self, conv, bn):
        if not self._uses_kernel(conv.out_channels):
            return None
        return self._memo(conv, _pack_block, bn)

    def _pack_strided(self, block):
        """The packed form of a stride-2 _ConvNormReLU; a layer the kernels do not take raises (conv.pack_conv)."""
        return self._memo(block.net[0], _conv.pack_conv, block.net[1] if isinstance(block.net[1], nn.BatchNorm2d) else None)

    def _conv(self, x, conv, bn, residual=None, out=None, out_c0=0):
        """One block convolution with its norm, optional identity add and ReLU: x, residual N x H x W x C float16 ->
        channels out_c0 ... of `out` (N x H x W x ld)."""
        p = self._pack(conv, bn)
        if p is not None:
            return _conv.conv3x3(x, p, residual=residual, relu=True, out=out, out_c0=out_c0)
        y = conv(x.permute(0, 3, 1, 2))          # a layer kept on torch: autocast's float16 convolution on the same view
        if bn is not None:
            y = bn(y)
        y = y.permute(0, 2, 3, 1)
        if residual is not None:
            y = y + residual
        dst = out[..., out_c0:out_c0 + conv.out_channels]
        dst.copy_(torch.relu(y))
        return dst

    def _scratch(self, dev, bs, h, w, strided_hw=None):
        """The buffers of a forward of `bs` pairs at h x w after the shared encoder's two stride-2 layers; with
        strided_hw = (h1, w1, h3, w3), the sizes after the stem and after the pair encoder's stride-2 layer, also theirs."""
        def e(n, hh, ww, c):
            return torch.empty((n, hh, ww, c), dtype=torch.float16, device=dev)

        def make():
            buf = {"x": e(2 * bs, h, w, 128), "t": e(2 * bs, h, w, 128), "ab": e(bs, h, w, 256), "t2": e(bs, h, w, 256)}
            if strided_hw is not None:
                h1, w1, h3, w3 = strided_hw
                buf.update({"s": e(2 * bs, h1, w1, 64), "y": e(bs, h3, w3, 512), "t3": e(bs, h3, w3, 512)})
            return buf

        return self._kept(self._buffers_nhwc, (dev, bs, h, w, strided_hw), make)

    def _encode_fused(self, A, B):
        bs = len(A)
        enc_a, enc_ab = self._encoders()
        hip = self.strided == "hip"
        if hip:
            if A.dtype != B.dtype or A.dtype not in (torch.float32, torch.float16):
                A, B = A.half(), B.half()                                      # autocast's cast of any other dtype
            h1, w1 = _conv.out_hw(A.shape[2], A.shape[3], enc_a[0].net[0])
            h, w = _conv.out_hw(h1, w1, enc_a[1].net[0])
            buf = self._scratch(A.device, bs, h, w, (h1, w1, *_conv.out_hw(h, w, enc_ab[2].net[0])))
            xa, t, ab, t2 = buf["x"], buf["t"], buf["ab"], buf["t2"]
            _conv.conv_stem(A.contiguous(), B.contiguous(), self._pack_strided(enc_a[0]), out=buf["s"])   # A and B as they are
            _conv.conv_strided(buf["s"], self._pack_strided(enc_a[1]), out=xa)
        else:
            x = enc_a[1](enc_a[0](torch.cat([A, B], dim=0)))               # the two stride-2 convolutions: torch
            h, w = int(x.shape[2]), int(x.shape[3])
            buf = self._scratch(x.device, bs, h, w)
            xa, t, ab, t2 = buf["x"], buf["t"], buf["ab"], buf["t2"]
            xa.copy_(x.permute(0, 2, 3, 1))                                # the one conversion to channels-last float16
        (c1, n1), (c2, n2) = enc_a[2].pairs()
        self._conv(xa, c1, n1, out=t)
        self._conv(t, c2, n2, residual=xa, out=xa)
        (c1, n1), (c2, n2) = enc_a[3].pairs()
        self._conv(xa, c1, n1, out=t)
        self._conv(t[:bs], c2, n2, residual=xa[:bs], out=ab, out_c0=0)     # the A half and the B half land side by side:
        self._conv(t[bs:], c2, n2, residual=xa[bs:], out=ab, out_c0=128)   # the channel concatenation costs no pass
        for blk in (enc_ab[0], enc_ab[1]):
            (c1, n1), (c2, n2) = blk.pairs()
            self._conv(ab, c1, n1, out=t2)
            self._conv(t2, c2, n2, residual=ab, out=ab)
        if hip:
            y, t3 = buf["y"], buf["t3"]
            _conv.conv_strided(ab, self._pack_strided(enc_ab[2]), out=y)       # 256 -> 512, stride 2
        else:
            y = enc_ab[2](ab.permute(0, 3, 1, 2))                          # 256 -> 512, stride 2: torch, zero-copy view
            y = y.permute(0, 2, 3, 1).contiguous()
            if y.dtype != torch.float16:
                y = y.half()
            t3 = torch.empty_like(y)
        for blk in (enc_ab[3], enc_ab[4]):
            (c1, n1), (c2, n2) = blk.pairs()
            self._conv(y, c1, n1, out=t3)
            self._conv(t3, c2, n2, residual=y, out=y)
        return y.reshape(bs, -1, y.shape[3])


class RefineNet(_PairNet):
    """cfg: 'use_BN' (default False), 'rot_rep' ('axis_angle' or '6d', default 'axis_angle'), 'c_in' when the argument
    is None (default 4)."""

    _enc_names = ("encodeA", "encodeAB")

    def __init__(self, cfg=None, c_in=None, n_view=1, backend="auto", heads="torch", strided="torch", linears="torch"):
        super().__init__()
        self.cfg = cfg
        norm = bool(_get(cfg, "use_BN", False))
        c_in = int(_get(cfg, "c_in", 4) if c_in is None else c_in)
        rot_rep = _get(cfg, "rot_rep", "axis_angle")
        if rot_rep not in ("axis_angle", "6d"):
            raise ValueError(f"RefineNet: rot_rep {rot_rep!r}")
        self.encodeA = _shared_encoder(c_in, norm)
        self.encodeAB = _pair_encoder(norm)
        self.pos_embed = _PositionTable(512, 400)
        self.trans_head = nn.Sequential(nn.TransformerEncoderLayer(d_model=512, nhead=4, dim_feedforward=512, batch_first=True),
                                        nn.Linear(512, 3))
        self.rot_head = nn.Sequential(nn.TransformerEncoderLayer(d_model=512, nhead=4, dim_feedforward=512, batch_first=True),
                                      nn.Linear(512, 3 if rot_rep == "axis_angle" else 6))
        self._init_backend(backend, heads, strided, linears)

    def _head_fused(self, head, tok, buf):
        """A head on the raw tokens: the encoder layer in five launches, then the mean and the final Linear in one."""
        y = _lin.encoder_layer_fused(head[0], tok, self._memo(head[0], _lin.pack_encoder_layer), self.pos_embed.pe,
                                     tok.shape[1], qkv=buf["qkv"], attn=buf["a"], out=buf["y"])
        return _lin.token_pool(y, len(tok), self._memo(head[1], _lin.pack_f32))

    def forward(self, A, B):
        tok = self.encode(A, B)
        if self._linears_fused(tok):
            tok, buf = self._tokens(tok)
            return {"trans": self._head_fused(self.trans_head, tok, buf), "rot": self._head_fused(self.rot_head, tok, buf)}
        ab = self.pos_embed(tok)
        if self._heads_fused(ab):
            trans = self.trans_head[1](_attn.encoder_layer(self.trans_head[0], ab))
            rot = self.rot_head[1](_attn.encoder_layer(self.rot_head[0], ab))
            return {"trans": trans.mean(dim=1), "rot": rot.mean(dim=1)}
        return {"trans": self.trans_head(ab).mean(dim=1), "rot": self.rot_head(ab).mean(dim=1)}


class ScoreNetMultiPair(_PairNet):
    """cfg: 'use_BN' (default False), 'c_in' when the argument is None (default 4)."""

    _enc_names = ("encoderA", "encoderAB")

    def __init__(self, cfg=None, c_in=None, backend="auto", heads="torch", strided="torch", linears="torch"):
        super().__init__()
        self.cfg = cfg
        norm = bool(_get(cfg, "use_BN", False))
        c_in = int(_get(cfg, "c_in", 4) if c_in is None else c_in)
        self.encoderA = _shared_encoder(c_in, norm)
        self.encoderAB = _pair_encoder(norm)
        self.att = nn.MultiheadAttention(embed_dim=512, num_heads=4, bias=True, batch_first=True)
        self.att_cross = nn.MultiheadAttention(embed_dim=512, num_heads=4, bias=True, batch_first=True)
        self.pos_embed = _PositionTable(512, 400)
        self.linear = nn.Linear(512, 1)
        self._init_backend(backend, heads, strided, linears)

    def _attend(self, mha, x):
        if self._heads_fused(x):
            return _attn.self_attention(mha, x)
        return mha(x, x, x)[0]

    def extract_feat(self, A, B):
        """A, B: (B*L) x C x H x W -> one 512-vector per pair."""
        tok = self.encode(A, B)
        if self._linears_fused(tok):
            tok, buf = self._tokens(tok, ("qkv", "a"))
            return _lin.attention_pooled_fused(self.att, tok, self._memo(self.att, _lin.pack_attention), self.pos_embed.pe,
                                               tok.shape[1], qkv=buf["qkv"], attn=buf["a"])
        ab = self.pos_embed(tok)
        ab = self._attend(self.att, ab)
        return ab.mean(dim=1).reshape(len(A), -1)

    def forward(self, A, B, L):
        bs = A.shape[0] // L
        x = self.extract_feat(A, B).reshape(bs, L, -1)
        if self._linears_fused(x):
            o = _lin.self_attention_fused(self.att_cross, x, self._memo(self.att_cross, _lin.pack_attention))
            return {"score_logit": _lin.token_pool(o, bs * L, self._memo(self.linear, _lin.pack_f32)).reshape(bs, L)}
        x = self._attend(self.att_cross, x)
        return {"score_logit": self.linear(x).reshape(bs, L)}


def _load(net, path_or_state, device):
    state = path_or_state
    if not hasattr(state, "keys"):
        state = torch.load(state, weights_only=True, map_location="cpu")
    if "model" in state:
        state = state["model"]
    net.load_state_dict(state, strict=True)
    return net.to(device).eval()


def load_refiner(path_or_state, cfg, backend="auto", device="cuda", heads="torch", strided="torch", linears="torch"):
    """RefineNet(cfg) with a checkpoint (a path, a state dict, or {'model': state dict}) loaded strictly, on the GPU in
    eval mode: `PoseRefinePredictor(model=load_refiner(path, cfg), cfg=cfg)`."""
    return _load(RefineNet(cfg, backend=backend, heads=heads, strided=strided, linears=linears), path_or_state, device)


def load_scorer(path_or_state, cfg, backend="auto", device="cuda", heads="torch", strided="torch", linears="torch"):
    """ScoreNetMultiPair(cfg) the same way: `ScorePredictor(model=load_scorer(path, cfg), cfg=cfg)`."""
    return _load(ScoreNetMultiPair(cfg, backend=backend, heads=heads, strided=strided, linears=linears), path_or_state, device)
