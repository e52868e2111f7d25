"""The attention path without a GPU: mha_reference and the decomposed encoder layer against torch's modules in float64, the
error bound's two facts on the numpy emulation of the kernel (tests/_attn_ref.py), and the networks' `heads` switch on the
CPU, where it must not change a bit."""
import numpy as np
import pytest

import _attn_ref as ar
import _net_fill

torch = pytest.importorskip("torch")


def _seeded(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.1 if p.dim() == 1 else 1.5 / np.sqrt(p.shape[-1])))
    return module.eval()


def _by_reference(mha, x):
    """self_attention's three steps with mha_reference in the middle, at x's dtype."""
    import torch.nn.functional as F
    from pedp_hip.attention import mha_reference

    e = mha.embed_dim
    q, k, v = F.linear(x, mha.in_proj_weight, mha.in_proj_bias).split(e, dim=-1)
    o = mha_reference(q, k, v, 1.0 / np.sqrt(e // mha.num_heads), num_heads=mha.num_heads)
    return F.linear(o, mha.out_proj.weight, mha.out_proj.bias)


@pytest.mark.parametrize("B,S", [(2, 3), (3, 24)])
def test_reference_formula_is_multihead_attention_in_float64(B, S):
    mha = _seeded(torch.nn.MultiheadAttention(512, 4, bias=True, batch_first=True).double(), 1)
    x = torch.randn((B, S, 512), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    with torch.no_grad():
        want, weights = mha(x, x, x)
        got = _by_reference(mha, x)
    assert weights is not None and float((got - want).abs().max()) < 1e-12


def test_reference_formula_on_head_shaped_operands():
    from pedp_hip.attention import mha_reference

    q, k, v = (torch.from_numpy(t.astype(np.float64)) for t in ar.gaussian_qkv(2, 17, 4, seed=5))
    o_ref, _ = ar.reference(q.numpy(), k.numpy(), v.numpy(), 4)
    assert np.abs(mha_reference(q, k, v, ar.SCALE, num_heads=4).numpy() - o_ref).max() < 1e-12
    heads = [t.reshape(2, 17, 4, 128).transpose(1, 2) for t in (q, k, v)]
    assert np.abs(mha_reference(*heads, ar.SCALE).transpose(1, 2).reshape(2, 17, 512).numpy() - o_ref).max() < 1e-12


@pytest.mark.parametrize("B,S", [(2, 16), (1, 5)])
def test_decomposed_encoder_layer_is_the_module_in_float64(B, S):
    from pedp_hip.attention import encoder_layer

    layer = _seeded(torch.nn.TransformerEncoderLayer(d_model=512, nhead=4, dim_feedforward=512, batch_first=True).double(), 3)
    x = torch.randn((B, S, 512), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    with torch.no_grad():
        want = layer(x)
        got = encoder_layer(layer, x, attn=_by_reference)
    assert float((got - want).abs().max()) < 1e-12


def test_encoder_layer_refuses_what_it_does_not_decompose():
    from pedp_hip import PedpError
    from pedp_hip.attention import encoder_layer

    x = torch.zeros((1, 2, 512))
    with pytest.raises(PedpError):
        encoder_layer(torch.nn.TransformerEncoderLayer(512, 4, 512, batch_first=True, norm_first=True).eval(), x, attn=_by_reference)
    with pytest.raises(PedpError):
        encoder_layer(torch.nn.TransformerEncoderLayer(512, 4, 512, batch_first=True, activation="gelu").eval(), x, attn=_by_reference)


def test_kernel_entry_points_refuse_cpu_tensors():
    from pedp_hip import PedpError
    from pedp_hip.attention import mha_core, self_attention

    with pytest.raises(PedpError):
        mha_core(torch.zeros((1, 4, 3 * 128), dtype=torch.float16), 1)
    with pytest.raises(PedpError):
        self_attention(torch.nn.MultiheadAttention(128, 1, batch_first=True).eval(), torch.zeros((1, 4, 128)))


def test_entry_point_checks_its_arguments_before_it_touches_the_device():
    """pedp_mha_f16's checks come before its first use of the context or the GPU, so they run here on host addresses."""
    import ctypes as C

    from pedp_hip import _lib

    lib = _lib.load()
    ctx = C.create_string_buffer(4096)
    buf = C.create_string_buffer(1 << 20)
    base = (C.addressof(buf) + 15) // 16 * 16

    def status(B=2, S=8, H=4, D=128, ld=(1536, 1536, 1536, 512), q=0, k=1024, v=2048, o=1 << 19, scale=0.1, prm=True):
        p = _lib.MhaParams()
        p.B, p.S, p.H, p.D = B, S, H, D
        p.q_ld, p.k_ld, p.v_ld, p.o_ld = ld
        p.scale = scale
        return lib.pedp_mha_f16(C.cast(ctx, C.c_void_p), C.byref(p) if prm else None, C.c_void_p(base + q), C.c_void_p(base + k),
                                C.c_void_p(base + v), C.c_void_p(base + o))

    bad = [dict(D=64), dict(D=256), dict(S=0), dict(S=4097), dict(B=0), dict(H=0), dict(ld=(1540, 1536, 1536, 512)),
           dict(ld=(1536, 1536, 1536, 504)), dict(q=8), dict(o=(1 << 19) + 8), dict(o=0), dict(o=2048), dict(o=1536 * 2 * 15),
           dict(scale=float("nan")), dict(prm=False)]
    for kw in bad:
        assert status(**kw) == -1, kw                                   # PEDP_ERR_BAD_ARG
        assert b"pedp_mha_f16" in lib.pedp_last_error()


# ---------------------------------------------------------------- the bound's two facts

@pytest.mark.parametrize("B,S,H", [(2, 17, 4), (2, 65, 4), (1, 252, 4), (1, 400, 4)])
def test_emulated_kernel_arithmetic_uses_a_part_of_the_bound(B, S, H):
    q, k, v = ar.gaussian_qkv(B, S, H, seed=S)
    o_ref, bound = ar.reference(q, k, v, H)
    share = ar.used_share(ar.emulate(q, k, v, H), o_ref, bound)
    print(f"{B} x {S} x {H}: float32 accumulation, float16 P and result use {share:.3f} of the bound")
    assert 0.05 < share < 1              # 0.33 .. 0.39 on these inputs: the final rounding alone may use half of 2^-11 |o_ref|


@pytest.mark.parametrize("S", [17, 65, 252, 400])
def test_each_designed_fault_exceeds_the_bound(S):
    B, H = 2, 4
    q, k, v = ar.gaussian_qkv(B, S, H, seed=S)
    qd, kd = ar.dominate_last_key(q, k, H)
    o_ref, bound = ar.reference(qd, kd, v, H)
    assert ar.used_share(ar.emulate(qd, kd, v, H), o_ref, bound) < 1
    assert ar.used_share(ar.emulate(qd, kd, v, H, drop_last_key=True), o_ref, bound) > 10      # a tail mask off by one
    loud_k, loud_v = k.copy(), v.copy()
    loud_k[1] = (k[1].astype(np.float32) * 8).astype(np.float16)
    loud_v[1] = 300.0
    o_ref, bound = ar.reference(q, loud_k, loud_v, H)
    assert ar.used_share(ar.emulate(q, loud_k, loud_v, H), o_ref, bound) < 1
    assert ar.used_share(ar.emulate(q, loud_k, loud_v, H, leak_keys=1)[:1], o_ref[:1], bound[:1]) > 10   # a read past the batch
    if S > ar.BK:
        key = S - 1
        ks = ar.spike(q, k, H, S // 3, key)
        o_ref, bound = ar.reference(q, ks, v, H)
        assert ar.used_share(ar.emulate(q, ks, v, H), o_ref, bound) < 1
        assert ar.used_share(ar.emulate(q, ks, v, H, skip_rescale_at=key // ar.BK), o_ref, bound) > 10   # a skipped rescale


@pytest.mark.parametrize("B,S,H", [(1, 129, 5), (1, 1025, 2), (1, 4096, 1)])
def test_emulation_on_the_new_shapes_uses_a_part_of_the_bound(B, S, H):
    """A second query tile with one live row, and 17 and 64 key tiles; the GPU tests' inputs (seed S + 7 B + H)."""
    q, k, v = ar.gaussian_qkv(B, S, H, seed=S + 7 * B + H)
    o_ref, bound = ar.reference(q, k, v, H)
    share = ar.used_share(ar.emulate(q, k, v, H), o_ref, bound)
    print(f"{B} x {S} x {H}: the emulation uses {share:.3f} of the bound")
    assert 0.05 < share < 1


@pytest.mark.parametrize("S,B,H", [(1025, 1, 2), (4096, 1, 1)])
def test_faults_at_the_last_of_many_tiles_exceed_the_bound(S, B, H):
    """The spike at the last key, as tests/test_attention_gpu.py places it: the maximum jumps in the last of 17 and 64 tiles."""
    key = S - 1
    q, k, v = ar.gaussian_qkv(B, S, H, seed=200 + key)
    ks = ar.spike(q, k, H, S // 3, key)
    o_ref, bound = ar.reference(q, ks, v, H)
    share = ar.used_share(ar.emulate(q, ks, v, H), o_ref, bound)
    skipped = ar.used_share(ar.emulate(q, ks, v, H, skip_rescale_at=key // ar.BK), o_ref, bound)
    dropped = ar.used_share(ar.emulate(q, ks, v, H, drop_last_key=True), o_ref, bound)
    print(f"S = {S}, spike at the last key: the emulation uses {share:.3f} of the bound, a skipped rescale at the last tile is "
          f"{skipped:.0f} times the bound, a dropped last key {dropped:.0f} times")
    assert share < 1 and skipped > 10 and dropped > 10


@pytest.mark.parametrize("scale", [0.0, -1.0 / np.sqrt(128), 1.0], ids=["zero", "negative", "one"])
def test_scales_zero_negative_and_one(scale):
    """At scale 0 every row is the mean of the values: the fault that tells is a key too few; at the others also a skipped
    rescale (the maximum moves in the second and third tile of 129 keys for some row)."""
    B, S, H = 2, 129, 2
    q, k, v = ar.gaussian_qkv(B, S, H, seed=3)
    o_ref, bound = ar.reference(q, k, v, H, scale=scale)
    share = ar.used_share(ar.emulate(q, k, v, H, scale=scale), o_ref, bound)
    dropped = ar.used_share(ar.emulate(q, k, v, H, scale=scale, drop_last_key=True), o_ref, bound)
    print(f"scale {scale:.4f}: the emulation uses {share:.3f} of the bound, a dropped last key is {dropped:.0f} times the bound")
    assert share < 1 and dropped > 10
    if scale:
        assert ar.used_share(ar.emulate(q, k, v, H, scale=scale, skip_rescale_at=1), o_ref, bound) > 10


def test_leak_at_129_keys_exceeds_the_bound():
    B, S, H = 3, 129, 4
    q, k, v = ar.gaussian_qkv(B, S, H, seed=100 + S)
    loud_k, loud_v = k.copy(), v.copy()
    loud_k[1] = (k[1].astype(np.float32) * 8).astype(np.float16)
    loud_v[1] = 300.0
    o_ref, bound = ar.reference(q, loud_k, loud_v, H)
    assert ar.used_share(ar.emulate(q, loud_k, loud_v, H), o_ref, bound) < 1
    assert ar.used_share(ar.emulate(q, loud_k, loud_v, H, leak_keys=1)[:1], o_ref[:1], bound[:1]) > 10


# ---------------------------------------------------------------- the networks' switch

def _net(kind, **kw):
    from pedp_hip import networks

    cfg = {"use_BN": True, "rot_rep": "axis_angle"}
    net = (networks.RefineNet if kind == "refiner" else networks.ScoreNetMultiPair)(cfg, c_in=6, **kw)
    torch.manual_seed(0)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn_like(p) * (0.05 if p.dim() > 1 else 0.1))
    return net.eval()


@pytest.mark.parametrize("kind,case", [("refiner", "refiner_3x32x32"), ("scorer", "scorer_4x32x32")])
def test_heads_hip_on_the_cpu_is_the_torch_path(kind, case):
    L = _net_fill.CASES[case][3]
    A, B = _net_fill.inputs(case, torch.float32)
    outs = []
    for heads in ("torch", "hip"):
        net = _net(kind, heads=heads)
        assert net.heads == heads
        with torch.no_grad():
            outs.append(net(A, B) if kind == "refiner" else net(A, B, L=L))
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
    net = _net(kind)
    assert net.heads == "torch" and net.set_heads("hip") is net and net.heads == "hip"
    assert list(net.state_dict().keys()) == list(_net(kind, heads="hip").state_dict().keys())


def test_bad_heads_value():
    from pedp_hip import networks

    with pytest.raises(ValueError):
        networks.RefineNet(heads="cuda")
    with pytest.raises(ValueError):
        networks.ScoreNetMultiPair().set_heads("auto")
    state = networks.ScoreNetMultiPair().state_dict()
    with pytest.raises(ValueError):
        networks.load_scorer(state, None, device="cpu", heads="fused")
    assert networks.load_scorer(state, None, device="cpu", heads="hip").heads == "hip"
    assert networks.load_refiner(networks.RefineNet().state_dict(), None, device="cpu").heads == "torch"
