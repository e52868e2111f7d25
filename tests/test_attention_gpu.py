"""attention.mha_core / attention / self_attention on the GPU (csrc/pedp_attn.hip).

Every comparison is of the full tensor against the float64 attention of the float16-rounded inputs, within
|o - o_ref| <= (2^-11 + 4 E_i + (S + 4) 2^-24) A + S 2^-25 max_j |v_jd| + 2^-11 |o_ref| + 2^-24 (tests/_attn_ref.py: reference).
The shapes cover one row, fewer rows than a 16-row block, the 64-key tile and the 128-row workgroup with and without a
tail, the networks' 252 and 400 tokens, a second query tile with one live row (129), whole numbers of key tiles (128, 192),
17 and 64 key tiles (1025 and 4096, the most the entry point takes), and a head count that is no power of two (5)."""
import copy

import numpy as np
import pytest

import _attn_ref as ar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(1, 1, 1), (2, 3, 4), (3, 16, 4), (2, 17, 4), (2, 63, 2), (1, 64, 4), (2, 65, 4), (2, 252, 4), (2, 400, 4),
          (2, 128, 1), (1, 129, 5), (1, 191, 2), (1, 192, 1), (1, 1025, 2), (1, 4096, 1)]
_CACHE = {}


def _batch_and_heads(S):
    """B, H of the tests that take S alone: 2 x 4 up to the networks' sizes, fewer beyond to keep the float64 reference quick."""
    return (2, 4) if S <= 400 else (1, 2) if S <= 1025 else (1, 1)


def _case(B, S, H):
    """(q, k, v, o_ref, bound) of a shape, computed once."""
    key = (B, S, H)
    if key not in _CACHE:
        q, k, v = ar.gaussian_qkv(B, S, H, seed=S + 7 * B + H)
        _CACHE[key] = (q, k, v) + ar.reference(q, k, v, H)
    return _CACHE[key]


def _packed(q, k, v):
    return torch.from_numpy(np.concatenate([q, k, v], axis=2)).cuda()


def _run_packed(q, k, v, H):
    from pedp_hip.attention import mha_core

    return mha_core(_packed(q, k, v), H).cpu().numpy()


def _check(o, o_ref, bound, what):
    share = ar.used_share(o, o_ref, bound)
    print(f"{what}: max |o - o_ref| {np.abs(o.astype(np.float64) - o_ref).max():.3e}, share of the bound {share:.3f}")
    assert np.isfinite(o).all() and share <= 1.0


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_packed_operands_within_the_bound_and_the_same_bits_twice(B, S, H):
    from pedp_hip.attention import mha_core

    q, k, v, o_ref, bound = _case(B, S, H)
    qkv = _packed(q, k, v)
    o = mha_core(qkv, H)
    assert o.shape == (B, S, H * ar.D) and o.dtype == torch.float16 and o.is_contiguous()
    _check(o.cpu().numpy(), o_ref, bound, f"packed {B} x {S} x {H}")
    assert torch.equal(mha_core(qkv, H), o), "two calls differ"


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_separate_operands_with_a_larger_row_stride(B, S, H):
    from pedp_hip.attention import attention

    q, k, v, o_ref, bound = _case(B, S, H)
    E = H * ar.D
    views = []
    for i, x in enumerate((q, k, v)):
        wide = torch.full((B, S, E + 8 * (i + 1)), 9.0, dtype=torch.float16, device="cuda")
        wide[..., :E] = torch.from_numpy(x).cuda()
        views.append(wide[..., :E])
    _check(attention(*views, H).cpu().numpy(), o_ref, bound, f"strided {B} x {S} x {H}")


def test_scale_argument():
    B, S, H = 2, 17, 4
    q, k, v = ar.gaussian_qkv(B, S, H, seed=3)
    from pedp_hip.attention import mha_core

    o_ref, bound = ar.reference(q, k, v, H, scale=0.05)
    _check(mha_core(_packed(q, k, v), H, scale=0.05).cpu().numpy(), o_ref, bound, "scale 0.05")


@pytest.mark.parametrize("scale", [0.0, -1.0 / np.sqrt(128), 1.0], ids=["zero", "negative", "one"])
def test_scale_zero_negative_and_one(scale):
    """Scale 0 makes every row the mean of the values over exactly S keys (a tail key let in, or a live one masked, moves it),
    a negative scale turns the order of the scores round, and scale 1 gives scores of some hundreds in float32."""
    from pedp_hip.attention import mha_core

    B, S, H = 2, 129, 2
    q, k, v = ar.gaussian_qkv(B, S, H, seed=3)
    o_ref, bound = ar.reference(q, k, v, H, scale=scale)
    _check(mha_core(_packed(q, k, v), H, scale=scale).cpu().numpy(), o_ref, bound, f"scale {scale:.4f} at {B} x {S} x {H}")


@pytest.mark.parametrize("S", [17, 65, 252, 400, 1025, 4096])
def test_dominant_last_key(S):
    B, H = _batch_and_heads(S)
    q, k, v = ar.gaussian_qkv(B, S, H, seed=S)
    q, k = ar.dominate_last_key(q, k, H)
    o_ref, bound = ar.reference(q, k, v, H)
    assert ar.used_share(ar.emulate(q, k, v, H, drop_last_key=True), o_ref, bound) > 10, "dropping the key stays inside the bound"
    o = _run_packed(q, k, v, H)
    _check(o, o_ref, bound, f"dominant last key, S = {S}")
    assert np.abs(o.astype(np.float64) - v[:, -1:, :].astype(np.float64)).max() < 1e-2  # every row is the last key's value


@pytest.mark.parametrize("S", [17, 65, 252, 129])
def test_neighbouring_batch_and_head_do_not_leak(S):
    B, H = 3, 4
    q, k, v = ar.gaussian_qkv(B, S, H, seed=100 + S)
    mine = np.zeros((B, 1, H, 1), bool)
    mine[0::2, :, 0::2] = True                                  # even batches' even heads are watched; every other one is loud
    mine = np.broadcast_to(mine, (B, S, H, ar.D)).reshape(B, S, H * ar.D)
    loud_k = np.where(mine, k, (k.astype(np.float32) * 8).astype(np.float16))
    loud_v = np.where(mine, v, np.float16(300.0))
    quiet_k, quiet_v = np.where(mine, k, np.float16(0)), np.where(mine, v, np.float16(0))
    o_ref, bound = ar.reference(q, loud_k, loud_v, H)
    loud, quiet = _run_packed(q, loud_k, loud_v, H), _run_packed(q, quiet_k, quiet_v, H)
    _check(loud, o_ref, bound, f"loud neighbours, S = {S}")
    moved = np.abs(loud.astype(np.float64) - quiet.astype(np.float64))[mine]
    print(f"S = {S}: the watched outputs moved by at most {moved.max():.3e}")
    assert (moved <= bound[mine]).all()
    # the emulation with a tile that runs into the next batch's keys is outside the bound
    assert ar.used_share(ar.emulate(q, loud_k, loud_v, H, leak_keys=1)[:1], o_ref[:1], bound[:1]) > 10


@pytest.mark.parametrize("S,key", [(400, 5), (400, 200), (400, 399), (252, 130), (65, 64), (1025, 1024), (4096, 4095)])
def test_running_maximum_jumps_at_a_chosen_tile(S, key):
    """With the spike at the last key of S = 1025 and 4096 the maximum has been rescaled over 16 and 63 tiles before it
    jumps in the last one: a tail tile of one key, and a full tile."""
    (B, H), row = _batch_and_heads(S), S // 3
    q, k, v = ar.gaussian_qkv(B, S, H, seed=200 + key)
    for name, kk in (("spike", ar.spike(q, k, H, row, key)), ("no spike", k)):
        o_ref, bound = ar.reference(q, kk, v, H)
        if name == "spike":
            x = ar.SCALE * q[:, row].astype(np.float64).reshape(B, H, 1, ar.D) @ \
                kk.astype(np.float64).reshape(B, S, H, ar.D).transpose(0, 2, 3, 1)
            others = np.delete(x, key, axis=3)
            assert (x[..., key] - others.max(-1) > 20).all(), "the spike does not lift the maximum by 20"
            if key >= ar.BK:
                broken = ar.emulate(q, kk, v, H, skip_rescale_at=key // ar.BK)
                assert ar.used_share(broken, o_ref, bound) > 10, "a skipped rescale stays inside the bound"
        _check(_run_packed(q, kk, v, H), o_ref, bound, f"{name} at key {key} of {S}")


@pytest.mark.parametrize("B,S,H", [(2, 3, 4), (2, 65, 4), (1, 252, 4)])
def test_nothing_is_written_outside_the_destination(B, S, H):
    from pedp_hip.attention import mha_core

    q, k, v, o_ref, bound = _case(B, S, H)
    E, ld, guard = H * ar.D, H * ar.D + 24, 3
    buf = torch.full((B * S + 2 * guard, ld), 777.0, dtype=torch.float16, device="cuda")
    out = buf[guard:guard + B * S].view(B, S, ld)[..., :E]
    res = mha_core(_packed(q, k, v), H, out=out)
    assert res.data_ptr() == out.data_ptr()
    _check(out.cpu().numpy(), o_ref, bound, f"out view {B} x {S} x {H}")
    buf = buf.cpu().numpy()
    assert (buf[:guard] == 777).all() and (buf[guard + B * S:] == 777).all() and (buf[:, E:] == 777).all()


def test_rejected_arguments():
    from pedp_hip import PedpError
    from pedp_hip.attention import attention, mha_core

    qkv = torch.zeros((2, 8, 3 * 512), dtype=torch.float16, device="cuda")
    with pytest.raises(PedpError):
        mha_core(qkv, 8)                                       # D = 64
    with pytest.raises(PedpError):
        mha_core(torch.zeros((2, 8, 3 * 64), dtype=torch.float16, device="cuda"), 1)
    wide = torch.zeros((2, 8, 512 + 4), dtype=torch.float16, device="cuda")
    ok = torch.zeros((2, 8, 512), dtype=torch.float16, device="cuda")
    with pytest.raises(PedpError):
        attention(wide[..., :512], ok, ok, 4)                  # a row stride that is no multiple of 8
    shifted = torch.zeros(2 * 8 * 512 + 4, dtype=torch.float16, device="cuda")[4:].view(2, 8, 512)
    with pytest.raises(PedpError):
        attention(ok, ok, shifted, 4)                          # 8-byte aligned only
    with pytest.raises(PedpError):
        mha_core(qkv.float(), 4)
    with pytest.raises(PedpError):
        mha_core(qkv.cpu(), 4)
    with pytest.raises(PedpError):
        mha_core(qkv, 4, out=qkv[..., :512])                   # out aliases q
    with pytest.raises(PedpError):
        mha_core(qkv, 4, out=qkv[..., 1024:])                  # ... and v
    with pytest.raises(PedpError):
        mha_core(torch.zeros((1, 4097, 3 * 128), dtype=torch.float16, device="cuda"), 1)
    assert mha_core(qkv, 4).shape == (2, 8, 512)


# ---------------------------------------------------------------- self_attention on modules

def _filled(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / np.sqrt(p.shape[1])))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if "norm" in name and name.endswith("weight") else 0.0))
    return module.cuda().eval()


def _three_errors(run_hip, run_stock, module, x):
    """(e_hip, e_torch, eps): the errors against the module in float64 of the kernel path and of the stock module, both
    under float16 autocast, and of the stock module in float32."""
    with torch.inference_mode():
        want = run_stock(copy.deepcopy(module).double(), x.double())
        eps = float((run_stock(module, x).double() - want).abs().max())
        with torch.autocast("cuda", dtype=torch.float16):
            e_torch = float((run_stock(module, x).double() - want).abs().max())
            e_hip = float((run_hip(module, x).double() - want).abs().max())
    return e_hip, e_torch, eps


@pytest.mark.parametrize("B,S", [(3, 24), (2, 400)])
def test_self_attention_on_a_multihead_attention_module(B, S):
    from pedp_hip.attention import self_attention

    mha = _filled(torch.nn.MultiheadAttention(512, 4, bias=True, batch_first=True), 1)
    x = torch.randn((B, S, 512), generator=torch.Generator().manual_seed(2)).cuda()
    e_hip, e_torch, eps = _three_errors(self_attention, lambda m, t: m(t, t, t)[0], mha, x)
    print(f"MultiheadAttention {B} x {S}: e_hip {e_hip:.3e}, e_torch {e_torch:.3e}, float32 {eps:.3e}")
    assert e_torch > 0 and e_hip <= 2 * e_torch + eps


@pytest.mark.parametrize("B,S", [(3, 16), (2, 400)])
def test_encoder_layer_with_the_kernel(B, S):
    from pedp_hip.attention import encoder_layer

    layer = _filled(torch.nn.TransformerEncoderLayer(d_model=512, nhead=4, dim_feedforward=512, batch_first=True), 3)
    x = torch.randn((B, S, 512), generator=torch.Generator().manual_seed(4)).cuda()
    e_hip, e_torch, eps = _three_errors(encoder_layer, lambda m, t: m(t), layer, x)
    print(f"TransformerEncoderLayer {B} x {S}: e_hip {e_hip:.3e}, e_torch {e_torch:.3e}, float32 {eps:.3e}")
    assert e_torch > 0 and e_hip <= 2 * e_torch + eps
