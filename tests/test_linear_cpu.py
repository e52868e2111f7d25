"""The heads' linear layers without a GPU: the error bounds' two facts on the numpy emulation of the kernels
(tests/_linear_ref.py), the entry points' argument checks on host addresses, the decomposed chain against
torch's modules in float64, and the networks' `linears` switch on the CPU, where it must not change a bit."""
import numpy as np
import pytest

import _linear_ref as lr
import _net_fill

torch = pytest.importorskip("torch")

NAMES = {lr.PLAIN: "PLAIN", lr.RELU: "RELU", lr.ADD_LN: "ADD_LN"}


def _args(d, epilogue, S=None, **kw):
    a = dict(x=d["x"], w=d["w"], bias=d["bias"], epilogue=epilogue, **kw)
    if S is not None:
        a.update(pos=d["pos"], S=S)
    if epilogue == lr.ADD_LN:
        a.update(res=d["res"], gamma=d["gamma"], beta=d["beta"])
    return a


# ---------------------------------------------------------------- the bounds' two facts

@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU, lr.ADD_LN])
@pytest.mark.parametrize("M,K,S", [(17, 64, None), (65, 512, None), (48, 512, 16), (130, 512, 24)])
def test_emulated_kernel_arithmetic_uses_a_part_of_the_bound(M, K, S, epilogue):
    d = lr.inputs(M, K, 512, seed=M + K, S=S)
    a = _args(d, epilogue, S)
    y_ref, bound = lr.reference(**a)
    share = lr.used_share(lr.emulate(**a), y_ref, bound)
    print(f"{NAMES[epilogue]} {M} x {K}, S = {S}: the emulation uses {share:.3f} of the bound")
    assert 0.05 < share < 1


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU, lr.ADD_LN])
def test_each_designed_fault_of_the_product_exceeds_the_bound(epilogue):
    M, K, S = 65, 512, 24
    d = lr.inputs(M, K, 512, seed=7, S=S)
    a = _args(d, epilogue, S)
    y_ref, bound = lr.reference(**a)
    assert lr.used_share(lr.emulate(**a), y_ref, bound) < 1
    faults = ["drop_last_k_block", "no_bias", "pos_no_wrap"] + (["res_shift"] if epilogue == lr.ADD_LN else [])
    for fault in faults:
        share = lr.used_share(lr.emulate(**a, **{fault: True}), y_ref, bound)
        print(f"{NAMES[epilogue]}: {fault} is {share:.1f} times the bound")
        assert share > 10, fault
    if epilogue == lr.ADD_LN:
        share = lr.used_share(lr.emulate(**a, stat_cols=448), y_ref, bound)
        print(f"ADD_LN: statistics over 448 of 512 columns are {share:.1f} times the bound")
        assert share > 10
        a = _args(d, epilogue, S, pos_a=False)                        # the table on the residual alone
        y_ref, bound = lr.reference(**a)
        assert 0.05 < lr.used_share(lr.emulate(**a), y_ref, bound) < 1
        assert lr.used_share(lr.emulate(**a, pos_no_wrap=True), y_ref, bound) > 10


# the shapes tests/test_linear_gpu.py adds: (M, K, N), the faults that shape is there for
_TILE, _K, _BIAS = "last_tile_first_weights", "drop_last_k_block", "no_bias"
NEW_PRODUCTS = {(130, 64, 192): (_TILE, _BIAS), (130, 192, 320): (_TILE, _K), (17, 128, 192): (_TILE, _K), (5, 64, 2112): (_TILE, _BIAS),
                (128, 128, 128): (_K, _BIAS), (256, 64, 64): (_BIAS,), (127, 64, 64): (_BIAS,), (129, 64, 64): (_BIAS,)}


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU])
@pytest.mark.parametrize("shape", list(NEW_PRODUCTS), ids=lambda v: "x".join(map(str, v)))
def test_new_product_shapes_tell_their_faults_from_the_bound(shape, epilogue):
    M, K, N = shape
    faults = NEW_PRODUCTS[shape]
    d = lr.inputs(M, K, N, seed=M + K + N)
    a = _args(d, epilogue)
    y_ref, bound = lr.reference(**a)
    share = lr.used_share(lr.emulate(**a), y_ref, bound)
    print(f"{NAMES[epilogue]} {M} x {K} -> {N}: the emulation uses {share:.3f} of the bound")
    assert share < 1
    for fault in faults:
        share = lr.used_share(lr.emulate(**a, **{fault: True}), y_ref, bound)
        print(f"{NAMES[epilogue]} {M} x {K} -> {N}: {fault} is {share:.0f} times the bound")
        assert share > 10, fault


@pytest.mark.parametrize("K", [128, 192, 1024])
@pytest.mark.parametrize("M", [63, 64, 128])
def test_new_add_norm_shapes_tell_their_faults_from_the_bound(M, K):
    d = lr.inputs(M, K, 512, seed=M + K)
    a = _args(d, lr.ADD_LN)
    y_ref, bound = lr.reference(**a)
    share = lr.used_share(lr.emulate(**a), y_ref, bound)
    print(f"ADD_LN {M} x {K}: the emulation uses {share:.3f} of the bound")
    assert share < 1
    for fault in ("drop_last_k_block", "no_bias", "res_shift"):
        share = lr.used_share(lr.emulate(**a, **{fault: True}), y_ref, bound)
        print(f"ADD_LN {M} x {K}: {fault} is {share:.0f} times the bound")
        assert share > 10, fault


def test_integer_operands_make_the_longest_product_exact():
    """K = 8192 for PLAIN and RELU: on gaussian operands the emulation uses a few hundredths of the bound, which tells
    little; on integer_inputs the result is the integer product bit for bit and a dropped K block changes most of it."""
    d = lr.inputs(33, 8192, 192, seed=0)
    y_ref, bound = lr.reference(**_args(d, lr.PLAIN))
    loose = lr.used_share(lr.emulate(**_args(d, lr.PLAIN)), y_ref, bound)
    print(f"PLAIN 33 x 8192 -> 192 on gaussian operands: the emulation uses {loose:.3f} of the bound")
    assert loose < 0.1
    for N in (192, 64):
        d = lr.integer_inputs(33, 8192, N, seed=0)
        y = d["x"].astype(np.float64) @ d["w"].astype(np.float64).T
        assert np.abs(y).max() <= 2048                                    # float16 holds every integer up to 2048
        for epilogue in (lr.PLAIN, lr.RELU):
            want = np.maximum(y, 0) if epilogue == lr.RELU else y
            assert np.array_equal(lr.emulate(d["x"], d["w"], None, epilogue).astype(np.float64), want)
        changed = float((lr.emulate(d["x"], d["w"], None, lr.PLAIN, drop_last_k_block=True).astype(np.float64) != y).mean())
        print(f"33 x 8192 -> {N}: max |y| {np.abs(y).max():.0f}, a dropped K block changes {changed:.2f} of the elements")
        assert changed > 0.9


@pytest.mark.parametrize("S", [None, 24])
def test_sparse_operands_keep_every_fault_of_the_longest_add_norm_outside_the_bound(S):
    """ADD_LN at K = 8192: on gaussian operands drop_last_k_block is only 4.8 times the bound; on sparse_inputs every fault
    is more than 10 times outside."""
    d = lr.sparse_inputs(33, 8192, 512, seed=3, S=S)
    assert all((row.reshape(-1, 32) != 0).sum(1).max() <= 1 for row in d["x"]) and (d["x"] != 0).sum() > 33 * 250
    a = _args(d, lr.ADD_LN, S, pos_a=False)
    y_ref, bound = lr.reference(**a)
    share = lr.used_share(lr.emulate(**a), y_ref, bound)
    print(f"ADD_LN 33 x 8192, sparse x, S = {S}: the emulation uses {share:.3f} of the bound")
    assert share < 1
    for kw in [dict(drop_last_k_block=True), dict(no_bias=True), dict(res_shift=True), dict(stat_cols=448)] + \
            ([dict(pos_no_wrap=True)] if S else []):
        share = lr.used_share(lr.emulate(**a, **kw), y_ref, bound)
        print(f"ADD_LN 33 x 8192, sparse x, S = {S}: {kw} is {share:.1f} times the bound")
        assert share > 10, kw


def test_an_operand_that_is_left_out_must_not_be_added():
    """bias = None and beta = None at (65, 128, 512): a kernel that adds the bias or the beta it was not given."""
    d = lr.inputs(65, 128, 512, seed=21)
    for epilogue in (lr.PLAIN, lr.RELU, lr.ADD_LN):
        without = _args(dict(d, bias=None), epilogue)
        y_ref, bound = lr.reference(**without)
        assert lr.used_share(lr.emulate(**without), y_ref, bound) < 1
        share = lr.used_share(lr.emulate(**_args(d, epilogue)), y_ref, bound)
        print(f"{NAMES[epilogue]}: a bias added anyway is {share:.0f} times the bound")
        assert share > 10
    without = _args(dict(d, beta=None), lr.ADD_LN)
    y_ref, bound = lr.reference(**without)
    assert lr.used_share(lr.emulate(**without), y_ref, bound) < 1
    share = lr.used_share(lr.emulate(**_args(d, lr.ADD_LN)), y_ref, bound)
    print(f"ADD_LN: a beta added anyway is {share:.0f} times the bound")
    assert share > 10


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU, lr.ADD_LN])
@pytest.mark.parametrize("M,S", [(130, 1), (130, 48), (40, 64)])
def test_new_table_periods(M, S, epilogue):
    """Period 1 and a period that does not divide M tell pos[r] from pos[r % S]; a period above M cannot (no row wraps)
    and is there for the entry point's pos_rows >= period path alone."""
    K, N = (128, 512) if epilogue == lr.ADD_LN else (128, 192)
    d = lr.inputs(M, K, N, seed=M + S, S=S)
    a = _args(d, epilogue, S, pos_a=epilogue != lr.ADD_LN)
    y_ref, bound = lr.reference(**a)
    assert lr.used_share(lr.emulate(**a), y_ref, bound) < 1
    share = lr.used_share(lr.emulate(**a, pos_no_wrap=True), y_ref, bound)
    print(f"{NAMES[epilogue]} {M} rows, period {S}: pos_no_wrap is {share:.1f} times the bound")
    assert share > 10 if S < M else share < 1


@pytest.mark.parametrize("B,S,n_out", [(3, 5, 8), (2, 7, None), (2, 401, 8), (4, 2, 3)])
def test_pool_emulation_and_its_fault_on_unequal_row_phases(B, S, n_out):
    d = lr.pool_inputs(B, S, n_out, seed=S + B, loud_next=True)
    ref, bound = lr.pool_reference(d["x"], B, S, d["w"], d["bias"])
    share = lr.used_share(lr.pool_emulate(d["x"], B, S, d["w"], d["bias"]), ref, bound)
    print(f"pool {B} x {S}, n_out {n_out}: {share:.3f} of the bound")
    assert share < 1
    assert lr.used_share(lr.pool_emulate(d["x"], B, S, d["w"], d["bias"], leak=True)[:1], ref[:1], bound[:1]) > 10


def test_bound_holds_on_loud_and_flat_rows():
    d = lr.inputs(65, 512, 512, seed=11)
    for name, dd in (("loud", lr.loud_row(d, 3)), ("flat", lr.flat_row(d, 5))):
        a = _args(dd, lr.ADD_LN)
        y_ref, bound = lr.reference(**a)
        share = lr.used_share(lr.emulate(**a), y_ref, bound)
        print(f"ADD_LN with a {name} row: {share:.3f} of the bound")
        assert share < 1
        assert lr.used_share(lr.emulate(**a, res_shift=True), y_ref, bound) > 10
    v = lr.flat_row(d, 5)
    row = v["res"][5].astype(np.float64) + v["bias"] + v["x"][5].astype(np.float64) @ v["w"].astype(np.float64).T
    assert row.var() < 10 * lr.EPS, "the flat row's variance is not near eps"


@pytest.mark.parametrize("n_out", [None, 1, 3, 6])
@pytest.mark.parametrize("B,S", [(1, 1), (3, 16), (2, 400), (252, 1)])
def test_pool_emulation_and_its_fault(B, S, n_out):
    d = lr.pool_inputs(B, S, n_out, seed=S + B)
    ref, bound = lr.pool_reference(d["x"], B, S, d["w"], d["bias"])
    share = lr.used_share(lr.pool_emulate(d["x"], B, S, d["w"], d["bias"]), ref, bound)
    print(f"pool {B} x {S}, n_out {n_out}: {share:.3f} of the bound")
    assert share < 1                 # (the mean of one row, S = 1 without w, is exact: no lower limit here)
    d = lr.pool_inputs(max(B, 2), S, n_out, seed=S + B, loud_next=True)
    ref, bound = lr.pool_reference(d["x"], max(B, 2), S, d["w"], d["bias"])
    assert lr.used_share(lr.pool_emulate(d["x"], max(B, 2), S, d["w"], d["bias"]), ref, bound) < 1
    assert lr.used_share(lr.pool_emulate(d["x"], max(B, 2), S, d["w"], d["bias"], leak=True)[:1], ref[:1], bound[:1]) > 10


# ---------------------------------------------------------------- argument checks on host addresses

def test_linear_entry_point_checks_its_arguments_before_it_touches_the_device():
    """pedp_linear_f16's checks come before its first use of the context or the GPU, so they run here on host addresses."""
    import ctypes as C

    from pedp_hip import _lib

    lib = _lib.load()
    ctx = C.create_string_buffer(4096)
    buf = C.create_string_buffer(4 << 20)
    base = (C.addressof(buf) + 15) // 16 * 16
    MB = 1 << 20
    at = dict(x=0, w=64 << 10, bias=MB, res=MB + (64 << 10), pos=MB + (128 << 10), gamma=MB + (256 << 10), beta=MB + (320 << 10),
              y=2 * MB)

    def status(M=8, N=512, K=512, x_ld=512, y_ld=512, res_ld=512, epi=_lib.LINEAR_PLAIN, pos_rows=0, period=0, pos_a=0, eps=1e-5,
               use=("x", "w", "bias", "y"), prm=True, context=True, **where):
        p = _lib.LinearParams()
        p.M, p.N, p.K, p.x_ld, p.y_ld, p.res_ld, p.epilogue = M, N, K, x_ld, y_ld, res_ld, epi
        p.pos_rows, p.pos_period, p.pos_a, p.eps = pos_rows, period, pos_a, eps
        ptr = {k: C.c_void_p(base + where.get(k, at[k]) if k in use else None) for k in at}
        return lib.pedp_linear_f16(C.cast(ctx, C.c_void_p) if context else None, C.byref(p) if prm else None, ptr["x"], ptr["w"],
                                   ptr["bias"], ptr["res"], ptr["pos"], ptr["gamma"], ptr["beta"], ptr["y"])

    ln = dict(epi=_lib.LINEAR_ADD_LN, use=("x", "w", "bias", "res", "gamma", "beta", "y"))
    with_pos = dict(use=("x", "w", "bias", "pos", "y"), pos_rows=16)
    bad = [dict(K=96), dict(K=0), dict(K=8256), dict(N=96), dict(N=0), dict(M=0), dict(x_ld=448), dict(x_ld=516), dict(y_ld=516),
           dict(y_ld=448), dict(x=8), dict(y=2 * MB + 8), dict(bias=MB + 4), dict(w=(64 << 10) + 8), dict(epi=3), dict(epi=-1),
           dict(ln, N=1024), dict(ln, N=64), dict(ln, use=("x", "w", "res", "beta", "y")), dict(ln, use=("x", "w", "gamma", "y")),
           dict(ln, res_ld=516), dict(ln, res_ld=256), dict(ln, eps=float("nan")), dict(use=("x", "w", "res", "y")),
           dict(use=("x", "w", "gamma", "y")), dict(with_pos, period=0), dict(with_pos, period=17),
           dict(ln, use=ln["use"] + ("pos",), pos_rows=16, period=16, pos_a=1, K=64),
           dict(y=0), dict(y=4096), dict(y=64 << 10), dict(y=MB), dict(with_pos, period=16, y=MB + (128 << 10)),
           dict(ln, y=MB + (64 << 10) + 16), dict(ln, y=MB + (64 << 10), y_ld=1024), dict(ln, y=MB + (256 << 10)),
           dict(ln, y=MB + (320 << 10)), dict(use=("w", "y")), dict(use=("x", "y")), dict(use=("x", "w")), dict(prm=False),
           dict(context=False)]
    for kw in bad:
        assert status(**kw) == -1, kw                                   # PEDP_ERR_BAD_ARG
        assert b"pedp_linear_f16" in lib.pedp_last_error(), kw


def test_pool_entry_point_checks_its_arguments_before_it_touches_the_device():
    import ctypes as C

    from pedp_hip import _lib

    lib = _lib.load()
    ctx = C.create_string_buffer(4096)
    buf = C.create_string_buffer(1 << 20)
    base = (C.addressof(buf) + 15) // 16 * 16

    def status(B=3, S=16, E=512, x_ld=512, n_out=3, x=0, w=256 << 10, bias=320 << 10, out=512 << 10, use=("x", "w", "bias", "out"),
               prm=True):
        p = _lib.TokenPoolParams()
        p.B, p.S, p.E, p.x_ld, p.n_out = B, S, E, x_ld, n_out
        ptr = {k: C.c_void_p(base + v if k in use else None) for k, v in dict(x=x, w=w, bias=bias, out=out).items()}
        return lib.pedp_token_pool_f16(C.cast(ctx, C.c_void_p), C.byref(p) if prm else None, ptr["x"], ptr["w"], ptr["bias"], ptr["out"])

    bad = [dict(E=256), dict(E=1024), dict(B=0), dict(S=0), dict(x_ld=504), dict(x_ld=516), dict(n_out=0), dict(n_out=9),
           dict(n_out=3, use=("x", "out")), dict(n_out=0, use=("x", "bias", "out")), dict(x=8), dict(w=(256 << 10) + 4), dict(out=(512 << 10) + 1),
           dict(out=0), dict(out=1024), dict(out=256 << 10), dict(out=320 << 10), dict(use=("w", "bias", "out")), dict(use=("x", "w", "bias")),
           dict(prm=False)]
    for kw in bad:
        assert status(**kw) == -1, kw
        assert b"pedp_token_pool_f16" in lib.pedp_last_error(), kw


def test_kernel_entry_points_refuse_what_they_do_not_take():
    from pedp_hip import PedpError
    from pedp_hip import linear as L

    lin = torch.nn.Linear(512, 512)
    packed = L.pack_linear(lin)
    assert packed.weight.dtype == torch.float16 and packed.bias.dtype == torch.float32 and (packed.n, packed.k) == (512, 512)
    assert torch.equal(packed.weight, lin.weight.detach().half())
    x = torch.zeros((2, 4, 512), dtype=torch.float16)
    with pytest.raises(PedpError):
        L.linear(x, packed)                                              # a CPU tensor: no fallback
    with pytest.raises(PedpError):
        L.linear_add_norm(x, packed, x, torch.nn.LayerNorm(512))
    with pytest.raises(PedpError):
        L.token_pool(x, 2)
    with pytest.raises(PedpError):
        L.linear(x, lin)                                                 # not packed


# ---------------------------------------------------------------- the decomposition in float64

def _seeded(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.1 if p.dim() == 1 else 1.5 / np.sqrt(p.shape[-1])))
    return module.eval()


def _by_reference(mha, x):
    import torch.nn.functional as F
    from pedp_hip.attention import mha_reference

    e = mha.embed_dim
    q, k, v = F.linear(x, mha.in_proj_weight, mha.in_proj_bias).split(e, dim=-1)
    o = mha_reference(q, k, v, 1.0 / np.sqrt(e // mha.num_heads), num_heads=mha.num_heads)
    return F.linear(o, mha.out_proj.weight, mha.out_proj.bias)


@pytest.mark.parametrize("B,S", [(2, 16), (1, 5)])
def test_decomposed_chain_is_the_stock_head_in_float64(B, S):
    """encoder_layer_fused's formula with the table folded in, and the mean taken before the final Linear."""
    from pedp_hip.linear import encoder_layer_formula, pooled_linear_formula
    from pedp_hip.networks import _PositionTable

    layer = _seeded(torch.nn.TransformerEncoderLayer(d_model=512, nhead=4, dim_feedforward=512, batch_first=True).double(), 3)
    lin = _seeded(torch.nn.Linear(512, 6).double(), 4)
    table = _PositionTable(512, 400).double()
    x = torch.randn((B, S, 512), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    with torch.no_grad():
        want = lin(layer(table(x))).mean(dim=1)
        got = pooled_linear_formula(lin, encoder_layer_formula(layer, x, table.pe[0, :S], _by_reference))
    assert float((got - want).abs().max()) < 1e-12


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
def test_linears_hip_on_the_cpu_is_the_torch_path(kind, case):
    L = _net_fill.CASES[case][3]
    A, B = _net_fill.inputs(case, torch.float32)
    outs = []
    for kw in (dict(), dict(heads="hip", linears="hip"), dict(linears="hip")):
        net = _net(kind, **kw)
        assert net.linears == kw.get("linears", "torch")
        with torch.no_grad():
            outs.append(net(A, B) if kind == "refiner" else net(A, B, L=L))
        assert not net._packed
    assert all(torch.equal(outs[0][k], o[k]) for o in outs[1:] for k in outs[0])
    net = _net(kind)
    assert net.set_linears("hip") is net and net.linears == "hip" and net.heads == "torch"
    assert list(net.state_dict().keys()) == list(_net(kind, heads="hip", linears="hip").state_dict().keys())


def test_bad_linears_value():
    from pedp_hip import networks

    with pytest.raises(ValueError):
        networks.RefineNet(linears="cuda")
    with pytest.raises(ValueError):
        networks.ScoreNetMultiPair().set_linears("auto")
    state = networks.ScoreNetMultiPair().state_dict()
    with pytest.raises(ValueError):
        networks.load_scorer(state, None, device="cpu", linears="fused")
    assert networks.load_scorer(state, None, device="cpu", heads="hip", linears="hip").linears == "hip"
    assert networks.load_refiner(networks.RefineNet().state_dict(), None, device="cpu").linears == "torch"
