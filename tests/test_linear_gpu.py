"""pedp_linear_f16 and pedp_token_pool_f16 on the GPU against the float64 references and bounds of tests/_linear_ref.py
(DESIGN.md s4.14): every epilogue over tails in M, K from 64 to the 8192 the entry point takes, one and several column
tiles with a full or a partial last one, dense and row-strided operands and operands at a column offset of a wider array,
with and without bias and beta, the position table with a period that divides M, does not, is 1 or exceeds M, loud and
flat rows, guard rows beyond M and guard columns around every output, and equal bits twice.  At K = 8192 PLAIN and RELU
are held to the exact integer product."""
import numpy as np
import pytest

import _linear_ref as lr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = {lr.PLAIN: "PLAIN", lr.RELU: "RELU", lr.ADD_LN: "ADD_LN"}
GUARD = -7.0
PAD = 8          # extra columns of a row-strided operand
LEFT = 64        # columns before the output in the `offset` mode


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Norm:
    """What linear_add_norm reads of an nn.LayerNorm."""

    def __init__(self, gamma, beta, eps=lr.EPS):
        self.weight, self.bias, self.eps, self.normalized_shape = _dev(gamma), None if beta is None else _dev(beta), eps, (len(gamma),)


def _call(d, epilogue, S=None, pos_a=True, view=False, in_place=False):
    """One call on the GPU -> (result M x N float16 numpy, second call's result).  Every output has one guard row beyond M,
    and with `view` x and the output are [..., :K] / [..., :N] views of arrays PAD columns wider; with view = "offset" x is
    the middle third [:, K:2K] of an M x 3K array and the output the columns LEFT .. LEFT + N of a wider one.  Guards and
    pads are checked.  d["bias"] and d["beta"] may be None."""
    from pedp_hip import linear as L

    M, K = d["x"].shape
    N = len(d["w"])
    packed = L.PackedLinear(_dev(d["w"]), None if d["bias"] is None else _dev(d["bias"]))
    x0 = {False: 0, True: 0, "offset": K}[view]
    c0 = LEFT if view == "offset" else 0
    if view:
        wide = torch.full((M, 3 * K if view == "offset" else K + PAD), 3.0, dtype=torch.float16, device="cuda")
        wide[:, x0:x0 + K] = _dev(d["x"])
        x = wide[:, x0:x0 + K]
    else:
        x = _dev(d["x"])
    outs = []
    for _ in range(2):
        full = torch.full((M + 1, c0 + N + (PAD if view else 0)), GUARD, dtype=torch.float16, device="cuda")
        out = full[:M, c0:c0 + N]
        if epilogue == lr.ADD_LN:
            pos = None if S is None else _dev(d["pos"][:, :N])
            if in_place:
                out.copy_(_dev(d["res"]))
                res = out
            else:
                res = _dev(d["res"])
            y = L.linear_add_norm(x, packed, res, _Norm(d["gamma"], d["beta"]), pos=pos, period=S, out=out, pos_on_x=pos_a)
        else:
            pos = None if S is None else _dev(d["pos"][:, :K])
            y = L.linear(x, packed, relu=epilogue == lr.RELU, pos=pos, period=S, out=out)
        assert y.data_ptr() == out.data_ptr()
        host = full.cpu().numpy()
        assert (host[M] == GUARD).all(), "the guard row beyond M was written"
        assert (host[:, c0 + N:] == GUARD).all(), "columns beyond N were written"
        assert (host[:, :c0] == GUARD).all(), "columns before the output were written"
        outs.append(host[:M, c0:c0 + N])
    if view:
        assert bool((wide[:, x0 + K:] == 3.0).all()) and bool((wide[:, :x0] == 3.0).all())
    return outs


def _check(d, epilogue, S=None, pos_a=True, views=(False, True), what=""):
    a = dict(x=d["x"], w=d["w"], bias=d["bias"], epilogue=epilogue, pos_a=pos_a)
    if S is not None:
        a.update(pos=d["pos"], S=S)
    if epilogue == lr.ADD_LN:
        a.update(res=d["res"], gamma=d["gamma"], beta=d["beta"])
    y_ref, bound = lr.reference(**a)
    worst = 0.0
    first = None
    for view in views:
        y, again = _call(d, epilogue, S, pos_a, view)
        assert np.array_equal(y.view(np.uint16), again.view(np.uint16)), f"{what}: two calls differ"
        if first is None:
            first = y
        assert np.array_equal(y.view(np.uint16), first.view(np.uint16)), f"{what}: a row-strided operand changes the bits"
        share = lr.used_share(y, y_ref, bound)
        assert share < 1, f"{what} view={view}: {share:.3f} of the bound"
        worst = max(worst, share)
    return worst


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU, lr.ADD_LN])
def test_linear_against_the_bound_over_tails_and_tiles(epilogue):
    worst = {}
    for M in (1, 17, 65, 130, 257):
        for K in (64, 512):
            for N in ((512,) if epilogue == lr.ADD_LN else (64, 512, 1536)):
                d = lr.inputs(M, K, N, seed=M + K + N)
                share = _check(d, epilogue, what=f"{NAMES[epilogue]} {M} x {K} -> {N}")
                worst[K] = max(worst.get(K, 0.0), share)
    print(f"{NAMES[epilogue]}: largest used share of the bound " + ", ".join(f"K = {k}: {v:.3f}" for k, v in sorted(worst.items())))


NEW_SHAPES = [(130, 64, 192), (130, 192, 320), (17, 128, 192), (5, 64, 2112), (128, 128, 128), (256, 64, 64), (127, 64, 64),
              (129, 64, 64)]


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU])
@pytest.mark.parametrize("M,K,N", NEW_SHAPES, ids=lambda v: str(v))
def test_partial_column_tile_behind_full_ones_and_two_or_three_k_tiles(M, K, N, epilogue):
    """N = 192, 320 and 2112 end in a tile of 64 columns behind one, two and sixteen full ones: with a.N / 16 in place of
    (a.N - n0) / 16 the last workgroup writes 64 columns past the row (the guard columns of the row-strided call) and
    reads W rows past N.  K = 128 and 192 are two and three K tiles; M = 127 .. 129 and 256 end at, before and behind a
    row tile's edge."""
    d = lr.inputs(M, K, N, seed=M + K + N)
    share = _check(d, epilogue, what=f"{NAMES[epilogue]} {M} x {K} -> {N}")
    print(f"{NAMES[epilogue]} {M} x {K} -> {N}: largest used share of the bound {share:.3f}")


@pytest.mark.parametrize("K", [128, 192, 1024])
def test_add_norm_over_four_six_and_thirty_two_k_tiles(K):
    worst = 0.0
    for M in (63, 64, 128):
        d = lr.inputs(M, K, 512, seed=M + K)
        worst = max(worst, _check(d, lr.ADD_LN, what=f"ADD_LN {M} x {K}"))
    print(f"ADD_LN, K = {K}: largest used share of the bound {worst:.3f}")


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU])
@pytest.mark.parametrize("N", [192, 64])
def test_the_longest_product_is_the_integer_product_bit_for_bit(N, epilogue):
    """K = 8192, the most the entry point takes: 128 K tiles.  The bound is loose there (the emulation uses 0.04 of it), so
    the operands are small integers instead: every partial sum is an integer below 2^24, which float32 holds in any order
    of the sums, and |y| <= 2048, which float16 holds.  A dropped, doubled or misplaced K tile changes the integers."""
    M, K = 33, 8192
    d = lr.integer_inputs(M, K, N, seed=0)
    y = d["x"].astype(np.float64) @ d["w"].astype(np.float64).T
    assert np.abs(y).max() <= 2048 and (y != 0).mean() > 0.9
    want = (np.maximum(y, 0) if epilogue == lr.RELU else y).astype(np.float16)
    assert np.array_equal(lr.emulate(d["x"], d["w"], None, epilogue).view(np.uint16), want.view(np.uint16))
    for view in (False, True):
        got, again = _call(d, epilogue, view=view)
        assert np.array_equal(got.view(np.uint16), again.view(np.uint16)), "two calls differ"
        wrong = int((got.view(np.uint16) != want.view(np.uint16)).sum())
        assert wrong == 0, f"{NAMES[epilogue]} {M} x {K} -> {N}, view={view}: {wrong} of {want.size} are not the integer product"


def test_add_norm_on_the_longest_product():
    """ADD_LN at K = 8192 (256 K tiles) on sparse_inputs, for which tests/test_linear_cpu.py shows every designed fault more
    than 10 times outside the bound; with and without the table on the residual."""
    M, K, S = 33, 8192, 24
    d = lr.sparse_inputs(M, K, 512, seed=3, S=S)
    plain = _check(d, lr.ADD_LN, what=f"ADD_LN {M} x {K}")
    table = _check(d, lr.ADD_LN, S, pos_a=False, what=f"ADD_LN {M} x {K} with a table")
    print(f"ADD_LN, K = {K}, sparse x: used share {plain:.3f}, with a table of period {S} {table:.3f}")


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU, lr.ADD_LN])
def test_without_bias_and_without_beta(epilogue):
    """A null bias and a null beta are accepted: the kernel must add neither (inputs() draws both, so one added anyway is
    thousands of times outside the bound: tests/test_linear_cpu.py)."""
    d = dict(lr.inputs(65, 128, 512, seed=21), bias=None)
    cases = [("no bias", d)]
    if epilogue == lr.ADD_LN:
        cases += [("no beta", dict(lr.inputs(65, 128, 512, seed=21), beta=None)), ("neither", dict(d, beta=None))]
    else:
        cases.append(("no bias, N = 192", dict(lr.inputs(130, 64, 192, seed=22), bias=None)))
    for name, dd in cases:
        share = _check(dd, epilogue, what=f"{NAMES[epilogue]} {name}")
        print(f"{NAMES[epilogue]}, {name}: used share {share:.3f}")


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU, lr.ADD_LN])
@pytest.mark.parametrize("M,S", [(130, 1), (130, 48), (40, 64)])
def test_position_table_whose_period_is_one_does_not_divide_the_rows_or_exceeds_them(M, S, epilogue):
    """Period 48 on 130 rows ends inside a period and wraps inside both row tiles; period 1 takes row 0 for every row.
    Period 64 on 40 rows never wraps: it runs the path of a table longer than the rows and cannot tell pos[r] from
    pos[r % S]."""
    K, N = (128, 512) if epilogue == lr.ADD_LN else (128, 192)
    d = lr.inputs(M, K, N, seed=M + S, S=S)
    share = _check(d, epilogue, S, pos_a=epilogue != lr.ADD_LN, what=f"{NAMES[epilogue]} {M} rows, period {S}")
    print(f"{NAMES[epilogue]} {M} rows with a table of period {S}: used share {share:.3f}")


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU, lr.ADD_LN])
def test_operands_at_a_column_offset_of_a_wider_array(epilogue):
    """x = wide[:, 512:1024] of an M x 1536 array, out = wide_out[:, 64:64 + N]: both base pointers lie inside a row; the
    columns on both sides of the output are guarded (_call), and the bits equal the dense call's."""
    M, K, N = (65, 512, 512) if epilogue == lr.ADD_LN else (130, 512, 192)
    d = lr.inputs(M, K, N, seed=31, S=24)
    for S in (None, 24):
        share = _check(d, epilogue, S, pos_a=epilogue != lr.ADD_LN, views=(False, "offset"),
                       what=f"{NAMES[epilogue]} at an offset, S = {S}")
        print(f"{NAMES[epilogue]} {M} x {K} -> {N} at a column offset, period {S}: used share {share:.3f}")


@pytest.mark.parametrize("epilogue", [lr.PLAIN, lr.RELU, lr.ADD_LN])
@pytest.mark.parametrize("B,S", [(3, 16), (2, 24), (1, 252)])
def test_position_table_is_added_by_period(B, S, epilogue):
    worst = 0.0
    for K in (64, 512):
        for N in ((512,) if epilogue == lr.ADD_LN else (64, 512, 1536)):
            d = lr.inputs(B * S, K, N, seed=B + S + K + N, S=S)
            modes = (True, False) if epilogue == lr.ADD_LN and K == N else ((False,) if epilogue == lr.ADD_LN else (True,))
            for pos_a in modes:                       # ADD_LN: the table on x and the residual, or on the residual alone
                worst = max(worst, _check(d, epilogue, S, pos_a, views=(False,), what=f"{NAMES[epilogue]} pos {B} x {S}, K {K}, N {N}"))
    print(f"{NAMES[epilogue]} with a table of period {S}: largest used share {worst:.3f}")


def test_add_norm_on_loud_and_flat_rows_and_in_place():
    d = lr.inputs(65, 512, 512, seed=11)
    for name, dd in (("loud", lr.loud_row(d, 3)), ("flat", lr.flat_row(d, 5)), ("loud last", lr.loud_row(d, 64))):
        share = _check(dd, lr.ADD_LN, what=f"ADD_LN with a {name} row")
        print(f"ADD_LN with a {name} row: used share {share:.3f}")
    for dd, S in ((d, None), (lr.inputs(48, 512, 512, seed=12, S=16), 16)):
        apart = _call(dd, lr.ADD_LN, S, pos_a=False)[0]
        same = _call(dd, lr.ADD_LN, S, pos_a=False, in_place=True)[0]
        assert np.array_equal(apart.view(np.uint16), same.view(np.uint16)), "out = residual changes the result"


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from pedp_hip import PedpError
    from pedp_hip import linear as L

    d = lr.inputs(8, 64, 64, seed=1, S=4)
    packed = L.PackedLinear(_dev(d["w"]), _dev(d["bias"]))
    x = _dev(d["x"])
    with pytest.raises(PedpError):
        L.linear(x.float(), packed)
    with pytest.raises(PedpError):
        L.linear(x, packed, pos=_dev(d["pos"][:, :64]))                       # a table without its period
    with pytest.raises(PedpError):
        L.linear(x, packed, out=x)                                            # overlap: refused by the entry point
    with pytest.raises(PedpError):
        L.linear(x.t().contiguous().t(), packed)                              # channels not contiguous
    with pytest.raises(PedpError):
        L.linear_add_norm(x, packed, x, _Norm(d["gamma"][:64], d["beta"][:64]))   # N = 64


def _pool(B, S, n_out):
    """token_pool on dense and row-strided x against the bound, a guard row, equal bits twice -> the largest used share."""
    from pedp_hip import linear as L

    worst = 0.0
    d = lr.pool_inputs(B, S, n_out, seed=B + S, loud_next=True)
    ref, bound = lr.pool_reference(d["x"], B, S, d["w"], d["bias"])
    packed = None if n_out is None else L.PackedLinear(_dev(d["w"]), _dev(d["bias"]))
    for view in (False, True):
        x = _dev(d["x"])
        if view:
            wide = torch.zeros((len(d["x"]), 512 + PAD), dtype=torch.float16, device="cuda")
            wide[:, :512] = x
            x = wide[:, :512]
        outs = []
        for _ in range(2):
            full = torch.full((B + 1, n_out or 512), GUARD, dtype=torch.float16, device="cuda")
            L.token_pool(x[:B * S], B, packed, out=full[:B])
            host = full.cpu().numpy()
            assert (host[B] == GUARD).all(), "the guard row beyond B was written"
            outs.append(host[:B])
        assert np.array_equal(outs[0].view(np.uint16), outs[1].view(np.uint16)), "two calls differ"
        share = lr.used_share(outs[0], ref, bound)
        assert share < 1, f"pool {B} x {S}, n_out {n_out}, view {view}: {share:.3f} of the bound"
        worst = max(worst, share)
    assert tuple(L.token_pool(_dev(d["x"])[:B * S].reshape(B, S, 512), B, packed).shape) == (B, n_out or 512)
    return worst


@pytest.mark.parametrize("B,S", [(1, 1), (3, 16), (2, 400), (252, 1)])
def test_token_pool(B, S):
    worst = max(_pool(B, S, n_out) for n_out in (None, 1, 3, 6))
    print(f"token_pool {B} x {S}: largest used share {worst:.3f}")


@pytest.mark.parametrize("B,S,n_out", [(3, 5, 8), (2, 7, None), (2, 401, 8), (4, 2, 3)])
def test_token_pool_with_unequal_row_phases_and_eight_outputs(B, S, n_out):
    """S = 5, 7, 401 and 2 give the four row phases 2 1 1 1, 2 2 2 1, 101 100 100 100 and 1 1 0 0 rows; n_out = 8 is the
    most the kernel takes."""
    print(f"token_pool {B} x {S}, n_out {n_out}: largest used share {_pool(B, S, n_out):.3f}")
