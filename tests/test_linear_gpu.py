"""pedp_linear_f16 and pedp_token_pool_f16 on the GPU against the float64 references and bounds of tests/_linear_ref.py
(DESIGN.md s4.14): every epilogue over tails in M, both K tile counts, one and several column tiles, dense and row-strided
operands, the position table, loud and flat rows, guard rows beyond M in every output, and equal bits twice."""
import numpy as np
import pytest

import _linear_ref as lr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = {lr.PLAIN: "PLAIN", lr.RELU: "RELU", lr.ADD_LN: "ADD_LN"}
GUARD = -7.0
PAD = 8          # extra columns of a row-strided operand


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Norm:
    """What linear_add_norm reads of an nn.LayerNorm."""

    def __init__(self, gamma, beta, eps=lr.EPS):
        self.weight, self.bias, self.eps, self.normalized_shape = _dev(gamma), None if beta is None else _dev(beta), eps, (len(gamma),)


def _call(d, epilogue, S=None, pos_a=True, view=False, in_place=False):
    """One call on the GPU -> (result M x N float16 numpy, second call's result).  Every output has one guard row beyond M,
    and with `view` x and the output are [..., :K] / [..., :N] views of arrays PAD columns wider; guards and pads are checked."""
    from pedp_hip import linear as L

    M, K = d["x"].shape
    N = len(d["w"])
    packed = L.PackedLinear(_dev(d["w"]), _dev(d["bias"]))
    if view:
        wide = torch.full((M, K + PAD), 3.0, dtype=torch.float16, device="cuda")
        wide[:, :K] = _dev(d["x"])
        x = wide[:, :K]
    else:
        x = _dev(d["x"])
    outs = []
    for _ in range(2):
        full = torch.full((M + 1, N + (PAD if view else 0)), GUARD, dtype=torch.float16, device="cuda")
        out = full[:M, :N]
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
        assert (host[:, N:] == GUARD).all(), "columns beyond N were written"
        outs.append(host[:M, :N])
    if view:
        assert bool((wide[:, K:] == 3.0).all())
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


@pytest.mark.parametrize("B,S", [(1, 1), (3, 16), (2, 400), (252, 1)])
def test_token_pool(B, S):
    from pedp_hip import linear as L

    worst = 0.0
    for n_out in (None, 1, 3, 6):
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
    print(f"token_pool {B} x {S}: largest used share {worst:.3f}")
