"""The pose-error metrics without a GPU: the numpy restatement of pedp_pose_errors (tests/_metrics_ref.py) against the
fixture that the reference's add_err / adds_err wrote (tests/golden/g11_metrics.npz) and against an 80-bit evaluation,
compute_auc_sklearn against the reference's values, symmetry_tfs_from_info, the exported names, the argument refusals
and the ABI symbol.

The tolerance is derived, not measured: u = 2^-53, S = max_i (|x_i| + |y_i| + |z_i|) max|R| + max|t|;
a transformed coordinate carries at most ~4 u S on either side, a distance at most sqrt(3) 8 u S, so two float64
implementations differ by less than 32 u S, and a mean of N non-negative terms in any order adds (N + 8) u relative on
each side: |got - want| <= 32 u S + 2 (N + 8) u want."""
import ctypes
import os
import re

import numpy as np
import pytest

import _metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g11_metrics.npz"))
CASES = [str(c) for c in GOLD["cases"]]
LD = np.longdouble


def case(name):
    n, scale, _ = name.split("_")
    return (GOLD[f"{name}/pred"].astype(np.float64), GOLD[f"{name}/gt"], GOLD[f"pts/{n}_{scale}"],
            float(GOLD[f"{name}/add"]), float(GOLD[f"{name}/adds"]))


def wide(kind, pred, gt, pts):
    """Either error with every operation in numpy's long double (80-bit here) and numpy's own summation."""
    def tf(M):
        M, p = M.astype(LD), pts.astype(LD)
        return [M[k, 0] * p[:, 0] + M[k, 1] * p[:, 1] + M[k, 2] * p[:, 2] + M[k, 3] for k in range(3)]
    a, b = tf(pred), tf(gt)
    if kind == "add":
        return np.sqrt(sum((a[k] - b[k]) ** 2 for k in range(3))).mean()
    best = np.empty(len(pts), LD)
    for i0 in range(0, len(pts), 256):
        sl = slice(i0, i0 + 256)
        best[sl] = sum((a[k][None, :] - b[k][sl, None]) ** 2 for k in range(3)).min(axis=1)
    return np.sqrt(best).mean()


@pytest.mark.parametrize("name", CASES)
def test_restatement_fixture_and_80_bit_agree_within_the_bound(name):
    assert np.finfo(LD).nmant >= 63, "numpy's long double is not the 80-bit format here"
    pred, gt, pts, w_add, w_adds = case(name)
    for kind, want in (("add", w_add), ("adds", w_adds)):
        got = float(ref.pose_error(kind, pred, gt, pts))
        exact = wide(kind, pred, gt, pts)
        tol = ref.bound(pred, gt, pts, want)
        assert tol < 1e-9 * max(np.abs(pts).max(), 1e-3), f"{name} {kind}: a bound of {tol} says nothing"
        # the fixture within half the bound of the 80-bit value: a wrong bound shows here and not on the GPU
        assert abs(float(LD(want) - exact)) <= tol / 2, f"{name} {kind}: fixture {want!r}, 80-bit {exact!r}, bound {tol}"
        assert abs(float(LD(got) - exact)) <= tol / 2, f"{name} {kind}: restatement {got!r}, 80-bit {exact!r}, bound {tol}"
        assert abs(got - want) <= tol, f"{name} {kind}: restatement {got!r}, fixture {want!r}, bound {tol}"
    if name.endswith("_same"):
        assert w_add == 0.0 and w_adds == 0.0 and ref.pose_error("add", pred, gt, pts) == 0.0 \
            and ref.pose_error("adds", pred, gt, pts) == 0.0


def test_restatement_orders_and_edges():
    rng = np.random.default_rng(5)
    v = rng.uniform(0, 1, 700)
    assert abs(ref.mean_in_order(v) - v.mean()) < 1e-15 and ref.mean_in_order(np.array([0.25])) == 0.25
    # the order is the one the docstring states: chunk 0 alone is (lanes by halving) then wave 0 + wave 1
    a = v[:256].reshape(2, 2, 64)
    t = a[0] + a[1]
    for h in (32, 16, 8, 4, 2, 1):
        t = t[:, :h] + t[:, h:2 * h]
    assert ref.mean_in_order(v[:256]) == (t[0, 0] + t[1, 0]) / 256
    P = np.eye(4)
    P[:3] = rng.standard_normal((3, 4))
    assert ref.same_bits(ref.pose_times_sym(P, np.eye(4)), P)
    pts = rng.standard_normal((5, 3))
    bad = P.copy()
    bad[1, 2] = np.inf
    assert np.isnan(ref.pose_error("add", bad, P, pts)) and np.isnan(ref.pose_error("adds", P, bad, pts))
    assert np.isnan(ref.pose_error("adds", P, P, np.where(np.arange(15).reshape(5, 3) == 7, np.nan, pts)))


def test_compute_auc_equals_the_reference_bit_for_bit():
    from pedp_hip.compat import compute_auc_sklearn

    for name in (str(c) for c in GOLD["auc/cases"]):
        errs, max_val, step = GOLD[f"auc/{name}/errs"], float(GOLD[f"auc/{name}/max_val"]), float(GOLD[f"auc/{name}/step"])
        got = compute_auc_sklearn(errs.copy(), max_val=max_val, step=step)
        assert ref.same_bits(got, GOLD[f"auc/{name}/out"]), f"{name}: {got!r} != {float(GOLD[f'auc/{name}/out'])!r}"
        assert ref.same_bits(compute_auc_sklearn(list(errs[::-1]), max_val, step), got), f"{name}: a list, unsorted"
    assert compute_auc_sklearn([0.0]) == 1.0 and compute_auc_sklearn([1.0]) == 0.0


def test_symmetry_tfs_from_info():
    from pedp_hip.compat import euler_matrix, symmetry_tfs_from_info

    none = symmetry_tfs_from_info({})
    assert none.shape == (1, 4, 4) and none.dtype == np.float64 and np.array_equal(none[0], np.eye(4))
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])
    flip[:3, 3] = [10.0, -20.0, 30.0]
    turn = np.array([[0.0, -1, 0, 4.0], [1, 0, 0, 0], [0, 0, 1, -8.0], [0, 0, 0, 1]])
    info = {"symmetries_discrete": [list(flip.reshape(-1)), list(turn.reshape(-1))]}
    keep = [list(m) for m in info["symmetries_discrete"]]
    got = symmetry_tfs_from_info(info)
    assert got.shape == (3, 4, 4) and np.array_equal(got[0], np.eye(4))
    for g, m in zip(got[1:], (flip, turn)):
        want = m.copy()
        want[:3, 3] *= 0.001
        assert np.array_equal(g, want)
    assert info["symmetries_discrete"] == keep, "the caller's lists were changed"
    for axis, pick in (([0, 0, 1], lambda r: (0, 0, r)), ([0, 1, 0], lambda r: (0, r, 0)), ([1, 0, 0], lambda r: (r, 0, 0))):
        cont = {"symmetries_continuous": [{"axis": axis, "offset": [0.5, -1.5, 2.0]}]}
        got = symmetry_tfs_from_info(cont)
        assert got.shape == (1 + 72, 4, 4) and np.array_equal(got[0], np.eye(4))
        for k, deg in enumerate(np.arange(0, 360, 5)):
            want = euler_matrix(*pick(deg / 180.0 * np.pi))
            want[:3, 3] = [0.5, -1.5, 2.0]
            assert np.array_equal(got[1 + k], want), f"axis {axis}, {deg} degrees"
    both = symmetry_tfs_from_info({**info, **cont}, rot_angle_discrete=90)
    assert both.shape == (1 + 2 + 4, 4, 4)
    still = symmetry_tfs_from_info({"symmetries_continuous": [{"axis": [0, 0, 0], "offset": [0, 0, 1.0]}]})
    assert still.shape == (2, 4, 4) and np.array_equal(still[1][:3, 3], [0, 0, 1.0]) and np.array_equal(still[1][:3, :3], np.eye(3))


def test_compat_exports_the_metrics():
    from pedp_hip import compat, metrics

    for name in ("add_err", "adds_err", "add_err_batch", "adds_err_batch", "compute_auc_sklearn", "symmetry_tfs_from_info"):
        assert name in compat.__all__ and getattr(compat, name) is getattr(metrics, name)
    ns = {}
    exec("from pedp_hip.compat import *", ns)
    assert callable(ns["add_err"]) and callable(ns["compute_auc_sklearn"])


def test_bad_arguments_are_refused_before_any_library_call(monkeypatch):
    from pedp_hip import _lib, metrics

    def no_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_call)
    monkeypatch.setattr(_lib, "default_context", no_call)
    P, pts = np.tile(np.eye(4), (3, 1, 1)), np.zeros((5, 3))
    E = _lib.PedpError
    for fn in (metrics.add_err_batch, metrics.adds_err_batch):
        for preds, gts, mp, kw in (
                (np.eye(4), np.eye(4), pts, {}),                                  # preds without a batch axis
                (np.zeros((3, 3, 4)), np.eye(4), pts, {}),
                (P, np.zeros((3, 4)), pts, {}),
                (P, np.tile(np.eye(4), (2, 1, 1)), pts, {}),                      # G is neither 1 nor B
                (P, np.tile(np.eye(4), (4, 1, 1)), pts, {}),
                (P, np.eye(4), np.zeros((5, 2)), {}),
                (P, np.eye(4), np.zeros(15), {}),
                (P, np.eye(4), np.zeros((0, 3)), {}),                             # no points
                (P, np.eye(4), pts, {"symmetry_tfs": np.zeros((2, 3, 3))}),
                (P, np.eye(4), pts, {"symmetry_tfs": np.zeros((0, 4, 4))}),
                (P, np.eye(4), pts, {"out": np.empty(2)}),                        # a wrong length
                (P, np.eye(4), pts, {"out": np.empty(3, np.float32)}),
                (P, np.eye(4), pts, {"out": np.empty(6)[::2]}),                   # strided
                (P, np.eye(4), pts, {"out": np.empty((3, 1))}),
                (P, np.eye(4), pts, {"out": [0.0, 0.0, 0.0]}),
                (np.zeros((65536, 4, 4), np.float32), np.eye(4), pts, {})):
            with pytest.raises(E):
                fn(preds, gts, mp, **kw)
        read_only = np.empty(3)
        read_only.flags.writeable = False
        with pytest.raises(E):
            fn(P, np.eye(4), pts, out=read_only)
        assert fn(np.zeros((0, 4, 4)), np.eye(4), pts).shape == (0,)              # no poses: nothing to launch
    for fn in (metrics.add_err, metrics.adds_err):
        with pytest.raises(E):
            fn(P, np.eye(4), pts)
        with pytest.raises(E):
            fn(np.eye(4), np.eye(3), pts)


def test_the_out_refusal_says_what_it_got():
    """The full text of the batch functions' refusal of `out`: a wrong dtype, a wrong shape, a strided array."""
    from pedp_hip import _lib, metrics

    P, pts = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), np.zeros((5, 3))
    for fn in (metrics.add_err_batch, metrics.adds_err_batch):
        want = f"{fn.__name__}: out must be a C-contiguous float64 array of 2 values in host memory, got a "
        for out, got in ((np.empty(2, np.float32), "float32 array of shape (2,)"),
                         (np.empty(3, np.float64), "float64 array of shape (3,)"),
                         (np.empty(4, np.float64)[::2], "float64 array of shape (2,), strided")):
            with pytest.raises(_lib.PedpError) as e:
                fn(P, P[0], pts, out=out)
            assert str(e.value) == want + got


def test_the_abi_symbol_is_declared_and_exported():
    from pedp_hip import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pedp.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pedp_pose_errors\s*\(", header) and re.search(r"PEDP_ERR_ADD = 0, PEDP_ERR_ADDS = 1", header)
    res, args = _lib.PROTOTYPES["pedp_pose_errors"]
    assert res is ctypes.c_int and len(args) == 12 and args[2] is ctypes.c_int64
    assert (_lib.ERR_ADD, _lib.ERR_ADDS) == (0, 1)
    assert hasattr(_lib.load(), "pedp_pose_errors")
    ctx = ctypes.c_void_p()        # a null context is refused before anything else is looked at
    assert _lib.load().pedp_pose_errors(ctx, None, 1, None, 1, None, 1, None, 0, 0, 0, None) == -1
