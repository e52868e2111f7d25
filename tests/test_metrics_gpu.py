"""pedp_pose_errors on the device: against the reference's fixture within the derived bound (tests/test_metrics_cpu.py
states it), bit for bit against the numpy restatement (tests/_metrics_ref.py) across the kernel's block sizes, padding,
independence of batch and stream, symmetries, non-finite inputs, and the estimator's hook.

The kernel's own sizes: 128 threads hold 2 points each (a chunk of 256 points gives one partial sum), pred points pass
through LDS in tiles of 256.  The N of the bit-for-bit cases straddle 128, 256, 1024 and go past 2048."""
import logging
import os

import numpy as np
import pytest

import _metrics_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g11_metrics.npz"))
GROUPS = sorted({str(c).rsplit("_", 1)[0] for c in GOLD["cases"]}, key=lambda g: (int(g.split("_")[0]), g))
OFFSETS = ("same", "1e-9", "1e-3", "0.3", "3.1")
NS = (1, 2, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2051)
KINDS = ("add", "adds")


def fns():
    from pedp_hip import compat

    return {"add": (compat.add_err, compat.add_err_batch), "adds": (compat.adds_err, compat.adds_err_batch)}


def cuda(a, dtype=None):
    return torch.as_tensor(np.asarray(a), device="cuda", dtype=dtype)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == np.float64
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def random_poses(rng, n, spread=0.02):
    """n ground truths (float64) and n predictions near them (float32, as the estimator's are)."""
    gts = np.tile(np.eye(4), (n, 1, 1))
    gts[:, :3, :3] = rotations(rng, n)
    gts[:, :3, 3] = rng.uniform(-0.2, 0.2, (n, 3)) + [0, 0, 0.6]
    preds = gts.copy()
    turn = rotations(rng, n)
    turn = np.eye(3) + 0.3 * (turn - np.eye(3))                      # not a rotation any more: the metric does not care
    preds[:, :3, :3] = turn @ gts[:, :3, :3]
    preds[:, :3, 3] += rng.normal(0, spread, (n, 3))
    return preds.astype(np.float32), gts


# ---------------------------------------------------------------- 1. the reference's fixture

@pytest.mark.parametrize("group", GROUPS)
def test_fixture_cases_within_the_bound_single_and_batch_forms_equal(group):
    pts = GOLD[f"pts/{group}"]
    preds = np.stack([GOLD[f"{group}_{o}/pred"] for o in OFFSETS])
    gts = np.stack([GOLD[f"{group}_{o}/gt"] for o in OFFSETS])
    assert preds.dtype == np.float32 and gts.dtype == np.float64
    for kind in KINDS:
        one, batch = fns()[kind]
        wants = np.array([float(GOLD[f"{group}_{o}/{kind}"]) for o in OFFSETS])
        from_numpy = batch(preds, gts, pts)
        from_cuda = batch(cuda(preds), cuda(gts), cuda(pts))
        assert isinstance(from_numpy, np.ndarray) and from_numpy.dtype == np.float64 and from_numpy.shape == (5,)
        assert from_cuda.is_cuda and from_cuda.dtype == torch.float64 and tuple(from_cuda.shape) == (5,)
        assert same(from_numpy, from_cuda), f"{group} {kind}: numpy and CUDA inputs differ"
        for k, o in enumerate(OFFSETS):
            tol = ref.bound(preds[k], gts[k], pts, wants[k])
            single = one(preds[k], gts[k], pts)
            single_cuda = one(cuda(preds[k]), cuda(gts[k]), cuda(pts, torch.float32))   # the points are float32 values
            alone = batch(preds[k:k + 1], gts[k], pts)
            print(f"{group}_{o} {kind}: got {float(single)!r} want {wants[k]!r} |diff| {abs(float(single) - wants[k]):.3e} bound {tol:.3e}")
            assert type(single) is np.float64 and type(single_cuda) is np.float64
            assert abs(float(single) - wants[k]) <= tol, f"{group}_{o} {kind}: {float(single)!r} != {wants[k]!r} (bound {tol})"
            assert same(single, from_numpy[k]) and same(single_cuda, single) and same(alone[0], single), \
                f"{group}_{o} {kind}: single {float(single)!r}, in the batch {from_numpy[k]!r}, alone {alone[0]!r}"
        assert wants[0] == 0.0 and from_numpy[0] == 0.0


# ---------------------------------------------------------------- 2. bit for bit against the restatement

@pytest.fixture(scope="module")
def cycle():
    """Three predictions and two ground truths; a batch of B poses pairs prediction b % 3 with ground truth b % 2 (G = B)
    or with ground truth 0 (G = 1), so that six restated values per N and kind cover every batch."""
    preds, gts = random_poses(np.random.default_rng(21), 3)
    return preds, gts[:2]


@pytest.mark.parametrize("n", NS)
def test_bit_for_bit_against_the_restatement(cycle, n):
    P, Gt = cycle
    pts = np.random.default_rng(100 + n).uniform(-0.06, 0.06, (n, 3)).astype(np.float32).astype(np.float64)
    for kind in KINDS:
        batch = fns()[kind][1]
        want = np.array([[ref.pose_error(kind, P[p], Gt[g], pts) for g in range(2)] for p in range(3)])
        assert np.isfinite(want).all() and (want > 0).all() and len(np.unique(want)) == 6
        for B in (1, 3, 252):
            idx = np.arange(B)
            preds = P[idx % 3]
            for gts, w in ((Gt[0], want[idx % 3, 0]), (Gt[idx % 2], want[idx % 3, idx % 2])):
                got = batch(cuda(preds), cuda(gts), cuda(pts))
                assert same(got, w), (f"n={n} {kind} B={B} G={1 if gts.ndim == 2 else B}: "
                                      f"{int((bits(got) != bits(w)).sum())} of {B} differ, first {got[0].item()!r} != {w[0]!r}")
            assert same(batch(preds, Gt[idx % 2], pts), want[idx % 3, idx % 2]), f"n={n} {kind} B={B}: host memory"


def test_bit_for_bit_with_every_pose_of_a_batch_distinct():
    rng = np.random.default_rng(31)
    preds, gts = random_poses(rng, 252)
    for kind, n in (("add", 2051), ("adds", 257)):
        pts = rng.uniform(-0.06, 0.06, (n, 3))
        batch = fns()[kind][1]
        assert same(batch(cuda(preds), cuda(gts), cuda(pts)), ref.pose_errors(kind, preds, gts, pts)), kind
        assert same(batch(cuda(preds), cuda(gts[7]), cuda(pts)), ref.pose_errors(kind, preds, gts[7], pts)), kind


# ---------------------------------------------------------------- 3. padding

@pytest.mark.parametrize("n", (129, 257, 513))
def test_padding_slots_and_padding_queries_contribute_nothing(n):
    """One point past a block of queries (129), past a tile and a chunk (257), past two (513).  Far from the origin a
    zero-filled pred slot would sit ~8.7 away and cannot win a minimum, but a padded query would add ~8.7 to the sum;
    around the origin, with gt points within 1e-5 of it, a zero-filled slot would win their minima (true distance 1e-3)."""
    rng = np.random.default_rng(n)
    gt = np.eye(4)
    pred = np.eye(4)
    pred[:3, 3] = [1e-3, 0, 0]
    far = rng.uniform(5, 6, (n, 3))
    near = rng.uniform(-0.5, 0.5, (n, 3))
    near[[0, n // 2, n - 1]] = rng.uniform(-1e-5, 1e-5, (3, 3))
    for name, pts in (("far", far), ("near", near)):
        for kind in KINDS:
            one = fns()[kind][0]
            got, want = one(pred, gt, pts), ref.pose_error(kind, pred, gt, pts)
            assert same(got, want), f"{name} n={n} {kind}: {float(got)!r} != {float(want)!r}"
            assert 0 < float(got) <= 1e-3 * (1 + 1e-9)


# ---------------------------------------------------------------- 4. independence

def test_a_pose_does_not_depend_on_its_batch_its_stream_or_the_run():
    rng = np.random.default_rng(41)
    preds, gts = random_poses(rng, 252)
    pts = rng.uniform(-0.06, 0.06, (700, 3))
    dp, dg, dm = cuda(preds), cuda(gts), cuda(pts)
    for kind in KINDS:
        batch = fns()[kind][1]
        whole = batch(dp, dg, dm)
        assert same(batch(dp, dg, dm), whole), f"{kind}: a second run differs"
        for b in (0, 1, 100, 251):
            assert same(batch(dp[b:b + 1], dg[b:b + 1], dm), whole[b:b + 1]), f"{kind}: pose {b} alone"
            assert same(batch(dp[b:b + 3], dg[b], dm)[:1], batch(dp[b:b + 1], dg[b], dm)), f"{kind}: pose {b}, shared gt"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = batch(dp, dg, dm)
        side.synchronize()
        assert same(on_side, whole), f"{kind}: another stream"
        out = torch.full((252,), -7.0, dtype=torch.float64, device="cuda")
        assert batch(dp, dg, dm, out=out) is out and same(out, whole)
        host_out = np.full(252, -7.0)
        got = batch(preds, gts, pts, out=host_out)
        assert got is host_out and same(host_out, whole)
        as_tensor = batch(torch.from_numpy(preds), torch.from_numpy(gts), torch.from_numpy(pts))
        assert torch.is_tensor(as_tensor) and not as_tensor.is_cuda and same(as_tensor, whole)
        from pedp_hip import _lib
        for bad in (torch.empty(252, dtype=torch.float64), torch.empty(252, dtype=torch.float32, device="cuda"),
                    torch.empty(504, dtype=torch.float64, device="cuda")[::2], np.empty(252)):
            with pytest.raises(_lib.PedpError):
                batch(dp, dg, dm, out=bad)


# ---------------------------------------------------------------- 5. symmetries

def test_symmetries():
    rng = np.random.default_rng(51)
    preds, gts = random_poses(rng, 7)
    preds[3, 0, 1] = -0.0                                              # a signed zero must not tell the two paths apart
    pts = rng.uniform(-0.06, 0.06, (300, 3))
    for kind in KINDS:
        batch = fns()[kind][1]
        plain = batch(cuda(preds), cuda(gts), cuda(pts))
        assert same(batch(cuda(preds), cuda(gts), cuda(pts), symmetry_tfs=cuda(np.eye(4)[None])), plain), f"{kind}: S=1 identity"
        assert same(batch(preds, gts, pts, symmetry_tfs=np.eye(4, dtype=np.float32)), plain), f"{kind}: one 4 x 4 identity"
        syms = np.tile(np.eye(4), (5, 1, 1))
        syms[1:, :3, :3] = rotations(rng, 4)
        syms[1:, :3, 3] = rng.normal(0, 0.01, (4, 3))
        got = batch(cuda(preds), cuda(gts[2]), cuda(pts), symmetry_tfs=cuda(syms))
        assert same(got, ref.pose_errors(kind, preds, gts[2], pts, sym=syms)), f"{kind}: five symmetries"
        assert (bits(got) != bits(batch(cuda(preds), cuda(gts[2]), cuda(pts)))).any() or kind == "adds"
    # a cloud closed under the half turn about z, coordinates dyadic; the prediction is the ground truth turned by it
    half = rng.integers(-512, 512, (150, 3)) / 1024.0
    cloud = np.concatenate([half, half * [-1, -1, 1]])
    turn = np.diag([-1.0, -1.0, 1.0, 1.0])
    gt = gts[0]
    pred = gt @ turn
    assert np.array_equal(pred[:, :2], -gt[:, :2]) and np.array_equal(pred[:, 2:], gt[:, 2:])
    group = np.stack([np.eye(4), turn])
    add, add_b = fns()["add"]
    adds, adds_b = fns()["adds"]
    assert float(add(pred, gt, cloud)) > 0.01
    assert float(add(pred, gt, cloud, symetry_tfs=group)) == float(add(pred, gt, cloud)), "add_err ignores its symmetries"
    with_group = add_b(pred[None], gt, cloud, symmetry_tfs=group)
    assert with_group[0] == 0.0 and not np.signbit(with_group[0])
    assert adds(pred, gt, cloud) == 0.0 and adds_b(pred[None], gt, cloud, symmetry_tfs=group)[0] == 0.0
    assert adds_b(cuda(pred[None]), cuda(gt), cuda(cloud), symmetry_tfs=cuda(group[::-1].copy()))[0].item() == 0.0


# ---------------------------------------------------------------- 6. non-finite inputs

def test_non_finite_inputs_give_nan_for_the_poses_that_read_them():
    rng = np.random.default_rng(61)
    preds, gts = random_poses(rng, 3)
    preds = preds.astype(np.float64)
    pts = rng.uniform(-0.06, 0.06, (600, 3))
    for kind in KINDS:
        batch = fns()[kind][1]
        clean = batch(preds, gts, pts)
        for where, value in (((1, 0, 2), np.nan), ((1, 2, 3), np.inf), ((1, 1, 1), -np.inf)):
            bad = preds.copy()
            bad[where] = value
            for got in (batch(bad, gts, pts), batch(cuda(bad), cuda(gts), cuda(pts)), batch(cuda(bad), cuda(gts[0]), cuda(pts))):
                got = got.cpu().numpy() if torch.is_tensor(got) else got
                assert np.isnan(got[1]) and np.isfinite(got[[0, 2]]).all(), f"{kind} pred{where}={value}: {got}"
            assert same(batch(bad, gts, pts)[[0, 2]], clean[[0, 2]]), f"{kind}: the other poses moved"
            bad_gt = gts.copy()
            bad_gt[where] = value
            got = batch(preds, bad_gt, pts)
            assert np.isnan(got[1]) and same(got[[0, 2]], clean[[0, 2]]), f"{kind} gt{where}={value}: {got}"
        bottom = preds.copy()
        bottom[1, 3] = np.nan                                          # the bottom row is not read
        assert same(batch(bottom, gts, pts), clean), f"{kind}: the bottom row was read"
        sym = np.tile(np.eye(4), (2, 1, 1))
        sym[1, 0, 3] = np.nan
        assert np.isnan(batch(preds, gts, pts, symmetry_tfs=sym)).all(), f"{kind}: a NaN in a symmetry"
        for row in (0, 300, 599):                                      # first block, a middle one, the last point
            for value in (np.inf, np.nan):
                p = pts.copy()
                p[row, 1] = value
                got = batch(cuda(preds), cuda(gts), cuda(p)).cpu().numpy()
                assert np.isnan(got).all(), f"{kind}: point {row} = {value}: {got}"
                assert np.isnan(ref.pose_errors(kind, preds, gts, p)).all()


# ---------------------------------------------------------------- 7. the estimator's hook

def test_the_estimators_hook(caplog):
    from test_estimator_gpu import K_, _Scene, _estimator
    from pedp_hip.compat import add_err_batch
    from pedp_hip.estimator import set_seed

    set_seed(0)
    scene = _Scene()
    est, *_ = _estimator(scene)
    rgb, depth, mask, _ = scene.frames[0]
    caplog.set_level(logging.INFO)
    assert est.gt_pose is None and est.add_errs is None
    assert float(est.compute_add_err_to_gt_pose(est.rot_grid).sum()) == -252
    est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=1)
    assert "add_errs" not in caplog.text and est.add_errs is None
    # a quarter turn about z at a dyadic translation: gt_pose @ inv(tf_to_center) is exact in float64 in any order
    X = np.array([[0.0, -1, 0, 0.0625], [1, 0, 0, -0.03125], [0, 0, 1, 0.5], [0, 0, 0, 1]])
    est.gt_pose = X
    c = np.asarray(est.model_center, np.float32).astype(np.float64)
    centred = X.copy()
    centred[:3, 3] = np.array([-c[1], c[0], c[2]]) + X[:3, 3]
    tf = est.get_tf_to_centered_mesh().cpu().numpy().astype(np.float64)
    back = np.eye(4)
    back[:3, 3] = c
    assert np.array_equal(tf @ back, np.eye(4)) and np.array_equal(centred, X @ back)
    centred = centred.astype(np.float32)
    zero = est.compute_add_err_to_gt_pose(cuda(centred[None]))
    assert zero.is_cuda and zero.dtype == torch.float32 and tuple(zero.shape) == (1,) and zero.item() == 0.0
    poses = est.rot_grid.clone()
    poses[:, :3, 3] = cuda([0.05, -0.02, 0.5], torch.float32)
    got = est.compute_add_err_to_gt_pose(poses)
    want = add_err_batch(poses, centred, est.pts, symmetry_tfs=est.symmetry_tfs)
    assert got.dtype == torch.float32 and tuple(got.shape) == (252,) and torch.equal(got, want.float())
    restated = ref.pose_errors("add", poses.cpu().numpy(), centred, est.pts.cpu().numpy(), sym=np.eye(4)[None])
    assert same(want, restated) and float(got.min()) > 0
    caplog.clear()
    est.register(K=K_, rgb=rgb, depth=depth, ob_mask=mask, iteration=1)
    lines = [r.getMessage() for r in caplog.records if "add_errs min:" in r.getMessage()]
    assert len(lines) == 2 and lines[0].startswith("after viewpoint, add_errs min:") and lines[1].startswith("final, add_errs min:")
    assert est.add_errs.dtype == torch.float32 and tuple(est.add_errs.shape) == (252,)
    assert torch.equal(est.add_errs, est.compute_add_err_to_gt_pose(est.poses)), "add_errs is not in the order of poses"
    assert lines[1] == f"final, add_errs min:{est.add_errs.min()}"
    assert not torch.equal(est.add_errs, est.add_errs.sort().values), "the scores' order happens to sort the errors"
