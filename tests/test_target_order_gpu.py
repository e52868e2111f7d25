"""The order of a target pack's rows: Hilbert runs (mode 1) against the balanced k-d split (mode 2) (GPU).

Any partition of a target's rows into tiles of 16 gives the same results: the filter keeps every tile that holds a
point within reach, the selection is exact and breaks ties by the original index.  So the bound between the two orders
is the strictest there is -- the raw bytes are equal -- and pedp_cloud_target_order shows that the order asked for really
was in force.  The split's rule is restated in numpy below (compact_order) and the device's permutation must equal it
entry for entry.  Modes are forced with pedp_cloud_set_target_order; only the automatic mode's test, which has to
know that PEDP_ICP_TARGET_ORDER is not set (read once per process), runs in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _nn_cases as cases

pytestmark = pytest.mark.gpu

HILBERT, COMPACT = 1, 2
FIXED = dict(relative_fitness=-1, relative_rmse=-1)


def compact_order(xyz):
    """The rule of csrc/icp/target_order.h on rows given in the cloud's Hilbert order (centred float32 x y z):
    positions of those rows in the compact order."""
    xyz = np.asarray(xyz, np.float32)
    order = np.arange(len(xyz))
    todo = [(0, len(xyz))]
    while todo:
        s, m = todo.pop()
        if m <= 16:
            continue
        seg = order[s:s + m]
        p = xyz[seg]
        ext = p.max(0) - p.min(0)                      # float32
        axis = 0
        if ext[1] > ext[axis]:
            axis = 1
        if ext[2] > ext[axis]:
            axis = 2
        order[s:s + m] = seg[np.argsort(p[:, axis], kind="stable")]   # ties: the position so far; -0 == +0
        u = 1024 if m > 1024 else 64 if m > 64 else 16
        h = u * -(-m // (2 * u))
        todo += [(s, h), (s + h, m - h)]
    return order


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _same_result(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        _same_bytes(np.asarray(a[k]), np.asarray(b[k]), f"{what}: {k}")


def _target(ctx, pts, nrm, mode):
    from pedp_hip import _lib

    t = _lib.Cloud(ctx, pts, nrm)
    _lib.cloud_set_target_order(t, mode)
    return t


@pytest.fixture(scope="module")
def parity(ctx):
    from pedp_hip import _lib, synth

    f = synth.Frame("parity")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    assert len(f.model_points) == 2000
    return f, _lib.Cloud(ctx, scene)


def _parity_calls(ctx, f, src, tgt):
    """Every way into the registration, on one target handle."""
    from pedp_hip import _lib, synth

    init = f.icp_init()
    out = {}
    out["p2pl"] = _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=20, want_corr=True, want_trace=True, **FIXED)
    assert out["p2pl"]["trace"].shape == (21, 18)
    out["p2pt"] = _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=6, estimator=_lib.POINT_TO_POINT, want_corr=True,
                           want_trace=True, **FIXED)
    _lib.icp_begin(ctx, src, tgt, 10.0, init, max_iteration=20, want_trace=True, **FIXED)
    out["beginend"] = _lib.icp_end(ctx, want_corr=True)
    inits = np.stack([np.linalg.inv(T) for T in synth.batched_start_poses(8)])
    out["batch8"] = dict(zip("T fit rmse its".split(), _lib.icp_batched_ex(ctx, src, tgt, np.full(8, 8.0), inits, max_iteration=15)))
    _lib.icp_configure(ctx, exhaustive=True)
    try:
        out["exhaustive"] = _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=4, want_corr=True, want_trace=True, **FIXED)
    finally:
        _lib.icp_configure(ctx, exhaustive=False)
    idx, d2 = _lib.nn(ctx, src, tgt, init)
    out["nn"] = {"idx": idx, "d2": d2}
    return out


def test_parity_frame_every_entry_point_equal_in_every_byte(ctx, parity):
    from pedp_hip import _lib

    f, src = parity
    res = {}
    for mode in (HILBERT, COMPACT):
        tgt = _target(ctx, f.model_points, f.normals, mode)
        assert _lib.cloud_target_order(tgt) == 0
        res[mode] = _parity_calls(ctx, f, src, tgt)
        assert _lib.cloud_target_order(tgt) == mode
    assert set(res[HILBERT]) == {"p2pl", "p2pt", "beginend", "batch8", "exhaustive", "nn"}
    for name in res[HILBERT]:
        _same_result(res[HILBERT][name], res[COMPACT][name], name)
    assert (res[COMPACT]["nn"]["idx"] >= 0).all()


def test_graphs_captured_before_the_order_changes_replay_after_it(ctx, parity):
    """One handle: batches in the Hilbert order capture their graphs (the fused batch's group graph; a radius beyond
    the fused pass replays one captured registration per pose on sub-contexts); the order then changes under them --
    the pack is rewritten where it is -- and the same batches run again."""
    from pedp_hip import _lib, synth

    f, src = parity
    tgt = _target(ctx, f.model_points, f.normals, HILBERT)
    inits8 = np.stack([np.linalg.inv(T) for T in synth.batched_start_poses(8)])

    def batches():
        a = _lib.icp_batched_ex(ctx, src, tgt, np.full(8, 8.0), inits8, max_iteration=15)
        b = _lib.icp_batched_ex(ctx, src, tgt, np.full(3, 500.0), inits8[:3], max_iteration=6)
        return a + b

    n0 = _lib.icp_graph_captures(ctx)
    before = batches()
    assert _lib.cloud_target_order(tgt) == HILBERT
    n1 = _lib.icp_graph_captures(ctx)
    assert n1 >= n0 + 2                            # the group graph and at least one per-pose graph exist now
    _lib.cloud_set_target_order(tgt, COMPACT)
    after = batches()
    assert _lib.cloud_target_order(tgt) == COMPACT
    assert _lib.icp_graph_captures(ctx) == n1      # ... and were replayed, not captured again
    for k, (a, b) in enumerate(zip(before, after)):
        _same_bytes(a, b, k)
    _lib.cloud_set_target_order(tgt, HILBERT)      # ... and back
    again = batches()
    assert _lib.cloud_target_order(tgt) == HILBERT
    assert _lib.icp_graph_captures(ctx) == n1
    for k, (a, b) in enumerate(zip(before, again)):
        _same_bytes(a, b, k)


@pytest.mark.parametrize("geometry", sorted(cases.GEOMETRIES))
def test_tie_and_adversarial_cases_against_the_oracle(ctx, oracle, geometry):
    from pedp_hip import _lib

    src, tgt, nrm = cases.GEOMETRIES[geometry](700, 3000, 31)
    S, Tg = _lib.Cloud(ctx, src), _target(ctx, tgt, nrm, COMPACT)
    idx, d2 = _lib.nn(ctx, S, Tg, np.eye(4))
    assert _lib.cloud_target_order(Tg) == COMPACT
    ridx, rd2 = oracle.nn(src, tgt)
    assert np.array_equal(idx, ridx), np.nonzero(idx != ridx)[0][:8]
    _same_bytes(d2, rd2, geometry)


def _shape(name):
    rng = np.random.default_rng(5)
    if name[1:].isdigit():
        return rng.normal(0.0, 1.0, (int(name[1:]), 3))
    if name == "identical":
        return np.tile([0.25, -0.5, 1.0], (1500, 1))
    if name == "collinear":
        t = np.zeros((1500, 3))
        t[:, 1] = rng.normal(0.0, 1.0, 1500)
        return t
    if name == "duplicated":      # three copies of every row: ties on every axis, and copies that a split separates
        return np.tile(rng.normal(0.0, 1.0, (700, 3)), (3, 1))
    assert name == "nonfinite"
    t = rng.normal(0.0, 1.0, (1500, 3))
    bad = rng.choice(1500, 90, replace=False)
    for j, i in enumerate(bad):
        t[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    return t


SHAPES = ["n1", "n15", "n16", "n17", "n63", "n65", "n1023", "n1024", "n1025", "n2049", "identical", "collinear", "duplicated",
          "nonfinite"]


@pytest.mark.parametrize("name", SHAPES)
def test_split_shapes(ctx, oracle, name):
    """tile_perm is a permutation of the finite rows and equals the numpy restatement; every sphere holds its rows;
    the neighbours are the brute-force ones."""
    from pedp_hip import _lib

    tgt = _shape(name)
    nrm = np.tile([0.0, 0.0, 1.0], (len(tgt), 1))
    rng = np.random.default_rng(6)
    finite = np.isfinite(tgt).all(1)
    src = tgt[finite][rng.integers(0, finite.sum(), 300)] + rng.normal(0.0, 0.05, (300, 3))
    S = _lib.Cloud(ctx, src)
    packs, found = {}, {}
    for mode in (HILBERT, COMPACT):
        Tg = _target(ctx, tgt, nrm, mode)
        found[mode] = _lib.nn(ctx, S, Tg, np.eye(4))
        assert _lib.cloud_target_order(Tg) == mode
        packs[mode] = _lib.debug_target_pack(ctx, Tg)
    h, c = packs[HILBERT], packs[COMPACT]
    n = int(finite.sum())
    assert h["rows"] == c["rows"] == n
    assert np.array_equal(np.sort(c["tile_perm"][:n]), np.nonzero(finite)[0])
    assert np.array_equal(c["tile_perm"][n:], h["tile_perm"][n:])          # non-finite rows stay last, never packed
    want = h["tile_perm"][:n][compact_order(h["tgt4"][:n, :3])]
    assert np.array_equal(c["tile_perm"][:n], want), np.nonzero(c["tile_perm"][:n] != want)[0][:8]
    _same_bytes(c["tgt4"][:n], h["tgt4"][:n][compact_order(h["tgt4"][:n, :3])], "rows of the operand")
    for pack in (h, c):
        rows = pack["tgt4"][:n, :3].astype(np.float64)
        for unit, sph in ((16, pack["sph16"]), (64, pack["sph64"]), (1024, pack["sph1024"])):
            sph = sph.astype(np.float64)
            k = np.arange(n) // unit
            d = np.linalg.norm(rows - sph[k, :3], axis=1)
            assert (d <= sph[k, 3]).all(), (unit, np.nonzero(d > sph[k, 3])[0][:8])
            assert (sph[-(-n // unit):, 3] < 0).all()                      # a unit without rows matches nothing
    ridx, rd2 = oracle.nn(src, tgt)
    for mode in (HILBERT, COMPACT):
        assert np.array_equal(found[mode][0], ridx), (mode, np.nonzero(found[mode][0] != ridx)[0][:8])
        _same_bytes(found[mode][1], rd2, mode)


_AUTO = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from pedp_hip import _lib
ctx = _lib.Context(0)
rng = np.random.default_rng(9)
for nt, orders in ((16400, [1, 2, 2]), (16000, [1, 1, 1])):
    tgt = rng.normal(0.0, 1.0, (nt, 3)) * [40.0, 30.0, 5.0]
    nrm = np.tile([0.0, 0.0, 1.0], (nt, 1))
    src = tgt[rng.integers(0, nt, 3000)] + rng.normal(0.0, 0.2, (3000, 3))
    T = np.eye(4); T[:3, 3] = [0.5, -0.4, 0.3]
    S, Tg = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    assert _lib.cloud_target_order(Tg) == 0
    idx0, d20 = _lib.nn(ctx, S, Tg, T)                      # a search is no registration: it does not count
    assert _lib.cloud_target_order(Tg) == 1
    seen, res = [], []
    for k in range(3):
        if k == 1:
            _lib.icp_begin(ctx, S, Tg, 3.0, T, max_iteration=8, want_trace=True, relative_fitness=-1, relative_rmse=-1)
            r = _lib.icp_end(ctx, want_corr=True)
        else:
            r = _lib.icp(ctx, S, Tg, 3.0, T, max_iteration=8, want_corr=True, want_trace=True, relative_fitness=-1, relative_rmse=-1)
        seen.append(_lib.cloud_target_order(Tg)); res.append(r)
    assert seen == orders, (nt, seen)
    assert res[0]["fitness"] > 0.5
    for r in res[1:]:
        for key in ("T", "trace", "corr"):
            assert np.array_equal(np.ascontiguousarray(r[key]).view(np.uint8), np.ascontiguousarray(res[0][key]).view(np.uint8)), (nt, key)
        assert r["fitness"] == res[0]["fitness"] and r["inlier_rmse"] == res[0]["inlier_rmse"] and r["iters"] == res[0]["iters"]
    idx1, d21 = _lib.nn(ctx, S, Tg, T)
    assert np.array_equal(idx0, idx1) and np.array_equal(d20.view(np.uint64), d21.view(np.uint64))
print("auto ok")
"""


def test_automatic_mode_upgrades_at_the_second_registration_of_a_large_target():
    """16,400 finite rows: Hilbert for the first registration, compact from the second; 16,000 rows: never.  The
    results are the same in both."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "PEDP_ICP_TARGET_ORDER"}
    p = subprocess.run([sys.executable, "-c", _AUTO, root], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"auto ok" in p.stdout, p.stdout.decode()


def test_bench_frame_equal_bytes_and_fewer_pairs(ctx):
    """The bench_100k registration once per order: every output byte equal, and the pairs the sweep evaluates per pass
    in the compact order at most 0.80 of the Hilbert order's (the CPU model, tools/target_tiles_model.py, gives 0.66;
    the margin covers its scene proxy and the cover's splitting of wide sub-blocks, which the model leaves out)."""
    from pedp_hip import _lib, synth

    f = synth.Frame("bench_100k")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    src = _lib.Cloud(ctx, f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"]))
    res, per_pass = {}, {}
    for mode in (HILBERT, COMPACT):
        tgt = _target(ctx, f.model_points, f.normals, mode)
        res[mode] = _lib.icp(ctx, src, tgt, 10.0, f.icp_init(), max_iteration=20, want_corr=True, want_trace=True, **FIXED)
        assert _lib.cloud_target_order(tgt) == mode
        passes, pairs, _ = _lib.icp_last_stats(ctx)
        assert passes == 21
        per_pass[mode] = pairs / passes
    _same_result(res[HILBERT], res[COMPACT], "bench_100k")
    print(f"pairs swept per pass: hilbert {per_pass[HILBERT]:.4g}, compact {per_pass[COMPACT]:.4g}, "
          f"ratio {per_pass[COMPACT] / per_pass[HILBERT]:.3f}")
    assert per_pass[COMPACT] <= 0.80 * per_pass[HILBERT]
