"""Case matrix of the registration's nearest-neighbour search against the float64 oracle (exact NN, strict
d^2 < r^2, lowest index on ties): geometries, sizes at chunk / tile / mask-word / list boundaries, radii on both
sides of the qt switch, and every path the library picks between.

Paths (pedp_icp.hip, icp_job_setup and icp_unit_size; BK_WCAP: icp/fused_close.h):
  fused      qt = 1: r^2 < diag^2 / 16 and Nt <= 524288 (BK_WCAP mask words of 1024 rows), not exhaustive;
  segmented  qt = 1: the same radius rule, a larger target;
  dense      qt = 4 (bf16 sweep): r^2 >= diag^2 / 16, or pedp_icp_configure(exhaustive).
Each case names the path the rule picks.  pedp_icp_last_stats shows culled against dense (pairs swept) and the
exact fallback (points re-searched); no counter tells fused from segmented, so that split rests on the rule and
the target size alone.

Every registration runs with relative_fitness = relative_rmse = -1 (a fixed number of passes) and is compared at
max_iteration 0, 1, 3 and its full count: correspondences equal, per-pass fitness equal, per-pass rmse within
1e-9, every pass's T and the result within POSE_TOL, iteration counts equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _nn_cases as cases

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-5
FULL = 10
BK_WCAP_ROWS = 524288


def _path(tgt, r, exhaustive=False):
    diag = cases.extent(tgt)
    if exhaustive or not (r * r < diag * diag / 16.0):
        return "dense"
    return "fused" if len(tgt) <= BK_WCAP_ROWS else "segmented"


def _init(tgt, deg=2.0, shift=0.0):
    """A rotation of `deg` about the target's centroid (finite rows) and a shift of `shift` along (1, -1, 1)/sqrt(3)."""
    from pedp_hip import synth

    t = np.asarray(tgt)
    c = t[np.isfinite(t).all(1)].mean(0)
    T = np.eye(4)
    T[:3, :3] = synth.axis_angle([0.3, -1.0, 0.5], np.deg2rad(deg))
    T[:3, 3] = c - T[:3, :3] @ c + shift * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    return T


def _check_nn(ctx, oracle, S, Tg, src, tgt, T):
    from pedp_hip import _lib

    idx, d2 = _lib.nn(ctx, S, Tg, T)
    ridx, rd2 = oracle.nn(oracle.transform(T, src), tgt)
    assert np.array_equal(idx, ridx), np.nonzero(idx != ridx)[0][:8]
    assert np.array_equal(d2.view(np.uint64), rd2.view(np.uint64)), np.nonzero(d2.view(np.uint64) != rd2.view(np.uint64))[0][:8]


def _check_icp(ctx, oracle, S, Tg, src, tgt, nrm, r, T, est, iters=(0, 1, 3, FULL), kdtree=True, scale=1.0):
    """Device registration against the oracle at each max_iteration of `iters`; returns pedp_icp_last_stats of
    each run (passes, pairs swept, fallback points).  scale < 1: the cloud's extent, the lengths' tolerances shrink
    with it."""
    from pedp_hip import _lib

    stats = []
    for mi in iters:
        res = _lib.icp(ctx, S, Tg, r, T, estimator=est, max_iteration=mi, relative_fitness=-1, relative_rmse=-1,
                       want_corr=True, want_trace=True)
        stats.append(_lib.icp_last_stats(ctx))
        ref = oracle.icp(src, tgt, nrm, r, T, estimator=est, max_iter=mi, rel_fitness=-1, rel_rmse=-1, kdtree=kdtree)
        _same(res, ref, mi, scale)
    return stats


def _same(res, ref, mi, scale=1.0):
    """The tolerances of the suite; on a cloud smaller than 1 (scale = its extent) the rmse and translation
    tolerances are relative to that extent instead (rotation entries keep POSE_TOL; a point-like target keeps all)."""
    s = min(1.0, scale) if scale > 0 else 1.0
    assert res["iters"] == ref["iters"] == mi
    bad = np.nonzero(res["corr"] != ref["corr"])[0]
    assert len(bad) == 0, (mi, bad[:8], res["corr"][bad[:8]], ref["corr"][bad[:8]])
    assert np.array_equal(res["trace"][:, 0], ref["trace"][:, 0])                          # per-pass fitness
    assert np.abs(res["trace"][:, 1] - ref["trace"][:, 1]).max() < 1e-9 * s                # per-pass rmse
    dT = np.abs(res["trace"][:, 2:] - ref["trace"][:, 2:]).reshape(-1, 4, 4)               # per-pass T
    assert dT[:, :3, :3].max() < POSE_TOL and dT[:, :3, 3].max() < POSE_TOL * s
    assert res["fitness"] == ref["fitness"] and abs(res["inlier_rmse"] - ref["inlier_rmse"]) < 1e-9 * s
    dT = np.abs(res["T"] - ref["T"])
    assert dT[:3, :3].max() < POSE_TOL and dT[:3, 3].max() < POSE_TOL * s


# (name, geometry, Ns, Nt, radius: number or (kind, value), estimator, init: "id" | "rot", expected path)
#   ("frac", f): f * diag; ("below", _) / ("above", _): diag / 4 * (1 -/+ 1e-6); ("over", _): 2 * diag.
P2PL, P2PT = 0, 1
CASES = [
    # fused: Ns at the 128-point chunk and 512-point boundaries, Nt at tile / list / mask-word boundaries
    ("fused_ns1", "blob", 1, 1025, 0.1, P2PL, "rot", "fused"),
    ("fused_ns127", "blob", 127, 1023, 0.1, P2PT, "rot", "fused"),
    ("fused_ns128", "blob", 128, 1024, 0.1, P2PL, "rot", "fused"),
    ("fused_ns129", "blob", 129, 65, ("frac", 0.1), P2PL, "rot", "fused"),
    ("fused_ns511", "blob", 511, 63, ("frac", 0.1), P2PT, "rot", "fused"),
    ("fused_ns512", "blob", 512, 64, ("frac", 0.1), P2PL, "rot", "fused"),
    ("fused_ns513", "blob", 513, 17, ("frac", 0.1), P2PL, "rot", "fused"),
    ("fused_nt16", "blob", 2000, 16, ("frac", 0.1), P2PT, "rot", "fused"),
    ("fused_nt15", "blob", 2000, 15, ("frac", 0.1), P2PL, "rot", "fused"),
    ("fused_nt2", "blob", 300, 2, ("frac", 0.2), P2PT, "rot", "fused"),
    ("fused_nt32767_tiny", "blob", 4000, 32767, ("frac", 1e-3), P2PL, "rot", "fused"),
    ("fused_nt32768", "blob", 4000, 32768, 0.1, P2PT, "rot", "fused"),
    ("fused_nt32769", "blob", 4000, 32769, 0.1, P2PL, "rot", "fused"),
    ("fused_below_qt", "blob", 511, 1023, ("below", 0), P2PL, "rot", "fused"),
    # scales and shapes
    # (far from the origin point-to-plane's 6 x 6 system in absolute coordinates has a condition number near
    # |c|^2 / extent^2 = 1e10: two float64 sums in different orders then differ by ~1e-4 in the pose, in the oracle as
    # much as on the device -- so the far cases solve point-to-point, which centres the data)
    ("far_typ", "far", 3000, 5000, 0.1, P2PT, "rot", "fused"),
    ("far_tiny", "far", 3000, 5000, ("frac", 1e-3), P2PT, "rot", "fused"),
    ("small_typ", "small", 3000, 5000, 1e-5, P2PL, "rot", "fused"),
    ("clusters", "clusters", 3000, 8000, 0.1, P2PL, "rot", "fused"),
    ("planar", "planar", 2000, 4000, 0.1, P2PL, "rot", "fused"),
    ("collinear", "collinear", 1000, 2000, 0.1, P2PL, "rot", "fused"),
    ("duplicated", "duplicated", 2000, 4000, 0.1, P2PT, "rot", "fused"),
    ("one_point", "one_point", 513, 1024, 0.5, P2PL, "rot", "dense"),
    ("nonfinite_source", "nonfinite_source", 1000, 2000, 0.1, P2PL, "rot", "fused"),
    ("nonfinite_source_dense", "nonfinite_source", 1000, 2000, ("over", 0), P2PT, "rot", "dense"),
    ("nonfinite_target", "nonfinite_target", 1000, 2000, 0.1, P2PL, "rot", "fused"),
    ("nonfinite_target_dense", "nonfinite_target", 1000, 2000, ("above", 0), P2PT, "rot", "dense"),
    # dense: radius at and beyond the qt switch, the same size boundaries
    ("dense_above_qt", "blob", 129, 1025, ("above", 0), P2PL, "rot", "dense"),
    ("dense_over_ns512", "blob", 512, 64, ("over", 0), P2PT, "rot", "dense"),
    ("dense_nt1", "blob", 1, 1, 0.5, P2PL, "rot", "dense"),
    ("dense_ns127", "blob", 127, 2, ("over", 0), P2PL, "rot", "dense"),
    ("dense_ns128", "blob", 128, 15, ("above", 0), P2PT, "rot", "dense"),
    ("dense_ns511", "blob", 511, 16, ("above", 0), P2PL, "rot", "dense"),
    ("dense_ns513", "blob", 513, 17, ("above", 0), P2PL, "rot", "dense"),
    ("dense_nt63", "blob", 1000, 63, ("over", 0), P2PT, "rot", "dense"),
    ("dense_nt65", "blob", 1000, 65, ("above", 0), P2PL, "rot", "dense"),
    ("dense_nt1023", "blob", 700, 1023, ("above", 0), P2PL, "rot", "dense"),
    ("dense_nt1024", "blob", 700, 1024, ("over", 0), P2PT, "rot", "dense"),
    ("dense_nt32767", "blob", 300, 32767, ("above", 0), P2PL, "rot", "dense"),
    ("dense_nt32768", "blob", 300, 32768, ("above", 0), P2PT, "rot", "dense"),
    ("dense_nt32769", "blob", 300, 32769, ("over", 0), P2PL, "rot", "dense"),
]


def _radius(spec, tgt):
    if not isinstance(spec, tuple):
        return float(spec)
    kind, v = spec
    diag = cases.extent(tgt)
    return {"frac": v * diag, "below": diag / 4 * (1 - 1e-6), "above": diag / 4 * (1 + 1e-6), "over": 2 * diag}[kind]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_icp_case_matrix(ctx, oracle, case):
    from pedp_hip import _lib

    name, geo, ns, nt, rspec, est, init, path = case
    src, tgt, nrm = cases.GEOMETRIES[geo](ns, nt, sum(map(ord, name)))
    assert (len(src), len(tgt)) == (ns, nt)
    r = _radius(rspec, tgt)
    assert _path(tgt, r) == path, (name, _path(tgt, r))
    T = _init(tgt) if init == "rot" else np.eye(4)
    S, Tg = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    _check_nn(ctx, oracle, S, Tg, src, tgt, T)
    # two target points: every update is rank-deficient (the rotation about their line is free), so only the
    # correspondence pass is defined
    its = (0,) if nt <= 2 else (0, 1, 3, FULL)
    stats = _check_icp(ctx, oracle, S, Tg, src, tgt, nrm, r, T, est, iters=its, kdtree=geo != "nonfinite_target",
                       scale=cases.extent(tgt))
    for (passes, swept, _), mi in zip(stats, its):
        assert passes == mi + 1
        if rspec == ("over", 0) and np.isfinite(src).all():   # a radius beyond the cloud: every pair swept every pass
            assert swept >= passes * ns * nt, (swept, passes)
        if name == "fused_nt32767_tiny":   # culled: a small part of the pairs
            assert 0 < swept < passes * ns * nt // 4, (swept, passes)


def test_far_point_to_plane_correspondences(ctx, oracle):
    """Point-to-plane 1e5 from the origin: the 6 x 6 system in absolute coordinates is ill-conditioned, so the pose is
    not compared; the correspondences, per-pass fitness and iteration counts of the first passes are."""
    from pedp_hip import _lib

    src, tgt, nrm = cases.far(3000, 5000, 71)
    T = _init(tgt)
    S, Tg = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    for mi in (0, 1):
        res = _lib.icp(ctx, S, Tg, 0.1, T, estimator=P2PL, max_iteration=mi, relative_fitness=-1, relative_rmse=-1,
                       want_corr=True, want_trace=True)
        ref = oracle.icp(src, tgt, nrm, 0.1, T, estimator=P2PL, max_iter=mi, rel_fitness=-1, rel_rmse=-1)
        assert res["iters"] == ref["iters"] == mi
        assert np.array_equal(res["corr"], ref["corr"]) and np.array_equal(res["trace"][:, 0], ref["trace"][:, 0])


def test_nonfinite_target_rows_are_never_neighbours(ctx, oracle):
    """A target with NaN / inf rows, made from host and from device memory: those rows are left out of the search
    (never a neighbour), the other rows are searched as usual; a target with no finite row gives no neighbour."""
    import torch
    from pedp_hip import _lib

    src, tgt, nrm = cases.nonfinite_target(1500, 3000, 81)
    T = _init(tgt)
    d_t = torch.from_numpy(tgt).to("cuda:0")
    d_n = torch.from_numpy(nrm).to("cuda:0")
    torch.cuda.synchronize()
    S = _lib.Cloud(ctx, src)
    for Tg in (_lib.Cloud(ctx, tgt, nrm), _lib.Cloud.from_device(ctx, d_t.data_ptr(), len(tgt), d_n.data_ptr())):
        _check_nn(ctx, oracle, S, Tg, src, tgt, T)
        for r in (0.1, _radius(("above", 0), tgt)):
            _check_icp(ctx, oracle, S, Tg, src, tgt, nrm, r, T, P2PL, iters=(0, 3), kdtree=False)
    bad = np.full((100, 3), np.nan)
    bad[::2, 1] = np.inf
    Tg = _lib.Cloud(ctx, bad, np.tile([0.0, 0.0, 1.0], (100, 1)))
    idx, d2 = _lib.nn(ctx, S, Tg, T)
    assert (idx == -1).all() and np.isinf(d2).all()
    res = _lib.icp(ctx, S, Tg, 0.1, T, max_iteration=2, relative_fitness=-1, relative_rmse=-1, want_corr=True)
    assert (res["corr"] == -1).all() and res["fitness"] == 0.0


@pytest.mark.parametrize("path", ["fused", "dense"])
def test_exact_ties_and_radius_boundary(ctx, oracle, path):
    """Exact 8-, 4- and 2-way ties inside the radius (lattice; the exact fallback must decide and it runs), and a
    neighbour at exactly d^2 == r^2: excluded at r, included at nextafter(r, inf)."""
    from pedp_hip import _lib

    src, tgt, nrm = cases.lattice(3000, 4096 if path == "fused" else 512, 7)
    r = 1.8 if path == "fused" else 7.0     # every tie (d^2 = 1, 2, 3) inside; 7 > diag / 4 = 6.06 on the 8^3 lattice
    assert _path(tgt, r) == path
    S, Tg = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    _check_nn(ctx, oracle, S, Tg, src, tgt, np.eye(4))
    stats = _check_icp(ctx, oracle, S, Tg, src, tgt, nrm, r, np.eye(4), P2PT)
    assert stats[0][2] > 0, stats    # the initial pass re-searched the tied points exactly

    if path == "fused":   # (the dense path's d^2 == r^2 case: test_radius_boundary_dense)
        src, tgt, nrm = cases.boundary(2000, 1000, 8)
        S, Tg = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
        _check_nn(ctx, oracle, S, Tg, src, tgt, np.eye(4))
        for r, inside in ((5.0, False), (float(np.nextafter(5.0, np.inf)), True)):
            assert _path(tgt, r) == path
            res = _lib.icp(ctx, S, Tg, r, np.eye(4), estimator=P2PT, max_iteration=0, relative_fitness=-1,
                           relative_rmse=-1, want_corr=True)
            assert (res["corr"] >= 0).all() if inside else (res["corr"] < 0).all()
            _check_icp(ctx, oracle, S, Tg, src, tgt, nrm, r, np.eye(4), P2PT)


def test_radius_boundary_dense(ctx, oracle):
    """d^2 == r^2 exactly on the dense path: two targets 10 apart, queries at (3, 4, 0) from one of them
    (d = 5, the other at >= 5.83), r = 5 is above diag / 4 = 2.5."""
    from pedp_hip import _lib

    tgt = np.array([[0.0, 0, 0], [10.0, 0, 0]])
    nrm = np.tile([0.0, 0.0, 1.0], (2, 1))
    src = np.vstack([np.tile([3.0, 4.0, 0.0], (300, 1)), np.tile([7.0, 0.0, 4.0], (213, 1)), [[1.0, 0.0, 0.0]]])
    S, Tg = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    _check_nn(ctx, oracle, S, Tg, src, tgt, np.eye(4))
    for r, n_in in ((5.0, 1), (float(np.nextafter(5.0, np.inf)), len(src))):
        assert _path(tgt, r) == "dense"
        res = _lib.icp(ctx, S, Tg, r, np.eye(4), estimator=P2PT, max_iteration=0, relative_fitness=-1,
                       relative_rmse=-1, want_corr=True)
        assert (res["corr"] >= 0).sum() == n_in     # only (1, 0, 0) is strictly inside at r = 5 (d^2 = 25 excluded)
        # (two target points: only the correspondence pass is defined, the update's rotation is free)
        _check_icp(ctx, oracle, S, Tg, src, tgt, nrm, r, np.eye(4), P2PT, iters=(0,))


def test_parity_frame_large_first_update(ctx, oracle):
    """The bench's synthetic frame started 20 degrees and 0.3 x extent off: the first updates are large, which is
    what the temporal-coherence search radius of the fused pass has to absorb."""
    from pedp_hip import _lib, synth

    f = synth.Frame("parity")
    depth = oracle.raycast(f.verts_posed, f.tris, f.rays6, bvh=True)["t_hit"]
    scene = f.scene(depth)
    ext = cases.extent(f.model_points)
    D = np.eye(4)
    D[:3, :3] = synth.axis_angle([1.0, 1.0, 0.0], np.deg2rad(20.0))
    D[:3, 3] = 0.3 * ext * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    T = D @ f.icp_init()
    for r in (10.0, 0.25 * ext):
        path = _path(f.model_points, r)
        assert path == ("fused" if r == 10.0 else "dense")
        S, Tg = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
        _check_icp(ctx, oracle, S, Tg, scene, f.model_points, f.normals, r, T, P2PL, iters=(0, 1, 3, 30))


def test_segmented_path_at_the_mask_word_capacity(ctx, oracle):
    """Nt = 524288 is the last fused target, 524289 the first segmented one (same radius, same source)."""
    from pedp_hip import _lib

    src, tgt, nrm = cases.blob(513, BK_WCAP_ROWS + 1, 21)
    r = 0.05
    T = _init(tgt)
    for nt, path in ((BK_WCAP_ROWS, "fused"), (BK_WCAP_ROWS + 1, "segmented")):
        assert _path(tgt[:nt], r) == path
        Tg = _lib.Cloud(ctx, tgt[:nt], nrm[:nt])
        for ns in (1, 127, 128, 129, 511, 512, 513):
            S = _lib.Cloud(ctx, src[:ns])
            its = (0, 1, 3) if ns in (129, 513) else (3,)
            stats = _check_icp(ctx, oracle, S, Tg, src[:ns], tgt[:nt], nrm[:nt], r, T, P2PL, iters=its)
            if ns == 513:
                assert 0 < stats[-1][1] < stats[-1][0] * ns * nt, stats   # culled: fewer than every pair


def test_exhaustive_configuration(oracle):
    """pedp_icp_configure(exhaustive): every pair through the dense sweep whatever the radius.  A context of its
    own (the session's stays in the default mode)."""
    from pedp_hip import _lib

    c = _lib.Context(0)
    try:
        _lib.icp_configure(c, exhaustive=True)
        for geo, ns, nt, r, est in (("blob", 513, 1025, 0.1, P2PL), ("nonfinite_source", 600, 700, 0.1, P2PT),
                                    ("lattice", 1000, 512, 1.8, P2PT), ("boundary", 700, 1000, 5.0, P2PT),
                                    ("boundary", 700, 1000, float(np.nextafter(5.0, np.inf)), P2PT)):
            src, tgt, nrm = cases.GEOMETRIES[geo](ns, nt, 31)
            assert _path(tgt, r, exhaustive=True) == "dense"
            S, Tg = _lib.Cloud(c, src), _lib.Cloud(c, tgt, nrm)
            T = np.eye(4) if geo in ("lattice", "boundary") else _init(tgt)
            stats = _check_icp(c, oracle, S, Tg, src, tgt, nrm, r, T, est)
            for passes, swept, fb in stats:
                assert geo == "nonfinite_source" or swept >= passes * ns * len(tgt), (geo, swept, passes)
            if geo == "lattice":
                assert stats[0][2] > 0
        _lib.icp_configure(c)
    finally:
        c.close()


def test_batched_mixed_radii_equal_single_calls(ctx, oracle):
    """pedp_icp_batched_ex with per-pose radii: all culled (one fused launch for the group), culled and dense mixed
    (one by one), one dense radius (graphs replayed on sub-contexts): each pose the same bits as its own pedp_icp,
    and within tolerance of the oracle."""
    from pedp_hip import _lib

    src, tgt, nrm = cases.blob(3000, 20000, 41)
    S, Tg = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    inits = np.stack([_init(tgt, deg=d, shift=s) for d, s in ((1, 0), (3, 0.05), (-2, 0.1), (5, 0.0), (0.5, 0.2))])
    q = _radius(("above", 0), tgt)
    for radii in ([0.05, 0.1, 0.2, 0.07, 0.3], [0.05, q, 0.2, 2 * q, 0.1], [q] * 5):
        Tb, fit, rmse, its = _lib.icp_batched_ex(ctx, S, Tg, radii, inits, estimator=P2PL, max_iteration=6,
                                                 relative_fitness=-1, relative_rmse=-1)
        for b, r in enumerate(radii):
            one = _lib.icp(ctx, S, Tg, r, inits[b], estimator=P2PL, max_iteration=6, relative_fitness=-1,
                           relative_rmse=-1)
            assert np.array_equal(Tb[b], one["T"]) and fit[b] == one["fitness"] and rmse[b] == one["inlier_rmse"]
            assert its[b] == one["iters"] == 6
            ref = oracle.icp(src, tgt, nrm, r, inits[b], estimator=P2PL, max_iter=6, rel_fitness=-1, rel_rmse=-1)
            assert np.abs(Tb[b] - ref["T"]).max() < POSE_TOL and fit[b] == ref["fitness"]
            assert abs(rmse[b] - ref["inlier_rmse"]) < 1e-9


def test_begin_end_on_the_matrix(ctx, oracle):
    """pedp_icp_begin / pedp_icp_end on a fused and a dense case: the blocking call's bits."""
    from pedp_hip import _lib

    src, tgt, nrm = cases.nonfinite_source(1500, 3000, 51)
    S, Tg = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    T = _init(tgt)
    for r in (0.1, _radius(("above", 0), tgt)):
        one = _lib.icp(ctx, S, Tg, r, T, max_iteration=FULL, relative_fitness=-1, relative_rmse=-1, want_corr=True,
                       want_trace=True)
        _lib.icp_begin(ctx, S, Tg, r, T, max_iteration=FULL, relative_fitness=-1, relative_rmse=-1, want_trace=True)
        two = _lib.icp_end(ctx, want_corr=True)
        for k in ("T", "corr", "trace"):
            assert np.array_equal(one[k], two[k]), k
        assert one["fitness"] == two["fitness"] and one["inlier_rmse"] == two["inlier_rmse"] and one["iters"] == two["iters"]
        ref = oracle.icp(src, tgt, nrm, r, T, max_iter=FULL, rel_fitness=-1, rel_rmse=-1)
        _same(two, ref, FULL)


_PLAN_PROBE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from pedp_hip import _lib
d = np.load(sys.argv[2])
ctx = _lib.Context(0)
src, tgt = _lib.Cloud(ctx, d["src"]), _lib.Cloud(ctx, d["tgt"], d["nrm"])
r = _lib.icp(ctx, src, tgt, float(d["r"]), d["T"], max_iteration=int(d["mi"]), relative_fitness=-1, relative_rmse=-1,
             want_corr=True, want_trace=True)
np.savez(sys.argv[3], T=r["T"], corr=r["corr"], trace=r["trace"], fitness=r["fitness"], rmse=r["inlier_rmse"],
         iters=r["iters"], planned=np.int64(_lib.icp_last_planned_passes(ctx)))
"""


def test_visit_plan_60k_source(tmp_path, oracle):
    """About 60k source points all near the target: 469 live 128-point chunks, between n_cu and 2 n_cu on a 256-CU
    part, so the visit plan is in force.  With and without it (PEDP_ICP_NO_VISIT_PLAN=1, a child process each):
    the same bits, and the oracle's correspondences."""
    src, tgt, nrm = cases.blob(60000, 30000, 61)
    r, mi = 0.1, 12
    assert _path(tgt, r) == "fused"
    T = _init(tgt)
    inp = str(tmp_path / "in.npz")
    np.savez(inp, src=src, tgt=tgt, nrm=nrm, r=r, T=T, mi=mi)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for flag in ("0", "1"):
        out = str(tmp_path / f"plan{flag}.npz")
        env = dict(os.environ, PEDP_ICP_NO_VISIT_PLAN=flag)
        p = subprocess.run([sys.executable, "-c", _PLAN_PROBE, root, inp, out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        outs.append(np.load(out))
    for k in outs[0].files:
        if k != "planned":
            assert np.array_equal(outs[0][k], outs[1][k]), k
    assert int(outs[1]["planned"]) == 0
    import torch
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert int(outs[0]["planned"]) > 0, int(outs[0]["planned"])
    ref = oracle.icp(src, tgt, nrm, r, T, max_iter=mi, rel_fitness=-1, rel_rmse=-1)
    _same({k: outs[0][k] for k in ("T", "corr", "trace")} | {"fitness": float(outs[0]["fitness"]),
          "inlier_rmse": float(outs[0]["rmse"]), "iters": int(outs[0]["iters"])}, ref, mi)
