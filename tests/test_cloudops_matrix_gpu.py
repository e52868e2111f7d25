"""Case matrix of the point-cloud operations (pedp_cloudops.hip) against the float64 oracle: the geometries of
_cloud_cases at N = 700 and N = 5000, sizes at every boundary between two kernels or two host rules, seeded fuzz,
the fused preprocess_source chain against the oracle's chain, and the refusal of non-finite coordinates.

Tolerances are the suite's: voxel means (with and without normals), DBSCAN labels, kNN means, the outlier filter's
indices, plane inlier lists and feature matches bit-equal; planes within 1e-12 (the offset relative to the largest
coordinate); normals within 1e-9; FPFH entries within 1e-9 (1 + |ref|) with at most 1 % of the rows differing (two
libms' acos / atan2 at a bin edge).

Branches, and the rule each case recomputes where the host decides (pedp_cloudops.hip):
  BND_DEVICE_MIN = 32768   the box from the device copy (bounds_kernel) instead of the host pass: normals, FPFH
                           (whose points are then "already uploaded"); the voxel grid and the fused chain always;
  KNN_SMALL_MAX = 4096     a wave per query over all points below, the grid kernels above;
  N >= 131072              the voxel sort's radix passes instead of the merge sort;
  RS_PLANES = 64           plane iterations per count slab (blockIdx.y); ransac_best_kernel folds 256 per stride;
  FM_CHUNK = 1024          target features per partial minimum, folded in chunk order;
  1024 block sums          refit_fold_kernel stages 4 block sums per thread and pass: N > 262144 walks the loop twice;
  clique / non-clique      DBSCAN cells below eps / sqrt(3) while the box has at most 2^24 of them (_dbscan_grid), else
                           cells of eps, doubled until they fit."""
import numpy as np
import pytest

import _cloud_cases as cases
import _cloudops_ref as ref

pytestmark = pytest.mark.gpu

BND_DEVICE_MIN = 32768
KNN_SMALL_MAX = 4096
RADIX_MIN = 131072
RS_PLANES = 64
FM_CHUNK = 1024
CELL_BUDGET = 16777216.0


def _make_grid(lo, hi, cell):
    """make_grid: cells of `cell` over the box, doubled until there are at most 2^24."""
    while True:
        dims = [min(max(np.floor((hi[k] - lo[k]) / cell) + 1.0, 1.0), 1e9) for k in range(3)]
        if dims[0] * dims[1] * dims[2] <= CELL_BUDGET:
            return cell
        cell *= 2.0


def _dbscan_grid(lo, hi, eps):
    """dbscan_core's choice: ("clique", cell) or ("cells_of_eps", cell); doubled = cell > eps (1 + 1e-9)."""
    cell = _make_grid(lo, hi, eps * 0.57735026918962576 * (1.0 - 1e-9))
    if cell * 1.7320508075688772 < eps:
        return "clique", cell
    return "cells_of_eps", _make_grid(lo, hi, eps * (1.0 + 1e-9))


def _fpfh_same(got, want, why=None):
    """At most 1 % of the rows differ.  `why` = (pts, normals, radius, max_nn): a failure also reports how many pairs of the
    cloud have their ordering test acos(|a1|) > acos(|a2|) within 4 ulp of a tie (ref.fpfh_order_ties)."""
    bad = (np.abs(got - want) > 1e-9 * (1.0 + np.abs(want))).any(axis=1)
    assert got.shape == want.shape
    if bad.mean() > 0.01:
        ties = ref.fpfh_order_ties(*why) if why is not None else None
        pytest.fail(f"FPFH: {bad.sum()} of {len(bad)} rows differ, max |d| {np.abs(got - want).max():.3g}; (pairs, pairs whose "
                    f"ordering test is within 4 ulp of a tie, rows reading such a pair, differing rows reading none) = {ties and ties(bad)}")


def _plane_same(got, want, pts):
    (gp, gi), (wp, wi) = got, want
    assert np.array_equal(gi, wi), (len(gi), len(wi))
    assert np.abs(gp[:3] - wp[:3]).max() <= 1e-12 and abs(gp[3] - wp[3]) <= 1e-12 * max(1.0, np.abs(pts).max()), (gp, wp)


def _check_fpfh(ctx, oracle, pts, prm):
    from pedp_hip import cloud_ops

    nrm = oracle.estimate_normals(pts, prm["normal_radius"], prm["normal_max_nn"])
    feat = oracle.fpfh(pts, nrm, prm["fpfh_radius"], prm["fpfh_max_nn"])
    _fpfh_same(cloud_ops.compute_fpfh(pts, nrm, prm["fpfh_radius"], prm["fpfh_max_nn"], ctx=ctx), feat,
               (pts, nrm, prm["fpfh_radius"], prm["fpfh_max_nn"]))


def _check_all(ctx, oracle, pts, prm, sor_ratio=1.0, fpfh=True):
    """Every operation on one cloud with one set of parameters, the device against the oracle (fpfh=False: FPFH has a
    test of its own for this cloud)."""
    from pedp_hip import cloud_ops

    nrm = oracle.estimate_normals(pts, prm["normal_radius"], prm["normal_max_nn"])
    # voxel grid, with and without normals
    got, gotn = cloud_ops.voxel_down_sample(pts, prm["voxel"], nrm, ctx=ctx)
    want, wantn = oracle.voxel_down_sample(pts, prm["voxel"], nrm)
    assert np.array_equal(got, want) and np.array_equal(gotn, wantn)
    assert np.array_equal(cloud_ops.voxel_down_sample(pts, prm["voxel"], ctx=ctx)[0], want)
    # DBSCAN
    labels = oracle.cluster_dbscan(pts, prm["eps"], prm["min_points"])
    assert np.array_equal(cloud_ops.cluster_dbscan(pts, prm["eps"], prm["min_points"], ctx=ctx), labels)
    # kNN mean distance and the outlier filter on it
    avg = oracle.knn_mean_distance(pts, prm["k"])
    assert np.array_equal(cloud_ops.knn_mean_distance(pts, prm["k"], ctx=ctx), avg)
    assert np.array_equal(cloud_ops.remove_statistical_outlier(pts, prm["k"], sor_ratio, ctx=ctx),
                          oracle.statistical_outlier_indices(avg, sor_ratio))
    # normals
    gn = cloud_ops.estimate_normals(pts, prm["normal_radius"], prm["normal_max_nn"], ctx=ctx)
    assert gn.shape == nrm.shape and (len(pts) == 0 or np.abs(gn - nrm).max() <= 1e-9), np.abs(gn - nrm).max()
    # FPFH over the oracle's normals, and the matches of one half's features in the whole cloud's
    feat = oracle.fpfh(pts, nrm, prm["fpfh_radius"], prm["fpfh_max_nn"])
    if fpfh:
        _fpfh_same(cloud_ops.compute_fpfh(pts, nrm, prm["fpfh_radius"], prm["fpfh_max_nn"], ctx=ctx), feat,
                   (pts, nrm, prm["fpfh_radius"], prm["fpfh_max_nn"]))
    fs = feat[::2] * 0.999
    assert np.array_equal(cloud_ops.match_features(fs, feat, ctx=ctx), oracle.feature_match(fs, feat))
    # plane
    _plane_same(cloud_ops.segment_plane(pts, prm["plane_threshold"], 3, prm["plane_iterations"], seed=prm["plane_seed"], ctx=ctx),
                oracle.segment_plane(pts, prm["plane_threshold"], prm["plane_iterations"], seed=prm["plane_seed"]), pts)
    return nrm, labels, avg


# ------------------------------------------------------------------ a. geometry sweep
@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_geometry_sweep(ctx, oracle, name, n):
    """N = 5000 is above KNN_SMALL_MAX: kNN takes the grid kernels there and the all-points kernel at 700.
    `collinear` and `one_point`: no neighbourhood has a plane, both sides give the default normal (0, 0, 1) for every
    point (the covariance's closed form returns the zero vector on both) -- compared like every other geometry."""
    pts = cases.cloud(name, n)
    assert (len(pts) > KNN_SMALL_MAX) == (n == 5000)
    prm = cases.params(pts)
    nrm, labels, avg = _check_all(ctx, oracle, pts, prm, fpfh=False)
    assert labels.max() >= 0 and np.isfinite(avg).all() and np.isfinite(nrm).all()
    if name in ("collinear", "one_point"):
        assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (len(pts), 1)))


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_geometry_sweep_fpfh(ctx, oracle, name, n):
    """FPFH (radius 5 h, max_nn 50, over the oracle's normals) of the same clouds.

    Feature.cpp orders a pair by `acos(|a1|) > acos(|a2|)`.  On `boundary` at N = 5000, 11,235 of the 240,737 pairs have two
    DIFFERENT arguments whose angles are within 4 ulp of each other (on `clusters` 4: two points with one neighbourhood,
    hence one normal), and the pair's frame flips with the answer: an acos of 1-2 ulp moved 113 of 4913 rows here.  The
    library decides such pairs with a correctly rounded acos (csrc/features/acos_cr.h), which orders every one of them as
    the host's libm does."""
    pts = cases.cloud(name, n)
    _check_fpfh(ctx, oracle, pts, cases.params(pts))


# ------------------------------------------------------------------ b. size boundaries
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257])
def test_every_operation_at_wave_and_block_tails(ctx, oracle, n):
    """N around the wave (64) and the 256-thread block: a wave per point (DBSCAN, kNN, hybrid lists), a thread per
    point (keys, cells, normals), and the first points at which an operation has something to say at all."""
    pts = cases.blob(n, 11)
    _check_all(ctx, oracle, pts, cases.params(pts))
    sh = cases.sheet(n, 12, span=2.0 * np.sqrt(n))
    _check_all(ctx, oracle, sh, cases.params(sh))


@pytest.mark.parametrize("n", [RADIX_MIN - 1, RADIX_MIN])
def test_voxel_sort_switch(ctx, oracle, n):
    """voxel_core: `passes = N >= 131072` -- the merge sort below, the radix passes from there on; host array and
    device array.  Row 65280 (bounds_kernel's last workgroup, its first thread) holds the box's minimum on every axis, so
    the voxel origin rests on that workgroup's partial."""
    torch = pytest.importorskip("torch")
    from pedp_hip import cloud_ops

    assert (n >= RADIX_MIN) == (n == 131072)
    pts = cases.sheet(n, 5, span=300.0)
    pts[255 * 256] = pts.min(axis=0) - 0.77
    want, _ = oracle.voxel_down_sample(pts, 1.0)
    assert 1000 < len(want) < n
    assert np.array_equal(cloud_ops.voxel_down_sample(pts, 1.0, ctx=ctx)[0], want)
    assert np.array_equal(cloud_ops.voxel_down_sample(torch.from_numpy(pts).cuda(), 1.0, ctx=ctx)[0], want)


@pytest.fixture(scope="module")
def sheets(oracle):
    """The wavy sheet at both sides of BND_DEVICE_MIN with the oracle's normals and features (computed once)."""
    out = {}
    for n in (BND_DEVICE_MIN - 1, BND_DEVICE_MIN):
        pts = cases.sheet(n, 21, span=100.0)
        pts[255 * 256 % n] = pts.max(axis=0) + 0.4     # (an extreme row in the last workgroup's share of bounds_kernel)
        nrm = oracle.estimate_normals(pts, 3.0, 30)
        out[n] = (pts, nrm, oracle.fpfh(pts, nrm, 4.0, 50))
    return out


@pytest.mark.parametrize("n", [BND_DEVICE_MIN - 1, BND_DEVICE_MIN])
def test_normals_and_fpfh_at_the_device_box_switch(ctx, sheets, n):
    """N < BND_DEVICE_MIN: the host's box; from 32768 on estimate_normals takes bounds_device and FPFH's bounds_of uploads
    first and reads the points where they are (d_pts = d_in)."""
    from pedp_hip import cloud_ops

    assert (n >= BND_DEVICE_MIN) == (n == 32768)
    pts, nrm, feat = sheets[n]
    assert np.abs(cloud_ops.estimate_normals(pts, 3.0, 30, ctx=ctx) - nrm).max() <= 1e-9
    _fpfh_same(cloud_ops.compute_fpfh(pts, nrm, 4.0, 50, ctx=ctx), feat)


@pytest.mark.parametrize("max_nn", [1, 2, 3, 128])
def test_normals_and_fpfh_neighbour_caps(ctx, oracle, max_nn):
    """max_nn below three (no covariance: the default normal), exactly three, and the cap of 128."""
    from pedp_hip import cloud_ops

    pts = cases.sheet(3000, 22, span=30.0)              # ~ 150 points within radius 4: the cap always cuts
    nrm = oracle.estimate_normals(pts, 4.0, max_nn)
    assert np.abs(cloud_ops.estimate_normals(pts, 4.0, max_nn, ctx=ctx) - nrm).max() <= 1e-9
    if max_nn < 3:
        assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (len(pts), 1)))
    good = oracle.estimate_normals(pts, 4.0, 30)
    _fpfh_same(cloud_ops.compute_fpfh(pts, good, 4.0, max_nn, ctx=ctx), oracle.fpfh(pts, good, 4.0, max_nn))


def test_normals_prior_zero_and_orthogonal(ctx, oracle):
    """A prior of zeros and a prior orthogonal to the estimate: n . prior == 0 is not < 0, nothing is flipped.  The
    orthogonal case is the exactly planar cloud, whose estimate has x = y = 0 exactly, against a prior of (1, 0, 0)."""
    from pedp_hip import cloud_ops

    pts = cases.sheet(3000, 23, span=40.0)
    zero = np.zeros_like(pts)
    want = oracle.estimate_normals(pts, 3.0, 30, zero)
    assert np.abs(cloud_ops.estimate_normals(pts, 3.0, 30, zero, ctx=ctx) - want).max() <= 1e-9
    assert np.abs(want - oracle.estimate_normals(pts, 3.0, 30)).max() == 0.0
    flat = cases.cloud("planar", 700)
    prm = cases.params(flat)
    side = np.tile([1.0, 0.0, 0.0], (len(flat), 1))
    want = oracle.estimate_normals(flat, prm["normal_radius"], 30, side)
    assert not want[:, :2].any() and np.abs(np.abs(want[:, 2]) - 1.0).max() < 1e-15     # n . prior is exactly +-0
    got = cloud_ops.estimate_normals(flat, prm["normal_radius"], 30, side, ctx=ctx)
    assert np.abs(got - want).max() <= 1e-9
    assert np.array_equal(want, oracle.estimate_normals(flat, prm["normal_radius"], 30))


def test_knn_neighbour_counts_and_one_cell(ctx, oracle):
    """k at and beyond the number of points (all of them are "the k nearest"), the largest k; and 5,000 identical points
    above KNN_SMALL_MAX: one grid cell holds everything, every mean is 0 and the outlier filter (0 < avg) keeps nothing."""
    from pedp_hip import cloud_ops

    pts = cases.blob(257, 31)
    for k in (1, 256, 257, 258, 300):
        assert np.array_equal(cloud_ops.knn_mean_distance(pts, k, ctx=ctx), oracle.knn_mean_distance(pts, k)), k
    big = cases.blob(5000, 32)
    assert len(big) > KNN_SMALL_MAX
    for k in (1, 300):
        assert np.array_equal(cloud_ops.knn_mean_distance(big, k, ctx=ctx), oracle.knn_mean_distance(big, k)), k
    same = cases.cloud("one_point", 5000)
    avg = cloud_ops.knn_mean_distance(same, 8, ctx=ctx)
    assert np.array_equal(avg, oracle.knn_mean_distance(same, 8)) and not avg.any()
    assert len(cloud_ops.remove_statistical_outlier(same, 8, 1.0, ctx=ctx)) == 0 == len(oracle.remove_statistical_outlier(same, 8, 1.0))


def test_dbscan_crowded_clique_cell_and_min_points(ctx, oracle):
    """200 points inside ONE clique cell (more than the 64 core points a wave lists at once) next to 300 scattered ones;
    min_points = 1 (every point is a core point) and min_points > N (none is)."""
    from pedp_hip import cloud_ops

    rng = np.random.default_rng(43)
    eps = 1.0
    scattered = rng.uniform(0.0, 6.0, (300, 3))
    pts = np.vstack([scattered, [3.0, 3.0, 3.0] + rng.uniform(0.0, 0.2, (200, 3))])
    pts = pts[rng.permutation(len(pts))]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    kind, cell = _dbscan_grid(lo, hi, eps)
    assert kind == "clique" and cell < eps / np.sqrt(3.0)
    clump = (pts >= 3.0).all(axis=1) & (pts <= 3.2).all(axis=1)
    assert clump.sum() >= 200 and len(np.unique(np.floor((pts[clump] - lo) / cell), axis=0)) == 1    # one cell holds them
    want = oracle.cluster_dbscan(pts, eps, 5)
    assert len(np.unique(want)) == 3                                # noise, the clump's cluster and one more
    assert np.array_equal(cloud_ops.cluster_dbscan(pts, eps, 5, ctx=ctx), want)
    for mp in (1, len(pts) + 1):
        want = oracle.cluster_dbscan(pts, eps, mp)
        assert np.array_equal(cloud_ops.cluster_dbscan(pts, eps, mp, ctx=ctx), want)
        assert (want.min() >= 0) if mp == 1 else (want.max() == -1)


def test_dbscan_strict_radius_on_the_lattice(ctx, oracle):
    """Lattice of spacing 2 at eps = 2.0 exactly: d^2 == eps^2 is NOT a neighbour (pedp.h: d^2 < eps^2), so every point
    has itself alone; one ulp more and the lattice is one cluster."""
    from pedp_hip import cloud_ops

    pts = cases.cloud("lattice", 512)
    assert len(pts) == 512
    for eps, mp, check in ((2.0, 2, lambda l: np.all(l == -1)), (2.0, 1, lambda l: np.array_equal(l, np.arange(512))),
                           (np.nextafter(2.0, 3.0), 2, lambda l: np.all(l == 0))):
        want = oracle.cluster_dbscan(pts, eps, mp)
        assert check(want), (eps, mp)
        assert np.array_equal(cloud_ops.cluster_dbscan(pts, eps, mp, ctx=ctx), want), (eps, mp)


@pytest.mark.parametrize("axes", [2, 3])
def test_dbscan_cells_of_eps_doubled(ctx, oracle, axes):
    """Two 120-point blobs 5e6 apart along two and along three axes: the box has no room for clique cells nor for cells
    of eps -- the non-clique kernels over doubled cells."""
    from pedp_hip import cloud_ops

    a = cases.blob(120, 43)
    pts = np.vstack([a, a + np.where(np.arange(3) < axes, 5e6, 0.0)])
    kind, cell = _dbscan_grid(pts.min(axis=0), pts.max(axis=0), 3.0)
    assert kind == "cells_of_eps" and cell > 3.0 * (1.0 + 1e-9)
    want = oracle.cluster_dbscan(pts, 3.0, 8)
    assert np.array_equal(np.unique(want[want >= 0], return_counts=True)[1], [120, 120]) or want.max() == 1
    assert np.array_equal(cloud_ops.cluster_dbscan(pts, 3.0, 8, ctx=ctx), want)


@pytest.mark.parametrize("iterations", [1, 63, 64, 65, 255, 256, 257])
def test_plane_iteration_slabs(ctx, oracle, iterations):
    """ransac_count_kernel runs RS_PLANES = 64 planes per slab (63 / 64 / 65: the last slab's tail), ransac_best_kernel
    folds the counts 256 per stride (255 / 256 / 257)."""
    from pedp_hip import cloud_ops

    rng = np.random.default_rng(51)
    pts = np.vstack([np.column_stack([rng.uniform(0, 50, (600, 2)), rng.normal(0, 0.3, 600)]), rng.uniform(0, 50, (300, 3))])
    for seed in (0, 1):
        _plane_same(cloud_ops.segment_plane(pts, 0.5, 3, iterations, seed=seed, ctx=ctx),
                    oracle.segment_plane(pts, 0.5, iterations, seed=seed), pts)


def test_plane_at_the_largest_iteration_count(ctx, oracle):
    """ransac_count_kernel takes RS_PLANES iterations per block in y and a launch holds 65535 of them
    (hipDeviceProp_t::maxGridSize[1] = 65536): 64 x 65535 iterations are accepted and run in one launch, one more is
    refused.  Four points have four samples: once the first 256 iterations have drawn them all, no later iteration can
    beat the best of those (ties go to the earliest), so the oracle's answer for 256 iterations is its answer for all of them
    (its loop opens a parallel region per iteration: 4 million of them take 17 s)."""
    from pedp_hip import _lib, cloud_ops

    most = RS_PLANES * 65535
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.0, 1.0, -0.1], [1.0, 1.0, 2.0]])
    assert len({frozenset(oracle.sample3(3, t, 4)) for t in range(256)}) == 4
    want = oracle.segment_plane(pts, 0.3, 256, seed=3)
    assert len(want[1]) == 3
    _plane_same(cloud_ops.segment_plane(pts, 0.3, 3, most, seed=3, ctx=ctx), want, pts)
    with pytest.raises(_lib.PedpError, match="num_iterations out of range"):
        cloud_ops.segment_plane(pts, 0.3, 3, most + 1, seed=3, ctx=ctx)


def test_plane_degenerate_inputs(ctx, oracle):
    """N = 3 (the one possible sample), threshold 0 (no distance is < 0: no inliers, the zero plane) and identical points (no
    valid sample)."""
    from pedp_hip import cloud_ops

    tri = np.array([[0.0, 0.0, 1.0], [2.0, 0.0, 1.5], [0.0, 3.0, 0.5]])
    got, want = cloud_ops.segment_plane(tri, 0.1, 3, 5, ctx=ctx), oracle.segment_plane(tri, 0.1, 5)
    _plane_same(got, want, tri)
    assert np.array_equal(want[1], [0, 1, 2])
    pts = cases.blob(300, 52)
    got, want = cloud_ops.segment_plane(pts, 0.0, 3, 20, ctx=ctx), oracle.segment_plane(pts, 0.0, 20)
    assert not want[0].any() and len(want[1]) == 0 and np.array_equal(got[0], want[0]) and len(got[1]) == 0
    same = cases.cloud("one_point", 300)
    got, want = cloud_ops.segment_plane(same, 1.0, 3, 20, ctx=ctx), oracle.segment_plane(same, 1.0, 20)
    assert not want[0].any() and len(want[1]) == 0 and np.array_equal(got[0], want[0]) and len(got[1]) == 0


def test_plane_ties_go_to_the_earliest_iteration(ctx, oracle):
    """`two_sheets`: every one-sheet sample has exactly 300 inliers, so the tie rule alone picks the sheet -- and the seeds
    0..7 do not all pick the same one."""
    from pedp_hip import cloud_ops

    pts = cases.cloud("two_sheets", 600)
    sheets_seen = set()
    for seed in range(8):
        want = oracle.segment_plane(pts, 0.5, 60, seed=seed)
        assert len(want[1]) == 300
        sheets_seen.add(float(pts[want[1][0], 2]))
        _plane_same(cloud_ops.segment_plane(pts, 0.5, 3, 60, seed=seed, ctx=ctx), want, pts)
        last = [t for t in range(60) if len(set(pts[oracle.sample3(seed, t, 600), 2])) == 1]
        if pts[oracle.sample3(seed, last[0], 600)[0], 2] != pts[oracle.sample3(seed, last[-1], 600)[0], 2]:
            sheets_seen.add("first and last tied iteration disagree")
    assert {0.0, 10.0} <= sheets_seen and "first and last tied iteration disagree" in sheets_seen


@pytest.mark.parametrize("nt", [1023, 1024, 1025, 2049])
@pytest.mark.parametrize("ns", [63, 64, 65])
def test_feature_match_chunks(ctx, oracle, ns, nt):
    """FM_CHUNK = 1024 targets per partial minimum (1023 / 1024 / 1025: one chunk, one full chunk, a chunk of one; 2049:
    three), 64 sources per workgroup.  An exact tie between a row of chunk 0 and a row of chunk 1: the lowest index."""
    from pedp_hip import cloud_ops

    rng = np.random.default_rng(61)
    ft = rng.uniform(0.0, 100.0, (nt, 33))
    fs = ft[rng.integers(0, nt, ns)] + rng.normal(0.0, 1e-3, (ns, 33))
    if nt > FM_CHUNK:
        ft[nt - 1] = ft[10]
        fs[5] = ft[10]
    want = oracle.feature_match(fs, ft)
    assert nt <= FM_CHUNK or want[5] == 10
    assert np.array_equal(cloud_ops.match_features(fs, ft, ctx=ctx), want)
    assert np.array_equal(want, ref.feature_match(fs, ft))


# ------------------------------------------------------------------ c. seeded fuzz
FUZZ_SEEDS = range(16)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_seeded_fuzz(ctx, oracle, seed):
    """N in [1, 600], the geometry and every parameter drawn from the seed (_cloud_cases.fuzz); FPFH below."""
    name, pts, prm = cases.fuzz(seed)
    _check_all(ctx, oracle, pts, prm, sor_ratio=0.5, fpfh=False)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_seeded_fuzz_fpfh(ctx, oracle, seed):
    """FPFH of the fuzz clouds.  Seed 1 is `small` with N = 74, radii larger than the cloud and max_nn > N: every point
    has every point as its neighbourhood -- one covariance, 74 normals equal to rounding, 1,912 of 5,390 pairs whose
    ordering test is within 4 ulp of a tie, and every row reads every pair (see test_geometry_sweep_fpfh)."""
    name, pts, prm = cases.fuzz(seed)
    _check_fpfh(ctx, oracle, pts, prm)


def test_seeded_fuzz_reaches_the_edges():
    """All 16 seeds together reach k >= N and a point with fewer than three neighbours within the normal radius."""
    k_at_least_n = few_neighbours = 0
    for seed in FUZZ_SEEDS:
        name, pts, prm = cases.fuzz(seed)
        k_at_least_n += prm["k"] >= len(pts)
        few_neighbours += min(len(x) for x in ref.neighbours(pts, prm["normal_radius"])) < 3
    assert k_at_least_n >= 1 and few_neighbours >= 1


# ------------------------------------------------------------------ d. the fused chain against the oracle's chain
def _oracle_chain(oracle, scene, voxel, thr, iterations, first_frame, seed=0):
    """preprocess_source (pose_estimation.py:186-268, box = False) put together from the oracle's operations."""
    down, _ = oracle.voxel_down_sample(scene, voxel)
    plane, inl = oracle.segment_plane(down, thr, iterations, seed=seed)
    nrm = oracle.estimate_normals(down, 2.0, 5) if first_frame else None
    keep = np.ones(len(down), bool)
    keep[inl] = False
    rest = down[keep]
    labels = oracle.cluster_dbscan(rest, 10, 10)
    ids, counts = np.unique(labels[labels >= 0], return_counts=True)
    sel = labels == ids[np.argmax(counts)]
    big = rest[sel]
    kept = oracle.remove_statistical_outlier(big, 75, 0.01)
    out = big[kept]
    normals = oracle.estimate_normals(out, 2.0, 5, nrm[keep][sel][kept]) if first_frame else None
    return {"points": out, "normals": normals, "plane": plane, "inliers": inl, "down": down, "rest": rest}


@pytest.fixture(scope="module")
def parity_scene(oracle):
    from pedp_hip import synth

    f = synth.Frame("parity")
    return f.scene(oracle.raycast(f.verts_posed, f.tris, f.rays6, bvh=True)["t_hit"])


def _fused_same(ctx, oracle, scene, voxel, first_frame):
    from pedp_hip import cloud_ops

    want = _oracle_chain(oracle, scene, voxel, 2.0, 200, first_frame)
    p, n, counts, status = cloud_ops.preprocess_source_fused(scene, voxel, 2.0, 200, first_frame=first_frame, seed=0, ctx=ctx)
    assert status == 0 and counts[0] == len(want["down"]) and counts[1] == len(want["rest"])
    assert np.array_equal(p, want["points"]) and len(p) > 200
    if first_frame:
        assert np.abs(n - want["normals"]).max() <= 1e-9
    else:
        assert n is None
    return want


@pytest.mark.parametrize("first_frame", [True, False])
def test_fused_chain_far_outlier(ctx, oracle, parity_scene, first_frame):
    """One outlier at (4e4, -3e4, 9e4).  The fused call shapes DBSCAN's grid from the INPUT's box -- cells of eps, doubled,
    the non-clique kernels -- the steps (and the oracle) from the remainder's own box, with clique cells: the same labels
    either way."""
    scene = np.vstack([parity_scene, [[4.0e4, -3.0e4, 9.0e4]]])
    want = _fused_same(ctx, oracle, scene, 4.0, first_frame)
    kind, cell = _dbscan_grid(scene.min(axis=0), scene.max(axis=0), 10.0)
    assert kind == "cells_of_eps" and cell > 10.0 * (1.0 + 1e-9)
    inner = want["rest"][np.abs(want["rest"]).max(axis=1) < 1e4]
    assert len(inner) == len(want["rest"]) - 1 and _dbscan_grid(inner.min(axis=0), inner.max(axis=0), 10.0)[0] == "clique"


@pytest.mark.parametrize("first_frame", [True, False])
def test_fused_chain_crowded_voxel(ctx, oracle, parity_scene, first_frame):
    """4,000 points in a 9-unit cube at voxel 0.5: more than 512 down-sampled points in one 10-unit cell of the average
    normal's grid, and DBSCAN cells (eps 10) with hundreds of core points each."""
    scene = np.vstack([parity_scene, np.random.default_rng(3).uniform([20, 20, 300], [29, 29, 309], (4000, 3))])
    _fused_same(ctx, oracle, scene, 0.5, first_frame)


def test_fused_chain_refit_over_more_than_1024_blocks(ctx, oracle):
    """A 263,000-point noisy plane (sigma 0.05, 600 x 600) and a 900-point blob 30 below it at voxel 0.05: more than
    262,144 voxels survive, so refit_fold_kernel walks more than 1024 block sums (a second pass of its staging loop);
    tracking frame with a report -- the refit plane against the oracle's, and the chain's points."""
    from pedp_hip import cloud_ops

    rng = np.random.default_rng(71)
    plane = np.column_stack([rng.uniform(0.0, 600.0, (263000, 2)), 100.0 + rng.normal(0.0, 0.05, 263000)])
    blob = rng.normal([300.0, 300.0, 70.0], 4.0, (900, 3))
    scene = np.vstack([plane, blob])[rng.permutation(263900)]
    down, _ = oracle.voxel_down_sample(scene, 0.05)
    assert (len(down) + 255) // 256 > 1024
    want_plane, want_inl = oracle.segment_plane(down, 1.0, 20, seed=0)
    assert len(want_inl) > 262144
    p, n, counts, status, rep = cloud_ops.preprocess_source_fused(scene, 0.05, 1.0, 20, first_frame=False, seed=0, ctx=ctx, report=True)
    assert status == 0 and counts[0] == len(down) and rep["inliers"] == len(want_inl)
    assert np.abs(rep["plane_model"][:3] - want_plane[:3]).max() <= 1e-12
    assert abs(rep["plane_model"][3] - want_plane[3]) <= 1e-12 * np.abs(down).max()
    want = _oracle_chain(oracle, scene, 0.05, 1.0, 20, False)
    assert np.array_equal(p, want["points"]) and 200 < len(p) <= 900


# ------------------------------------------------------------------ e. non-finite rows
BAD_VALUES = (np.nan, np.inf, -np.inf)


def _bad_copies(pts):
    """(description, copy) for one bad value at row 0, N // 2 and N - 1; the coordinate cycles."""
    n, j = len(pts), 0
    for row in (0, n // 2, n - 1):
        for v in BAD_VALUES:
            bad = pts.copy()
            bad[row, j % 3] = v
            yield f"{v} at [{row}, {j % 3}]", bad
            j += 1


@pytest.fixture(scope="module")
def valid(oracle):
    """A small valid cloud and the oracle's answers: the call after every refusal, on the same context."""
    pts = cases.blob(700, 81)
    prm = cases.params(pts)
    nrm = oracle.estimate_normals(pts, prm["normal_radius"], 30)
    return {"pts": pts, "prm": prm, "normals": nrm, "voxel": oracle.voxel_down_sample(pts, prm["voxel"])[0],
            "dbscan": oracle.cluster_dbscan(pts, prm["eps"], 5), "knn": oracle.knn_mean_distance(pts, 8),
            "fpfh": oracle.fpfh(pts, nrm, prm["fpfh_radius"], 50),
            "plane": oracle.segment_plane(pts, prm["plane_threshold"], 60, seed=2)}


def _operations(ctx):
    """name -> (call on a cloud, call on the valid cloud and its comparison)."""
    from pedp_hip import cloud_ops

    def ok_fpfh(v):
        _fpfh_same(cloud_ops.compute_fpfh(v["pts"], v["normals"], v["prm"]["fpfh_radius"], 50, ctx=ctx), v["fpfh"])

    def ok_fused(v):
        assert cloud_ops.preprocess_source_fused(v["pts"], v["prm"]["voxel"], v["prm"]["plane_threshold"], 60, first_frame=False,
                                                 seed=2, ctx=ctx)[2][0] == len(v["voxel"])

    up = np.tile([0.0, 0.0, 1.0], (1, 1))
    return {
        "voxel_down_sample": (lambda p: cloud_ops.voxel_down_sample(p, 1.0, ctx=ctx),
                              lambda v: np.testing.assert_array_equal(cloud_ops.voxel_down_sample(v["pts"], v["prm"]["voxel"], ctx=ctx)[0], v["voxel"])),
        "cluster_dbscan": (lambda p: cloud_ops.cluster_dbscan(p, 1.0, 5, ctx=ctx),
                           lambda v: np.testing.assert_array_equal(cloud_ops.cluster_dbscan(v["pts"], v["prm"]["eps"], 5, ctx=ctx), v["dbscan"])),
        "knn_mean_distance": (lambda p: cloud_ops.knn_mean_distance(p, 8, ctx=ctx),
                              lambda v: np.testing.assert_array_equal(cloud_ops.knn_mean_distance(v["pts"], 8, ctx=ctx), v["knn"])),
        "estimate_normals": (lambda p: cloud_ops.estimate_normals(p, 1.0, 30, ctx=ctx),
                             lambda v: np.testing.assert_allclose(cloud_ops.estimate_normals(v["pts"], v["prm"]["normal_radius"], 30, ctx=ctx),
                                                                  v["normals"], rtol=0, atol=1e-9)),
        "fpfh": (lambda p: cloud_ops.compute_fpfh(p, np.repeat(up, len(p), axis=0), 1.0, 50, ctx=ctx), ok_fpfh),
        "segment_plane": (lambda p: cloud_ops.segment_plane(p, 0.5, 3, 60, seed=2, ctx=ctx),
                          lambda v: _plane_same(cloud_ops.segment_plane(v["pts"], v["prm"]["plane_threshold"], 3, 60, seed=2, ctx=ctx),
                                                v["plane"], v["pts"])),
        "preprocess_source": (lambda p: cloud_ops.preprocess_source_fused(p, 1.0, 0.5, 60, first_frame=True, ctx=ctx), ok_fused),
    }


@pytest.mark.parametrize("n", [700, 5000, 33000])
@pytest.mark.parametrize("op", ["voxel_down_sample", "cluster_dbscan", "knn_mean_distance", "estimate_normals", "fpfh", "segment_plane",
                                "preprocess_source"])
def test_non_finite_rows_are_refused(ctx, valid, op, n):
    """One NaN / +inf / -inf in the first, the middle and the last row: PEDP_ERR_BAD_ARG naming the entry point and
    "non-finite coordinates", and the next valid call on the same context gives the oracle's result.  700: the host's box
    (kNN: no grid at all); 5000: kNN's grid; 33000 >= BND_DEVICE_MIN: the box from the device copy for normals and FPFH."""
    from pedp_hip import _lib

    call, ok = _operations(ctx)[op]
    pts = cases.sheet(n, 82, span=np.sqrt(n))
    for what, bad in _bad_copies(pts):
        with pytest.raises(_lib.PedpError, match=f"pedp_{op}: non-finite coordinates"):
            call(bad)
            pytest.fail(f"{op} accepted {what}")
        ok(valid)


def test_non_finite_rows_are_refused_in_device_arrays(ctx, valid):
    """The device-input voxel grid and the device-input fused chain at N = 33000: the same refusal, found by the bounds
    kernel's flag (no host pass exists)."""
    torch = pytest.importorskip("torch")
    from pedp_hip import _lib, cloud_ops

    ops = _operations(ctx)
    pts = cases.sheet(33000, 83, span=180.0)
    for what, bad in _bad_copies(pts):
        dev = torch.from_numpy(bad).cuda()
        with pytest.raises(_lib.PedpError, match="pedp_voxel_down_sample: non-finite coordinates"):
            cloud_ops.voxel_down_sample(dev, 1.0, ctx=ctx)
        ops["voxel_down_sample"][1](valid)
        with pytest.raises(_lib.PedpError, match="pedp_preprocess_source: non-finite coordinates"):
            cloud_ops.preprocess_source_fused(dev, 1.0, 0.5, 60, first_frame=False, ctx=ctx)
        ops["preprocess_source"][1](valid)
    good = torch.from_numpy(pts).cuda()
    assert np.array_equal(cloud_ops.voxel_down_sample(good, 1.0, ctx=ctx)[0], cloud_ops.voxel_down_sample(pts, 1.0, ctx=ctx)[0])


def test_non_finite_feature_rows_are_never_a_match(ctx, oracle):
    """Feature rows are not refused (pedp.h): a target row with a NaN or infinite component is never the nearest, and a
    source row with one matches -1 -- the registration's rule for non-finite rows, against a numpy argmin that applies it.
    Ns = 65 (a second workgroup of one), Nt = 1025 (a second chunk of one: the bad target row)."""
    from pedp_hip import cloud_ops

    rng = np.random.default_rng(91)
    ft = rng.uniform(0.0, 100.0, (1025, 33))
    fs = ft[rng.integers(0, 1025, 65)] + rng.normal(0.0, 1e-3, (65, 33))
    for v in BAD_VALUES:
        s, t = fs.copy(), ft.copy()
        s[64, 7] = v                     # a bad source row: no finite distance, -1
        s[3] = t[1024]
        s[4] = t[500]
        t[1024, 20] = v                  # bad target rows, one of them alone in the last chunk: never the nearest
        t[500, 0] = v
        want = ref.feature_match(s, t)
        assert want[64] == -1 and want[3] not in (-1, 1024) and want[4] not in (-1, 500)
        assert np.array_equal(cloud_ops.match_features(s, t, ctx=ctx), want)
