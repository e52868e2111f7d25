"""tests/golden/g10_reference.npz holds what the reference's own numpy / torch functions gave on stored inputs
(tests/golden/make_reference_golden.py).  Here, without a GPU: the fixture has the arrays and the discriminating cases it
is meant to have, and the package's host-side functions, the oracle and the restatements the GPU tests trust
(tests/_crop_ref.py, _estimator_ref.py, _pose_ref.py) reproduce it.  Everything that is a sequence of single IEEE
operations or an exact selection is equal in every bit; the three comparisons that are not say why and by how much."""
import types

import numpy as np
import pytest

import _crop_ref
import _estimator_ref
import _pose_ref
import _reference_golden as g
from pedp_hip import estimator, icp_refine, ray_projection, render

F32 = np.float32
STATS, GT_CASES, DIAM_CASES = g.STATS, g.GT_CASES, g.DIAM_CASES


@pytest.fixture(scope="module")
def fx():
    return g.fixture()


def _camera(K):
    return types.SimpleNamespace(intrinsic_matrix=np.asarray(K, np.float64))


# ---------------------------------------------------------------- the fixture itself

SHAPES = {
    "xyz/K": ((3, 3), "f8"), "xyz/depth": ((17, 65), "f4"), "xyz/uvs": ((64, 2), "f8"), "xyz/out": ((17, 65, 3), "f4"),
    "xyz/out_uvs": ((17, 65, 3), "f4"), "xyz/depth1": ((1, 1), "f4"), "xyz/out1": ((1, 1, 3), "f4"),
    "xyzb/depths": ((3, 17, 65), "f4"), "xyzb/Ks": ((3, 3, 3), "f4"), "xyzb/zfars": ((2,), "f8"),
    "xyzb/out_inf": ((3, 17, 65, 3), "f4"), "xyzb/out_0.8": ((3, 17, 65, 3), "f4"), "xyzb/clean": ((1, 17, 65), "f4"),
    "xyzb/clean_out_0.8": ((1, 17, 65, 3), "f4"),
    "gt/K": ((3, 3), "f8"), "gt/depth/37x53_c": ((37, 53), "f4"), "gt/depth/37x53_q": ((37, 53), "f4"),
    "gt/depth/64x96_q": ((64, 96), "f4"), "gt/depth/1x1_a": ((1, 1), "f4"),
    "crop/trans": ((2000, 3), "f4"), "crop/K": ((3, 3), "f4"), "crop/diameters": ((3,), "f8"), "crop/crop_ratio": ((), "f8"),
    "crop/out_sizes": ((2, 2), "i8"), "crop/d0/keep": (None, "i4"), "crop/d1_o1/tx": ((2000,), "f4"),
    "crop/half/trans": ((24, 3), "f4"), "crop/half/tf": ((24, 3, 3), "f4"),
    "pose/A": ((300, 4, 4), "f4"), "pose/td": ((300, 3), "f4"), "pose/Rd": ((300, 3, 3), "f4"), "pose/B": ((300, 4, 4), "f4"),
    "diam/513/pts": ((513, 3), "f8"), "diam/513/out": ((), "f8"), "diam/1/pts": ((1, 3), "f8"),
    "proj/0/K": ((3, 3), "f8"), "proj/0/y_down": ((4, 4), "f8"), "proj/2/y_up": ((4, 4), "f8"),
    "heat/h9": ((9, 11), "f8"), "heat/h48": ((48, 64), "f4"), "heat/thresholds": ((3,), "f8"), "heat/K_tiny": ((3, 3), "f8"),
    "heat/K_parity": ((3, 3), "f8"), "heat/h9_t0/xy": (None, "i8"), "heat/h48_t0/rays_parity": (None, "f8"),
    "p3d/heat": ((9, 11), "f8"), "p3d/depth_f32": ((9, 11), "f4"), "p3d/depth_u16": ((9, 11), "u2"),
    "p3d/depth_small": ((7, 9), "f4"), "p3d/points": ((12, 2), "i8"), "p3d/f32_t0/out": (None, "f8"),
    "p3d/f32/coords": ((11, 3), "f8"),
    "flip/planes": ((6, 4), "f8"), "flip/normals": ((6, 3), "f8"), "flip/out_planes": ((6, 4), "f8"), "flip/out_normals": ((6, 3), "f8"),
}


def test_fixture_keys_and_shapes(fx):
    for key, (shape, dtype) in SHAPES.items():
        assert key in fx, key
        assert fx[key].dtype == np.dtype(dtype), f"{key}: {fx[key].dtype}"
        if shape is not None:
            assert fx[key].shape == shape, f"{key}: {fx[key].shape}"
    assert all(v.dtype.kind in "biufU" for v in fx.values()), "numbers and names only"
    assert list(fx["gt/cases"]) == GT_CASES and list(fx["diam/cases"]) == DIAM_CASES
    for name in GT_CASES:
        depth = fx[f"gt/depth/{fx[f'gt/{name}/depth']}"]
        assert fx[f"gt/{name}/mask"].shape == depth.shape
        assert fx[f"gt/{name}/center"].shape == (3,) and fx[f"gt/{name}/median"].dtype == np.float32
        assert all(f"gt/{name}/{k}" in fx for k in STATS + ("uc", "vc"))
    assert {str(fx[f"gt/{n}/mask"].dtype) for n in GT_CASES} == {"bool", "uint8", "float32"}
    assert sorted(fx[f"gt/{n}/mask"].shape for n in GT_CASES)[::6] == [(1, 1), (37, 53), (64, 96)]
    for di, oi in g.CROP_CASES:
        assert all(fx[f"crop/d{di}_o{oi}/{k}"].shape == (2000,) for k in ("sx", "sy", "tx", "ty"))
    for name in ("h9", "h48"):
        for ti in range(3):
            n = len(fx[f"heat/{name}_t{ti}/xy"])
            assert fx[f"heat/{name}_t{ti}/xy"].shape == (n, 2) and fx[f"heat/{name}_t{ti}/intensity"].shape == (n,)
            assert fx[f"heat/{name}_t{ti}/intensity"].dtype == fx[f"heat/{name}"].dtype
        for cam in ("tiny", "parity"):
            assert fx[f"heat/{name}_t0/rays_{cam}"].shape == (len(fx[f"heat/{name}_t0/xy"]), 3)


def test_fixture_holds_the_discriminating_cases(fx):
    """Minimum counts of the inputs that tell a right reading from a plausible wrong one, so that a regenerated fixture
    cannot quietly lose them."""
    uv = fx["xyz/uvs"]
    half = (uv % 1) == 0.5
    even = half & (np.floor(uv) % 2 == 0)
    assert half.any(1).sum() >= 16 and even.any(1).sum() >= 8 and (half & ~even).any(1).sum() >= 8
    # numpy rounds half to even: exactly the .5 entries with an even floor land elsewhere under half-away-from-zero
    assert np.array_equal(np.round(uv) != np.floor(uv + 0.5), even) and even.any(1).sum() >= 8
    assert len(uv) - len(np.unique(np.round(uv), axis=0)) >= 4, "duplicates after rounding"
    d = fx["xyz/depth"]
    for v in (0.0, F32(0.000999), F32(0.001), F32(-0.5), np.inf):
        assert (d == v).sum() >= 8, v
    assert np.isnan(d).sum() >= 8
    assert all(float(k) != np.floor(k) for k in (fx["xyz/K"][0, 2], fx["xyz/K"][1, 2]))
    listed = d[np.round(uv[:, 1]).astype(int), np.round(uv[:, 0]).astype(int)]
    assert (~(listed >= F32(0.001))).sum() >= 6, "listed pixels that are invalid or NaN"

    db, z8 = fx["xyzb/depths"], F32(0.8)
    assert fx["xyzb/zfars"].tolist() == [np.inf, 0.8]
    assert (db == z8).sum() >= 16 and (db == np.nextafter(z8, F32(1))).sum() >= 16
    assert np.isnan(db).sum() >= 16 and (db < 0).sum() >= 16 and np.isinf(db).sum() >= 16
    assert (fx["xyzb/out_0.8"][db == z8][:, 2] == z8).all(), "an entry equal to zfar is kept: the test is >"
    assert (fx["xyzb/out_0.8"][db == np.nextafter(z8, F32(1))] == 0).all()
    assert len({fx["xyzb/Ks"][b].tobytes() for b in range(3)}) == 3

    odd = 0
    for name in GT_CASES:
        m = fx[f"gt/{name}/mask"]
        with np.errstate(invalid="ignore"):
            odd += int((m.astype(bool) & ~(m > 0)).sum())           # truthy, not positive: negative and NaN entries
        if m.dtype == np.uint8 and m.any() and m.size > 1:
            assert set(np.unique(m)) == {0, 1, 2, 255}
        if m.dtype == np.float32 and m.size > 1:
            assert (m < 0).sum() >= 16 and np.isnan(m).sum() >= 16 and (np.signbit(m) & (m == 0)).sum() >= 16
            assert int(fx[f"gt/{name}/n_med"]) > int(fx[f"gt/{name}/n_valid"]), "the median sees more than the box"
    assert odd >= 200
    for dk in ("37x53_c", "37x53_q", "64x96_q"):
        dd = fx[f"gt/depth/{dk}"]
        for v in (0.0, F32(-0.4), F32(0.000999), F32(0.001), np.inf):
            assert (dd == v).sum() >= 4, (dk, v)
        assert np.isnan(dd).sum() >= 4
    assert {int(fx[f"gt/{n}/n_med"]) % 2 for n in GT_CASES[:4]} == {0, 1} == {int(fx[f"gt/{n}/n_med"]) % 2 for n in GT_CASES[4:8]}
    q = fx["gt/depth/64x96_q"]
    assert len(np.unique(q[np.isfinite(q)])) < q.size // 3, "quantised depths: ties"
    assert int(fx["gt/zero_mask/n_pos"]) == 0 and int(fx["gt/no_valid/n_pos"]) > 0 and int(fx["gt/no_valid/n_med"]) == 0
    assert int(fx["gt/1x1_negative/n_pos"]) == 0 and float(fx["gt/1x1_negative/mask"][0, 0]) < 0

    for di in range(3):
        left_out = 2000 - len(fx[f"crop/d{di}/keep"])
        print(f"crop diameter {fx['crop/diameters'][di]}: {left_out} of 2000 poses left out")
        assert 0 < left_out <= 0.02 * 2000

    edges = g.half_edges(fx)
    assert (edges % 1 == 0.5).all() and edges.astype(F32).astype(np.float64).tolist() == edges.tolist()
    differ = np.rint(edges) != np.floor(edges + 0.5)              # half-even against half-away: the even floors
    assert differ.sum() >= 8 and (~differ).sum() >= 8 and differ.any(1).all()

    for name, least in (("h9", 4), ("h48", 32)):
        h = fx[f"heat/{name}"]
        for ti, thr in enumerate(fx["heat/thresholds"].tolist()):
            equal = h == h.dtype.type(thr)
            assert equal.sum() >= least, (name, thr)
            sel = np.zeros(h.shape, bool)
            sel[fx[f"heat/{name}_t{ti}/xy"][:, 1], fx[f"heat/{name}_t{ti}/xy"][:, 0]] = True
            assert not sel[equal].any(), "an entry equal to the threshold is not above it"
        assert np.isnan(h).sum() >= 4
    t3 = F32(0.3)
    assert float(t3) > 0.3 and (fx["heat/h48"] == t3).sum() >= 32, "float32(0.3) entries: above 0.3 only if widened first"
    assert (fx["heat/h48"] == np.nextafter(t3, F32(1))).sum() >= 32
    assert (fx["heat/thresholds"] < 0).any()

    assert int(fx["p3d/equal_to_threshold"]) >= 4
    for k in ("f32", "small"):
        assert (fx[f"p3d/depth_{k}"] == 0).sum() >= 2 and (fx[f"p3d/depth_{k}"] < 0).sum() >= 2
    px = fx["p3d/points"]
    assert (fx["p3d/depth_f32"][px[:, 1], px[:, 0]] == 0).sum() == 1 and len(fx["p3d/f32/coords"]) == len(px) - 1
    flipped = (fx["flip/out_planes"] != fx["flip/planes"]).any(1)
    assert flipped.sum() >= 2 and (~flipped).sum() >= 2
    n = fx["flip/planes"][:, :3] / np.linalg.norm(fx["flip/planes"][:, :3], axis=1, keepdims=True)
    assert ((n * fx["flip/normals"]).sum(1) == 0).any(), "a dot product of exactly zero: not flipped"


# ---------------------------------------------------------------- back-projection

def test_oracle_depth2xyzmap(fx, oracle):
    g.assert_bits(oracle.depth2xyzmap(fx["xyz/depth"], fx["xyz/K"]), fx["xyz/out"], "17x65")
    g.assert_bits(oracle.depth2xyzmap(fx["xyz/depth1"], fx["xyz/K"]), fx["xyz/out1"], "1x1")


def test_listed_pixels_are_the_full_maps(fx):
    """What depth2xyzmap's wrapper relies on for `uvs`: the reference's map of listed pixels is its full map at the
    pixels numpy's round (half to even) sends them to, zero elsewhere."""
    uv = np.round(fx["xyz/uvs"]).astype(int)
    want = np.zeros_like(fx["xyz/out"])
    want[uv[:, 1], uv[:, 0]] = fx["xyz/out"][uv[:, 1], uv[:, 0]]
    g.assert_bits(want, fx["xyz/out_uvs"], "listed pixels")
    away = np.floor(fx["xyz/uvs"] + 0.5).astype(int)
    wrong = np.zeros_like(want)
    wrong[away[:, 1], away[:, 0]] = fx["xyz/out"][away[:, 1], away[:, 0]]
    assert not g.same_bits(wrong, fx["xyz/out_uvs"]), "half-away-from-zero rounding would not show"


def test_oracle_depth2xyzmap_batch(fx, oracle):
    for tag, zfar in (("inf", np.inf), ("0.8", 0.8)):
        g.assert_bits(oracle.depth2xyzmap_batch(fx["xyzb/depths"], fx["xyzb/Ks"], zfar), fx[f"xyzb/out_{tag}"], f"zfar {zfar}")
    g.assert_bits(oracle.depth2xyzmap_batch(fx["xyzb/clean"], fx["xyzb/Ks"][:1], 0.8), fx["xyzb/clean_out_0.8"], "clean")
    d = fx["xyzb/depths"][0]
    with np.errstate(invalid="ignore"):
        g.assert_bits(np.where((d >= F32(0.001)) & (d < F32(100)), d, F32(0)), fx["xyzb/clean"][0], "the clean image")


# ---------------------------------------------------------------- guess_translation

@pytest.mark.parametrize("name", GT_CASES)
def test_mask_depth_statistics_and_centre(fx, name):
    depth, mask, K = fx[f"gt/depth/{fx[f'gt/{name}/depth']}"], fx[f"gt/{name}/mask"], fx["gt/K"]
    want = g.stats_record(fx, name)
    centre = fx[f"gt/{name}/center"]
    tol = 1e-12 * np.abs(centre).max()          # inv(K) and the product are LAPACK / BLAS in float64; cond(K) ~ 1e3
    for who, rec in (("_estimator_ref.stats", _estimator_ref.stats(depth, mask)), ("estimator._host_stats", estimator._host_stats(depth, mask))):
        assert {k: int(rec[k]) for k in want} == want, f"{who}: {rec} for {want}"
        if "n_med" in want:
            g.assert_bits(np.float32(rec["median"]), fx[f"gt/{name}/median"], f"{who} median")
        if want.get("n_med"):
            assert (rec["umin"] + rec["umax"]) / 2.0 == float(fx[f"gt/{name}/uc"]), who
            assert (rec["vmin"] + rec["vmax"]) / 2.0 == float(fx[f"gt/{name}/vc"]), who
        got = estimator._center_from(rec, K)
        assert got.shape == (3,) and np.abs(got - centre).max() <= tol, f"{who} centre {got} for {centre}"
    got = _estimator_ref.guess_translation(depth, mask, K)
    assert got.shape == (3,) and np.abs(got - centre).max() <= tol, f"_estimator_ref.guess_translation: {got} for {centre}"


# ---------------------------------------------------------------- crop windows

@pytest.mark.parametrize("di,oi", g.CROP_CASES)
def test_crop_window_restatement(fx, di, oi):
    keep = fx[f"crop/d{di}/keep"]
    w, h = (int(v) for v in fx["crop/out_sizes"][oi])
    radius = float(fx["crop/diameters"][di]) * float(fx["crop/crop_ratio"]) / 2
    tf, _ = _crop_ref.crop_window(g.crop_poses(fx["crop/trans"]), fx["crop/K"], radius, w, h)
    g.assert_bits(tf[keep], g.crop_tf(fx, di, oi)[keep], f"diameter {di} out_size {w}x{h}")


def test_crop_window_restatement_at_half_integer_edges(fx):
    """Edges at exactly a half-integer (exact arithmetic, so no device's matmul decides): round half to even."""
    radius = float(fx["crop/half/diameter"]) * float(fx["crop/half/crop_ratio"]) / 2
    tf, _ = _crop_ref.crop_window(g.crop_poses(fx["crop/half/trans"]), fx["crop/K"], radius, 160, 160)
    g.assert_bits(tf, fx["crop/half/tf"], "half-integer edges")
    edges = g.half_edges(fx)
    want = fx["crop/half/tf"].astype(np.float64)
    # the reference's own windows say half to even (their entries are float32 quotients: the nearest integer is the edge)
    assert np.array_equal(np.rint(-want[:, 0, 2] / want[:, 0, 0]), np.rint(edges[:, 0])), "left edges"
    assert np.array_equal(np.rint(160 / want[:, 0, 0]), np.rint(edges[:, 1]) - np.rint(edges[:, 0])), "widths"


# ---------------------------------------------------------------- pose composition

def test_pose_composition_restatement(fx):
    A, td, Rd, B = fx["pose/A"], fx["pose/td"], fx["pose/Rd"], fx["pose/B"]
    exact = Rd.astype(np.float64) @ A[:, :3, :3].astype(np.float64)
    bound = g.compose_bound(Rd, A)
    assert (np.abs(B[:, :3, :3] - exact) <= bound).all(), "the fixture against its own formula"
    g.assert_bits(B[:, :3, 3], A[:, :3, 3] + td, "B[:3, 3] = A[:3, 3] + td")
    g.assert_bits(B[:, 3], np.tile(F32([0, 0, 0, 1]), (len(B), 1)), "last row")
    g.assert_bits(_pose_ref._mat3(Rd, A[:, :3, :3]), _pose_ref._mat3(Rd, A[:, :3, :3]).astype(F32), "float32 throughout")
    assert (np.abs(_pose_ref._mat3(Rd, A[:, :3, :3]) - B[:, :3, :3]) <= bound).all()
    # through the restatement's whole update, from raw 6d outputs whose Gram-Schmidt result is Rd up to rounding
    out, td_r, Rd_r = _pose_ref.pose_update(td, g.rot6d_of(Rd), A, trans_rep="raw", rot_rep="6d")
    err = np.abs(Rd_r.astype(np.float64) - Rd).max()
    print(f"restated 6d: max |rdelta - Rd| = {err / g.U23:.2f} x 2^-23")
    assert err <= 4 * g.U23
    g.assert_bits(td_r, td, "trans_delta")
    g.assert_bits(out[:, :3, 3], B[:, :3, 3], "translation")
    assert (np.abs(out[:, :3, :3] - Rd_r.astype(np.float64) @ A[:, :3, :3].astype(np.float64)) <= g.compose_bound(Rd_r, A)).all()
    transposed = np.abs(_pose_ref._mat3(Rd.transpose(0, 2, 1), A[:, :3, :3]) - B[:, :3, :3]) <= bound
    assert not transposed.all(1).all(1).any(), "a transposed Rd would not show"


# ---------------------------------------------------------------- diameter

@pytest.mark.parametrize("name", DIAM_CASES)
def test_max_pair_distance_restatement(fx, name):
    got = _pose_ref.max_pair_distance(fx[f"diam/{name}/pts"])
    g.assert_bits(np.float64(got), fx[f"diam/{name}/out"], name)


def test_extreme_pair_sits_in_two_tiles(fx):
    p = fx["diam/far/pts"]
    d = np.linalg.norm(p[None] - p[:, None], axis=-1)
    i, j = np.unravel_index(np.argmax(d), d.shape)
    assert i // 256 != j // 256 and d[i, j] == float(fx["diam/far/out"])
    assert float(fx["diam/equal/out"]) == 0.0 and float(fx["diam/1/out"]) == 0.0


# ---------------------------------------------------------------- projection matrix

def test_projection_matrix(fx):
    assert int(fx["proj/n"]) == 3 and fx["proj/0/near_far"].tolist() == [0.001, 100.0]
    for i in range(3):
        (h, w), (near, far) = (int(v) for v in fx[f"proj/{i}/hw"]), fx[f"proj/{i}/near_far"].tolist()
        for wc in ("y_down", "y_up"):
            g.assert_bits(render.projection_matrix_from_intrinsics(fx[f"proj/{i}/K"], h, w, near, far, wc), fx[f"proj/{i}/{wc}"],
                          f"set {i} {wc}")
    g.assert_bits(render.projection_matrix_from_intrinsics(fx["proj/2/K"], 144, 160, 0.05, 3, "y_up"), fx["proj/2/y_up"],
                  "an integer zfar")


# ---------------------------------------------------------------- heat map to rays

def _points(fx, name, ti):
    h = fx[f"heat/{name}"]
    with np.errstate(invalid="ignore"):
        return ray_projection.heatmap_to_points(h, float(fx["heat/thresholds"][ti]))


@pytest.mark.parametrize("name", ["h9", "h48"])
def test_heatmap_to_points(fx, name):
    for ti in range(3):
        pts = _points(fx, name, ti)
        xy, inten = fx[f"heat/{name}_t{ti}/xy"], fx[f"heat/{name}_t{ti}/intensity"]
        assert len(pts) == len(xy)
        g.assert_bits(np.array([[p[0], p[1]] for p in pts], np.int64), xy, f"{name} t{ti} order")
        assert all(type(p[2]) is inten.dtype.type for p in pts)
        g.assert_bits(np.array([p[2] for p in pts], inten.dtype), inten, f"{name} t{ti} intensities")


def _check_rays(got, want, what):
    """<= 1 ulp in float64 per component (the reference normalises each ray with np.linalg.norm, the whole-array forms
    divide by one square root of a sum formed in another order), and equal after the cast to float32 wherever the
    float64 values are equal."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    steps = g.ulps64(got, want)
    print(f"{what}: {int((steps > 0).sum())} of {steps.size} components differ, at most {int(steps.max(initial=0))} ulp")
    assert steps.max(initial=0) <= 1, what
    same = steps == 0
    assert np.array_equal(got.astype(F32)[same].view(np.uint32), want.astype(F32)[same].view(np.uint32)), what


@pytest.mark.parametrize("name", ["h9", "h48"])
@pytest.mark.parametrize("cam", ["tiny", "parity"])
def test_compute_rays(fx, oracle, name, cam):
    K = fx[f"heat/K_{cam}"]
    want = fx[f"heat/{name}_t0/rays_{cam}"]
    rays, inten = ray_projection.compute_rays(_points(fx, name, 0), _camera(K))
    _check_rays(rays, want, f"compute_rays {name} {cam}")
    g.assert_bits(inten, fx[f"heat/{name}_t0/intensity"], "intensities")
    verts, tris = g.big_triangle()
    with np.errstate(invalid="ignore"):
        o = oracle.project_heatmap(verts, tris, fx[f"heat/{name}"], K, float(fx["heat/thresholds"][0]), bvh=False)
    assert o["n_rays"] == len(want) == len(o["pixels"]), "every ray of the oracle hits the triangle"
    g.assert_bits(o["pixels"].astype(np.int64), fx[f"heat/{name}_t0/xy"], "oracle pixels")
    g.assert_bits(o["intensities"], fx[f"heat/{name}_t0/intensity"].astype(np.float64), "oracle intensities")
    # the oracle keeps its directions as float32 only: equal to the reference's cast wherever the float32 grid decides
    near = np.abs(o["rays6"][:, 3:].astype(np.float64) - want) <= np.spacing(np.abs(want).astype(F32)) / 2 * (1 + 2.0 ** -20)
    assert near.all() and (o["rays6"][:, :3] == 0).all()


@pytest.mark.parametrize("name", ["h9", "h48"])
def test_oracle_selection_at_every_threshold(fx, oracle, name):
    verts, tris = g.big_triangle()
    for ti, thr in enumerate(fx["heat/thresholds"].tolist()):
        with np.errstate(invalid="ignore"):
            o = oracle.project_heatmap(verts, tris, fx[f"heat/{name}"], fx["heat/K_tiny"], thr, bvh=False)
        assert o["n_rays"] == len(fx[f"heat/{name}_t{ti}/xy"]), f"{name} threshold {thr}: {o['n_rays']} rays"
        g.assert_bits(o["pixels"].astype(np.int64), fx[f"heat/{name}_t{ti}/xy"], f"{name} threshold {thr}")
        g.assert_bits(o["intensities"], fx[f"heat/{name}_t{ti}/intensity"].astype(np.float64), f"{name} threshold {thr}")


def test_compute_rays_of_no_points(fx):
    rays, inten = ray_projection.compute_rays([], _camera(fx["heat/K_tiny"]))
    assert np.asarray(rays).shape + np.asarray(inten).shape == tuple(fx["heat/empty_rays_shape"])


# ---------------------------------------------------------------- depth-based projection

@pytest.mark.parametrize("name", ["f32", "u16", "small"])
def test_heatmap_to_point3d(fx, name):
    cam = _camera(fx["p3d/K"])
    for ti, thr in enumerate(fx["p3d/thresholds"].tolist()):
        got = ray_projection.heatmap_to_point3d(fx["p3d/heat"], fx[f"p3d/depth_{name}"], cam, thr)
        g.assert_bits(got, fx[f"p3d/{name}_t{ti}/out"], f"{name} threshold {thr}")


@pytest.mark.parametrize("name", ["f32", "u16"])
def test_calc_coordinates(fx, name):
    got = ray_projection.calc_coordinates(fx[f"p3d/depth_{name}"], fx["p3d/points"], _camera(fx["p3d/K"]))
    g.assert_bits(got, fx[f"p3d/{name}/coords"], name)


# ---------------------------------------------------------------- plane orientation

def test_flip_plane_normal(fx):
    for i, (plane, normal) in enumerate(zip(fx["flip/planes"], fx["flip/normals"])):
        model, n = icp_refine.flip_plane_normal_if_needed(list(plane), normal.copy())
        g.assert_bits(np.asarray(model, np.float64), fx["flip/out_planes"][i], f"plane {i}")
        g.assert_bits(np.asarray(n), fx["flip/out_normals"][i], f"normal {i}")
