"""The kernels against tests/golden/g10_reference.npz: what the reference's own numpy / torch functions gave on the stored
inputs (tests/golden/make_reference_golden.py; tests/test_reference_cpu.py checks the fixture and the restatements).
Each kernel runs on the fixture's inputs, from host arrays and from CUDA tensors where its wrapper takes both.  Nothing
else is read.  Back-projections, statistics, windows, the diameter and the selection are equal in every bit; the centre,
the composed rotation and the ray directions say why they are not and by how much.

Not pinned here: so3_exp_map and rotation_6d_to_matrix (pytorch3d is not installed where the fixture is made), so the
maps from the refiner's output to rot_mat_delta rest on tests/_pose_ref.py alone; pose_update's composition after them is
pinned."""
import numpy as np
import pytest

import _reference_golden as g
from _reference_golden import DIAM_CASES, GT_CASES

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32


@pytest.fixture(scope="module")
def fx():
    return g.fixture()


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _both(*arrays):
    """The same inputs as host arrays and as CUDA tensors."""
    yield "host", arrays
    yield "device", tuple(torch.as_tensor(np.array(a), device="cuda") for a in arrays)


# ---------------------------------------------------------------- back-projection

def test_depth2xyzmap(fx):
    from pedp_hip.compat import depth2xyzmap

    K = fx["xyz/K"]
    for where, (depth, depth1) in _both(fx["xyz/depth"], fx["xyz/depth1"]):
        g.assert_bits(_np(depth2xyzmap(depth, K)), fx["xyz/out"], f"17x65 [{where}]")
        g.assert_bits(_np(depth2xyzmap(depth1, K)), fx["xyz/out1"], f"1x1 [{where}]")
        g.assert_bits(_np(depth2xyzmap(depth, K, uvs=fx["xyz/uvs"])), fx["xyz/out_uvs"], f"listed pixels [{where}]")
    uvs = torch.as_tensor(fx["xyz/uvs"].copy(), device="cuda")
    g.assert_bits(_np(depth2xyzmap(fx["xyz/depth"], K, uvs=uvs)), fx["xyz/out_uvs"], "listed pixels given as a tensor")


def test_depth2xyzmap_batch(fx):
    from pedp_hip.compat import depth2xyzmap_batch

    for where, (depths, Ks) in _both(fx["xyzb/depths"], fx["xyzb/Ks"]):
        for tag, zfar in (("inf", np.inf), ("0.8", 0.8)):
            g.assert_bits(_np(depth2xyzmap_batch(depths, Ks, zfar)), fx[f"xyzb/out_{tag}"], f"zfar {zfar} [{where}]")


def test_depth_to_scene_xyz_map(fx):
    """The xyz map of the one-call depth entry, given the same filtered image: with both filters at radius 0 the filtered
    image of `xyzb/clean` is itself (asserted), and its back-projection is the reference's of that image."""
    from pedp_hip.depth_filters import depth_to_scene

    clean, K, want = fx["xyzb/clean"][0], fx["xyzb/Ks"][0], fx["xyzb/clean_out_0.8"][0]
    for where, (depth,) in _both(clean):
        filtered, xyz, pts = depth_to_scene(depth, K, erode_radius=0, bilateral_radius=0, xyz_zfar=0.8, buffers={})
        g.assert_bits(_np(filtered), clean, f"filtered image [{where}]")
        g.assert_bits(_np(xyz), want, f"xyz map [{where}]")
        assert len(pts) == int((want[..., 2] >= F32(0.001)).sum())


# ---------------------------------------------------------------- guess_translation

@pytest.mark.parametrize("name", GT_CASES)
def test_mask_depth_stats_and_guess_translation(fx, name):
    from pedp_hip.estimator import guess_translation, mask_depth_stats

    want = g.stats_record(fx, name)
    centre, K = fx[f"gt/{name}/center"], fx["gt/K"]
    tol = 1e-12 * np.abs(centre).max()          # inv(K) and the product are LAPACK / BLAS in float64; cond(K) ~ 1e3
    for where, (depth, mask) in _both(fx[f"gt/depth/{fx[f'gt/{name}/depth']}"], fx[f"gt/{name}/mask"]):
        rec = mask_depth_stats(depth, mask)
        print(f"{name} [{where}]: {rec}")
        assert {k: rec[k] for k in want} == want, f"{name} [{where}]: {rec} for {want}"
        if "n_med" in want:
            assert isinstance(rec["median"], np.float32)
            g.assert_bits(rec["median"], fx[f"gt/{name}/median"], f"{name} [{where}] median")
        if want.get("n_med"):
            assert (rec["umin"] + rec["umax"]) / 2.0 == float(fx[f"gt/{name}/uc"])
            assert (rec["vmin"] + rec["vmax"]) / 2.0 == float(fx[f"gt/{name}/vc"])
        got = guess_translation(depth, mask, K)
        print(f"{name} [{where}]: centre {got!r}, off by {np.abs(got - centre).max():.3e} (allowed {tol:.3e})")
        assert got.shape == (3,) and got.dtype == np.float64 and np.abs(got - centre).max() <= tol


# ---------------------------------------------------------------- crop windows

@pytest.mark.parametrize("di,oi", g.CROP_CASES)
def test_crop_window(fx, di, oi):
    from pedp_hip.compat import compute_crop_window_tf_batch

    keep = fx[f"crop/d{di}/keep"]
    size = tuple(int(v) for v in fx["crop/out_sizes"][oi])
    want = g.crop_tf(fx, di, oi)[keep]
    for where, (poses,) in _both(g.crop_poses(fx["crop/trans"])):
        tf = compute_crop_window_tf_batch(poses=poses, K=fx["crop/K"], crop_ratio=float(fx["crop/crop_ratio"]), out_size=size,
                                          method="box_3d", mesh_diameter=float(fx["crop/diameters"][di]))
        g.assert_bits(_np(tf)[keep], want, f"diameter {di} out_size {size} [{where}]")


def test_crop_window_at_half_integer_edges(fx):
    """Window edges at exactly a half-integer, which the kept poses above cannot have: every operation before the
    rounding is exact in float32 here, so the rounding mode alone decides (half to even, as torch rounds)."""
    from pedp_hip.compat import compute_crop_window_tf_batch

    for where, (poses,) in _both(g.crop_poses(fx["crop/half/trans"])):
        tf = compute_crop_window_tf_batch(poses=poses, K=fx["crop/K"], crop_ratio=float(fx["crop/half/crop_ratio"]), out_size=(160, 160),
                                          method="box_3d", mesh_diameter=float(fx["crop/half/diameter"]))
        g.assert_bits(_np(tf), fx["crop/half/tf"], f"half-integer edges [{where}]")


# ---------------------------------------------------------------- pose composition

def _check_composition(poses, td, rd, A, what):
    """poses against egocentric_delta_pose_to_pose's formula on the kernel's own deltas: B[:3, 3] = A[:3, 3] + td is one
    addition (equal in every bit), B[:3, :3] = Rd @ A[:3, :3] a three-term dot product per entry (the bound)."""
    poses, td, rd = _np(poses), _np(td), _np(rd)
    g.assert_bits(poses[:, :3, 3], A[:, :3, 3] + td, f"{what}: translation")
    g.assert_bits(poses[:, 3], np.tile(F32([0, 0, 0, 1]), (len(A), 1)), f"{what}: last row")
    exact = rd.astype(np.float64) @ A[:, :3, :3].astype(np.float64)
    over = np.abs(poses[:, :3, :3] - exact) / g.compose_bound(rd, A)
    print(f"{what}: rotation entries at most {over.max():.3f} of the bound")
    assert over.max() <= 1, what


def test_pose_update_on_the_fixture_triples(fx):
    from pedp_hip.pose import pose_update

    A, td, Rd, B = fx["pose/A"], fx["pose/td"], fx["pose/Rd"], fx["pose/B"]
    for where, (t, r, a) in _both(td, g.rot6d_of(Rd), A):
        poses, tdelta, rdelta = pose_update(t, r, a, want_deltas=True, trans_rep="raw", rot_rep="6d")
        poses, tdelta, rdelta = _np(poses), _np(tdelta), _np(rdelta)
        g.assert_bits(tdelta, td, f"trans_delta [{where}]")
        err = np.abs(rdelta.astype(np.float64) - Rd)
        print(f"[{where}] max |rdelta - Rd| = {err.max() / g.U23:.2f} x 2^-23")
        assert err.max() <= 4 * g.U23, "the emitted rot_mat_delta is the fixture's Rd up to float32 rounding"
        _check_composition(poses, tdelta, rdelta, A, f"fixture triples [{where}]")
        g.assert_bits(poses[:, :3, 3], B[:, :3, 3], f"translation against the fixture [{where}]")
        # against the fixture's B: the bound for Rd, and A's column sums for the (at most 4 * 2^-23) the deltas differ by
        room = g.compose_bound(Rd, A) + 4 * g.U23 * np.abs(A[:, :3, :3].astype(np.float64)).sum(1)[:, None, :]
        assert (np.abs(poses[:, :3, :3].astype(np.float64) - B[:, :3, :3]) <= room).all()
        transposed = np.abs(rdelta.transpose(0, 2, 1).astype(np.float64) - Rd).reshape(len(Rd), -1).max(1)
        assert (transposed > 1e-3).all(), "a transposed delta would not show"


@pytest.mark.parametrize("rot_rep", ["axis_angle", "6d"])
@pytest.mark.parametrize("trans_rep", ["tracknet", "raw"])
def test_pose_update_composes_its_own_deltas(fx, rot_rep, trans_rep):
    from pedp_hip.pose import pose_update

    A = fx["pose/A"]
    rng = np.random.default_rng(11)
    trans = rng.normal(0, 1.5, (len(A), 3)).astype(F32)
    rot = rng.normal(0, 1.5, (len(A), 6 if rot_rep == "6d" else 3)).astype(F32)
    for where, (t, r, a) in _both(trans, rot, A):
        poses, td, rd = pose_update(t, r, a, want_deltas=True, trans_rep=trans_rep, rot_rep=rot_rep, trans_normalizer=[0.02, 0.03, 0.05],
                                    rot_normalizer=0.35)
        _check_composition(poses, td, rd, A, f"{rot_rep} {trans_rep} [{where}]")
        rd = _np(rd).astype(np.float64)
        assert np.abs(rd @ rd.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5, "a rotation"


# ---------------------------------------------------------------- diameter

@pytest.mark.parametrize("name", DIAM_CASES)
def test_max_pair_distance(fx, name):
    from pedp_hip.estimator import compute_mesh_diameter
    from pedp_hip.pose import max_pair_distance

    want = fx[f"diam/{name}/out"]
    for where, (pts,) in _both(fx[f"diam/{name}/pts"]):
        got = max_pair_distance(pts)
        assert isinstance(got, float)
        g.assert_bits(np.float64(got), want, f"{name} [{where}]")
    g.assert_bits(np.float64(compute_mesh_diameter(model_pts=fx[f"diam/{name}/pts"], n_sample=None)), want, f"{name} compute_mesh_diameter")


# ---------------------------------------------------------------- heat map to rays

@pytest.mark.parametrize("name", ["h9", "h48"])
def test_project_heatmap_selection_and_rays(fx, ctx, name):
    """Every pixel ray hits the one large triangle, so the hits are the selection: pixels, intensities and n_rays are the
    reference's heatmap_to_points (order included).  The hit points o + d t (o = 0), normalised here, give the device's
    float64 directions back; in units of u = 2^-53 relative error: the product d t 1, its effect on the norm 1, the norm's
    own five operations and square root 2.5, the quotient 1, the device's d being a unit vector only up to its own
    length's and quotients' rounding 2; and the device's length sqrt((x x + y y) + 1) is within one step (2 u) of the
    reference's BLAS dot product's, each quotient rounding once more on either side (2 u): 11.5 u in all, on components of
    at most 1, so 12 * 2^-53 absolute."""
    from pedp_hip import _lib

    verts, tris = g.big_triangle()
    mesh = _lib.Mesh(ctx, verts, tris)
    h = fx[f"heat/{name}"]
    for ti, thr in enumerate(fx["heat/thresholds"].tolist()):
        xy, inten = fx[f"heat/{name}_t{ti}/xy"], fx[f"heat/{name}_t{ti}/intensity"]
        for cam in ("tiny", "parity") if ti == 0 else ("tiny",):
            for where, (heat,) in _both(h):
                out = mesh.project_heatmap(heat, fx[f"heat/K_{cam}"], thr)
                what = f"{name} threshold {thr} {cam} [{where}]"
                assert out["n_rays"] == len(xy) == len(out["pixels"]), f"{what}: {out['n_rays']} rays, {len(out['pixels'])} hits for {len(xy)}"
                g.assert_bits(out["pixels"].astype(np.int64), xy, f"{what} pixels")
                g.assert_bits(out["intensities"], inten.astype(np.float64), f"{what} intensities")
                assert (out["primitive_ids"] == 0).all()
                if ti == 0:
                    p = out["points"]
                    d = p / np.sqrt((p * p).sum(1))[:, None]
                    off = np.abs(d - fx[f"heat/{name}_t0/rays_{cam}"]).max()
                    print(f"{what}: directions off by {off / 2.0 ** -53:.2f} x 2^-53")
                    assert off <= 12 * 2.0 ** -53, what
