"""GPU tests of pedp_fit_to_surface and the functions over it (surface_fit.py) against the numpy restatement
(tests/_surface_fit_ref.py): the sums of pass 0 within the first-order bound of any summation order, the whole result
bit for bit across the search kernels, the memory forms and the context's history, the loop against the reference loop,
the edges, and the composition with the depth frame and the deviation heat map."""
import ctypes as C

import numpy as np
import pytest

import _closest_ref as ref
import _surface_fit_ref as sf

pytestmark = pytest.mark.gpu

# (triangles, points): test_closest_gpu's pairing of the counts around one cluster (16), one super-cluster (1024) and the
# parity torus with the batch sizes around one wave (64) and one block of the sums (256)
PACKET_CASES = [(1, 3072), (16, 65), (17, 64), (1024, 255), (1025, 257), (4000, 256), (1025, 1), (1025, 63)]
LOSS_SCALE = {"l2": None, "huber": 0.4, "tukey": 1.5}
GATE = 20.0                                          # the queries 200 off a face, and most scattered ones, lie beyond it


def same(a, b):
    """Bit for bit, NaN as NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_result(a, b):
    """The first field in which two results of fit_to_surface differ in a bit, or None."""
    for k in ("transformation", "fitness", "inlier_rmse", "iterations", "inliers", "weight_sum", "singular", "finite_rows",
              "packet", "trace"):
        x, y = getattr(a, k), getattr(b, k)
        if not ((x is None and y is None) or same(x, y)):
            return k
    return None


@pytest.fixture
def modes(ctx):
    """Runs fn() in every closest-point mode (0 by N, 1 exhaustive, 2 a lane per point, 3 a wave per point)."""
    from pedp_hip import _lib

    def run(fn):
        out = []
        for mode in (0, 1, 2, 3):
            _lib.closest_configure(ctx, mode)
            out.append(fn())
        _lib.closest_configure(ctx, 0)
        return out

    yield run
    _lib.closest_configure(ctx, 0)


def mesh_and_queries(F, N):
    if F == 4000:
        verts, tris = sf.torus_mesh()
    else:
        verts, tris = sf.soup(F, F)
    pts = sf.queries(verts, tris, N, 100 + F + N)
    if N >= 63:
        pts[[2, N // 2, N - 1], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    return verts, tris, pts


@pytest.mark.parametrize("loss", sorted(LOSS_SCALE))
@pytest.mark.parametrize("F,N", PACKET_CASES)
def test_packet_of_pass_0(ctx, modes, F, N, loss):
    """max_iteration = 0 closes pass 0 alone and returns its packet.  Every entry lies within (n - 1) 2^-52 sum |term| of
    math.fsum over the reference's terms, the first-order bound of ANY order of n terms; the counts are exact."""
    from pedp_hip import _lib, surface_fit

    verts, tris, pts = mesh_and_queries(F, N)
    scale = LOSS_SCALE[loss]
    terms, rows, finite = sf.row_terms(ref.records(verts, tris), pts, np.eye(4), loss, scale, GATE)
    if N >= 63:
        d = np.sqrt(terms[:, 27])
        assert (d == 0.0).any() and len(rows) < finite < N, "the case must hold rows on the surface, beyond the gate, non-finite"
    exact, mass = sf.exact_sum(terms)
    bound = max(len(terms) - 1, 0) * 2.0 ** -52 * mass
    mesh = _lib.Mesh(ctx, verts, tris)
    runs = modes(lambda: surface_fit.fit_to_surface(mesh, pts, loss=loss, scale=scale, gate=GATE, max_iteration=0, trace=True))
    for r in runs:
        err = np.abs(r.packet - exact)
        print(f"F {F} N {N} {loss}: rows {len(terms)}, worst error over bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert (err <= bound).all(), f"entries {np.nonzero(err > bound)[0]}: {err[err > bound]} above {bound[err > bound]}"
        assert r.inliers == len(terms) and r.packet[28] == len(terms) and r.finite_rows == finite
        assert r.iterations == 0 and same(r.transformation, np.eye(4)) and r.trace.shape == (1, 18)
        assert r.fitness == (len(terms) / finite if len(terms) else 0.0)
        assert same_result(r, runs[0]) is None
    mesh.close()


def big_torus_points(n):
    """n points on the dented torus of the shared case, moved like it (more of them than the case holds)."""
    return sf.torus_case(True, n, 11)[2]


@pytest.mark.parametrize("N", [16384, 16385])
def test_modes_memory_and_history_do_not_change_a_bit(ctx, modes, N):
    """Up to 16384 points the culled search runs a wave per point, above a lane per point: T, the statistics and the trace
    are the same bits either way, and in the exhaustive search, from device memory, and after other work on the context."""
    import torch
    from pedp_hip import _lib, surface_fit

    verts, tris = sf.torus_mesh()
    pts = big_torus_points(N)
    mesh = _lib.Mesh(ctx, verts, tris)
    kw = dict(loss="tukey", scale=1.5, gate=10.0, max_iteration=3, trace=True)
    runs = modes(lambda: surface_fit.fit_to_surface(mesh, pts, **kw))
    first = runs[0]
    assert first.iterations == 3 and first.trace.shape == (4, 18) and first.inliers == N and not first.singular
    assert first.trace[-1, 1] < first.trace[0, 1]
    for name, r in zip(("by N", "exhaustive", "a lane per point", "a wave per point"), runs):
        assert same_result(r, first) is None, f"{name}: {same_result(r, first)}"
    dev = surface_fit.fit_to_surface(mesh, torch.from_numpy(pts.copy()).cuda(), **kw)
    assert same_result(dev, first) is None, f"device memory: {same_result(dev, first)}"
    mesh.closest_points(pts[:1000] + 3.0)                                     # unrelated work on the same context
    cloud_a, cloud_b = _lib.Cloud(ctx, pts[:500]), _lib.Cloud(ctx, pts[500:2000])
    _lib.nn(ctx, cloud_a, cloud_b)
    again = surface_fit.fit_to_surface(mesh, pts, **kw)
    assert same_result(again, first) is None, f"after other calls: {same_result(again, first)}"
    cloud_a.close()
    cloud_b.close()
    mesh.close()


def device_fit(ctx, verts, tris, pts, **kw):
    from pedp_hip import _lib, surface_fit

    mesh = _lib.Mesh(ctx, verts, tris)
    try:
        return surface_fit.fit_to_surface(mesh, pts, trace=True, **kw)
    finally:
        mesh.close()


def check_against_reference(got, want, n_finite):
    assert got.iterations == want["iterations"] and len(got.trace) == len(want["trace"])
    assert same(got.trace[:, 0], want["trace"][:, 0]), "fitness per pass"
    assert same(np.rint(got.trace[:, 0] * n_finite), want["trace"][:, 2]), "K per pass"
    assert got.inliers == want["K"] and got.fitness == want["fitness"] and got.singular == want["singular"]
    dT, dr = np.abs(got.transformation - want["T"]).max(), abs(got.inlier_rmse - want["rmse"])
    print(f"against the reference loop: T {dT:.3g} (bound {sf.BOUND_T:.3g}), rmse {dr:.3g} (bound {sf.BOUND_RMSE:.3g})")
    assert dT <= sf.BOUND_T and dr <= sf.BOUND_RMSE


@pytest.fixture(scope="module")
def torus_fits(ctx):
    """The device fits of the four shared torus cases (once for the tests that read them)."""
    out = {}
    for name, case in sf.CASES.items():
        verts, tris, pts, _ = sf.torus_case(case["dent"])
        out[name] = device_fit(ctx, verts, tris, pts, loss=case["loss"], scale=case["scale"], gate=case["gate"])
    return out


@pytest.mark.parametrize("name", sorted(sf.CASES))
def test_torus_cases_against_the_reference_loop(torus_fits, name):
    check_against_reference(torus_fits[name], sf.torus_fit(name), 2000)


def test_soup_against_the_reference_loop(ctx):
    verts, tris, pts = sf.soup_case()
    check_against_reference(device_fit(ctx, verts, tris, pts, **sf.SOUP_FIT), sf.soup_fit(), 3072)


def test_tukey_keeps_the_dent_out_of_the_pose(torus_fits):
    l2, huber, tukey = (sf.pose_errors(torus_fits[k].transformation, sf.MOTION) for k in ("dent_l2", "dent_huber", "dent_tukey"))
    print(f"rotation / translation errors: l2 {l2}, huber {huber}, tukey {tukey}")
    for k in (0, 1):
        assert tukey[k] <= l2[k] / 10.0 and tukey[k] <= huber[k] <= l2[k]
    clean = torus_fits["clean"]
    assert clean.inlier_rmse < 1e-6 * clean.trace[0, 1] and clean.iterations <= 10


# ---------------------------------------------------------------- edges

def test_no_points_no_finite_points_and_none_within_the_gate(ctx):
    import torch
    from pedp_hip import _lib, surface_fit

    verts, tris = sf.torus_mesh()
    mesh = _lib.Mesh(ctx, verts, tris)
    init = sf.rigid([0.01, -0.02, 0.03], [1.0, 2.0, 3.0])
    far = sf.torus_case(False)[2][:300] + np.array([0.0, 0.0, 400.0])
    cases = {"no points": np.zeros((0, 3)), "none finite": np.full((70, 3), np.nan), "none within the gate": far}
    for name, pts in cases.items():
        for p in (pts, torch.from_numpy(pts).cuda()):
            r = surface_fit.fit_to_surface(mesh, p, init=init, loss="l2", gate=5.0, trace=True)
            assert same(r.transformation, init), name
            assert r.fitness == 0.0 and r.inlier_rmse == 0.0 and r.iterations == 0 and r.inliers == 0 and not r.singular, name
            assert r.finite_rows == (300 if name == "none within the gate" else 0)
            assert len(r.trace) == (0 if name == "no points" else 1)
    mesh.close()


def test_one_triangle_is_rank_deficient_and_never_nan(ctx):
    from pedp_hip import _lib, surface_fit

    verts = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]], np.float32)
    tris = np.array([[0, 1, 2]], np.uint32)
    mesh = _lib.Mesh(ctx, verts, tris)
    rng = np.random.default_rng(2)
    inside = np.stack([rng.uniform(1, 4, 90), rng.uniform(1, 4, 90), rng.uniform(0.1, 0.3, 90)], axis=1)     # all above the face
    for pts in (inside, inside[:1], np.zeros((5, 3))):
        for loss, scale in LOSS_SCALE.items():
            r = surface_fit.fit_to_surface(mesh, pts, loss=loss, scale=scale, max_iteration=5, trace=True)
            print(f"{len(pts)} points, {loss}: {r.iterations} updates, singular {r.singular}, rmse {r.inlier_rmse:.3g}")
            assert np.isfinite(r.transformation).all() or r.singular
            for v in (r.transformation, r.trace, r.packet, [r.fitness, r.inlier_rmse, r.weight_sum]):
                assert not np.isnan(v).any()
            assert 0.0 <= r.fitness <= 1.0 and isinstance(r.singular, bool)
    mesh.close()


def test_max_iteration_0_and_init(ctx, torus_fits):
    from pedp_hip import _lib, surface_fit

    verts, tris, pts, _ = sf.torus_case(False)
    mesh = _lib.Mesh(ctx, verts, tris)
    init = sf.rigid([0.004, -0.003, 0.005], [0.2, -0.1, 0.15])
    zero = surface_fit.fit_to_surface(mesh, pts, init=init, loss="l2", max_iteration=0)
    assert same(zero.transformation, init) and zero.iterations == 0 and zero.trace is None
    moved = np.ascontiguousarray(pts @ init[:3, :3].T + init[:3, 3])
    first = surface_fit.fit_to_surface(mesh, moved, loss="l2", max_iteration=0)
    assert zero.fitness == first.fitness == 1.0 and abs(zero.inlier_rmse - first.inlier_rmse) <= sf.BOUND_RMSE
    one = torus_fits["clean"]
    assert surface_fit.fit_to_surface(mesh, pts, loss="l2", max_iteration=0).inlier_rmse == one.trace[0, 1]
    # a start value is honoured: the fit from `init` is the fit of the pre-moved points, composed with init
    a = surface_fit.fit_to_surface(mesh, pts, init=init, loss="l2")
    b = surface_fit.fit_to_surface(mesh, moved, loss="l2")
    assert a.iterations == b.iterations and a.inliers == b.inliers == 2000
    dT = np.abs(a.transformation - b.transformation @ init).max()
    print(f"init against pre-moved points: T {dT:.3g} (bound {sf.BOUND_T:.3g})")
    assert dT <= sf.BOUND_T and abs(a.inlier_rmse - b.inlier_rmse) <= sf.BOUND_RMSE
    assert np.abs(a.transformation - one.transformation).max() <= sf.BOUND_T
    mesh.close()


def test_refusals(ctx):
    from pedp_hip import _lib, surface_fit, synth

    verts, tris, pts, _ = sf.torus_case(False)
    mesh = _lib.Mesh(ctx, verts, tris)
    with pytest.raises(_lib.PedpError, match="scale"):
        surface_fit.fit_to_surface(mesh, pts, loss="tukey")
    with pytest.raises(_lib.PedpError, match="gate"):
        surface_fit.fit_to_surface(mesh, pts, loss="l2", gate=-1.0)
    lib = _lib.load()
    T = np.empty(16)

    def raw(c=ctx, loss=2, scale=1.5, gate=10.0, iters=3, n=len(pts)):
        return lib.pedp_fit_to_surface(c._h, mesh._h, _lib._ptr(pts), n, _lib.HOST, None, loss, scale, gate, iters, 1e-6, 1e-6,
                                       _lib._ptr(T), None, None)

    assert raw() == 0
    for bad, word in ((dict(loss=3), b"loss"), (dict(scale=0.0), b"scale"), (dict(loss=1, scale=-1.0), b"scale"),
                      (dict(gate=-0.5), b"gate"), (dict(gate=float("nan")), b"gate"), (dict(iters=-1), b"max_iteration"),
                      (dict(n=(1 << 24) + 1), b"at most")):
        assert raw(**bad) == -1 and word in lib.pedp_last_error(), bad                    # PEDP_ERR_BAD_ARG
    assert raw(loss=0, scale=0.0) == 0                                                    # l2 needs no scale
    other = _lib.Context(0)
    assert raw(c=other) == -1 and b"another context" in lib.pedp_last_error()
    with pytest.raises(_lib.PedpError, match="another context"):
        surface_fit.fit_to_surface(mesh, pts, loss="l2", ctx=other)
    other.close()
    f = synth.Frame("tiny")
    cast = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(cast.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    kw = dict(max_iteration=6, relative_fitness=-1, relative_rmse=-1)
    want = _lib.icp(ctx, src, tgt, 10.0, f.icp_init(), **kw)
    _lib.icp_begin(ctx, src, tgt, 10.0, f.icp_init(), **kw)
    try:
        with pytest.raises(_lib.PedpError, match="pending"):
            surface_fit.fit_to_surface(mesh, pts, loss="l2")
    finally:
        got = _lib.icp_end(ctx)
    assert same(got["T"], want["T"])
    assert surface_fit.fit_to_surface(mesh, pts, loss="l2").inliers == 2000
    for h in (src, tgt, cast, mesh):
        h.close()


# ---------------------------------------------------------------- composition

def test_frame_fit_and_refit_pose(ctx):
    """A 48 x 40 depth frame of the torus at the true pose, the mesh posed a little off it: fit_frame_to_surface fits the
    points deviation_heatmap would test, and the pose it implies brings the mean deviation down."""
    from pedp_hip import _lib, surface_distance as sd, surface_fit, synth
    from pedp_hip.depth_filters import depth2xyzmap

    f = synth.Frame("tiny")
    assert (f.width, f.height) == (48, 40)
    verts, tris, _ = synth.bumpy_torus(50, 40)
    truth = _lib.Mesh(ctx, synth.posed_vertices(verts, f.T_gt), tris)
    t_hit = truth.cast_rays(f.rays6, want_uv=False)["t_hit"]
    depth = np.where(np.isfinite(t_hit), t_hit * f.dirs[:, 2] / 1000.0, 0.0).astype(np.float32).reshape(f.height, f.width)
    valid = depth >= 0.001
    assert 200 < valid.sum() < valid.size - 200
    off = sf.rigid([0.01, -0.015, 0.008], [0.6, -0.4, 0.5]) @ f.T_gt
    posable = _lib.Mesh(ctx, verts.astype(np.float64), tris, posable=True)
    posable.set_pose(off)
    mask = np.ones_like(valid)
    mask[:, :3] = False
    keep = valid & mask
    kw = dict(loss="tukey", scale=5.0, gate=20.0, trace=True)
    got = surface_fit.fit_frame_to_surface(depth, f.K, posable, mask=mask, **kw)
    xyz = depth2xyzmap(depth, f.K).astype(np.float64) * 1000.0
    want = surface_fit.fit_to_surface(posable, np.ascontiguousarray(xyz[keep]), **kw)
    assert same_result(got, want) is None and got.inliers == got.finite_rows == keep.sum() and got.iterations >= 2
    holes = np.where(keep[..., None], xyz, np.nan)                  # the same rows at other indices: another order of the sums
    padded = surface_fit.fit_to_surface(posable, holes, **kw)
    assert padded.iterations == got.iterations and padded.inliers == got.inliers and padded.finite_rows == got.finite_rows
    assert np.abs(padded.transformation - got.transformation).max() <= sf.BOUND_T
    saturation, gate = 1.0, 20.0
    before = sd.deviation_heatmap(depth, f.K, posable, saturation, gate)
    pose = surface_fit.refit_pose(off, got)
    posable.set_pose(pose)
    after = sd.deviation_heatmap(depth, f.K, posable, saturation, gate)
    print(f"mean deviation over the valid pixels: {before[valid].mean():.4g} before the fit, {after[valid].mean():.4g} after")
    assert after[valid].mean() < before[valid].mean()
    rot0, tr0 = sf.pose_errors(off, f.T_gt)
    rot, tr = sf.pose_errors(pose, f.T_gt)
    print(f"pose error: {rot0:.3g} deg, {tr0:.3g} before, {rot:.3g} deg, {tr:.3g} after")
    assert rot < rot0 and tr < tr0
    truth.close()
    posable.close()
