"""The surface sampler (pedp_sample.hip) on the device against tests/_sample_ref.py's numpy restatement:
every comparison of points, face ids, barycentrics, normals, kept indices and r* is bit equality.  Then the two guarantees
of the thinning on the device's output alone, and what the feature is for: a cloud that lies on its mesh, maps back to CAD
faces, and serves as an ICP target."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import _sample_ref as S

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def assert_is_ref(got, ref, normals=True):
    assert same_bits(got.points, ref["points"])
    assert same_bits(host(got.face_ids), ref["face_ids"])
    assert same_bits(host(got.barycentric), ref["barycentric"])
    if ref["normals"] is None:
        assert not got.has_normals()
    elif normals:
        assert same_bits(got.normals, ref["normals"])


def check_uniform(ctx, v, t, n, seed=0, first=0, mesh=None, use_triangle_normal=False):
    from pedp_hip.mesh_sample import sample_points_uniformly

    got = sample_points_uniformly(mesh if mesh is not None else (v, t), n, use_triangle_normal, seed=seed, first=first, ctx=ctx)
    vn = mesh.vertex_normals if mesh is not None and mesh.has_vertex_normals() else None
    mode = S.NORMALS_TRIANGLE if use_triangle_normal else (S.NORMALS_VERTEX if vn is not None else S.NORMALS_NONE)
    assert_is_ref(got, S.sample(v, t, n, seed, first, mode, vn))
    assert len(got) == n
    return got


@pytest.fixture(scope="module")
def fine_cube():
    """The unit cube refined to 12,288 faces."""
    v, t = S.cube()
    rv, rt, _, _ = S.refine(v, t, 0.05)
    assert len(rt) == 12288
    return rv, rt


@pytest.fixture(scope="module")
def cube_cloud():
    """20,000 samples of the unit cube, seed 0, with their keys."""
    v, t = S.cube()
    s = S.sample(v, t, 20000, seed=0)
    return s["points"], S.keys(s["z"])


# ---------------------------------------------------------------- sampling against the restatement
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_one_triangle(ctx, n):
    v, t = S.one_triangle()
    got = check_uniform(ctx, v, t, n)
    assert (host(got.face_ids) == 0).all()


def test_two_triangles_of_areas_1_to_3(ctx):
    v, t = S.two_triangles_1_3()
    got = check_uniform(ctx, v, t, 4096)
    share = (host(got.face_ids) == 1).mean()
    assert abs(share - 0.75) < 4 * np.sqrt(0.75 * 0.25 / 4096)


@pytest.mark.parametrize("faces", [8, 257])
def test_equal_areas(ctx, faces):
    v, t = S.strip(faces)
    assert len(set(S.face_table(v, t)[2])) == 1          # every C[f] is a multiple of 2^32: t == C[f] is met at word boundaries
    got = check_uniform(ctx, v, t, 3000, seed=1)
    assert len(np.unique(host(got.face_ids))) == faces


def test_faces_without_weight_are_never_chosen_and_are_counted(ctx):
    from pedp_hip.mesh_sample import MeshSampler

    v, t = S.with_dead_faces()
    got = check_uniform(ctx, v, t, 5000, seed=3)
    assert set(np.unique(host(got.face_ids))) == {0, 2}
    with MeshSampler((v, t), ctx) as s:
        area, amax, _, _, total, a_sum = S.face_table(v, t)
        assert s.unsampled_faces == 2 and s.n_faces == 4 and s.total_weight == total == 2 ** 33
        assert s.area == a_sum and s.largest_area == amax and not s.has_vertex_normals


def test_icosphere_and_the_refined_cube(ctx, fine_cube):
    v, t = S.icosphere(2)
    assert len(t) == 320
    check_uniform(ctx, v, t, 4000, seed=2)
    rv, rt = fine_cube
    got = check_uniform(ctx, rv, rt, 30000, seed=0)
    assert len(np.unique(host(got.face_ids))) > 10000


def test_counter_carry(ctx):
    v, t = S.cube()
    check_uniform(ctx, v, t, 20, seed=5, first=2 ** 32 - 10)
    check_uniform(ctx, v, t, 4, seed=5, first=2 ** 64 - 2)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
def test_seeds(ctx, seed):
    v, t = S.icosphere(1)
    check_uniform(ctx, v, t, 777, seed=seed)


def test_a_slice_is_a_slice(ctx):
    v, t = S.cube()
    whole, part = check_uniform(ctx, v, t, 150, seed=7), check_uniform(ctx, v, t, 50, seed=7, first=100)
    assert same_bits(part.points, whole.points[100:150])


@pytest.mark.parametrize("use_triangle_normal", [False, True], ids=["vertex", "triangle"])
def test_normals(ctx, use_triangle_normal):
    from pedp_hip.geometry import TriangleMesh

    v, t = S.icosphere(2)
    mesh = TriangleMesh(v, t)
    mesh.vertex_normals = S.vertex_normals(v, t)
    got = check_uniform(ctx, v, t, 2000, seed=4, mesh=mesh, use_triangle_normal=use_triangle_normal)
    assert got.has_normals() and (np.einsum("ij,ij->i", got.normals, got.points) > 0).all()
    if use_triangle_normal:
        assert np.abs(np.linalg.norm(got.normals, axis=1) - 1.0).max() < 1e-15


def test_numpy_input_against_cuda_tensor_input(ctx):
    import torch
    from pedp_hip.geometry import TriangleMesh
    from pedp_hip.mesh_sample import sample_points_poisson_disk, sample_points_uniformly

    v, t = S.icosphere(2)
    tv, tt = torch.from_numpy(v).cuda(), torch.from_numpy(t.astype(np.int32)).cuda()
    ref = S.sample(v, t, 1500, 6, 0, S.NORMALS_TRIANGLE)
    got = sample_points_uniformly((tv, tt), 1500, True, seed=6)
    assert got.device_points.is_cuda and got.face_ids.is_cuda and got.barycentric.is_cuda and got.device_normals.is_cuda
    assert_is_ref(got, ref)
    assert same_bits(got.device_points.cpu().numpy(), ref["points"]) and same_bits(got.device_normals.cpu().numpy(), ref["normals"])
    disk, want = sample_points_poisson_disk((tv, tt), 200, seed=6), S.sample_disk(v, t, 200, seed=6)
    assert disk.index.is_cuda and same_bits(host(disk.index), want["index"]) and disk.spacing == want["spacing"]
    assert_is_ref(disk, want)
    on_host = TriangleMesh(v, t).sample_points_poisson_disk(200, seed=6, ctx=ctx)
    assert same_bits(on_host.points, disk.points) and same_bits(on_host.index, host(disk.index))


# ---------------------------------------------------------------- thinning
def guarantees(p, kept, r):
    """On the output alone: no two kept points are closer than r, every point is closer than r to a kept one."""
    p, q = np.asarray(p, np.float64), np.asarray(p, np.float64)[kept]
    if len(p) == 0:
        return
    assert len(q) > 0
    if r * r > 0.0:
        pairs = cKDTree(q).query_pairs(r * (1 + 1e-6), output_type="ndarray").reshape(-1, 2)
        assert not (S._dist2(q[pairs[:, 0]], q[pairs[:, 1]]) < r * r).any()
        near = cKDTree(q).query(p)[1]
        assert (S._dist2(p, q[near]) < r * r).all()
    else:
        assert len(q) == len(p)


def check_thin(ctx, p, r, seed=0):
    from pedp_hip.mesh_sample import thin_to_spacing

    got = thin_to_spacing(p, r, seed=seed, ctx=ctx)
    want = np.flatnonzero(S.thin(p, S.cloud_keys(len(p), seed), r)).astype(np.int32)
    assert same_bits(got, want)
    guarantees(p, got, r)
    return got


def test_thin_nothing_and_one_point(ctx):
    assert len(check_thin(ctx, np.zeros((0, 3)), 1.0)) == 0
    assert list(check_thin(ctx, np.array([[1.0, 2.0, 3.0]]), 1.0)) == [0]
    assert list(check_thin(ctx, np.array([[1.0, 2.0, 3.0]]), 0.0)) == [0]


def test_thin_identical_points_keeps_the_lowest_key(ctx):
    got = check_thin(ctx, np.full((300, 3), 0.25), 1e-3, seed=5)
    assert list(got) == [int(np.argmin(S.cloud_keys(300, 5)))]


def test_thin_comparison_is_strict(ctx):
    p = np.array([[0, 0, 0], [3, 4, 0]], np.float64)
    assert len(check_thin(ctx, p, 5.0)) == 2
    assert len(check_thin(ctx, p, np.nextafter(5.0, np.inf))) == 1


@pytest.mark.parametrize("r", [1.0, 1.0000001])
def test_thin_unit_lattice(ctx, r):
    g = np.arange(8, dtype=np.float64)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    got = check_thin(ctx, p, r)
    assert (len(got) == 512) == (r == 1.0)


def test_thin_collinear_points_in_order(ctx):
    r = 0.1
    p = np.stack([np.arange(500) * 0.6 * r, np.zeros(500), np.zeros(500)], axis=1)
    got = check_thin(ctx, p, r)
    assert 250 > len(got) > 166


def test_thin_far_from_the_origin_and_across_cell_faces(ctx):
    rng = np.random.default_rng(11)
    p = rng.uniform(-1.0, 1.0, (3000, 3))
    check_thin(ctx, p, 0.2)                                       # straddles zero
    check_thin(ctx, p + np.array([1e6, -1e6, 1e6]), 0.2, seed=1)
    q = np.round(p / 0.2) * 0.2 + rng.choice([-1e-12, 0.0, 1e-12], (3000, 3))      # on and next to multiples of the spacing
    check_thin(ctx, q, 0.2, seed=2)


def test_thin_a_crowded_cell(ctx):
    rng = np.random.default_rng(12)
    r = 0.1
    d = rng.normal(size=(5000, 3))
    ball = d / np.linalg.norm(d, axis=1, keepdims=True) * (rng.uniform(size=(5000, 1)) ** (1 / 3)) * (r / 4) + 0.5
    p = np.vstack([ball, rng.uniform(0, 1, (2000, 3))])[rng.permutation(7000)]
    check_thin(ctx, p, r)


def test_thin_spacing_beyond_the_box_and_below_the_cell_cap(ctx):
    rng = np.random.default_rng(13)
    p = rng.uniform(0, 1, (2000, 3))
    assert len(check_thin(ctx, p, 10.0)) == 1
    assert len(check_thin(ctx, p, 1e-12)) == 2000
    assert len(check_thin(ctx, p, 0.0)) == 2000
    assert len(check_thin(ctx, p, 1e-200)) == 2000                # r * r underflows to 0: nothing conflicts


def test_thin_cube_samples(ctx, cube_cloud):
    """20,000 samples of the unit cube at r = 0.05 under their own keys (the spacing form's thinning): 1,365 stay."""
    from pedp_hip.mesh_sample import MeshSampler

    p, key = cube_cloud
    want = np.flatnonzero(S.thin(p, key, 0.05))
    assert len(want) == 1365
    guarantees(p, want, 0.05)
    check_thin(ctx, p, 0.05, seed=3)                              # the same cloud under hashed keys
    v, t = S.cube()
    with MeshSampler((v, t), ctx) as s:                           # M = ceil(5 * 6 / r^2) = 20,000 at this spacing
        r = np.sqrt(30.0 / 20000.0)
        got = s.sample_disk(spacing=r)
        assert got.drawn == 20000
        assert same_bits(got.index, np.flatnonzero(S.thin(p, key, r)).astype(np.int32))
        print(f"spacing {r:.5f}: kept {len(got)} of {got.drawn} in {got.rounds} rounds")


# ---------------------------------------------------------------- the disk forms
@pytest.mark.parametrize("n", [100, 500])
def test_count_form(ctx, n):
    from pedp_hip.geometry import TriangleMesh

    v, t = S.cube()
    got, want = TriangleMesh(v, t).sample_points_poisson_disk(n, ctx=ctx), S.sample_disk(v, t, n)
    print(f"N = {n}: r* = {got.spacing!r} = {got.spacing / np.sqrt(6.0 / n):.4f} sqrt(A / N), {got.probes} thinnings, the last in {got.rounds} rounds")
    assert len(got) == n and got.drawn == 5 * n
    assert got.spacing == want["spacing"] and same_bits(got.index, want["index"])
    assert_is_ref(got, want)
    pairs = cKDTree(got.points).query_pairs(got.spacing * (1 + 1e-6), output_type="ndarray").reshape(-1, 2)
    assert not (S._dist2(got.points[pairs[:, 0]], got.points[pairs[:, 1]]) < got.spacing * got.spacing).any()


def test_spacing_form(ctx):
    from pedp_hip.geometry import TriangleMesh

    v, t = S.cube()
    mesh = TriangleMesh(v, t)
    mesh.vertex_normals = S.vertex_normals(v, t)
    got = mesh.sample_points_poisson_disk(spacing=0.05, seed=2, ctx=ctx)
    want = S.sample_disk(v, t, spacing=0.05, seed=2, normals=S.NORMALS_VERTEX, vertex_normals=mesh.vertex_normals)
    assert got.drawn == want["drawn"] == 12000 and got.spacing == 0.05
    assert same_bits(got.index, want["index"])
    assert_is_ref(got, want)
    drawn = S.sample(v, t, 12000, seed=2)["points"]
    guarantees(drawn, got.index, 0.05)
    # the point recomputed from the returned ids and barycentrics
    tri, b = v[t.astype(np.int64)[got.face_ids]], got.barycentric
    assert same_bits(got.points, (b[:, :1] * tri[:, 0] + b[:, 1:2] * tri[:, 1]) + b[:, 2:] * tri[:, 2])


def test_pcl_form(ctx):
    from pedp_hip.geometry import PointCloud, TriangleMesh

    v, t = S.cube()
    s = S.sample(v, t, 3000, seed=9, normals=S.NORMALS_TRIANGLE)
    pcl = PointCloud(s["points"], s["normals"])
    got = TriangleMesh(v, t).sample_points_poisson_disk(300, pcl=pcl, seed=1, ctx=ctx)
    idx, r = S.thin_to_count(s["points"], S.cloud_keys(3000, 1), 300, 2.0 * np.sqrt(S.face_table(v, t)[5] / 300))
    assert got.spacing == r and same_bits(got.index, idx)
    assert same_bits(got.points, s["points"][idx]) and same_bits(got.normals, s["normals"][idx])
    at = TriangleMesh(v, t).sample_points_poisson_disk(spacing=0.07, pcl=s["points"], seed=1, ctx=ctx)
    assert same_bits(at.index, np.flatnonzero(S.thin(s["points"], S.cloud_keys(3000, 1), 0.07)).astype(np.int32))


# ---------------------------------------------------------------- use
def test_samples_lie_on_their_mesh(ctx):
    """Vertices on a 2^-12 grid: the mesh handle's float32 records (a vertex and two edge vectors) then hold the float64
    mesh exactly, and the distance of a sample to it is the rounding of its own three products."""
    from pedp_hip.geometry import TriangleMesh
    from pedp_hip.surface_distance import compute_distance

    v, t = S.icosphere(2)
    v = np.round(v * 4096.0) / 4096.0
    mesh = TriangleMesh(v, t)
    got = mesh.sample_points_uniformly(3000, seed=1, ctx=ctx)
    d = compute_distance(mesh, got.points, ctx=ctx)
    print(f"largest distance of a sample to its mesh: {d.max():.3e}")
    assert d.max() <= 1e-12 * 2.0


def test_parent_of_maps_samples_back_to_cad_faces(ctx):
    from pedp_hip.mesh_refine import refine_mesh

    v, t = S.cube()
    same = refine_mesh((v, t), 10.0, ctx=ctx)
    assert same.rounds == 0
    got = same.sample_points_uniformly(2000, seed=8, ctx=ctx)
    assert same_bits(same.parent_of(got.face_ids), S.sample(v, t, 2000, seed=8)["face_ids"])
    fine = refine_mesh((v, t), 0.3, ctx=ctx)
    disk = fine.sample_points_poisson_disk(300, seed=8, ctx=ctx)
    cad = fine.parent_of(disk.face_ids)
    assert len(disk) == 300 and set(np.unique(cad)) == set(range(12))
    n = np.cross(v[t[:, 1].astype(int)] - v[t[:, 0].astype(int)], v[t[:, 2].astype(int)] - v[t[:, 0].astype(int)])
    assert np.abs(np.einsum("ij,ij->i", disk.points - v[t[cad, 0].astype(int)], n[cad])).max() < 1e-15    # in the CAD face's plane


def test_a_sampled_cloud_is_an_icp_target(ctx):
    """Target: 2,000 evenly spaced samples with the faces' normals; source: another sampling (seed + 1) moved by 2 mm and
    1 degree.  On the six separated squares every source point pairs with a target point of its own plane, whose normal is
    exact, so the known motion is a fixed point of point-to-plane ICP and is recovered to test_icp_gpu.py's 1e-8."""
    from pedp_hip import synth
    from pedp_hip.geometry import PointCloud, TriangleMesh
    from pedp_hip.registration import ICPConvergenceCriteria, TransformationEstimationPointToPlane, registration_icp

    v, t = S.separated_squares()
    mesh = TriangleMesh(v, t)
    target = mesh.sample_points_poisson_disk(2000, use_triangle_normal=True, seed=3, ctx=ctx)
    source = mesh.sample_points_poisson_disk(700, seed=4, ctx=ctx)
    assert target.has_normals() and target.spacing < 5.0
    M = np.eye(4)
    M[:3, :3] = synth.axis_angle([0.3, -1.0, 0.5], np.deg2rad(1.0))
    M[:3, 3] = [1.2, -1.0, 1.2]
    moved = PointCloud(source.points @ M[:3, :3].T + M[:3, 3])
    res = registration_icp(moved, target, 5.0, np.eye(4), TransformationEstimationPointToPlane(),
                           ICPConvergenceCriteria(1e-12, 1e-12, 60), ctx=ctx)
    print(f"fitness {res.fitness:.4f}, largest pose error {np.abs(res.transformation - np.linalg.inv(M)).max():.2e}")
    assert res.fitness > 0.99
    assert np.abs(res.transformation - np.linalg.inv(M)).max() < 1e-8


def test_mesh_to_pcd(ctx):
    from pedp_hip.compat import mesh_to_pcd
    from pedp_hip.geometry import TriangleMesh

    v, t = S.cube(0.0, 10.0)
    pcd = mesh_to_pcd(TriangleMesh(v, t), {"mesh": {"number_of_points": 400}})
    assert len(pcd) == 400 and pcd.has_normals() and same_bits(pcd.points, S.sample_disk(v, t, 400)["points"])
    assert np.abs(np.linalg.norm(pcd.normals, axis=1) - 1.0).max() < 1e-9


# ---------------------------------------------------------------- errors
def test_errors_name_the_argument(ctx):
    from pedp_hip import PedpError
    from pedp_hip.geometry import TriangleMesh
    from pedp_hip.mesh_sample import sample_points_poisson_disk, sample_points_uniformly, thin_to_spacing

    v, t = S.cube()
    mesh = TriangleMesh(v, t)
    bad_v = v.copy()
    bad_v[5, 1] = np.inf
    bad_t = t.copy()
    bad_t[7, 2] = 8
    flat = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [1, 1, 1]], np.float64), np.array([[0, 1, 2], [0, 0, 3]], np.uint32)
    for call, word in [(lambda: sample_points_uniformly(mesh, 0, ctx=ctx), "number_of_points"),
                       (lambda: sample_points_poisson_disk(mesh, 0, ctx=ctx), "number_of_points"),
                       (lambda: sample_points_poisson_disk(mesh, ctx=ctx), "number_of_points or spacing"),
                       (lambda: sample_points_poisson_disk(mesh, 10, spacing=0.1, ctx=ctx), "number_of_points or spacing"),
                       (lambda: sample_points_poisson_disk(mesh, 10, init_factor=0, ctx=ctx), "init_factor"),
                       (lambda: sample_points_poisson_disk(mesh, spacing=-1.0, ctx=ctx), "spacing"),
                       (lambda: sample_points_poisson_disk(mesh, spacing=float("nan"), ctx=ctx), "spacing"),
                       (lambda: sample_points_poisson_disk(mesh, 10, pcl=np.zeros((5, 3)), ctx=ctx), "number_of_points"),
                       (lambda: thin_to_spacing(np.zeros((3, 3)), -1.0, ctx=ctx), "spacing"),
                       (lambda: thin_to_spacing(np.zeros((3, 3)), float("nan"), ctx=ctx), "spacing"),
                       (lambda: thin_to_spacing(np.array([[0, 0, np.nan]]), 1.0, ctx=ctx), "points"),
                       (lambda: sample_points_uniformly((bad_v, t), 10, ctx=ctx), "vertices"),
                       (lambda: sample_points_uniformly((v, bad_t), 10, ctx=ctx), "triangles"),
                       (lambda: sample_points_uniformly(flat, 10, ctx=ctx), "triangles"),
                       (lambda: sample_points_uniformly((v, t[:0]), 10, ctx=ctx), "triangles")]:
        with pytest.raises(PedpError, match=word):
            call()
    assert len(sample_points_uniformly(mesh, 10, ctx=ctx)) == 10      # the context still serves after the refusals
