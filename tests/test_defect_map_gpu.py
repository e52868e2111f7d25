"""The defect map on the device (csrc/pedp_defectmap.hip) against its restatement
(tests/_defect_map_ref.py): bit for bit, except the two floating-point sums, which are held to the bound of any
summation order and to repeatability."""
import ctypes as C
import functools

import numpy as np
import pytest

import _defect_map_ref as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MESHES = {
    "single": lambda: (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]), np.array([[0, 1, 2]], dtype=np.uint32)),
    "cube": ref.cube,
    "torus16": lambda: ref.torus(4, 2),
    "torus1022": lambda: ref.torus(73, 7),
    "torus16000": lambda: ref.torus(100, 80),
    "seam16000": lambda: ref.torus_with_seam(100, 80),
    "fin": ref.fin,
    "two_tori": lambda: ref.two_tori(50, 40),
    "strip4096": lambda: ref.strip(4096),
    "oddities": ref.oddities,
}


@functools.lru_cache(maxsize=None)
def model(name):
    return ref.Model(*MESHES[name]())


_maps = {}


@pytest.fixture
def dmap(ctx):
    """name -> the (cleared) DefectMap of that mesh on the session's context, built once."""
    from pedp_hip import DefectMap

    def get(name):
        if name not in _maps:
            m = model(name)
            _maps[name] = DefectMap((m.verts, m.tris), ctx)
        _maps[name].clear()
        return _maps[name]

    return get


def same_faces(got, want):
    assert ref.same_bits(got["peak"], want["peak"]), "peak"
    assert np.array_equal(got["hits"], want["hits"]) and got["hits"].dtype == np.int64, "hits"
    assert np.array_equal(got["frames"], want["frames"]) and got["frames"].dtype == np.int32, "frames"


def same_regions(got, want):
    assert got["n_regions"] == want["n_regions"]
    assert np.array_equal(got["labels"], want["labels"])
    for k in ref.INT_COLUMNS:
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    for k in ref.BIT_COLUMNS:
        assert ref.same_bits(got[k], want[k]), k
    n = want["n_faces"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        err_a = np.abs(got["area"] - want["area"])
        err_m = np.abs(got["moment"] - want["moment"])
        assert np.array_equal(np.isnan(got["area"]), np.isnan(want["area"]))
        assert np.array_equal(np.isnan(got["moment"]), np.isnan(want["moment"]))
        ok_a, ok_m = ~np.isnan(want["area"]), ~np.isnan(want["moment"])
        assert (err_a[ok_a] <= (n * EPS * want["area"])[ok_a]).all(), "area beyond n_faces 2^-52 of fsum"
        assert (err_m[ok_m] <= (n[:, None] * EPS * want["abs_moment"])[ok_m]).all(), "moment beyond n_faces 2^-52 sum |area c|"
        quotient = got["moment"] / got["area"][:, None]
        quotient[~(got["area"] > 0) & ~np.isnan(got["area"])] = np.nan
    assert np.array_equal(got["centroid"], quotient, equal_nan=True)


def same_table_bits(a, b):
    from pedp_hip.defect_map import REGION_DTYPE

    assert a["n_regions"] == b["n_regions"] and np.array_equal(a["labels"], b["labels"])
    for k in REGION_DTYPE.names:
        assert ref.same_bits(a[k], b[k]), k


# ------------------------------------------------------------------ the model: adjacency
@pytest.mark.parametrize("name", sorted(MESHES))
def test_adjacency(dmap, name):
    m, dm = model(name), dmap(name)
    assert (dm.V, dm.F) == (len(m.verts), m.F)
    dm.add(np.arange(m.F, dtype=np.uint32), np.ones(m.F))
    st = ref.State(m.F).add(np.arange(m.F), np.ones(m.F))
    same_regions(dm.regions(), ref.regions(m, st))
    faces = np.arange(m.F) if m.F <= 1100 else np.sort(np.random.default_rng(1).choice(m.F, 256, replace=False))
    if name == "seam16000":                          # and every face with a neighbour that the weld alone gives it
        raw = ref.Model(m.verts, m.tris, welded=False)
        across = np.array([f for f in range(m.F) if len(m.neighbours[f]) > len(raw.neighbours[f])])
        assert len(across) == 160 and all(len(raw.neighbours[f]) == 2 for f in across)
        faces = np.union1d(faces, across)
    for f in faces:                                  # one marked face grown once: the face and its neighbours
        dm.clear()
        dm.add(np.array([f], dtype=np.uint32), np.ones(1))
        got = dm.regions(grow=1, capacity=0)
        assert got["n_regions"] == 1
        assert np.array_equal(np.nonzero(got["labels"] == 0)[0], np.sort(np.append(m.neighbours[f], f))), f
        assert (got["labels"][got["labels"] != 0] == -1).all()


def test_geometry_columns_of_single_faces(dmap):
    """Every face of the mesh with the oddities as a region of its own: area, moment, centroid and box are the face's."""
    m, dm = model("oddities"), dmap("oddities")
    for f in range(m.F):
        dm.clear()
        dm.add(np.array([f]), np.ones(1))
        got = dm.regions()
        assert got["n_regions"] == 1 and got["first_face"][0] == f
        assert np.array_equal(got["area"], m.area[f:f + 1], equal_nan=True)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got["moment"][0], m.area[f] * m.centroid[f], equal_nan=True)
        same_regions(got, ref.regions(m, ref.State(m.F).add([f], [1.0])))


def test_a_map_without_faces(ctx):
    from pedp_hip import DefectMap

    dm = DefectMap((np.zeros((3, 3)), np.zeros((0, 3), np.uint32)), ctx)
    dm.add(np.array([0, ref.MISS], dtype=np.uint32), np.ones(2))
    assert dm.stats() == {"observations": 1, "rows_added": 0, "rows_ignored": 2}
    assert dm.faces()["peak"].shape == (0,) and dm.regions()["n_regions"] == 0 and dm.face_colors().shape == (0, 3)
    dm.close()


def test_create_refuses_an_index_beyond_the_vertices(ctx):
    from pedp_hip import _lib

    v, t = ref.cube()
    t = t.copy()
    t[5, 1] = 8
    h = C.c_void_p()
    assert _lib.load().pedp_defect_map_create(ctx._h, _lib._ptr(v), 8, _lib._ptr(t), 12, C.byref(h)) == -1
    assert b"names vertex 8" in _lib.load().pedp_last_error() and not h.value


# ------------------------------------------------------------------ add
def rows(F, n, seed):
    """n rows on F faces: misses, ids beyond F, NaN, negative intensities and both zeros among them."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, F, n).astype(np.uint32)
    x = rng.uniform(-1.0, 1.0, n)
    if n >= 63:
        ids[rng.choice(n, n // 16, replace=False)] = ref.MISS
        ids[rng.choice(n, n // 16, replace=False)] = rng.integers(F, 2 ** 32 - 1, n // 16)
        x[rng.choice(n, n // 16, replace=False)] = np.nan
        x[rng.choice(n, n // 8, replace=False)] = rng.choice([0.0, -0.0], n // 8)
        ids[rng.choice(n, n // 8, replace=False)] = ids[0]          # a face with many rows
    return ids, x


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 100000])
def test_add(dmap, n):
    m, dm = model("torus16000"), dmap("torus16000")
    ids, x = rows(m.F, n, n)
    dm.add(ids, x)
    st = ref.State(m.F).add(ids, x)
    first = dm.faces()
    same_faces(first, st.faces())
    assert dm.stats() == st.stats() and st.stats()["observations"] == 1
    ids2, x2 = rows(m.F, max(n // 2, 1), n + 1000)                   # a second observation
    dm.add(ids2, x2)
    st.add(ids2, x2)
    two = dm.faces()
    same_faces(two, st.faces())
    assert dm.stats() == st.stats() and (two["frames"] <= 2).all()
    # the same rows in another order, and the ids as int64 / int32, give the same bits
    p = np.random.default_rng(7).permutation(n)
    dm.clear()
    dm.add(ids[p].astype(np.int64), x[p])
    dm.add(ids2.view(np.int32), x2)
    same_faces(dm.faces(), two)
    assert dm.stats() == st.stats()
    # clear, then add: a fresh map
    dm.clear()
    assert dm.stats() == {"observations": 0, "rows_added": 0, "rows_ignored": 0} and not dm.faces()["hits"].any()
    dm.add(ids, x)
    same_faces(dm.faces(), first)


def test_all_rows_on_one_face_and_the_zeros(dmap):
    m, dm = model("torus16000"), dmap("torus16000")
    n = 20000
    x = np.random.default_rng(3).uniform(-2.0, -1.0, n)
    dm.add(np.full(n, 4321, np.uint32), x)
    f = dm.faces()
    assert f["hits"][4321] == n and f["frames"][4321] == 1 and f["peak"][4321] == x.max() and f["hits"].sum() == n
    for pair in ([0.0, -0.0], [-0.0, 0.0]):                         # +0 is above -0 whatever the order
        dm.clear()
        dm.add(np.array([7, 7, 9], np.uint32), np.array(pair + [-0.0]))
        assert ref.same_bits(dm.faces()["peak"][[7, 9]], np.array([0.0, -0.0]))


def test_runs_of_equal_neighbouring_ids(dmap):
    """Rows in pixel order carry runs of one face; the kernel sends a run inside a wave through its first lane.  Runs of
    1 ... 200 rows that start at every lane offset and cross the wave and block boundaries, with ignored rows inside
    them and the same face again after another one."""
    m, dm = model("torus16000"), dmap("torus16000")
    rng = np.random.default_rng(17)
    lengths = np.concatenate([[1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257], rng.integers(1, 70, 300)])
    faces = rng.integers(0, 50, len(lengths))                        # few faces: the same face comes back in later runs
    ids = np.repeat(faces, lengths).astype(np.uint32)
    x = rng.uniform(-1.0, 1.0, len(ids))
    holes = rng.choice(len(ids), len(ids) // 10, replace=False)
    x[holes[::2]] = np.nan
    ids[holes[1::2]] = ref.MISS
    dm.add(ids, x)
    st = ref.State(m.F).add(ids, x)
    same_faces(dm.faces(), st.faces())
    assert dm.stats() == st.stats()
    dm.add(ids[::-1].copy(), x[::-1].copy())
    st.add(ids[::-1], x[::-1])
    same_faces(dm.faces(), st.faces())


def test_an_observation_split_in_two_differs_in_frames_alone(dmap):
    m, dm = model("torus16000"), dmap("torus16000")
    ids, x = rows(m.F, 30000, 11)
    dm.add(ids, x)
    whole, s1 = dm.faces(), dm.stats()
    dm.clear()
    dm.add(ids[:12345], x[:12345])
    dm.add(ids[12345:], x[12345:])
    split, s2 = dm.faces(), dm.stats()
    assert ref.same_bits(split["peak"], whole["peak"]) and np.array_equal(split["hits"], whole["hits"])
    st = ref.State(m.F).add(ids[:12345], x[:12345]).add(ids[12345:], x[12345:])
    assert np.array_equal(split["frames"], st.frames) and (split["frames"] >= whole["frames"]).all() and (split["frames"] == 2).any()
    assert s2 == dict(s1, observations=2)


def test_cuda_tensors_on_a_side_stream():
    import torch
    from pedp_hip import DefectMap, _lib

    m = model("torus1022")
    side = torch.cuda.Stream()
    sctx = _lib.Context(0, stream=side.cuda_stream)
    dm = DefectMap((m.verts, m.tris), sctx)
    ids, x = rows(m.F, 5000, 21)
    dm.add(ids, x)
    host = dm.faces()
    same_faces(host, ref.State(m.F).add(ids, x).faces())
    for cast in (lambda a: a.astype(np.int64), lambda a: a.view(np.int32)):
        dm.clear()
        with torch.cuda.stream(side):
            dm.add(torch.from_numpy(cast(ids)).cuda(), torch.from_numpy(x).cuda())
        same_faces(dm.faces(), host)
    dm.clear()
    dm.add(torch.from_numpy(ids.astype(np.int64)).cuda(), torch.from_numpy(x.astype(np.float32)).cuda())   # torch's default stream
    same_faces(dm.faces(), ref.State(m.F).add(ids, x.astype(np.float32)).faces())
    dm.clear()
    dm.add(torch.from_numpy(ids.astype(np.int64)), torch.from_numpy(x))                                     # CPU tensors
    same_faces(dm.faces(), host)
    with pytest.raises(_lib.PedpError, match="one length"):
        dm.add(ids, x[:-1])
    assert dm.stats()["observations"] == 1
    dm.close()
    sctx.close()


# ------------------------------------------------------------------ regions
def two_observations(F, density, seed):
    rng = np.random.default_rng(seed)
    a = np.nonzero(rng.uniform(size=F) < density)[0]
    b = np.concatenate([a[rng.uniform(size=len(a)) < 0.5], rng.integers(0, F, max(len(a) // 8, 1))])
    return (a.astype(np.uint32), rng.uniform(-1.0, 1.0, len(a))), (b.astype(np.uint32), rng.uniform(-1.0, 1.0, len(b)))


@pytest.mark.parametrize("grow", [0, 1, 3])
@pytest.mark.parametrize("density", [0.01, 0.3, 0.9])
@pytest.mark.parametrize("name", ["torus16000", "two_tori"])
def test_regions(dmap, name, density, grow):
    m, dm = model(name), dmap(name)
    o1, o2 = two_observations(m.F, density, int(density * 100) + grow)
    dm.add(*o1)
    dm.add(*o2)
    st = ref.State(m.F).add(*o1).add(*o2)
    same_faces(dm.faces(), st.faces())
    for min_frames in (1, 2):
        for threshold in (0.25, -0.5):
            got = dm.regions(threshold, min_frames, grow)
            same_regions(got, ref.regions(m, st, threshold, min_frames, grow))
            assert got["n_regions"] >= 1
    # the same bits on every call, and after the handle has seen other rows in between
    a = dm.regions(-0.5, 1, grow)
    b = dm.regions(-0.5, 1, grow)
    same_table_bits(a, b)
    dm.add(*rows(m.F, 5000, 5))
    dm.regions(0.0, 1, 1)
    dm.clear()
    dm.add(*o1)
    dm.add(*o2)
    same_table_bits(dm.regions(-0.5, 1, grow), a)


def test_regions_of_the_strip(dmap):
    m, dm = model("strip4096"), dmap("strip4096")
    ids = np.arange(m.F, dtype=np.uint32)
    x = np.random.default_rng(2).uniform(0.6, 1.0, m.F)
    dm.add(ids, x)
    st = ref.State(m.F).add(ids, x)
    whole = dm.regions()
    assert whole["n_regions"] == 1 and whole["n_faces"][0] == 4096 and whole["first_face"][0] == 0
    same_regions(whole, ref.regions(m, st))
    dm.clear()
    dm.add(ids[::2], x[::2])
    st = ref.State(m.F).add(ids[::2], x[::2])
    every_second = dm.regions()
    assert every_second["n_regions"] == 2048 and (every_second["n_faces"] == 1).all()
    same_regions(every_second, ref.regions(m, st))
    joined = dm.regions(grow=1)
    assert joined["n_regions"] == 1 and joined["n_faces"][0] == 4096 and joined["n_seed_faces"][0] == 2048
    same_regions(joined, ref.regions(m, st, grow=1))


def test_a_region_longer_than_one_summing_block(dmap):
    """All 16,000 faces in one region: its run is summed in four blocks whose partial sums a second pass adds."""
    m, dm = model("seam16000"), dmap("seam16000")
    ids = np.arange(m.F, dtype=np.uint32)
    dm.add(ids, np.linspace(0.6, 1.0, m.F))
    st = ref.State(m.F).add(ids, np.linspace(0.6, 1.0, m.F))
    got = dm.regions()
    assert got["n_regions"] == 1 and got["n_faces"][0] == 16000
    same_regions(got, ref.regions(m, st))
    same_table_bits(dm.regions(), got)


def test_more_regions_than_room(dmap):
    from pedp_hip import _lib

    m, dm = model("two_tori"), dmap("two_tori")
    dm.add(np.arange(m.F, dtype=np.uint32), np.ones(m.F))
    with pytest.raises(_lib.PedpError, match="2 regions, room for 1"):
        dm.regions(capacity=1)
    from pedp_hip.defect_map import REGION_DTYPE

    table = np.full(1, 7, dtype=np.uint8).repeat(REGION_DTYPE.itemsize).view(REGION_DTYPE)
    before = table.tobytes()
    labels, n = np.empty(m.F, np.int32), C.c_int64()
    rc = _lib.load().pedp_defect_map_regions(dm._h, 0.5, 1, 0, _lib.HOST, _lib._ptr(labels), 1, _lib._ptr(table), C.byref(n))
    assert rc == -1 and n.value == 2 and table.tobytes() == before
    assert (labels[:m.F // 2] == 0).all() and (labels[m.F // 2:] == 1).all()
    assert dm.regions()["n_regions"] == 2                            # the first guess is retried with room
    rc = _lib.load().pedp_defect_map_regions(dm._h, 0.5, 1, 65, _lib.HOST, None, 0, None, C.byref(n))
    assert rc == -1 and b"grow" in _lib.load().pedp_last_error()


def test_device_outputs_equal_the_host_ones(ctx, dmap):
    """PEDP_DEVICE writes labels, table and the faces' columns into the caller's device arrays: the bits of PEDP_HOST."""
    import torch
    from pedp_hip import _lib
    from pedp_hip.defect_map import REGION_DTYPE

    m, dm = model("two_tori"), dmap("two_tori")
    o1, o2 = two_observations(m.F, 0.3, 77)
    dm.add(*o1)
    dm.add(*o2)
    host, faces = dm.regions(0.25, 1, 1), dm.faces()
    R = host["n_regions"]
    assert R > 64
    lib = _lib.load()
    labels = torch.full((m.F,), -7, dtype=torch.int32, device="cuda")
    table = torch.zeros(R * REGION_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    peak = torch.empty(m.F, dtype=torch.float64, device="cuda")
    hits = torch.empty(m.F, dtype=torch.int64, device="cuda")
    frames = torch.empty(m.F, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = C.c_int64()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.pedp_defect_map_regions(dm._h, 0.25, 1, 1, _lib.DEVICE, vp(labels), R, vp(table), C.byref(n)) == 0 and n.value == R
    assert lib.pedp_defect_map_faces(dm._h, _lib.DEVICE, vp(peak), vp(hits), vp(frames)) == 0
    ctx.synchronize()
    rows = table.cpu().numpy().view(REGION_DTYPE)
    assert np.array_equal(labels.cpu().numpy(), host["labels"])
    for k in REGION_DTYPE.names:
        assert ref.same_bits(np.ascontiguousarray(rows[k]), host[k]), k
    same_faces({"peak": peak.cpu().numpy(), "hits": hits.cpu().numpy(), "frames": frames.cpu().numpy()}, faces)
    only = np.empty(m.F, np.int64)                                   # every pointer of faces is nullable
    assert lib.pedp_defect_map_faces(dm._h, _lib.HOST, None, _lib._ptr(only), None) == 0 and np.array_equal(only, faces["hits"])


def test_face_colors(dmap):
    from pedp_hip.ray_projection import jet

    m, dm = model("cube"), dmap("cube")
    assert np.array_equal(dm.face_colors(), np.full((12, 3), 0.5))
    dm.add(np.array([0, 3, 5, 5], np.uint32), np.array([0.25, 0.625, 1.0, 0.5]))
    want = np.tile([0.1, 0.2, 0.3], (12, 1))
    want[[0, 3, 5]] = jet(np.array([0.0, 0.5, 1.0]))
    assert np.array_equal(dm.face_colors(unhit=(0.1, 0.2, 0.3)), want)


# ------------------------------------------------------------------ end to end
def dented_heatmap(ctx, f, W, H, foc):
    """A W x H depth frame of the posed parity torus with a dent pressed in at pixels hit well inside a triangle that
    faces the camera, through deviation_heatmap: heat about 0.5 on the dented pixels, 0 elsewhere."""
    from pedp_hip import _lib, surface_distance as sd, synth

    K = np.array([[foc, 0.0, (W - 1) / 2], [0.0, foc, (H - 1) / 2], [0.0, 0.0, 1.0]])
    dirs = synth.pixel_rays(W, H, foc, (W - 1) / 2, (H - 1) / 2)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    hit = mesh.cast_rays(synth.rays6_from_dirs(dirs))
    ok = np.isfinite(hit["t_hit"])
    v = f.verts_posed.astype(np.float64)
    tri = f.tris[np.where(ok, hit["primitive_ids"], 0)]
    nrm = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cosine = np.abs((dirs * nrm).sum(axis=1))
    uv = hit["primitive_uvs"]
    dented = np.nonzero(ok & (uv[:, 0] > 0.15) & (uv[:, 1] > 0.15) & (uv[:, 0] + uv[:, 1] < 0.85) & (cosine > 0.7))[0]
    assert len(dented) >= 10
    along = np.where(ok, (v[tri[:, 0]] * nrm).sum(axis=1) / (dirs * nrm).sum(axis=1), 0.0)
    along[dented] += 0.5 / cosine[dented]
    depth = (along * dirs[:, 2] / 1000.0).astype(np.float32).reshape(H, W)
    heat = sd.deviation_heatmap(depth, K, mesh, 1.0, 5.0)
    assert (heat.reshape(-1)[dented] > 0.4).all() and (heat > 0.4).sum() == len(dented)
    mesh.close()
    return heat, K


def test_end_to_end_on_a_dented_frame(ctx):
    import torch
    from pedp_hip import DefectMap, _lib, synth

    f = synth.Frame("parity")
    heat, K = dented_heatmap(ctx, f, 64, 48, 90.0)
    nudge = np.eye(4)
    nudge[:3, :3] = synth.axis_angle([0.0, 1.0, 0.0], np.deg2rad(0.2))
    nudge[:3, 3] = [0.3, -0.2, 0.5]
    poses = [f.T_gt, nudge @ f.T_gt]
    posable = _lib.Mesh(ctx, f.verts.astype(np.float64), f.tris, posable=True)
    m = ref.Model(f.verts.astype(np.float64), f.tris)
    dm = DefectMap((m.verts, m.tris), ctx)
    st = ref.State(m.F)
    for i, T in enumerate(poses):
        posable.set_pose(T)
        h = torch.from_numpy(heat).cuda() if i else heat            # a heat map on the host, then one on the device
        n_hits = dm.add_projection(posable, h, K, threshold=0.1)
        host = posable.project_heatmap(heat, K, threshold=0.1)
        assert n_hits == len(host["primitive_ids"]) >= 10
        st.add(host["primitive_ids"], host["intensities"])
    same_faces(dm.faces(), st.faces())
    assert dm.stats() == st.stats() and st.stats()["observations"] == 2
    for grow in (0, 1):
        got, want = dm.regions(0.3, 2, grow), ref.regions(m, st, 0.3, 2, grow)
        assert want["n_regions"] >= 1 and (want["max_frames"] == 2).all()
        same_regions(got, want)
    colors = dm.face_colors()
    assert colors.shape == (m.F, 3) and (colors[st.hits == 0] == 0.5).all()
    other = _lib.Mesh(ctx, f.verts_posed[:30], f.tris[:4] % 30)
    with pytest.raises(_lib.PedpError, match="faces"):
        dm.add_projection(other, heat, K)
    dm.close()


def test_device_add_while_a_registration_is_pending(ctx):
    """pedp_defect_map_add with PEDP_DEVICE only enqueues and has no workspace: a pending registration's result is
    unchanged.  The calls that wait on the stream are refused."""
    import torch
    from pedp_hip import DefectMap, _lib, synth

    f = synth.Frame("tiny")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    kw = dict(max_iteration=6, relative_fitness=-1, relative_rmse=-1)
    one = _lib.icp(ctx, src, tgt, 10.0, f.icp_init(), want_corr=True, **kw)
    dm = DefectMap((f.verts.astype(np.float64), f.tris), ctx)
    ids, x = rows(dm.F, 257, 31)
    d_ids, d_x = torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    _lib.icp_begin(ctx, src, tgt, 10.0, f.icp_init(), **kw)
    try:
        lib = _lib.load()
        assert lib.pedp_defect_map_add(dm._h, C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_x.data_ptr()), 257, _lib.DEVICE) == 0
        n = C.c_int64()
        assert lib.pedp_defect_map_add(dm._h, _lib._ptr(ids), _lib._ptr(x), 257, _lib.HOST) == -1
        assert lib.pedp_defect_map_regions(dm._h, 0.5, 1, 0, _lib.HOST, None, 0, None, C.byref(n)) == -1
        assert lib.pedp_defect_map_stats(dm._h, C.byref(n), C.byref(n), C.byref(n)) == -1
    finally:
        two = _lib.icp_end(ctx, want_corr=True)
    assert np.array_equal(one["T"], two["T"]) and np.array_equal(one["corr"], two["corr"])
    assert one["fitness"] == two["fitness"] and one["inlier_rmse"] == two["inlier_rmse"]
    same_faces(dm.faces(), ref.State(dm.F).add(ids, x).faces())
    assert dm.stats()["observations"] == 1
    dm.close()
