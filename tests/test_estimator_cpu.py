"""The estimator's host side, without a GPU: the numpy restatement of guess_translation on cases with known answers,
the view set and the rotation grid, the predictors' configuration, the seeds and the drop-in names."""
import random
import types

import numpy as np
import pytest

import _estimator_ref as ref
from pedp_hip import estimator

K_ = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])


def _frame(h=6, w=8):
    return np.zeros((h, w), np.float32), np.zeros((h, w), np.uint8)


def _expect(u, v, z):
    z = float(z)
    return np.array([(u - 319.5) / 600.0 * z, (v - 239.5) / 600.0 * z, z])


def _host_path(d, m):
    """The package's numpy path, which a float64 frame takes (the same values: float32 widens exactly)."""
    return estimator.guess_translation(d.astype(np.float64), m, K_)


def test_restated_guess_translation_on_known_cases():
    d, m = _frame()
    d[2, 5], m[2, 5] = 0.75, 1                                     # one pixel
    assert np.allclose(ref.guess_translation(d, m, K_), _expect(5, 2, np.float32(0.75)), rtol=0, atol=1e-15)
    assert np.allclose(_host_path(d, m), _expect(5, 2, 0.75), rtol=0, atol=1e-15)

    d, m = _frame()
    d[1:3, 3:5], m[1:3, 3:5] = [[0.5, 0.7], [0.9, 0.6]], 1         # 2 x 2 block: the mean of the two middle depths
    z = (np.float32(0.6) + np.float32(0.7)) / np.float32(2)
    assert ref.stats(d, m)["median"] == z and ref.stats(d, m)["n_med"] == 4
    assert np.allclose(ref.guess_translation(d, m, K_), _expect(3.5, 1.5, z), rtol=0, atol=1e-15)

    d, m = _frame()
    d[:] = 0.5                                                      # empty mask
    assert np.array_equal(ref.guess_translation(d, m, K_), np.zeros(3)) and ref.stats(d, m)["umin"] == -1
    assert np.array_equal(_host_path(d, m), np.zeros(3))

    d, m = _frame()
    m[1:4, 1:4] = 1
    d[1:4, 1:4] = 0.0005                                            # a mask, but no depth of a millimetre or more
    d[2, 2] = np.nan
    assert np.array_equal(ref.guess_translation(d, m, K_), np.zeros(3))
    assert ref.stats(d, m) | {"median": 0} == dict(n_pos=9, n_valid=0, n_med=0, umin=1, umax=3, vmin=1, vmax=3, median=0)

    d, _ = _frame()
    m = np.zeros(d.shape, np.float32)
    d[:] = 0.4
    m[1, 1], m[4, 6] = 1.0, 2.0                                     # the box comes from these two ...
    m[0, 0], m[5, 7] = -1.0, np.nan                                 # ... the median also sees these (truthy, not > 0)
    d[0, 0], d[5, 7], d[1, 1], d[4, 6] = 0.1, 0.2, 0.3, 0.9
    rec = ref.stats(d, m)
    assert (rec["n_pos"], rec["n_valid"], rec["n_med"]) == (2, 2, 4)
    assert (rec["umin"], rec["umax"], rec["vmin"], rec["vmax"]) == (1, 6, 1, 4)
    assert rec["median"] == (np.float32(0.2) + np.float32(0.3)) / np.float32(2)
    assert np.allclose(ref.guess_translation(d, m, K_), _expect(3.5, 2.5, rec["median"]), rtol=0, atol=1e-15)
    assert np.allclose(_host_path(d, m), _expect(3.5, 2.5, (float(np.float32(0.2)) + float(np.float32(0.3))) / 2), rtol=0, atol=1e-15)

    d, m = _frame()
    m[0, :3] = 1
    d[0, :3] = [0.5, np.inf, np.inf]                                # inf enters the set and orders last
    assert ref.stats(d, m)["median"] == np.inf
    d[0, :3] = [0.5, 0.6, np.inf]
    assert ref.stats(d, m)["median"] == np.float32(0.6)
    m[0, 3], d[0, 3] = 1, -np.inf                                   # -inf (and any negative depth) never does
    assert ref.stats(d, m)["n_med"] == 3


def test_host_path_of_guess_translation_equals_the_restatement():
    """Dtypes the kernel does not read (float64 depth, integer masks) take numpy on the host: no library call."""
    guess_translation = estimator.guess_translation

    rng = np.random.default_rng(3)
    d = rng.uniform(0.3, 1.2, (40, 50))
    d[rng.random(d.shape) < 0.2] = 0
    m = (rng.random(d.shape) < 0.3).astype(np.int64) * rng.integers(-1, 3, d.shape)
    assert ref.same_bits(guess_translation(d, m, K_), ref.guess_translation(d, m, K_))
    assert ref.same_bits(guess_translation(d.astype(np.float32), m, K_), ref.guess_translation(d.astype(np.float32), m, K_))
    assert np.array_equal(guess_translation(d, np.zeros_like(m), K_), np.zeros(3))


def test_view_set_is_the_icosahedron_and_its_edge_midpoints():
    from pedp_hip.estimator import sample_views_icosphere

    cams = sample_views_icosphere(n_views=40)
    assert cams.shape == (42, 4, 4) and sample_views_icosphere(12).shape == (42, 4, 4)   # the reference starts at one subdivision
    assert sample_views_icosphere(43).shape == (162, 4, 4) and sample_views_icosphere(1, subdivisions=0).shape == (12, 4, 4)
    pos = cams[:, :3, 3]
    assert np.allclose(np.linalg.norm(pos, axis=1), 1, atol=1e-15)
    t = (1 + np.sqrt(5)) / 2
    ico = np.array([s for a in (-1, 1) for b in (-t, t) for s in ((0, a, b), (a, b, 0), (b, 0, a))]) / np.sqrt(1 + t * t)
    edge = np.linalg.norm(ico[:, None] - ico[None], axis=-1)
    i, j = np.nonzero(np.triu(np.isclose(edge, edge[edge > 0].min()), 1))
    mids = (ico[i] + ico[j]) / 2
    want = np.concatenate([ico, mids / np.linalg.norm(mids, axis=1, keepdims=True)])
    assert len(want) == 42
    dist = np.linalg.norm(pos[:, None] - want[None], axis=-1)
    assert (dist.min(axis=1) < 1e-12).all() and len(set(dist.argmin(axis=1))) == 42       # the same set, order unpinned
    R = cams[:, :3, :3]
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-14)
    assert np.allclose(np.linalg.det(R), 1, atol=1e-14)
    assert np.allclose(R[:, :, 2], -pos, atol=1e-15)                                       # z looks at the origin
    assert np.array_equal(cams[:, 3], np.tile([0, 0, 0, 1.0], (42, 1)))
    r = sample_views_icosphere(40, radius=0.5)
    assert np.allclose(np.linalg.norm(r[:, :3, 3], axis=1), 0.5, atol=1e-15)


def test_euler_matrix_is_a_turn_about_z():
    from pedp_hip.estimator import euler_matrix

    a = np.deg2rad(60)
    want = np.eye(4)
    want[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    assert np.array_equal(euler_matrix(0, 0, a), want)
    x, y, z = 0.3, -0.7, 1.1
    Rx, Ry, Rz = (np.eye(3) for _ in range(3))
    Rx[1:, 1:] = [[np.cos(x), -np.sin(x)], [np.sin(x), np.cos(x)]]
    Ry[::2, ::2] = [[np.cos(y), np.sin(y)], [-np.sin(y), np.cos(y)]]
    Rz[:2, :2] = [[np.cos(z), -np.sin(z)], [np.sin(z), np.cos(z)]]
    assert np.allclose(euler_matrix(x, y, z)[:3, :3], Rz @ Ry @ Rx, atol=1e-15)
    with pytest.raises(NotImplementedError):
        euler_matrix(0, 0, 0, axes="rzyx")


def test_rotation_grid_counts_under_identity_and_a_half_turn(capsys):
    from pedp_hip.estimator import euler_matrix, rotation_grid, sample_views_icosphere

    grid = rotation_grid(min_n_views=40, inplane_step=60)
    assert grid.shape == (252, 4, 4) and grid.dtype == np.float32
    R = grid[:, :3, :3].astype(np.float64)
    tr = np.einsum("aij,bij->ab", R, R)
    np.fill_diagonal(tr, -1)
    closest = np.degrees(np.arccos(np.clip((tr.max() - 1) / 2, -1, 1)))
    assert 31.6 < closest < 31.8                                     # 31.72 degrees: above cluster_poses' 30
    raw = np.asarray([np.linalg.inv(c @ euler_matrix(0, 0, a)) for c in sample_views_icosphere(40)
                      for a in np.deg2rad(np.arange(0, 360, 60))])
    assert np.array_equal(grid, raw.astype(np.float32))              # nothing dropped, the order kept
    eye = np.eye(4)[None]
    half = np.diag([-1.0, -1.0, 1.0, 1.0])                           # 180 degrees about the object's z
    sym = np.concatenate([eye, half[None]])
    assert len(ref.greedy_rotation_clusters(raw, eye)) == 252
    kept = ref.greedy_rotation_clusters(raw, sym)
    assert len(kept) == 126
    got = rotation_grid(symmetry_tfs=sym)
    assert got.shape == (126, 4, 4) and np.array_equal(got, raw[kept].astype(np.float32))


def test_predictor_config_defaults_for_mappings_and_objects():
    from pedp_hip.estimator import PoseRefinePredictor, ScorePredictor

    def net(*a, **k):
        return {}

    base = {"input_resize": [160, 160], "trans_normalizer": [0.02, 0.02, 0.05], "rot_normalizer": 0.35}
    for cfg in (dict(base), types.SimpleNamespace(**base)):
        r = PoseRefinePredictor(net, cfg)
        want = dict(use_normal=False, use_mask=False, use_BN=False, c_in=4, crop_ratio=1.2, n_view=1, trans_rep="tracknet",
                    rot_rep="axis_angle", zfar=3, normalize_xyz=False, normal_uint8=False, enable_amp=True)
        assert {k: r.cfg[k] for k in want} == want and r.cfg.use_normal is False and r.amp is True
        assert list(r.cfg["input_resize"]) == [160, 160] and r.cfg.rot_normalizer == 0.35
        assert r.last_trans_update is None and r.last_rot_update is None
        s = ScorePredictor(net, cfg, amp=False)
        want = dict(use_normal=False, use_BN=False, zfar=np.inf, c_in=4, normalize_xyz=False, crop_ratio=1.2)
        assert {k: s.cfg[k] for k in want} == want and s.amp is False
    r = PoseRefinePredictor(net, dict(base, crop_ratio=None, zfar="Inf", rot_rep="6d", normalize_xyz=True))
    assert r.cfg["crop_ratio"] == 1.2 and r.cfg["zfar"] == np.inf and r.cfg["rot_rep"] == "6d" and r.cfg["normalize_xyz"]
    assert base == {"input_resize": [160, 160], "trans_normalizer": [0.02, 0.02, 0.05], "rot_normalizer": 0.35}   # not written to


def test_missing_pieces_raise():
    from pedp_hip.estimator import FoundationPose, PoseRefinePredictor, ScorePredictor

    base = {"input_resize": [160, 160], "trans_normalizer": 0.02, "rot_normalizer": 0.35}

    def net(*a, **k):
        return {}

    with pytest.raises(ValueError, match="model="):
        PoseRefinePredictor(cfg=base)
    with pytest.raises(ValueError, match="model="):
        ScorePredictor(cfg=base)
    with pytest.raises(NotImplementedError, match="deepim"):
        PoseRefinePredictor(net, dict(base, trans_rep="deepim"))
    for lacking in ("input_resize", "trans_normalizer", "rot_normalizer"):
        with pytest.raises(KeyError, match=lacking):
            PoseRefinePredictor(net, {k: v for k, v in base.items() if k != lacking})
    with pytest.raises(KeyError, match="input_resize"):
        ScorePredictor(net, {})
    r = PoseRefinePredictor(net, base)
    with pytest.raises(NotImplementedError):
        r.predict(None, None, None, None, None, get_vis=True)
    with pytest.raises(NotImplementedError):
        ScorePredictor(net, base).predict(None, None, None, None, get_vis=True)
    with pytest.raises(ValueError, match="scorer"):
        FoundationPose(None, None, mesh=None)
    with pytest.raises(NotImplementedError):
        FoundationPose(None, None, scorer=ScorePredictor(net, base), refiner=r, debug=2)


def test_compat_carries_the_estimator_names():
    from pedp_hip import compat, estimator

    for name in ("FoundationPose", "PoseRefinePredictor", "ScorePredictor", "guess_translation", "mask_depth_stats", "set_seed",
                 "sample_views_icosphere", "euler_matrix", "compute_mesh_diameter"):
        assert name in compat.__all__ and getattr(compat, name) is getattr(estimator, name)


def test_set_seed_leaves_the_generators_where_seeding_them_does():
    import torch
    from pedp_hip.estimator import set_seed

    np.random.seed(0)
    random.seed(0)
    torch.manual_seed(0)
    want = (np.random.get_state(), random.getstate(), torch.get_rng_state())
    np.random.rand(5), random.random(), torch.rand(3)
    set_seed(0)
    got = (np.random.get_state(), random.getstate(), torch.get_rng_state())
    assert got[0][0] == want[0][0] and np.array_equal(got[0][1], want[0][1]) and got[0][2:] == want[0][2:]
    assert got[1] == want[1] and torch.equal(got[2], want[2])
    set_seed(7)
    a = (np.random.rand(), random.random(), float(torch.rand(1)))
    np.random.seed(7), random.seed(7), torch.manual_seed(7)
    assert a == (np.random.rand(), random.random(), float(torch.rand(1)))


def test_mask_depth_stats_refuses_bad_inputs_before_any_library_call():
    from pedp_hip import _lib
    from pedp_hip.estimator import mask_depth_stats

    d, m = np.zeros((4, 5), np.float32), np.zeros((4, 5), np.uint8)
    for depth, mask in ((d, m[:3]), (d[None], m[None]), (d.astype(np.float64), m), (d, m.astype(np.int32)),
                        (d, m.astype(np.float64)), (d.reshape(-1), m.reshape(-1)), ([[0.5]], [[1]]),
                        (np.zeros((0, 5), np.float32), np.zeros((0, 5), np.uint8))):
        with pytest.raises(_lib.PedpError, match="mask_depth_stats"):
            mask_depth_stats(depth, mask)
