"""The crop restatements on analytic cases (no GPU): tests/_crop_ref.py's contract and its torch restatement of kornia
0.7.2's warp_perspective, which the GPU tests compare the kernels against; and the library's crop entry points."""
import ctypes
import os

import numpy as np
import pytest

import _crop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(C=3, H=6, W=8, seed=0):
    return np.random.default_rng(seed).random((1, C, H, W)).astype(np.float32)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_identity_align_corners_returns_source(mode):
    s = _src()
    out = ref.warp(s, np.eye(3, dtype=np.float32)[None], (6, 8), mode, True)
    assert np.array_equal(out, s)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_integer_translation(mode):
    s = _src()
    M = np.eye(3, dtype=np.float32)
    M[0, 2], M[1, 2] = 2, -1  # destination = source + (2, -1)
    out = ref.warp(s, M[None], (6, 8), mode, True)
    want = np.zeros_like(s)
    want[0, :, 0:5, 2:8] = s[0, :, 1:6, 0:6]
    assert np.array_equal(out, want)


def test_align_corners_false_stretches_by_w_over_w_minus_1():
    # the identity under align_corners=False samples x * W / (W - 1) - 0.5, not x
    H, W = 4, 5
    mp = ref.make_map(np.eye(3, dtype=np.float32), H, W, False)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ix, iy = ref.map_coords64(mp, x, y)
    assert np.allclose(ix, x * W / (W - 1) - 0.5, rtol=0, atol=1e-12)
    assert np.allclose(iy, y * H / (H - 1) - 0.5, rtol=0, atol=1e-12)
    # a linear ramp along x comes out stretched accordingly (inside the image: the first and last rows and columns reach
    # 0.5 px beyond it)
    s = np.tile(np.arange(W, dtype=np.float32), (1, 1, H, 1))
    out = ref.warp(s, np.eye(3, dtype=np.float32)[None], (H, W), "bilinear", False)[0, 0]
    assert np.allclose(out[1:H - 1, 1:W - 1], (np.arange(W) * W / (W - 1) - 0.5)[1:W - 1], atol=1e-6)
    assert np.allclose(out[:, 0], 0.0)  # x = -0.5: half the weight on a zero-padded column, half on value 0


def test_nearest_ties_round_half_to_even():
    ix = np.array([0.5, 1.5, 2.5, -0.5, 3.5], np.float32)
    ok, xi, _ = ref.nearest_index(ix, np.zeros_like(ix), 1, 4)
    assert list(xi[ok]) == [0, 2, 2, 0] and list(ok) == [True, True, True, True, False]
    img = np.arange(4, dtype=np.float32).reshape(1, 1, 4) + 1
    assert list(ref.sample_nearest(img, ix, np.zeros_like(ix))[0]) == [1, 3, 3, 1, 0]


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_out_of_range_gives_zero(mode):
    s = _src() + 1
    M = np.eye(3, dtype=np.float32)
    M[0, 2] = 100
    assert not ref.warp(s, M[None], (6, 8), mode, True).any()
    sing = np.zeros((1, 3, 3), np.float32)
    assert not ref.warp(s, sing, (6, 8), mode, True).any()


def _homographies(n, H, W, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        A = np.eye(3)
        A[:2, :2] = np.array([[1, 0], [0, 1]]) * rng.uniform(0.7, 1.4) + rng.normal(0, 0.15, (2, 2))
        A[:2, 2] = rng.uniform(-0.2, 0.2, 2) * [W, H]
        A[2, :2] = rng.normal(0, 2e-3, 2)
        out.append(A.astype(np.float32))
    return np.stack(out)


@pytest.mark.parametrize("align", [False, True])
def test_contract_agrees_with_kornia_restatement(align):
    torch = pytest.importorskip("torch")
    H, W, h, w = 48, 64, 40, 56
    s = np.random.default_rng(3).random((1, 3, H, W)).astype(np.float32)
    M = _homographies(6, H, W, 5)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with torch.no_grad():
        kn = ref.kornia_warp_perspective(s, M, (h, w), "nearest", align).numpy()
        kb = ref.kornia_warp_perspective(s, M, (h, w), "bilinear", align).numpy()
    cn = ref.warp(s, M, (h, w), "nearest", align)
    cb = ref.warp(s, M, (h, w), "bilinear", align)
    step = float(np.abs(np.diff(s, axis=-1)).max() + np.abs(np.diff(s, axis=-2)).max())
    for b in range(len(M)):
        ix, iy = ref.map_coords64(ref.make_map(M[b], H, W, align), x, y)
        near_tie = (np.abs(ix - np.floor(ix) - 0.5) < 1e-4) | (np.abs(iy - np.floor(iy) - 0.5) < 1e-4)
        diff = (cn[b] != kn[b]).any(axis=0)
        assert not (diff & ~near_tie).any(), f"pose {b}: nearest differs away from a .5 boundary"
        assert np.abs(cb[b] - kb[b]).max() <= 1e-4 * 2 * step + 1e-6, f"pose {b}: bilinear beyond the coordinate tolerance"


def test_crop_window_restatement():
    K = np.array([[500.0, 0, 319.5], [0, 500.0, 239.5], [0, 0, 1]])
    P = np.eye(4, dtype=np.float32)[None].repeat(2, 0)
    P[0, :3, 3] = [0, 0, 1]
    P[1, :3, 3] = [0.1, -0.05, 0.8]
    tf, bb = ref.crop_window(P, K, np.float32(0.1), 160, 160, (159, 159))
    # pose 0: centre (319.5, 239.5), radius 50 -> left 270 (269.5 rounds to even), right 370, top 190, bottom 290.
    # The scale is torch's `160 / tensor(100.)`: float32(1/100) * 160, which rounds to 1.5999999 (0x3FCCCCCC), not 1.6.
    s = np.float32(np.float32(1) / np.float32(100)) * np.float32(160)
    assert s.view(np.uint32) == 0x3FCCCCCC
    assert np.array_equal(tf[0], np.array([[s, 0, s * np.float32(-270)], [0, s, s * np.float32(-190)], [0, 0, 1]], np.float32))
    assert np.allclose(bb[0], [270, 190, 270 + 159 / 1.6, 190 + 159 / 1.6], atol=1e-3)
    assert tf.dtype == np.float32 and bb.shape == (2, 4)


def test_transform_xyz_branches():
    xyz = np.array([[0.0, 0.0, 0.05], [0.01, 0.0, 0.5], [0.3, 0.0, 0.5]], np.float32).T.reshape(1, 3, 1, 3)
    t = np.array([[0.0, 0.0, 0.5]], np.float32)
    out = ref.transform_xyz(xyz, t, True, 0.1, 0.2)[0, :, 0]
    assert np.array_equal(out[:, 0], [0, 0, 0])                    # z < 0.1: every channel zeroed
    assert np.allclose(out[:, 1], [0.1, 0, 0])                     # scaled by 1 / 0.1
    assert np.array_equal(out[:, 2], np.float32([0, 0, 0]))        # |3.0| >= 2 zeroes x; y and z are 0 anyway
    raw = ref.transform_xyz(xyz, t, False, 0.1, 0.2)[0, :, 0]
    assert np.allclose(raw[:, 0], [0, 0, -0.45])                   # no normalisation: no zeroing


def test_library_exports_crop_entries():
    from pedp_hip import _lib

    _lib.load()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pedp_warp_perspective", "pedp_crop_window", "pedp_crop_batch"):
        assert hasattr(lib, name), name
    from pedp_hip import compat

    assert compat.kornia.geometry.transform.warp_perspective is compat.warp_perspective
    for name in ("make_crop_data_batch", "make_score_crop_data_batch", "compute_crop_window_tf_batch"):
        assert callable(getattr(compat, name))


def test_unsupported_modes_raise():
    from pedp_hip.compat import compute_crop_window_tf_batch, warp_perspective

    s, M = np.zeros((1, 1, 4, 4), np.float32), np.eye(3, dtype=np.float32)[None]
    with pytest.raises(NotImplementedError):
        warp_perspective(s, M, (4, 4), mode="bicubic")
    with pytest.raises(NotImplementedError):
        warp_perspective(s, M, (4, 4), padding_mode="border")
    with pytest.raises(NotImplementedError):
        compute_crop_window_tf_batch(poses=np.eye(4)[None], K=np.eye(3), out_size=(8, 8), method="min_box", mesh_diameter=1)


def test_crop_window_scale_follows_torch_number_over_tensor():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(7)
    P = np.eye(4, dtype=np.float32)[None].repeat(64, 0)
    P[:, :3, 3] = np.stack([rng.uniform(-0.1, 0.1, 64), rng.uniform(-0.1, 0.1, 64), rng.uniform(0.3, 1.2, 64)], 1)
    K = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
    tf, _ = ref.crop_window(P, K, np.float32(0.09), 160, 128)
    t = P[:, :3, 3]
    # extents from the restatement's own window, the scales as Utils.py:595-596 computes them in torch
    ext_x = np.float32(160) / tf[:, 0, 0]
    left = -tf[:, 0, 2] / tf[:, 0, 0]
    assert np.all(np.abs(left - np.rint(left)) < 1e-2) and len(t) == 64
    w = torch.as_tensor(np.rint(ext_x).astype(np.float32))
    h = torch.as_tensor(np.rint(np.float32(128) / tf[:, 1, 1]).astype(np.float32))
    assert np.array_equal(tf[:, 0, 0], (160 / w).numpy())
    assert np.array_equal(tf[:, 1, 1], (128 / h).numpy())
