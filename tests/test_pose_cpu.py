"""The pose kernels' numpy restatement (tests/_pose_ref.py) against independent references, and the parameter mapping
of pose.py; no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _pose_ref as ref


def test_axis_angle_matches_scipy_rotvec():
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(0)
    axes = rng.normal(size=(500, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    angles = np.concatenate([[0.01, 0.0101, 0.05], rng.uniform(0.01, 3.1, 497)])
    v = (axes * angles[:, None]).astype(np.float32)
    got = ref.so3_exp(v)
    want = Rotation.from_rotvec(v.astype(np.float64)).as_matrix()
    assert np.abs(got - want).max() < 1e-6


def test_zero_axis_angle_is_identity_and_the_clamp_shows_below_0_01():
    from scipy.spatial.transform import Rotation

    assert np.array_equal(ref.so3_exp(np.zeros((2, 3), np.float32)), np.repeat(np.eye(3, dtype=np.float32)[None], 2, 0))
    v = np.array([[1e-3, 0, 0]], np.float32)
    got = ref.so3_exp(v)[0]
    # theta is clamped to 0.01: sin(0.01) / 0.01 * 1e-3 instead of sin(1e-3)
    assert abs(got[2, 1] - np.sin(0.01) / 0.01 * 1e-3) < 1e-9
    assert abs(got[2, 1] - Rotation.from_rotvec(v[0].astype(np.float64)).as_matrix()[2, 1]) > 1e-8


def test_6d_rotation_is_orthonormal_and_right_handed():
    rng = np.random.default_rng(1)
    R = ref.rot6d(rng.normal(size=(300, 6)).astype(np.float32)).astype(np.float64)
    eye = np.einsum("nij,nkj->nik", R, R)
    assert np.abs(eye - np.eye(3)).max() < 5e-6          # float32 Gram-Schmidt
    assert np.abs(np.linalg.det(R) - 1).max() < 5e-6


def test_update_composes_delta_with_the_pose():
    rng = np.random.default_rng(2)
    B = 20
    PA = np.zeros((B, 4, 4), np.float32)
    PA[:, :3, :3] = ref.so3_exp(rng.normal(size=(B, 3)).astype(np.float32))
    PA[:, :3, 3] = rng.normal(size=(B, 3))
    PA[:, 3, 3] = 1
    tr, rot = rng.normal(size=(B, 3)).astype(np.float32), rng.normal(size=(B, 3)).astype(np.float32)
    out, td, Rd = ref.pose_update(tr, rot, PA, trans_normalizer=[0.02, 0.03, 0.05], rot_normalizer=0.3)
    assert np.allclose(out[:, :3, :3], Rd.astype(np.float64) @ PA[:, :3, :3], atol=1e-6)
    assert np.allclose(td, np.tanh(tr.astype(np.float64)) * [0.02, 0.03, 0.05], rtol=1e-6)
    assert np.array_equal(out[:, 3], np.repeat([[0, 0, 0, 1]], B, 0))
    out2, td2, _ = ref.pose_update(tr, rot, PA, normalize_xyz=True, mesh_diameter=0.3)
    assert np.array_equal(td2, tr * np.float32(0.15))     # tracknet under normalize_xyz: no tanh


def test_pair_maximum_restatement():
    rng = np.random.default_rng(3)
    p = rng.normal(size=(300, 3))
    want = max(np.linalg.norm(a - b) for a in p[::7] for b in p)
    assert ref.max_pair_distance(p, block=64) >= want
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)).max()
    assert abs(ref.max_pair_distance(p, block=64) - d) <= 1e-15 * d
    p[5, 1] = np.inf
    assert np.isnan(ref.max_pair_distance(p, block=64))


def test_update_params_mapping():
    from pedp_hip import _lib
    from pedp_hip.pose import update_params

    p = update_params("tracknet", "6d", True, [0.1, 0.2, 0.3], 0.35, 0.25)
    assert (p.trans_rep, p.rot_rep, p.normalize_xyz) == (_lib.TRANS_TRACKNET, _lib.ROT_6D, 1)
    assert list(p.trans_normalizer) == [np.float32(0.1), np.float32(0.2), np.float32(0.3)]
    assert p.rot_normalizer == np.float32(0.35) and p.mesh_diameter == 0.25
    assert list(update_params(trans_normalizer=0.05).trans_normalizer) == [np.float32(0.05)] * 3
    assert update_params("raw").trans_rep == _lib.TRANS_RAW
    with pytest.raises(NotImplementedError):
        update_params("deepim")
    with pytest.raises(RuntimeError):
        update_params(rot_rep="quat")
    with pytest.raises(_lib.PedpError):
        update_params(trans_normalizer=[1, 2])


def test_pose_update_checks_its_arguments_before_any_launch():
    """Shapes, the output array and the parameters are checked on the host; nothing here reaches the library."""
    from pedp_hip import _lib
    from pedp_hip.pose import pose_update, update_params

    P = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
    t = np.zeros((6, 3), np.float32)
    bad_out = [np.empty((6, 4, 4)), np.empty((6, 4, 4), np.float16), np.empty((6, 4, 8), np.float32)[:, :, :4],
               np.empty((5, 4, 4), np.float32), np.empty((6, 16), np.float32), [0.0] * 96]
    ro = np.empty((6, 4, 4), np.float32)
    ro.flags.writeable = False
    for o in bad_out + [ro]:
        with pytest.raises(_lib.PedpError):
            pose_update(t, t, P, out=o)
    with pytest.raises(_lib.PedpError):
        pose_update(t, t, P[:, :3])
    with pytest.raises(_lib.PedpError):
        pose_update(t[:5], t, P)
    with pytest.raises(_lib.PedpError):
        pose_update(t, t, P, rot_rep="6d")
    with pytest.raises(TypeError):
        pose_update(t, t, P, params=update_params(), rot_rep="6d")
    with pytest.raises(NotImplementedError):
        pose_update(t, t, P, trans_rep="deepim")


def test_the_out_refusal_says_what_it_got():
    """The full text of pose_update's refusal of `out`: a wrong dtype, a wrong shape, a strided array."""
    from pedp_hip import _lib
    from pedp_hip.pose import pose_update

    P = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    t = np.zeros((2, 3), np.float32)
    want = "pose_update: out must be a C-contiguous 2 x 4 x 4 float32 array in host memory, got a "
    for out, got in ((np.empty((2, 4, 4), np.float64), "float64 array of shape (2, 4, 4)"),
                     (np.empty((3, 4, 4), np.float32), "float32 array of shape (3, 4, 4)"),
                     (np.empty((2, 4, 8), np.float32)[:, :, ::2], "float32 array of shape (2, 4, 4), strided")):
        with pytest.raises(_lib.PedpError) as e:
            pose_update(t, t, P, out=out)
        assert str(e.value) == want + got


def test_the_kernel_wrappers_do_not_load_the_crop_builder_the_renderer_or_the_depth_filters():
    """In a fresh interpreter: the wrappers take their plumbing from _bridge, not from the modules written before them."""
    code = ("import sys, pedp_hip.linear, pedp_hip.attention, pedp_hip.conv, pedp_hip.pose, pedp_hip.metrics\n"
            "print(*sorted(m for m in ('pedp_hip.crop', 'pedp_hip.render', 'pedp_hip.depth_filters') if m in sys.modules))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", code], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().split() == []
