"""numpy restatement of the pose kernels' contract (csrc/pedp_pose.hip), operation for operation:
float32 products and sums in the kernel's order, tanh / sin / cos in float64 rounded once to float32."""
import numpy as np

F32 = np.float32


def tanh32(x):
    return np.tanh(np.asarray(x, np.float32).astype(np.float64)).astype(F32)


def _mat3(a, b):
    """Row-major 3 x 3 products, each entry ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j), float32."""
    return (a[:, :, 0, None] * b[:, None, 0, :] + a[:, :, 1, None] * b[:, None, 1, :]) + a[:, :, 2, None] * b[:, None, 2, :]


def so3_exp(x):
    """pytorch3d 0.7 _so3_exp_map at eps 1e-4 on N x 3 float32."""
    x = np.asarray(x, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        n = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
        th = np.sqrt(np.maximum(n, F32(1e-4)))           # np.maximum keeps a NaN, as torch.clamp does
        ti = F32(1) / th
        f1 = ti * np.sin(th.astype(np.float64)).astype(F32)
        f2 = (ti * ti) * (F32(1) - np.cos(th.astype(np.float64)).astype(F32))
        z = np.zeros_like(x[:, 0])
        K = np.stack([z, -x[:, 2], x[:, 1], x[:, 2], z, -x[:, 0], -x[:, 1], x[:, 0], z], 1).reshape(-1, 3, 3)
        return (f1[:, None, None] * K + f2[:, None, None] * _mat3(K, K)) + np.eye(3, dtype=F32)


def _normalize(v):
    with np.errstate(all="ignore"):
        nr = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        return v / np.maximum(nr, F32(1e-12))[:, None]


def rot6d(a):
    """pytorch3d rotation_6d_to_matrix on N x 6 float32: rows b1, b2, b1 x b2."""
    a = np.asarray(a, F32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        b1 = _normalize(a[:, :3])
        dot = (b1[:, 0] * a[:, 3] + b1[:, 1] * a[:, 4]) + b1[:, 2] * a[:, 5]
        b2 = _normalize(a[:, 3:] - dot[:, None] * b1)
        b3 = np.stack([b1[:, 1] * b2[:, 2] - b1[:, 2] * b2[:, 1], b1[:, 2] * b2[:, 0] - b1[:, 0] * b2[:, 2],
                       b1[:, 0] * b2[:, 1] - b1[:, 1] * b2[:, 0]], 1)
        return np.stack([b1, b2, b3], 1)


def pose_update(trans, rot, poseA, trans_rep="tracknet", rot_rep="axis_angle", normalize_xyz=False, trans_normalizer=1.0,
                rot_normalizer=1.0, mesh_diameter=1.0):
    """-> (poses N x 4 x 4, trans_delta N x 3, rot_mat_delta N x 3 x 3), all float32."""
    t = np.asarray(trans, F32).reshape(-1, 3)
    tn = np.broadcast_to(np.asarray(trans_normalizer, np.float64).astype(F32).reshape(-1), (3,))
    with np.errstate(all="ignore"):
        td = tanh32(t) * tn if (trans_rep == "tracknet" and not normalize_xyz) else t.copy()
        if normalize_xyz:
            td = td * F32(mesh_diameter / 2)
        if rot_rep == "axis_angle":
            R = so3_exp(tanh32(np.asarray(rot, F32).reshape(-1, 3)) * F32(rot_normalizer))
        else:
            R = rot6d(rot)
        Rd = np.ascontiguousarray(R.transpose(0, 2, 1))
        PA = np.asarray(poseA, F32).reshape(-1, 4, 4)
        out = np.zeros_like(PA)
        out[:, :3, :3] = _mat3(Rd, PA[:, :3, :3])
        out[:, :3, 3] = PA[:, :3, 3] + td
    out[:, 3, 3] = 1
    return out, td.astype(F32), Rd


def max_pair_distance(p, block=256):
    """numpy's `np.linalg.norm(p[None] - p[:, None], axis=-1).max()`, computed in row blocks (NaN propagates)."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    best = -np.inf
    for i in range(0, len(p), block):
        m = np.linalg.norm(p[None] - p[i:i + block, None], axis=-1).max()
        if np.isnan(m):
            return np.nan
        best = max(best, m)
    return best
