"""What the estimator's tests compare against: numpy restatements of the frame statistics and of guess_translation
(estimater.py:135-154, :182-183), the two predictors' loops composed by hand from the package's public pieces (each of
which has tests of its own), two tiny seeded stand-in networks, and a float64 restatement of cluster_poses' greedy rule."""
import numpy as np


# ---------------------------------------------------------------- frame statistics in numpy

def stats(depth, mask):
    """The record of pedp_mask_depth_stats from numpy's own operations."""
    with np.errstate(invalid="ignore"):
        positive = mask > 0
        truthy = mask.astype(bool)
    near = depth >= 0.001          # numpy compares a float32 frame with this number in float32
    rows, cols = np.where(positive)
    picked = depth[truthy & near]
    rec = {"n_pos": int(len(cols)), "n_valid": int((near & positive).sum()), "n_med": int(picked.size)}
    rec.update(zip(("umin", "umax", "vmin", "vmax"),
                   (int(cols.min()), int(cols.max()), int(rows.min()), int(rows.max())) if len(cols) else (-1,) * 4))
    with np.errstate(over="ignore", invalid="ignore"):
        rec["median"] = np.float32(np.median(picked)) if picked.size else np.float32(np.nan)
    return rec


def guess_translation(depth, mask, K):
    """Box midpoint of `mask > 0`, at the median of the depths >= 0.001 under the truthy mask, through inv(K)."""
    with np.errstate(invalid="ignore"):
        rows, cols = np.where(mask > 0)
        truthy = mask.astype(bool)
    if len(cols) == 0:
        return np.zeros(3)
    u_mid = (cols.min() + cols.max()) / 2.0
    v_mid = (rows.min() + rows.max()) / 2.0
    chosen = truthy & (depth >= 0.001)
    if not chosen.any():
        return np.zeros(3)
    with np.errstate(over="ignore", invalid="ignore"):
        z_mid = np.median(depth[chosen])
        return ((np.linalg.inv(K) @ np.asarray([u_mid, v_mid, 1]).reshape(3, 1)) * z_mid).reshape(3)


def same_bits(a, b):
    """Equal bit for bit, except that any NaN equals any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    ua, ub = a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")
    return bool(np.all((ua == ub) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------- cluster_poses' greedy rule in float64

def greedy_rotation_clusters(poses, symmetry_tfs, angle_deg=30.0):
    """Indices kept by the rule of mycpp.cluster_poses with an unlimited distance: a pose is dropped when, under some
    symmetry, its rotation is within angle_deg of a pose kept before it."""
    R = np.asarray(poses, np.float64)[:, :3, :3]
    S = np.asarray(symmetry_tfs, np.float64)[:, :3, :3]
    kept = []
    for i in range(len(R)):
        near = False
        for k in kept:
            for s in S:
                c = (np.trace((R[i] @ s).T @ R[k]) - 1.0) / 2.0
                if np.degrees(np.arccos(np.clip(c, -1.0, 1.0))) < angle_deg:
                    near = True
                    break
            if near:
                break
        if not near:
            kept.append(i)
    return kept


# ---------------------------------------------------------------- stand-in networks

def _fill(module, seed, scale):
    import torch

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * scale)


def _trunk():
    import torch.nn as nn

    return nn.Conv2d(6, 8, 4, stride=4), nn.Conv2d(16, 8, 3, padding=1)


def make_refine_net(rot_width=3, seed=1):
    """model(A, B) -> {'trans': n x 3, 'rot': n x rot_width}: two conv layers, a mean over the pixels, one linear
    layer.  Every sample is computed on its own (no batch statistics)."""
    import torch
    import torch.nn as nn

    class RefineStandIn(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.c2 = _trunk()
            self.head = nn.Linear(8, 3 + rot_width)

        def forward(self, A, B):
            f = torch.cat([torch.relu(self.c1(A)), torch.relu(self.c1(B))], 1)
            o = self.head(torch.relu(self.c2(f)).mean((2, 3)))
            return {"trans": o[:, :3], "rot": o[:, 3:]}

    net = RefineStandIn()
    _fill(net, seed, 0.3)
    return net.eval()


def make_score_net(seed=2):
    """model(A, B, L=) -> {'score_logit': 1 x L}."""
    import torch
    import torch.nn as nn

    class ScoreStandIn(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.c2 = _trunk()
            self.head = nn.Linear(8, 1)

        def forward(self, A, B, L):
            f = torch.cat([torch.relu(self.c1(A)), torch.relu(self.c1(B))], 1)
            return {"score_logit": self.head(torch.relu(self.c2(f)).mean((2, 3))).reshape(-1, L)}

    net = ScoreStandIn()
    _fill(net, seed, 0.3)
    return net.eval()


# ---------------------------------------------------------------- the loops, composed by hand

def refine_loop(model, cfg, amp, rgb, depth, K, poses, xyz_map, mesh_tensors, mesh_diameter, iteration, glctx=None):
    """predict_pose_refine.py:182-234 from make_crop_data_batch, torch.cat, the model and pose_update."""
    import torch
    from pedp_hip.compat import make_crop_data_batch, pose_update

    poses = torch.as_tensor(poses, device="cuda", dtype=torch.float)
    with torch.inference_mode():
        for _ in range(iteration):
            data = make_crop_data_batch(cfg["input_resize"], poses, None, rgb, depth, K, crop_ratio=cfg.get("crop_ratio", 1.2),
                                        xyz_map=xyz_map, cfg=cfg, glctx=glctx, mesh_tensors=mesh_tensors,
                                        mesh_diameter=mesh_diameter)
            nxt = []
            for b in range(0, len(poses), 1024):
                A = torch.cat([data.rgbAs[b:b + 1024], data.xyz_mapAs[b:b + 1024]], dim=1).float()
                B = torch.cat([data.rgbBs[b:b + 1024], data.xyz_mapBs[b:b + 1024]], dim=1).float()
                with torch.autocast("cuda", enabled=amp):
                    out = model(A, B)
                new, td, rd = pose_update(out["trans"].float(), out["rot"].float(), data.poseA[b:b + 1024], want_deltas=True,
                                          trans_rep=cfg.get("trans_rep", "tracknet"), rot_rep=cfg.get("rot_rep", "axis_angle"),
                                          normalize_xyz=cfg.get("normalize_xyz", False), trans_normalizer=cfg["trans_normalizer"],
                                          rot_normalizer=cfg["rot_normalizer"], mesh_diameter=mesh_diameter)
                nxt.append(new)
            poses = torch.cat(nxt, dim=0)
    return poses, td, rd


def score_once(model, cfg, amp, rgb, depth, K, poses, mesh_tensors, mesh_diameter, glctx=None):
    """predict_score.py:180-210 from make_score_crop_data_batch, torch.cat and the model."""
    import torch
    from pedp_hip.compat import make_score_crop_data_batch

    poses = torch.as_tensor(poses, device="cuda", dtype=torch.float)
    with torch.inference_mode():
        data = make_score_crop_data_batch(cfg["input_resize"], poses, None, rgb, depth, K, crop_ratio=cfg.get("crop_ratio", 1.2),
                                          glctx=glctx, mesh_tensors=mesh_tensors, cfg=cfg, mesh_diameter=mesh_diameter)
        A = torch.cat([data.rgbAs, data.xyz_mapAs], dim=1).float()
        B = torch.cat([data.rgbBs, data.xyz_mapBs], dim=1).float()
        with torch.autocast("cuda", enabled=amp):
            out = model(A, B, L=len(A))
        return out["score_logit"].float().reshape(-1) + 100
