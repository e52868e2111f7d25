"""Timing of the fused crop pass (pedp_crop_batch, the render excluded) at FoundationPose's shapes:
python tools/crop_time.py [--reps R] [--out profiles/crop_time.json].

B = 1, 252 and 512 poses, 160 x 160 crops of a 480 x 640 frame (uint8 rgb as the scorer receives it, float32 depth, xyz
and normal maps), windows from compute_crop_window_tf_batch around poses 0.3-0.45 m away.  Variants: the refiner with and
without use_normal, the scorer; normalize_xyz on.  Against the torch restatement of the reference's kornia composition
on the same GPU (tests/_crop_ref.kornia_warp_perspective: kornia 0.7.2's normalisation, float32 inverse, grid_sample),
with transform_batch in torch; the scorer's includes the frame-sized round trip.  hipEvents around R back-to-back calls
on one explicit stream after 3 warm-ups, the median of 5 such spans.  The floor is the compulsory bytes at 8 TB/s: the
B-side writes (rgb, xyz 24 B/px; + normal 12; scorer + depth 4), the A normalisation (24 B/px read, 24 written).
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import _crop_ref as ref
from pedp_hip import synth
from pedp_hip.crop import _crop_window, crop_pass

H, W, S = 480, 640, 160
K = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])


def poses(n, seed):
    rng = np.random.default_rng(seed)
    P = np.empty((n, 4, 4), np.float32)
    for i in range(n):
        T = np.eye(4)
        T[:3, :3] = synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.pi))
        T[:3, 3] = [rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(0.3, 0.45)]
        P[i] = T
    return P


def torch_reference(variant, use_normal, tf, poseA, rgb, depth, xyz, normal, rgb_r, xyz_r, diameter):
    """predict_*.make_crop_data_batch after the render, then transform_batch, in torch (the kornia calls restated)."""
    B = len(tf)
    kw = dict(align_corners=False)
    out = {"rgbAs": (rgb_r.permute(0, 3, 1, 2) * 255) / 255.0}
    out["rgbBs"] = ref.kornia_warp_perspective(rgb.float().permute(2, 0, 1)[None].expand(B, -1, -1, -1), tf, (S, S),
                                               "bilinear", **kw) / 255.0
    z_inv = 0.1 if variant == 1 else 0.001
    if variant == 0:
        xB = ref.kornia_warp_perspective(xyz.permute(2, 0, 1)[None].expand(B, -1, -1, -1), tf, (S, S), "nearest", **kw)
        if use_normal:
            out["normalBs"] = ref.kornia_warp_perspective(normal.permute(2, 0, 1)[None].expand(B, -1, -1, -1), tf, (S, S),
                                                          "nearest", **kw)
    else:
        dB = ref.kornia_warp_perspective(depth[None, None].expand(B, -1, -1, -1), tf, (S, S), "nearest", **kw)
        out["depthBs"] = dB
        d_ori = ref.kornia_warp_perspective(dB, tf.inverse(), (H, W), "nearest", **kw)[:, 0]
        vs, us = torch.meshgrid(torch.arange(H, device=dB.device), torch.arange(W, device=dB.device), indexing="ij")
        z = d_ori
        x = (us.float() - float(K[0, 2])) * z / float(K[0, 0])
        y = (vs.float() - float(K[1, 2])) * z / float(K[1, 1])
        x_ori = torch.stack([x, y, z], 1)
        x_ori = x_ori * (~(z < 0.001))[:, None]
        xB = ref.kornia_warp_perspective(x_ori, tf, (S, S), "nearest", **kw)
    radius = torch.ones(B, device=tf.device) * diameter / 2
    for name, m in (("xyz_mapAs", xyz_r.permute(0, 3, 1, 2)), ("xyz_mapBs", xB)):
        inv = m[:, 2:3] < z_inv
        m = m - poseA[:, :3, 3].reshape(B, 3, 1, 1)
        m = m * (1 / radius.reshape(B, 1, 1, 1))
        inv = inv.expand(B, 3, -1, -1) | (torch.abs(m) >= 2)
        m[inv] = 0
        out[name] = m
    return out


def timed(call, stream, reps):
    for _ in range(3):
        call()
    spans = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            call()
        e1.record(stream)
        e1.synchronize()
        spans.append(e0.elapsed_time(e1) / reps)
    return float(np.median(spans)), [round(min(spans), 4), round(max(spans), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_time.json"))
    ap.add_argument("--no-torch", action="store_true", help="skip the torch restatement (the kernel trace run)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    rng = np.random.default_rng(0)
    rgb = torch.as_tensor(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), device=dev)
    depth = torch.as_tensor(rng.uniform(0.2, 0.6, (H, W)).astype(np.float32), device=dev)
    xyz = torch.as_tensor(rng.normal(0, 0.2, (H, W, 3)).astype(np.float32), device=dev)
    normal = torch.as_tensor(rng.normal(0, 1, (H, W, 3)).astype(np.float32), device=dev)
    diameter = 0.17
    res = {"what": "fused crop pass (pedp_crop_batch) at 160x160 of 480x640, render excluded; normalize_xyz on",
           "floor_TBps": 8.0, "runs": []}
    for B in (1, 252, 512):
        P = torch.as_tensor(poses(B, B), device=dev)
        tf, _ = _crop_window(P, K, diameter * 1.4 / 2, S, S, (S - 1, S - 1), True)
        rgb_r = torch.rand(B, S, S, 3, device=dev)
        xyz_r = torch.rand(B, S, S, 3, device=dev) * 0.1 + torch.tensor([0, 0, 0.4], device=dev)
        for variant, use_normal, name in ((0, False, "refiner"), (0, True, "refiner+normal"), (1, False, "scorer")):
            def call():
                return crop_pass(variant, tf, P, K, diameter, rgb, rgb_r, xyz_r, xyz_map=xyz, normal_map=normal, depth=depth,
                                 normalize_xyz=True, use_normal=use_normal)
            ms, spread = timed(call, stream, a.reps)
            bpx = 24 + (12 if use_normal else 0) + (4 if variant == 1 else 0) + 48
            floor_ms = B * S * S * bpx / 8e12 * 1e3
            run = {"variant": name, "B": B, "fused_ms": round(ms, 4), "spread_ms": spread, "floor_ms": round(floor_ms, 4),
                   "floor_fraction": round(floor_ms / ms, 3)}
            if not a.no_torch:
                try:
                    tms, _ = timed(lambda: torch_reference(variant, use_normal, tf, P, rgb, depth, xyz, normal, rgb_r, xyz_r,
                                                           diameter), stream, max(1, a.reps // 4))
                    run["torch_reference_ms"] = round(tms, 4)
                    run["speedup"] = round(tms / ms, 1)
                except torch.cuda.OutOfMemoryError:
                    run["torch_reference_ms"] = "out of memory"
                    torch.cuda.empty_cache()
            res["runs"].append(run)
            print(run, file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
