"""Timing of the fused renderer (nvdiffrast_render) at FoundationPose's shapes: python tools/render_time.py [--reps R].

N = 1, 252 and 512 poses rendered at 160 x 160 from 640 x 480 crops shaped like FoundationPose's (a square window
around the object, 1.0-1.4 times its projected size), use_light=True and get_normal=True, against the parity torus
(4k triangles) and the bench_100k torus (100k).  Torch tensors on one explicit stream shared with the library; hipEvents
around R back-to-back calls after 3 warm-ups; the median of 5 such spans per call.  The floor is the compulsory write
(colour, depth, normal, xyz: 40 B per pixel) at 8 TB/s.  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pedp_hip import synth
from pedp_hip.compat import nvdiffrast_render


def poses_and_boxes(n, K, seed=0):
    rng = np.random.default_rng(seed)
    P = np.empty((n, 4, 4), np.float32)
    B = np.empty((n, 4), np.float32)
    for i in range(n):
        T = np.eye(4)
        T[:3, :3] = synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.pi))
        T[:3, 3] = [rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(0.3, 0.45)]
        P[i] = T
        u = K[0, 0] * T[0, 3] / T[2, 3] + K[0, 2]
        v = K[1, 1] * T[1, 3] / T[2, 3] + K[1, 2]
        half = rng.uniform(1.0, 1.4) * K[0, 0] * 0.085 / T[2, 3]  # torus outer radius 85 mm
        B[i] = [u - half, v - half, u + half, v + half]
    return P, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    K = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
    res = {"what": "nvdiffrast_render 160x160, use_light, get_normal", "floor_TBps": 8.0, "runs": []}
    for config in ("parity", "bench_100k"):
        Wt, Ht = synth.CONFIGS[config][:2]
        v, t, nrm = synth.bumpy_torus(Wt, Ht)
        mt = {"pos": torch.as_tensor(v * 0.001, device=dev, dtype=torch.float32),
              "faces": torch.as_tensor(t.astype(np.int32), device=dev),
              "vnormals": torch.as_tensor(nrm, device=dev, dtype=torch.float32),
              "vertex_color": torch.full((len(v), 3), 0.6, device=dev)}
        for N in (1, 252, 512):
            P, B = poses_and_boxes(N, K, seed=N)
            P, B = torch.as_tensor(P, device=dev), torch.as_tensor(B, device=dev)

            def call():
                return nvdiffrast_render(K=K, H=480, W=640, ob_in_cams=P, mesh_tensors=mt, bbox2d=B, output_size=(160, 160),
                                         use_light=True, get_normal=True, extra={})
            for _ in range(3):
                out = call()
            cover = float((out[1] > 0).float().mean())
            spans = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    call()
                e1.record(stream)
                e1.synchronize()
                spans.append(e0.elapsed_time(e1) / a.reps)
            ms = float(np.median(spans))
            floor_ms = N * 160 * 160 * 40 / 8e12 * 1e3
            res["runs"].append({"mesh": config, "triangles": int(len(t)), "N": N, "ms": round(ms, 4),
                                "spread_ms": [round(min(spans), 4), round(max(spans), 4)], "coverage": round(cover, 3),
                                "write_floor_ms": round(floor_ms, 4), "floor_fraction": round(floor_ms / ms, 3)})
            print(res["runs"][-1], file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
