"""Times of the estimator on cuda:0 -> profiles/estimator_time.json (or the path given), at 576 x 640 and 720 x 1280, a
bumpy torus from synth, stand-in networks of negligible cost (a strided mean and one linear layer).

    guess_translation    the kernel path on the filtered device frame (the call includes the record's read-back) beside the
                         reference-shaped path (the frame's download, then numpy's where / median), alternating in one loop;
                         and both paths for a frame that starts on the host (upload + kernel against numpy alone)
    register             252 hypotheses, 5 iterations, per call
    track_one            2 iterations, per call

Host wall clock around calls that end in a read-back, after a warm-up.  Kernel times, launches and device-to-host copies per
call come from a run of its own under rocprofv3 (no counters in it), which runs each call once between marker launches:

    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d TRACE -- python tools/estimator_time.py --traced
    python tools/estimator_time.py --summarize TRACE profiles/estimator_kernel_stats.csv"""
import collections
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [(576, 640), (720, 1280)]
CROP = 160
PHASES = ["warm-up", "guess_translation 576x640", "register 576x640", "track_one 576x640", "end"]

from pedp_hip.estimator import FoundationPose, PoseRefinePredictor, ScorePredictor, guess_translation  # noqa: E402


class _Refine(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.head = torch.nn.Linear(12, 6)
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)

    def forward(self, A, B):
        o = self.head(torch.cat([A[:, :, ::16, ::16].mean((2, 3)), B[:, :, ::16, ::16].mean((2, 3))], 1))
        return {"trans": o[:, :3], "rot": o[:, 3:]}


class _Score(_Refine):
    def forward(self, A, B, L):
        return {"score_logit": super().forward(A, B)["trans"][:, 0].reshape(-1, L)}


def _setup(H, W):
    from pedp_hip import synth
    from pedp_hip.compat import TriangleMesh, make_mesh_tensors, nvdiffrast_render

    v, t, n = synth.bumpy_torus(60, 40)
    v = v * 0.0008
    mesh = TriangleMesh(v, t)
    mesh.vertex_normals = np.asarray(n, np.float64)
    K = np.array([[W * 0.9, 0, W / 2 - 0.5], [0, W * 0.9, H / 2 - 0.5], [0, 0, 1]])
    cfg = {"input_resize": (CROP, CROP), "trans_normalizer": [0.02, 0.02, 0.05], "rot_normalizer": 0.35}
    est = FoundationPose(v, mesh.vertex_normals, mesh=mesh, refiner=PoseRefinePredictor(_Refine().cuda(), cfg),
                         scorer=ScorePredictor(_Score().cuda(), cfg))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = synth.rot_x(0.4) @ synth.rot_z(0.3)
    T[:3, 3] = [0.01, -0.01, 0.5]
    color, depth, _ = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=torch.as_tensor(T[None], device="cuda"),
                                        mesh_tensors=make_mesh_tensors(mesh))
    rgb = (color[0] * 255).clamp(0, 255).to(torch.uint8).cpu().numpy()
    d = depth[0].cpu().numpy()
    mask = d > 0
    rng = np.random.default_rng(0)
    d = (d + rng.normal(0, 0.002, d.shape).astype(np.float32) * mask + 1.2 * ~mask).astype(np.float32)
    return est, K, rgb, d, mask


def _reference_shaped(depth_d, mask, K):
    """What the reference does with a frame that sits on the device: download it, then estimater.py:136-148 in numpy."""
    depth = depth_d.cpu().numpy()
    vs, us = np.where(mask > 0)
    uc, vc = (us.min() + us.max()) / 2.0, (vs.min() + vs.max()) / 2.0
    zc = np.median(depth[mask.astype(bool) & (depth >= 0.001)])
    return ((np.linalg.inv(K) @ np.asarray([uc, vc, 1]).reshape(3, 1)) * zc).reshape(3)


def _wall_ms(fns, reps, warm=3):
    """Mean and minimum wall-clock milliseconds of each function, the functions taking turns within one loop."""
    for _ in range(warm):
        for f in fns:
            f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [{"mean_ms": float(np.mean(x)), "min_ms": float(np.min(x)), "max_ms": float(np.max(x)), "reps": reps} for x in t]


def _filtered(depth):
    from pedp_hip.compat import bilateral_filter_depth, erode_depth

    return bilateral_filter_depth(erode_depth(torch.as_tensor(depth, device="cuda"), radius=2), radius=2)


def main(out_path):
    res = {"device": torch.cuda.get_device_name(0), "hypotheses": 252, "crop": CROP, "sizes": {}}
    for H, W in SIZES:
        est, K, rgb, depth, mask = _setup(H, W)
        dd = _filtered(depth)
        dh = dd.cpu().numpy()
        same = bool(np.array_equal(guess_translation(dd, mask, K), _reference_shaped(dd, mask, K)))
        dev_kernel, dev_ref = _wall_ms([lambda: guess_translation(dd, mask, K), lambda: _reference_shaped(dd, mask, K)], 40)
        host_kernel, host_numpy = _wall_ms([lambda: guess_translation(dh, mask, K),
                                            lambda: _reference_shaped(torch.from_numpy(dh), mask, K)], 40)
        reg, = _wall_ms([lambda: est.register(K=K, rgb=rgb, depth=depth, ob_mask=mask, iteration=5)], 8, warm=2)
        trk, = _wall_ms([lambda: est.track_one(rgb=rgb, depth=depth, K=K, iteration=2)], 30)
        res["sizes"][f"{H}x{W}"] = {
            "mask_pixels": int(mask.sum()),
            "guess_translation": {"device_frame": {"kernel_path": dev_kernel, "download_plus_numpy": dev_ref},
                                  "host_frame": {"upload_plus_kernel": host_kernel, "numpy": host_numpy}, "equal": same},
            "register_5_iterations": reg, "track_one_2_iterations": trk}
    g = res["sizes"]["576x640"]["guess_translation"]["device_frame"]
    res["kernel_path_faster_at_576x640"] = bool(g["kernel_path"]["mean_ms"] < g["download_plus_numpy"]["mean_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def _marker(k):
    """One launch no other code here makes (a fill of an int16 tensor): the trace is cut into phases at these."""
    torch.empty(1, dtype=torch.int16, device="cuda").fill_(k)
    torch.cuda.synchronize()


def traced():
    H, W = SIZES[0]
    est, K, rgb, depth, mask = _setup(H, W)
    dd = _filtered(depth)
    for _ in range(2):
        guess_translation(dd, mask, K)
        est.register(K=K, rgb=rgb, depth=depth, ob_mask=mask, iteration=5)
        est.track_one(rgb=rgb, depth=depth, K=K, iteration=2)
    torch.cuda.synchronize()
    _marker(1)
    guess_translation(dd, mask, K)
    _marker(2)
    est.register(K=K, rgb=rgb, depth=depth, ob_mask=mask, iteration=5)
    _marker(3)
    est.track_one(rgb=rgb, depth=depth, K=K, iteration=2)
    _marker(4)


def summarize(trace_dir, out_csv):
    """Per phase of the traced run: every kernel's launches and time, and the copies by direction.  Copies that the
    runtime does with a kernel of its own (small read-backs into page-locked memory, device-to-device copies) appear
    among the kernels as __amd_rocclr_copyBuffer, memsets as __amd_rocclr_fillBufferAligned."""
    def rows(pattern):
        paths = sorted(glob.glob(os.path.join(trace_dir, "**", pattern), recursive=True))
        return list(csv.DictReader(open(paths[-1]))) if paths else []

    kernels = sorted(rows("*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    cuts = [int(r["Start_Timestamp"]) for r in kernels if "short" in r["Kernel_Name"] and "Fill" in r["Kernel_Name"]]
    if len(cuts) != len(PHASES) - 1:
        raise SystemExit(f"expected {len(PHASES) - 1} marker launches, found {len(cuts)}")

    def phase(ts):
        return PHASES[sum(ts >= c for c in cuts)]

    groups = collections.defaultdict(list)
    for r in kernels:
        name = re.sub(r"^void |\(anonymous namespace\)::", "", r["Kernel_Name"]).split("(")[0]
        if "Fill" in name and "short" in r["Kernel_Name"]:
            continue
        groups[(phase(int(r["Start_Timestamp"])), "kernel", name[:70])].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for r in rows("*memory_copy_trace.csv"):
        key = (phase(int(r["Start_Timestamp"])), "copy", r.get("Direction", r.get("Kind", "?")))
        groups[key].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["phase", "kind", "name", "calls", "total_ns", "mean_ns"])
        for key, d in sorted(groups.items(), key=lambda kv: (PHASES.index(kv[0][0]), kv[0][1], kv[0][2])):
            if key[0] not in ("warm-up", "end"):
                w.writerow([*key, len(d), sum(d), int(sum(d) / len(d))])
        for p in PHASES[1:-1]:
            n = sum(len(d) for k, d in groups.items() if k[0] == p and k[1] == "kernel")
            w.writerow([p, "total", "kernel launches", n, sum(sum(d) for k, d in groups.items() if k[0] == p and k[1] == "kernel"), ""])
    print(open(out_csv).read())


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
    elif len(sys.argv) > 1 and sys.argv[1] == "--traced":
        traced()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "estimator_time.json"))
