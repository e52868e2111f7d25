"""Times of the pose kernels and the packed crop pass on cuda:0 -> profiles/fpose_time.json (or the path given).

    pose_update          pedp_pose_update against the same update written in torch ops, at B = 1, 252, 1024
    max_pair_distance    pedp_max_pair_distance at n = 10,000 against numpy's all-pairs norm maximum (time, peak memory)
    crop pass            pedp_crop_batch_packed against pedp_crop_batch + torch.cat of A and B, at B = 252, 160 x 160

Call times are CUDA-event means over back-to-back calls from Python after a warm-up (for the small calls that is the
launch path, not the kernel); host times are wall clock.  Kernel times come from a run of its own under rocprofv3:

    rocprofv3 --kernel-trace --output-format csv -d TRACE -- python tools/fpose_time.py OUT.json
    python tools/fpose_time.py --summarize TRACE profiles/fpose_kernel_stats.csv"""
import collections
import csv
import glob
import json
import re
import os
import sys
import time
import tracemalloc

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H_, W_, CROP = 480, 640, 160
K_ = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])

from pedp_hip.pose import max_pair_distance, pose_update, update_params  # noqa: E402


def dev_ms(fn, reps=200, warm=20):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_update(t, r, P, rn, tn):
    x = torch.tanh(r) * rn
    th = (x * x).sum(1).clamp(1e-4).sqrt()
    z = torch.zeros_like(x[:, 0])
    K = torch.stack([z, -x[:, 2], x[:, 1], x[:, 2], z, -x[:, 0], -x[:, 1], x[:, 0], z], 1).view(-1, 3, 3)
    R = (1.0 / th * th.sin())[:, None, None] * K + (1.0 / th * (1.0 / th) * (1 - th.cos()))[:, None, None] * torch.bmm(K, K) \
        + torch.eye(3, device=t.device)
    out = torch.eye(4, device=t.device)[None].expand(len(P), -1, -1).contiguous()
    out[:, :3, 3] = P[:, :3, 3] + torch.tanh(t) * tn
    out[:, :3, :3] = R.permute(0, 2, 1) @ P[:, :3, :3]
    return out


def _rotations(n, rng):
    from pedp_hip import synth

    return np.stack([synth.axis_angle(rng.normal(size=3), rng.uniform(0, np.pi)) for _ in range(n)]).astype(np.float32)


def _scene(B=252):
    """A 100 x 60 bumpy torus rendered at a known pose into a 480 x 640 frame (rgb, depth, xyz map) and B hypotheses
    around it."""
    from pedp_hip import synth
    from pedp_hip.compat import depth2xyzmap_batch, nvdiffrast_render

    v, t, n = synth.bumpy_torus(60, 40)
    v = (v * 0.0008).astype(np.float32)
    rng = np.random.default_rng(0)
    mt = {"pos": torch.as_tensor(v, device="cuda"), "faces": torch.as_tensor(t.astype(np.int32), device="cuda"),
          "vnormals": torch.as_tensor(n.astype(np.float32), device="cuda"),
          "vertex_color": torch.as_tensor(rng.random((len(v), 3), dtype=np.float32), device="cuda")}
    diameter = float(np.linalg.norm(v.max(0) - v.min(0)))
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.01, -0.01, 0.5]
    color, depth, _ = nvdiffrast_render(K=K_, H=H_, W=W_, ob_in_cams=torch.as_tensor(T[None], device="cuda"), mesh_tensors=mt)
    rgb = (color[0] * 255).clamp(0, 255).to(torch.uint8)
    xyz = depth2xyzmap_batch(depth[0][None], K_.astype(np.float32)[None], zfar=np.inf)[0]
    P = np.repeat(T[None], B, 0)
    P[:, :3, :3] = _rotations(B, rng)
    P[:, :3, 3] += rng.normal(0, 0.01, (B, 3))
    return mt, diameter, rgb, depth[0], xyz, torch.as_tensor(P, device="cuda")


def summarize(trace_dir, out_csv):
    """Per (kernel, grid) call count and duration of a rocprofv3 kernel trace, for the kernels this tool times."""
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))[-1]
    keep = re.compile(r"update_kernel|pair_max_kernel|crop_kernel|crop_prep_kernel|cat|elementwise|bmm|gemm|Cijk", re.I)
    groups = collections.defaultdict(list)
    regs = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r"^void |\(anonymous namespace\)::", "", r["Kernel_Name"]).split("(")[0]
        if not keep.search(name):
            continue
        key = (name[:60], r.get("Grid_Size_X", ""), r.get("Grid_Size_Y", ""))
        groups[key].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        regs[key] = (r.get("Arch_VGPR_Count", r.get("VGPR_Count", "")), r.get("SGPR_Count", ""),
                     r.get("Private_Segment_Size", r.get("Scratch_Size", "")))
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "grid_x", "grid_y", "calls", "mean_ns", "min_ns", "max_ns", "vgpr", "sgpr", "scratch"])
        for key, d in sorted(groups.items()):
            w.writerow([*key, len(d), int(sum(d) / len(d)), min(d), max(d), *regs[key]])
    print(open(out_csv).read())


def main(out_path):
    res = {"device": torch.cuda.get_device_name(0), "pose_update": {}, "crop_pass": {}}
    rng = np.random.default_rng(0)
    prm = update_params(trans_normalizer=0.02, rot_normalizer=0.3)
    for B in (1, 252, 1024):
        P = np.zeros((B, 4, 4), np.float32)
        P[:, :3, :3] = _rotations(B, rng)
        P[:, 3, 3] = 1
        P, t, r = (torch.as_tensor(x, device="cuda") for x in (P, rng.normal(size=(B, 3)).astype(np.float32),
                                                              rng.normal(size=(B, 3)).astype(np.float32)))
        out = torch.empty_like(P)
        res["pose_update"][str(B)] = {"hip_ms": dev_ms(lambda: pose_update(t, r, P, prm, out=out)),
                                      "torch_ms": dev_ms(lambda: torch_update(t, r, P, 0.3, 0.02))}
    n = 10000
    p = rng.normal(0, 0.05, (n, 3))
    max_pair_distance(p)
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        got = max_pair_distance(p)
    hip_host_ms = (time.perf_counter() - t0) * 1e3 / reps
    pd = torch.as_tensor(p, device="cuda")
    t0 = time.perf_counter()
    for _ in range(reps):
        max_pair_distance(pd)
    hip_dev_ms = (time.perf_counter() - t0) * 1e3 / reps
    tracemalloc.start()
    t0 = time.perf_counter()
    want = np.linalg.norm(p[None] - p[:, None], axis=-1).max()
    np_ms = (time.perf_counter() - t0) * 1e3
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    res["max_pair_distance"] = {"n": n, "hip_call_ms_host_points": hip_host_ms, "hip_call_ms_device_points": hip_dev_ms,
                                "numpy_ms": np_ms, "numpy_peak_bytes": peak, "bit_equal": bool(got == want)}

    from pedp_hip.crop import _crop_window, crop_pass  # noqa: E402
    from pedp_hip.compat import nvdiffrast_render  # noqa: E402

    mt, diameter, rgb, depth, xyz, P = _scene()
    tf, bbox = _crop_window(P, K_, diameter * 1.2 / 2, CROP, CROP, (CROP - 1, CROP - 1), True)
    extra = {}
    rgb_r, _, _ = nvdiffrast_render(K=K_, H=480, W=640, ob_in_cams=P, mesh_tensors=mt, output_size=(CROP, CROP), bbox2d=bbox,
                                    use_light=True, extra=extra)
    xyz_r = extra["xyz_map"]

    def plain():
        o = crop_pass(0, tf, P, K_, diameter, rgb, rgb_r, xyz_r, xyz_map=xyz)
        return torch.cat([o["rgbA"], o["xyzA"]], 1), torch.cat([o["rgbB"], o["xyzB"]], 1)

    def packed():
        o = crop_pass(0, tf, P, K_, diameter, rgb, rgb_r, xyz_r, xyz_map=xyz, packed=True)
        return o["A"], o["B"]

    res["crop_pass"] = {"B": int(P.shape[0]), "size": CROP, "packed_ms": dev_ms(packed, 50, 5),
                        "unpacked_plus_cat_ms": dev_ms(plain, 50, 5)}
    a, b = packed(), plain()
    res["crop_pass"]["bit_equal"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fpose_time.json"))
