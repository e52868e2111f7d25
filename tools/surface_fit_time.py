"""Times and pose errors of the surface fit on cuda:0 -> profiles/surface_fit_time.json (or the path given).

    python tools/surface_fit_time.py [OUT.json]

Cases (the bumpy torus posed as in the benchmark, points in the camera frame, millimetres):

    frame_100k      the 368,640 points of the 640 x 576 depth frame (rendered by the ray caster, misses on the back plane,
                    0.5 mm noise) against the 100,000-triangle torus
    scattered_100k  1,000 points drawn uniformly from the torus' box, inflated by 50 mm, against the same torus

Times.  fit: the median hipEvent interval around one PEDP_DEVICE pedp_fit_to_surface on a torch stream the context shares
(float64 points resident on the device, T and the statistics written to device memory), after WARM unmeasured calls.
"per pass": the thresholds are set to -1, so exactly PASSES + 1 passes run, and the interval is divided by their number;
"per fit": the default thresholds, with the passes it took read from the statistics afterwards.  Beside it, in the same
run: search, pedp_closest_points of the same points (closest point, distance and face written: what a pass of the fit
asks of it), the same kind of interval; and icp, registration of the same frame against the model's 50,000 vertices with
their normals, point to plane, as the wall clock of the blocking call with the thresholds at -1, divided by its passes.

Pose errors (frame_100k): the rotation (degrees) and translation (mm) error against the pose the frame was rendered at, of
pedp_icp alone from the benchmark's start pose and of pedp_icp followed by the fit against the mesh posed by ICP's answer,
without and with a dent: the object's points within 0.35 rad of azimuth 1.0 (in the model frame) lifted 3 mm along the
torus' outward normal.  Nothing falls back: without a GPU the first call raises."""
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pedp_hip import _lib, surface_fit, synth  # noqa: E402

WARM = 2
REPS = 10
PASSES = 10
GATE = 10.0
LOSSES = {"l2": (0, 0.0), "tukey": (2, 1.5)}


def median(xs):
    return float(np.median(np.asarray(xs)))


def event_ms(stream, call, reps=REPS):
    ms = []
    for k in range(WARM + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        stream.synchronize()
        if k >= WARM:
            ms.append(e0.elapsed_time(e1))
    return ms


def time_fit(ctx, stream, mesh, d_pts, loss, scale, max_iteration, threshold):
    n = len(d_pts)
    out = torch.zeros(16 + surface_fit.STATS_DOUBLES, dtype=torch.float64, device="cuda")
    lib = _lib.load()

    def call():
        _lib.check(lib.pedp_fit_to_surface(ctx._h, mesh._h, C.c_void_p(d_pts.data_ptr()), n, _lib.DEVICE, None, loss, scale, GATE,
                                           max_iteration, threshold, threshold, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(out.data_ptr() + 128), None), "pedp_fit_to_surface")

    ms = event_ms(stream, call)
    stats = out.cpu().numpy()[16:]
    passes = int(stats[2]) + 1
    return {"reps": REPS, "event_ms_median": median(ms), "event_ms_min": float(min(ms)), "passes": passes,
            "event_ms_per_pass": median(ms) / passes, "fitness": float(stats[0]), "rmse": float(stats[1])}


def time_search(ctx, stream, mesh, d_pts):
    n = len(d_pts)
    out = [torch.empty(s, dtype=t, device="cuda") for s, t in (((n, 3), torch.float64), ((n,), torch.float64), ((n,), torch.uint32))]
    ms = event_ms(stream, lambda: mesh.closest_points_device(d_pts.data_ptr(), n, *(o.data_ptr() for o in out)))
    return {"reps": REPS, "event_ms_median": median(ms), "event_ms_min": float(min(ms))}


def rigid(rotvec, t):
    T = np.eye(4)
    T[:3, :3] = synth.axis_angle(rotvec, float(np.linalg.norm(rotvec)))
    T[:3, 3] = t
    return T


def pose_errors(T, want):
    R = T[:3, :3] @ want[:3, :3].T
    return {"rotation_deg": math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0)))),
            "translation_mm": float(np.linalg.norm(T[:3, 3] - want[:3, 3]))}


def dented(scene, T_gt, lift=3.0):
    """The scene with the object's points near azimuth 1.0 lifted along the torus' outward normal; the share lifted."""
    inv = np.linalg.inv(T_gt)
    m = scene @ inv[:3, :3].T + inv[:3, 3]
    az = np.arctan2(m[:, 1], m[:, 0])
    ring = 60.0 * np.stack([np.cos(az), np.sin(az), np.zeros_like(az)], axis=1)
    out_n = m - ring
    dist = np.linalg.norm(out_n, axis=1)
    on_object = dist < 45.0                                         # (the tube's radius is 25 (1 +- 0.15); the back plane is far)
    patch = on_object & (np.abs(np.angle(np.exp(1j * (az - 1.0)))) < 0.35)
    m = m + lift * patch[:, None] * out_n / dist[:, None]
    return np.ascontiguousarray(m @ T_gt[:3, :3].T + T_gt[:3, 3]), float(patch.sum() / max(on_object.sum(), 1))


def icp_then_fit(ctx, f, scene):
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    icp = _lib.icp(ctx, src, tgt, f.max_correspondence_distance, f.icp_init())
    pose_icp = np.linalg.inv(icp["T"])
    row = {"icp": dict(pose_errors(pose_icp, f.T_gt), iters=icp["iters"], fitness=icp["fitness"], rmse=icp["inlier_rmse"])}
    mesh = _lib.Mesh(ctx, f.verts.astype(np.float64), f.tris, posable=True)
    mesh.set_pose(pose_icp)
    for loss, (_, scale) in LOSSES.items():
        fit = surface_fit.fit_to_surface(mesh, scene, loss=loss, scale=scale or None, gate=GATE)
        row[f"icp_then_fit_{loss}"] = dict(pose_errors(surface_fit.refit_pose(pose_icp, fit), f.T_gt), passes=fit.iterations + 1,
                                           fitness=fit.fitness, rmse=fit.inlier_rmse, singular=fit.singular)
    for h in (src, tgt, mesh):
        h.close()
    return row


def time_icp(ctx, f, scene):
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    ms = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        r = _lib.icp(ctx, src, tgt, f.max_correspondence_distance, f.icp_init(), max_iteration=PASSES, relative_fitness=-1,
                     relative_rmse=-1)
        t1 = time.perf_counter()
        if k >= WARM:
            ms.append((t1 - t0) * 1e3)
    src.close()
    tgt.close()
    return {"reps": REPS, "targets": len(f.model_points), "passes": r["iters"] + 1, "wall_ms_median": median(ms),
            "wall_ms_per_pass": median(ms) / (r["iters"] + 1)}


def main(out_path):
    assert torch.cuda.is_available(), "surface_fit_time.py measures on a GPU"
    import _surface_fit_ref as sf

    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    f = synth.Frame("bench_100k")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    v = f.verts_posed.astype(np.float64)
    scattered = np.random.default_rng(0).uniform(v.min(axis=0) - 50.0, v.max(axis=0) + 50.0, (1000, 3))
    # the points a little off the mesh, so that the passes have a pose to find
    off = np.linalg.inv(rigid(np.deg2rad(0.5) * np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0), [0.3, -0.4, 0.3]))
    rows = []
    for case, pts in (("frame_100k", scene), ("scattered_100k", scattered)):
        pts = np.ascontiguousarray(pts @ off[:3, :3].T + off[:3, 3])
        row = {"case": case, "N": len(pts), "F": int(mesh.F), "gate": GATE, "fit": []}
        with torch.cuda.stream(stream):
            d_pts = torch.from_numpy(pts).cuda()
            stream.synchronize()
            for loss, (code, scale) in LOSSES.items():
                fixed = time_fit(ctx, stream, mesh, d_pts, code, scale, PASSES, -1.0)
                whole = time_fit(ctx, stream, mesh, d_pts, code, scale, 30, 1e-6)
                row["fit"].append({"loss": loss, "scale": scale, "per_pass": fixed, "per_fit": whole})
            row["search"] = time_search(ctx, stream, mesh, d_pts)
        row["pass_over_search"] = row["fit"][-1]["per_pass"]["event_ms_per_pass"] / row["search"]["event_ms_median"]
        if case == "frame_100k":
            row["icp"] = time_icp(ctx, f, scene)
            row["fit_pass_over_icp_pass"] = row["fit"][-1]["per_pass"]["event_ms_per_pass"] / row["icp"]["wall_ms_per_pass"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    mesh.close()
    poses = {"clean": icp_then_fit(ctx, f, scene)}
    dent, share = dented(scene, f.T_gt)
    poses["dent"] = dict(icp_then_fit(ctx, f, dent), share_of_object_points_lifted=share, lift_mm=3.0)
    print(json.dumps(poses), flush=True)
    result = {"device": torch.cuda.get_device_name(0),
              "what": "fit: median hipEvent interval of one PEDP_DEVICE pedp_fit_to_surface (ms), per pass with the thresholds "
                      "at -1 and per fit with the default ones; search: the same interval of pedp_closest_points writing "
                      "closest point, distance and face; icp: wall clock of the blocking pedp_icp against the model's "
                      "vertices over its passes; pose_errors: against the pose the frame was rendered at",
              "rows": rows, "pose_errors": poses,
              "test_bound": {"what": "tests/_surface_fit_ref.py: the reference loop with its sums forwards against reversed, "
                                     "measured on the CPU over the tests' five cases (floor), and 100 times that, which the "
                                     "GPU tests allow the device (bound)",
                             "floor_T": sf.FLOOR_T, "floor_rmse": sf.FLOOR_RMSE, "bound_T": sf.BOUND_T, "bound_rmse": sf.BOUND_RMSE}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "surface_fit_time.json"))
