"""Times of the closest-point query on cuda:0 -> profiles/closest_time.json (or the path given).

    python tools/closest_time.py [OUT.json]

Cases (the bumpy torus posed as in the benchmark, points in the camera frame, millimetres):

    frame_100k      the 368,640 points of the 640 x 576 depth frame (rendered by the ray caster, misses on the back plane,
                    0.5 mm noise) against the 100,000-triangle torus: culled and exhaustive
    frame_1m        the 921,600 points of the 1280 x 720 frame against the 1,000,000-triangle torus: culled only
    scattered_100k  1,000 points drawn uniformly from the torus' box, inflated by 50 mm, against the 100,000-triangle torus

The first mode of a case is the default one (pedp_closest_configure 0: a wave per point up to 16384 points, a lane per
point above); "lanes" and "waves" force one of the two culled kernels, so that both are timed on every case.

Each closest-point time is the median of hipEvent intervals around one PEDP_DEVICE call on a torch stream the context
shares (float64 points resident on the device, all five outputs written), after WARM unmeasured calls; pairs_tested is
read after the last call.  Beside it, in the same run: what align_to_surface does for the same purpose, pedp_nn of the
same points against the mesh's vertices as resident clouds (its search structures built by the warm-up), as host wall
clock around the blocking call, and the closest-point call's wall clock (call + stream wait) to set against that.
Nothing falls back: without a GPU the first call raises."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pedp_hip import _lib, synth  # noqa: E402

WARM = 2
MODES = {0: "default", 1: "exhaustive", 2: "lanes", 3: "waves"}


def median(xs):
    return float(np.median(np.asarray(xs)))


def time_closest(ctx, stream, mesh, pts, exhaustive, reps):
    n = len(pts)
    _lib.closest_configure(ctx, exhaustive)
    with torch.cuda.stream(stream):
        d = torch.from_numpy(pts).cuda()
        out = [torch.empty(s, dtype=t, device="cuda") for s, t in (((n, 3), torch.float64), ((n,), torch.float64),
                                                                   ((n,), torch.uint32), ((n, 2), torch.float64), ((n,), torch.int8))]
        stream.synchronize()
        ev_ms, wall_ms = [], []
        for k in range(WARM + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            mesh.closest_points_device(d.data_ptr(), n, *(o.data_ptr() for o in out))
            e1.record(stream)
            stream.synchronize()
            t1 = time.perf_counter()
            if k >= WARM:
                ev_ms.append(e0.elapsed_time(e1))
                wall_ms.append((t1 - t0) * 1e3)
    pairs = _lib.closest_last_stats(ctx)
    _lib.closest_configure(ctx, 0)
    return {"mode": MODES[exhaustive], "reps": reps, "event_ms_median": median(ev_ms), "event_ms_min": float(min(ev_ms)),
            "wall_ms_median": median(wall_ms), "pairs_tested": pairs, "pairs_share_of_NF": pairs / (n * mesh.F)}, out[1].cpu().numpy()


def time_nn(ctx, pts, verts, reps):
    src, tgt = _lib.Cloud(ctx, pts), _lib.Cloud(ctx, verts)
    ms = []
    for k in range(WARM + reps):
        t0 = time.perf_counter()
        idx, d2 = _lib.nn(ctx, src, tgt)
        t1 = time.perf_counter()
        if k >= WARM:
            ms.append((t1 - t0) * 1e3)
    return {"reps": reps, "wall_ms_median": median(ms), "targets": len(verts)}, np.sqrt(d2)


def main(out_path):
    assert torch.cuda.is_available(), "closest_time.py measures on a GPU"
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    rows = []
    for case, config, modes in (("frame_100k", "bench_100k", (0, 1, 3)), ("frame_1m", "bench_1m", (0, 3)),
                                ("scattered_100k", "bench_100k", (0, 2))):
        f = synth.Frame(config)
        mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
        if case.startswith("frame"):
            pts = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
        else:
            v = f.verts_posed.astype(np.float64)
            pts = np.random.default_rng(0).uniform(v.min(axis=0) - 50.0, v.max(axis=0) + 50.0, (1000, 3))
        pts = np.ascontiguousarray(pts)
        row = {"case": case, "N": len(pts), "F": int(mesh.F), "V": int(mesh.V), "closest": []}
        dist = {}
        for exhaustive in modes:
            r, dist[exhaustive] = time_closest(ctx, stream, mesh, pts, exhaustive, 3 if exhaustive == 1 else 10)
            row["closest"].append(r)
        row["all_modes_same_distances"] = all(np.array_equal(dist[0], d, equal_nan=True) for d in dist.values())
        row["nn_vertices"], dv = time_nn(ctx, pts, f.verts_posed.astype(np.float64), 10)
        row["max_vertex_minus_surface_distance"] = float(np.nanmax(dv - dist[0]))
        row["min_vertex_minus_surface_distance"] = float(np.nanmin(dv - dist[0]))
        row["nn_wall_over_closest_wall"] = row["nn_vertices"]["wall_ms_median"] / row["closest"][0]["wall_ms_median"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        mesh.close()
    result = {"device": torch.cuda.get_device_name(0),
              "what": "closest: median hipEvent interval of one PEDP_DEVICE call (ms) and the wall clock of call + stream "
                      "wait; nn_vertices: wall clock of the blocking pedp_nn of the same points against the mesh's vertices",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "closest_time.json"))
