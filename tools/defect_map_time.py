"""Times of the defect map on cuda:0 -> profiles/defect_map_time.json (or the path given).

    python tools/defect_map_time.py [OUT.json]

Cases (the bumpy torus of the benchmark configurations, 100,000 and 1,000,000 triangles):

    create    pedp_defect_map_create from host arrays: the upload, the faces' geometry, the weld, the edge sort and the
              runs.  The call returns after the build, so both the hipEvent interval and the wall clock cover it
    add       pedp_defect_map_add (PEDP_DEVICE) of the hits of one 640 x 576 frame on the 100,000-triangle torus at the
              benchmark's pose: every pixel's ray that hits (a heat map above the threshold everywhere), ids and
              intensities resident on the device, in the row-major pixel order the projection leaves them in; and
              add_piled, 368,640 rows on 64 faces in sorted order (hits piled onto a few large faces): the shape on which
              the atomics of a row-per-lane kernel contend, which the in-wave combine of equal neighbouring ids answers
              (its A/B against a kernel without it: profiles/defect_map_add_combine_ab.json)
    regions   pedp_defect_map_regions (PEDP_DEVICE labels and table) with 1 %, 30 % and 100 % of the faces marked, drawn
              uniformly, at grow 0 and 2; the call waits for its region count, so event interval and wall clock agree

Every time is the median of hipEvent intervals on the torch stream the context shares, after WARM unmeasured calls.

Beside them, what the package does today to the same end:

    transform_history   run.py:196-201's loop: pedp_transform_points over k stored hit clouds of that frame's size, for
                        k = 1, 10, 100, host wall clock (the map replaces the list: its cost does not grow with k)
    scipy_labelling     the restatement's labelling on the host (tests/_defect_map_ref.py: growth by sparse products and
                        scipy.sparse.csgraph.connected_components on the marked sub-graph; the adjacency given), host
                        wall clock: context, not credit

Nothing falls back: without a GPU the first call raises."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pedp_hip import DefectMap, _lib, synth  # noqa: E402
from pedp_hip.defect_map import REGION_DTYPE  # noqa: E402

WARM = 2
REPS = 10


def median(xs):
    return float(np.median(np.asarray(xs)))


def timed(stream, call, reps=REPS):
    ev, wall = [], []
    for k in range(WARM + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        call()
        e1.record(stream)
        stream.synchronize()
        t1 = time.perf_counter()
        if k >= WARM:
            ev.append(e0.elapsed_time(e1))
            wall.append((t1 - t0) * 1e3)
    return {"reps": reps, "event_ms_median": median(ev), "event_ms_min": float(min(ev)), "wall_ms_median": median(wall)}


def time_create(ctx, stream, verts, tris):
    made = []

    def call():
        made.append(DefectMap((verts, tris), ctx))
        if len(made) > 1:
            made.pop(0).close()

    r = timed(stream, call, reps=5)
    return r, made[-1]


def time_add(ctx, stream, dm, f):
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    heat = np.ones((f.height, f.width))
    hits = mesh.project_heatmap(heat, f.K, threshold=0.5)
    n = len(hits["primitive_ids"])
    with torch.cuda.stream(stream):
        ids = torch.from_numpy(hits["primitive_ids"].view(np.int32).copy()).cuda()
        x = torch.from_numpy(np.random.default_rng(0).uniform(0.0, 1.0, n)).cuda()
        stream.synchronize()
        lib = _lib.load()
        r = timed(stream, lambda: _lib.check(lib.pedp_defect_map_add(dm._h, C.c_void_p(ids.data_ptr()), C.c_void_p(x.data_ptr()), n,
                                                                     _lib.DEVICE), "pedp_defect_map_add"))
    faces = dm.faces()
    r.update(rows=n, faces_hit=int((faces["hits"] > 0).sum()), max_rows_on_a_face=int(faces["hits"].max() // dm.stats()["observations"]))
    piled = np.sort(np.random.default_rng(0).integers(0, 64, f.width * f.height)).astype(np.int32)
    with torch.cuda.stream(stream):
        p_ids = torch.from_numpy(piled).cuda()
        p_x = torch.from_numpy(np.random.default_rng(1).uniform(0.0, 1.0, len(piled))).cuda()
        stream.synchronize()
        rp = timed(stream, lambda: _lib.check(lib.pedp_defect_map_add(dm._h, C.c_void_p(p_ids.data_ptr()), C.c_void_p(p_x.data_ptr()),
                                                                      len(piled), _lib.DEVICE), "pedp_defect_map_add"))
    rp.update(rows=len(piled), faces_hit=64)
    # run.py:196-201: every stored cloud of that frame's size moved by the relative transformation, on the host
    T = synth.start_pose() @ np.linalg.inv(synth.gt_pose())
    history = {}
    cloud = np.ascontiguousarray(hits["points"])
    for k in (1, 10, 100):
        clouds = [cloud.copy() for _ in range(k)]
        ms = []
        for rep in range(WARM + 3):
            t0 = time.perf_counter()
            clouds = [_lib.transform_points(T, c) for c in clouds]
            if rep >= WARM:
                ms.append((time.perf_counter() - t0) * 1e3)
        history[str(k)] = median(ms)
    mesh.close()
    return r, rp, {"points_per_cloud": n, "wall_ms_median_by_k": history}


def time_regions(ctx, stream, dm, share, grow, seed=0):
    F = dm.F
    rng = np.random.default_rng(seed)
    marked = np.arange(F) if share >= 1.0 else np.sort(rng.choice(F, int(F * share), replace=False))
    dm.clear()
    dm.add(marked.astype(np.uint32), np.ones(len(marked)))
    first = dm.regions(grow=grow, capacity=0)
    R = first["n_regions"]
    lib = _lib.load()
    with torch.cuda.stream(stream):
        labels = torch.empty(F, dtype=torch.int32, device="cuda")
        table = torch.empty(max(R, 1) * REGION_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        n = C.c_int64()
        stream.synchronize()
        r = timed(stream, lambda: _lib.check(lib.pedp_defect_map_regions(dm._h, 0.5, 1, grow, _lib.DEVICE, C.c_void_p(labels.data_ptr()),
                                                                         max(R, 1), C.c_void_p(table.data_ptr()), C.byref(n)),
                                             "pedp_defect_map_regions"))
    rows = table.cpu().numpy().view(REGION_DTYPE)[:R]
    r.update(share_marked=share, grow=grow, n_regions=R, largest_region_faces=int(rows["n_faces"].max()) if R else 0,
             faces_in_regions=int((first["labels"] >= 0).sum()))
    return r, marked


def time_scipy(model, marked, grow):
    import _defect_map_ref as ref
    from scipy.sparse.csgraph import connected_components

    mark = np.zeros(model.F, bool)
    mark[marked] = True
    ms = []
    for rep in range(3):
        t0 = time.perf_counter()
        g = ref.grown(model, mark, grow)
        idx = np.nonzero(g)[0]
        connected_components(model.graph[idx][:, idx], directed=False)
        ms.append((time.perf_counter() - t0) * 1e3)
    return median(ms)


def main(out_path):
    assert torch.cuda.is_available(), "defect_map_time.py measures on a GPU"
    import _defect_map_ref as ref

    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    rows = []
    for config in ("bench_100k", "bench_1m"):
        f = synth.Frame(config)
        verts = f.verts.astype(np.float64)
        row = {"config": config, "F": int(len(f.tris)), "V": int(len(verts))}
        row["create"], dm = time_create(ctx, stream, verts, f.tris)
        if config == "bench_100k":
            row["add"], row["add_piled"], row["transform_history"] = time_add(ctx, stream, dm, f)
            model = ref.Model(verts, f.tris)        # the restatement's adjacency (a Python loop over the edges: not timed)
        row["regions"] = []
        for share in (0.01, 0.3, 1.0):
            for grow in (0, 2):
                r, marked = time_regions(ctx, stream, dm, share, grow)
                if config == "bench_100k":
                    r["scipy_labelling_wall_ms"] = time_scipy(model, marked, grow)
                row["regions"].append(r)
        rows.append(row)
        print(json.dumps(row), flush=True)
        dm.close()
    result = {"device": torch.cuda.get_device_name(0),
              "what": "median hipEvent interval (ms) and wall clock of call + stream wait; transform_history: host wall clock of "
                      "pedp_transform_points over k stored hit clouds; scipy_labelling: host wall clock of the restatement's labelling",
              "not_measured": ["add without the in-wave combine (no such kernel is built; its A/B is profiles/defect_map_add_combine_ab.json)",
                               "scipy's labelling at 1,000,000 faces (the restatement's adjacency is a Python loop)",
                               "add and regions under a concurrent registration", "DefectMap.add_projection end to end"],
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "defect_map_time.json"))
