"""Times of the solid's creation and of the signed-distance query on cuda:0 -> profiles/signed_time.json (or the path given).

    python tools/signed_time.py [OUT.json] [--parent PARENT.json]
    python tools/signed_time.py OUT.json --distance-only [--root CHECKOUT]

Creation: _lib.Solid and DefectMap from the same model-frame arrays (both build the weld and the sorted edge slots), at
the 100,000- and the 1,000,000-triangle torus.

Query: surface_distance.compute_signed_distance beside surface_distance.compute_distance on the three shapes of
tools/closest_time.py (the bumpy torus posed as in the benchmark, points in the camera frame, millimetres):

    frame_100k      the 368,640 points of the 640 x 576 depth frame against the 100,000-triangle torus
    frame_1m        the 921,600 points of the 1280 x 720 frame against the 1,000,000-triangle torus
    scattered_100k  1,000 points drawn uniformly from the torus' box, inflated by 50 mm, against the 100,000-triangle torus

Every time is host wall clock around the blocking operation (for a query: the call with a float64 CUDA tensor on a torch
stream the context shares, then the stream's wait), the median of REPS runs after WARM unmeasured ones.

--distance-only times compute_distance alone, and with --root on the package of another checkout (the parent commit's,
built there): its JSON, given back with --parent, is set beside this checkout's times as `parent_distance_ms` and the
ratio signed / parent distance.  Nothing falls back: without a GPU the first call raises."""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 2, 10
CASES = (("frame_100k", "bench_100k"), ("frame_1m", "bench_1m"), ("scattered_100k", "bench_100k"))


def wall_ms(fn):
    ms = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= WARM:
            ms.append((t1 - t0) * 1e3)
    return {"wall_ms_median": float(np.median(ms)), "wall_ms_min": float(min(ms)), "reps": REPS}


def main(argv):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out", nargs="?", default=os.path.join(HERE, "profiles", "signed_time.json"))
    ap.add_argument("--parent", help="the JSON of a --distance-only run on the parent commit's checkout")
    ap.add_argument("--distance-only", action="store_true", help="time compute_distance alone")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed")
    a = ap.parse_args(argv)
    root, out_path, distance_only = os.path.abspath(a.root), a.out, a.distance_only
    parent = {r["case"]: r for r in json.load(open(a.parent))["queries"]} if a.parent else None
    sys.path.insert(0, root)
    from pedp_hip import _lib, surface_distance as sd, synth

    assert torch.cuda.is_available(), "signed_time.py measures on a GPU"
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    creation, queries = [], []
    frames = {}
    for case, config in CASES:
        f = frames.get(config) or frames.setdefault(config, synth.Frame(config))
        mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
        model = f.verts.astype(np.float64)
        solid = None
        if not distance_only:
            if case.startswith("frame"):
                from pedp_hip.defect_map import DefectMap

                row = {"F": int(mesh.F), "V": int(mesh.V),
                       "solid": wall_ms(lambda: _lib.Solid(ctx, model, f.tris).close()),
                       "defect_map": wall_ms(lambda: DefectMap((model, f.tris), ctx).close())}
                row["solid_over_defect_map"] = row["solid"]["wall_ms_median"] / row["defect_map"]["wall_ms_median"]
                creation.append(row)
                print(json.dumps(row), flush=True)
            solid = _lib.Solid(ctx, model, f.tris)
            assert solid.info["closed"] == 1
        if case.startswith("frame"):
            pts = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
        else:
            v = f.verts_posed.astype(np.float64)
            pts = np.random.default_rng(0).uniform(v.min(axis=0) - 50.0, v.max(axis=0) + 50.0, (1000, 3))
        row = {"case": case, "N": len(pts), "F": int(mesh.F)}
        with torch.cuda.stream(stream):
            d = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
            stream.synchronize()
            keep = {}

            def distance():
                keep["d"] = sd.compute_distance(mesh, d)
                stream.synchronize()

            def signed():
                keep["s"] = sd.compute_signed_distance(mesh, d, solid)
                stream.synchronize()

            row["distance"] = wall_ms(distance)
            if not distance_only:
                row["signed"] = wall_ms(signed)
                row["signed_over_distance"] = row["signed"]["wall_ms_median"] / row["distance"]["wall_ms_median"]
                same = torch.equal(keep["s"].abs().view(torch.int64), keep["d"].view(torch.int64))
                row["abs_signed_has_the_distance_bits"] = bool(same)
                row["inside"] = int((keep["s"] < 0).sum())
                if parent is not None:
                    row["parent_distance_ms"] = parent[case]["distance"]["wall_ms_median"]
                    row["signed_over_parent_distance"] = row["signed"]["wall_ms_median"] / row["parent_distance_ms"]
        queries.append(row)
        print(json.dumps(row), flush=True)
        if solid is not None:
            solid.close()
        mesh.close()
    result = {"device": torch.cuda.get_device_name(0),
              "what": "host wall clock (ms), median of %d runs after %d unmeasured ones; creation: the constructor and close(); "
                      "queries: the call on a resident float64 CUDA tensor and the stream's wait" % (REPS, WARM),
              "creation": creation, "queries": queries}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(out_path)


if __name__ == "__main__":
    main(sys.argv[1:])
