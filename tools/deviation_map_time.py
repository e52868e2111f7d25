"""Times of the deviation map on cuda:0 -> profiles/deviation_map_time.json (or the path given).

    python tools/deviation_map_time.py [OUT.json] [--parent-root CHECKOUT]
    python tools/deviation_map_time.py OUT.json --signed-only [--root CHECKOUT]      (a child of the first form)
    python tools/deviation_map_time.py OUT.json --add-only                           (a child of the first form)

The bench frame: the 368,640 points of the 640 x 576 depth frame (0.5 mm depth noise) against the 100,000-triangle torus
posed as in the benchmark, points in the camera frame, millimetres.

    signed            surface_distance.compute_signed_distance: the search, the vertex table, the sign, one N-sized result
    parent_signed     the same call on the package of CHECKOUT (the parent commit's, built there), in a process of its own
                      within this run: the yardstick of add_points
    add_points        DeviationMap.add_points: the same search, the vertex table, the fused sign + accumulate
    two_searches      the way to the same state without add_points: signed_closest_points (which searches twice) + add
    add               DeviationMap.add alone on resident rows: `natural` (the frame's own rows) and `piled` (every row on one
                      of two faces), with the in-wave combine on and, in a process of its own, off (PEDP_DEVIATION_COMBINE=0)
    faces, regions    the read-outs on the host

Every time is host wall clock around the blocking operation (the call on resident CUDA tensors on a torch stream the
context shares, then the stream's wait), the median of REPS runs after WARM unmeasured ones.

clean_part: the faces of a part WITHOUT defects that are marked after 1, 4 and 16 noisy frames -- by a peak over frames
(DefectMap fed the same rows with |d| as intensity: peak > LIMIT) and by the deviation map (|mean| > LIMIT; |mean| > 0 at
z = 4; both again over the faces with at least MIN_SAMPLES rows; and |mean| > LIMIT / 3 at z = 4 over those).  Nothing falls back: without a GPU the first call raises."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 3, 15
GATE, LIMIT, Z = 10.0, 1.5, 4.0        # mm: the back plane is gated out; 1.5 mm is three sigma of the depth noise
MIN_SAMPLES = 8                        # a face with one row has no spread: the z rule needs min_samples beside it


def wall_ms(fn):
    ms = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= WARM:
            ms.append((t1 - t0) * 1e3)
    return {"wall_ms_median": float(np.median(ms)), "wall_ms_min": float(min(ms)), "reps": REPS}


def child(out, *flags, env=None):
    """This script once more in a process of its own; its JSON."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out, *flags], env=dict(os.environ, **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()
    return json.load(open(out))


def time_adds(dm, prim, sdist, stream):
    """add alone: the frame's own rows, and every row piled on one of two faces."""
    piled = (torch.arange(len(prim), device=prim.device, dtype=torch.int32) // 64) % 2      # whole waves on one face
    out = {}
    for name, ids in (("natural", prim), ("piled", piled)):
        def add():
            dm.add(ids, sdist, gate=GATE)
            stream.synchronize()
        out[name] = wall_ms(add)
        dm.clear()
    return out


def main(argv):
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out", nargs="?", default=os.path.join(HERE, "profiles", "deviation_map_time.json"))
    ap.add_argument("--parent-root", help="the parent commit's checkout, built: compute_signed_distance there is the yardstick")
    ap.add_argument("--signed-only", action="store_true", help="time compute_signed_distance alone")
    ap.add_argument("--add-only", action="store_true", help="time add alone")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed")
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.root))
    from pedp_hip import _lib, surface_distance as sd, synth

    assert torch.cuda.is_available(), "deviation_map_time.py measures on a GPU"
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    f = synth.Frame("bench_100k")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    model = f.verts.astype(np.float64)
    solid = _lib.Solid(ctx, model, f.tris)
    assert solid.info["closed"] == 1
    t_hit = mesh.cast_rays(f.rays6, want_uv=False)["t_hit"]
    result = {"device": torch.cuda.get_device_name(0), "N": int(len(t_hit)), "F": int(mesh.F),
              "what": "host wall clock (ms), median of %d runs after %d unmeasured ones: the call on resident CUDA tensors and "
                      "the stream's wait" % (REPS, WARM)}
    with torch.cuda.stream(stream):
        pts = torch.from_numpy(f.scene(t_hit)).cuda()
        stream.synchronize()
        keep = {}

        def signed():
            keep["s"] = sd.compute_signed_distance(mesh, pts, solid)
            stream.synchronize()

        if a.signed_only:
            result["signed"] = wall_ms(signed)
        else:
            from pedp_hip import DefectMap, DeviationMap

            defects = DefectMap((model, f.tris), ctx)
            dm = DeviationMap(defects, ctx)
            both = sd.signed_closest_points(mesh, pts, solid)
            prim, sdist = both["primitive_ids"].view(torch.int32), both["signed_distances"]
            result["combine"] = os.environ.get("PEDP_DEVIATION_COMBINE", "1") != "0"
            result["add"] = time_adds(dm, prim, sdist, stream)
            if not a.add_only:
                def add_points(origin=None):
                    dm.add_points(mesh, pts, solid, gate=GATE, origin=origin)
                    stream.synchronize()

                def two_searches():
                    out = sd.signed_closest_points(mesh, pts, solid)
                    dm.add(out["primitive_ids"].view(torch.int32), out["signed_distances"], gate=GATE)
                    stream.synchronize()

                result["signed"] = wall_ms(signed)
                if a.parent_root:
                    result["parent_signed"] = child(a.out + ".parent", "--signed-only", "--root", a.parent_root)["signed"]
                    os.remove(a.out + ".parent")
                result["signed_again"] = wall_ms(signed)          # around the child: the drift of the yardstick itself
                result["add_points"] = wall_ms(add_points)
                result["add_points_origin"] = wall_ms(lambda: add_points((0.0, 0.0, 0.0)))
                result["two_searches"] = wall_ms(two_searches)
                yard = result.get("parent_signed", result["signed"])["wall_ms_median"]
                result["add_points_over_parent_signed" if a.parent_root else "add_points_over_signed"] = \
                    result["add_points"]["wall_ms_median"] / yard
                result["two_searches_over_add_points"] = result["two_searches"]["wall_ms_median"] / result["add_points"]["wall_ms_median"]
                # the same state either way
                dm.clear()
                dm.add_points(mesh, pts, solid, gate=GATE)
                one = dm.faces()
                dm.clear()
                dm.add(prim, sdist, gate=GATE)
                two = dm.faces()
                result["add_points_has_the_state_of_two_searches"] = all(one[k].tobytes() == two[k].tobytes() for k in one)
                result["rows"] = dm.stats()
                result["faces"] = wall_ms(dm.faces)
                result["regions"] = wall_ms(lambda: dm.regions(0.2, min_samples=2))
                result["regions_found"] = int(dm.regions(0.2, min_samples=2)["n_regions"])
                off = child(a.out + ".off", "--add-only", env={"PEDP_DEVIATION_COMBINE": "0"})
                os.remove(a.out + ".off")
                assert off["combine"] is False
                result["add_combine_off"] = off["add"]
                # a clean part under the sensor's noise: what a peak over frames marks, and what the mean marks
                dm.clear()
                defects.clear()
                clean = []
                for k in range(16):
                    p = torch.from_numpy(synth.scene_from_depth(t_hit, f.dirs, seed=100 + k)).cuda()
                    out = sd.signed_closest_points(mesh, p, solid)
                    ids, d = out["primitive_ids"].view(torch.int32), out["signed_distances"]
                    dm.add(ids, d, gate=GATE)
                    heat = torch.where(d.abs() <= GATE, d.abs(), torch.full_like(d, float("nan")))     # the gate of the heat image
                    defects.add(ids, heat)
                    if k + 1 in (1, 4, 16):
                        faces = dm.faces()
                        clean.append({"frames": k + 1, "faces_measured": int((faces["n"] > 0).sum()),
                                      "marked_by_peak": int((defects.faces()["peak"] > LIMIT).sum()),
                                      "marked_by_mean": int(dm.summary(threshold=LIMIT)["marked_faces"]),
                                      "marked_by_mean_at_z": int(dm.summary(threshold=0.0, z=Z)["marked_faces"]),
                                      "faces_with_min_samples": int((faces["n"] >= MIN_SAMPLES).sum()),
                                      "marked_by_mean_min_samples": int(dm.summary(threshold=LIMIT, min_samples=MIN_SAMPLES)["marked_faces"]),
                                      "marked_by_mean_at_z_min_samples": int(dm.summary(threshold=0.0, z=Z, min_samples=MIN_SAMPLES)["marked_faces"]),
                                      "marked_by_mean_and_z_min_samples": int(dm.summary(threshold=LIMIT / 3, z=Z, min_samples=MIN_SAMPLES)["marked_faces"]),
                                      "median_samples": float(np.median(faces["n"][faces["n"] > 0])),
                                      "largest_abs_mean_mm": float(dm.summary()["max_abs_mean"])})
                result["clean_part"] = {"limit_mm": LIMIT, "z": Z, "gate_mm": GATE, "noise_sigma_mm": 0.5, "min_samples": MIN_SAMPLES,
                                        "after": clean}
            dm.close()
            defects.close()
    solid.close()
    mesh.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(a.out)


if __name__ == "__main__":
    main(sys.argv[1:])
