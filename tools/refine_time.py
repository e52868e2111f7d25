"""Times of refine_mesh on cuda:0 -> profiles/refine_time.json (or the path given).

    python tools/refine_time.py [OUT.json]

Cases:

    cube        the unit cube (12 triangles) at max_edge 0.02: seven rounds to roughly 100,000 faces, the last one a
                1-split of every face (the diagonals alone are still long)
    torus       the bumpy 100,000-triangle torus of the benchmark configurations at max_edge = half its median edge
    no_op       that torus at max_edge = its longest edge: one round's flags, sort and scans find nothing, 0 rounds

Every time is the host wall clock from a synchronised stream to the next synchronise around pedp_mesh_refine with
host-memory arrays (the call waits for the stream once per round, so there is no event interval that would say more),
median of REPS calls after WARM unmeasured ones; the handle is destroyed outside the timed span.

Beside them, measured in the same run, as context and not as credit:

    defect_map_create   DefectMap creation on each output: what the refined model costs the next set-up step
    numpy_restatement   tests/_refine_ref.py's vectorised refine on the host, the only other way to the same arrays

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
import _refine_ref as ref  # noqa: E402

WARM = 2
REPS = 7


def median(xs):
    return float(np.median(np.asarray(xs)))


def wall(stream, call, after=None, reps=REPS):
    ms = []
    for k in range(WARM + reps):
        stream.synchronize()
        t0 = time.perf_counter()
        out = call()
        stream.synchronize()
        t1 = time.perf_counter()
        if after:
            after(out)
        if k >= WARM:
            ms.append((t1 - t0) * 1e3)
    return {"reps": reps, "wall_ms_median": median(ms), "wall_ms_min": float(min(ms))}


def time_case(ctx, stream, name, v, t, max_edge):
    lib = _lib.load()
    v, t = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(t, np.uint32)

    def call():
        h, reached = C.c_void_p(), C.c_int64()
        _lib.check(lib.pedp_mesh_refine(ctx._h, _lib._ptr(v), len(v), _lib._ptr(t), len(t), _lib.HOST, float(max_edge), 1 << 24,
                                        C.byref(h), C.byref(reached)), "pedp_mesh_refine")
        return h

    row = {"case": name, "V_in": int(len(v)), "F_in": int(len(t)), "max_edge": float(max_edge)}
    row["refine"] = wall(stream, call, after=lambda h: lib.pedp_refined_destroy(h))
    from pedp_hip.mesh_refine import refine_mesh

    fine = refine_mesh((v, t), max_edge, ctx=ctx)
    row.update(V_out=int(len(fine.vertices)), F_out=int(len(fine.triangles)), rounds=fine.rounds)
    row["defect_map_create"] = wall(stream, lambda: DefectMap(fine, ctx), after=lambda m: m.close(), reps=5)
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = ref.refine(v, t, max_edge)
        ms.append((time.perf_counter() - t0) * 1e3)
    row["numpy_restatement_wall_ms_median"] = median(ms)
    row["same_bits_as_restatement"] = bool(got[0].tobytes() == fine.vertices.tobytes() and got[1].tobytes() == fine.triangles.tobytes()
                                           and got[2].tobytes() == fine.parent_face.tobytes())
    fine.close()
    return row


def main(out_path):
    assert torch.cuda.is_available(), "refine_time.py measures on a GPU"
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    f = synth.Frame("bench_100k")
    tv, tt = f.verts.astype(np.float64), np.asarray(f.tris)
    p = tv[tt.astype(np.int64)]
    edges = np.sqrt(ref.len2(p, p[:, ref.NXT]))
    rows = []
    for name, v, t, max_edge in (("cube", *ref.cube(), 0.02), ("torus", tv, tt, 0.5 * float(np.median(edges))),
                                 ("no_op", tv, tt, float(edges.max()) * (1.0 + 1e-12))):   # above the square root's rounding
        rows.append(time_case(ctx, stream, name, v, t, max_edge))
        print(json.dumps(rows[-1]), flush=True)
    result = {"device": torch.cuda.get_device_name(0),
              "what": "host wall clock (ms) from a synchronised stream to the next synchronise: pedp_mesh_refine with host arrays "
                      "(handle destroyed outside the span), DefectMap creation on its output, and the numpy restatement on the host",
              "not_measured": ["refine_mesh end to end from Python (the read-back of the arrays and the holder)",
                               "device-memory inputs", "outputs above 1,000,000 faces", "a context shared with a running registration",
                               "pedp_refined_reduce"],
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine_time.json"))
