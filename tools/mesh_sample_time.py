"""Times of the surface sampler on cuda:0 -> profiles/mesh_sample_time.json (or the path given).

    python tools/mesh_sample_time.py [OUT.json]
    python tools/mesh_sample_time.py --restatement [OUT.json]     # the numpy / scipy restatement alone; needs no GPU

The model is the bumpy 100,000-triangle torus of the benchmark configurations (synth.Frame("bench_100k")), in device
memory; the sampler handle is built once, outside the timed spans (its own time is the row `create`).

    uniform     pedp_mesh_sample: 1,000,000 samples with face ids and barycentrics, one launch
    spacing     pedp_mesh_sample_disk at the spacing that keeps about 50,000 points (found by one trial at
                sqrt(0.54 area / 50,000) and one correction), and pedp_mesh_sample_disk_read of the kept rows
    count       pedp_mesh_sample_disk for number_of_points = 50,000 (250,000 samples, 24 halvings), and the read

Every time is the interval between two events on the context's stream around the call, warm, the median of REPS calls.
The thinning calls wait for the stream once per group of rounds and once per count, so their intervals include those
waits: they are what a caller sees.  Rounds per thinning and thinnings per count form are reported beside the times.

--restatement times tests/_sample_ref.py on the same inputs, once each, on the host: context, not credit.
Nothing falls back: without a GPU the first call raises."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pedp_hip import _lib, synth  # noqa: E402
import _sample_ref as ref  # noqa: E402

WARM = 2
REPS = 20
UNIFORM = 1000000
KEEP = 50000


def model():
    f = synth.Frame("bench_100k")
    return np.ascontiguousarray(f.verts, np.float64), np.ascontiguousarray(f.tris, np.uint32)


def first_spacing(area):
    return float(np.sqrt(0.54 * area / KEEP))


def corrected(r, kept):
    return float(r * np.sqrt(kept / KEEP))


def restatement(out_path):
    v, t = model()
    rows = {}

    def timed(name, call):
        t0 = time.perf_counter()
        out = call()
        rows[name] = {"wall_ms": (time.perf_counter() - t0) * 1e3}
        print(name, rows[name], flush=True)
        return out

    timed("uniform", lambda: ref.sample(v, t, UNIFORM))
    area = ref.face_table(v, t)[5]
    r = first_spacing(area)
    r = corrected(r, len(ref.sample_disk(v, t, spacing=r)["index"]))
    d = timed("spacing", lambda: ref.sample_disk(v, t, spacing=r))
    rows["spacing"].update(spacing=r, drawn=d["drawn"], kept=len(d["index"]))
    d = timed("count", lambda: ref.sample_disk(v, t, KEEP))
    rows["count"].update(spacing=d["spacing"], drawn=d["drawn"], kept=len(d["index"]))
    with open(out_path, "w") as fh:
        json.dump({"what": "tests/_sample_ref.py on the host, one run each, wall clock (ms)", "rows": rows}, fh, indent=1)
        fh.write("\n")
    print(out_path)


def main(out_path):
    import torch

    assert torch.cuda.is_available(), "mesh_sample_time.py measures on a GPU"
    from pedp_hip.mesh_sample import MeshSampler

    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    lib = _lib.load()
    v, t = model()
    dev = torch.device("cuda:0")

    def events(call, reps=REPS):
        ms = []
        with torch.cuda.stream(stream):
            for k in range(WARM + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                if k >= WARM:
                    ms.append(e0.elapsed_time(e1))
        return {"reps": reps, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}

    rows = {}
    with torch.cuda.stream(stream):
        tv, tt = torch.from_numpy(v).to(dev), torch.from_numpy(t.view(np.int32)).to(dev)
        stream.synchronize()
        made = []
        rows["create"] = events(lambda: made.append(MeshSampler((tv, tt), ctx)), reps=5)
        for s in made[:-1]:
            s.close()
        s = made[-1]
        rows["create"].update(faces=s.n_faces, unsampled_faces=s.unsampled_faces, area=s.area)

        pts, bary = torch.empty((UNIFORM, 3), dtype=torch.float64, device=dev), torch.empty((UNIFORM, 3), dtype=torch.float64, device=dev)
        face = torch.empty(UNIFORM, dtype=torch.int32, device=dev)
        rows["uniform"] = events(lambda: _lib.check(lib.pedp_mesh_sample(s._h, 0, 0, UNIFORM, 0, _lib.DEVICE, C.c_void_p(pts.data_ptr()),
                                                                         C.c_void_p(face.data_ptr()), C.c_void_p(bary.data_ptr()), None),
                                                    "pedp_mesh_sample"))
        rows["uniform"]["samples"] = UNIFORM

        got = {}

        def disk(n, r):
            count, drawn, r_out, rounds, probes = C.c_int64(), C.c_int64(), C.c_double(), C.c_int32(), C.c_int32()
            _lib.check(lib.pedp_mesh_sample_disk(s._h, 0, n, r, 5, 0, C.byref(count), C.byref(drawn), C.byref(r_out), C.byref(rounds),
                                                 C.byref(probes)), "pedp_mesh_sample_disk")
            got.update(kept=count.value, drawn=drawn.value, spacing=r_out.value, rounds_of_last_thinning=rounds.value, thinnings=probes.value)

        def read():
            k = got["kept"]
            _lib.check(lib.pedp_mesh_sample_disk_read(s._h, _lib.DEVICE, C.c_void_p(pts.data_ptr()), C.c_void_p(face.data_ptr()),
                                                      C.c_void_p(bary.data_ptr()), None, None), "pedp_mesh_sample_disk_read")
            return k

        r = first_spacing(s.area)
        disk(0, r)
        r = corrected(r, got["kept"])
        rows["spacing"] = events(lambda: disk(0, r))
        rows["spacing"].update(got)
        rows["spacing_read"] = events(read)
        rows["count"] = events(lambda: disk(KEEP, -1.0))
        rows["count"].update(got)
        rows["count_read"] = events(read)
        s.close()
    for name, row in rows.items():
        print(name, json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0),
              "what": "interval (ms) between two events on the context's stream around each call, device-memory arrays, warm, "
                      f"median of {REPS}; the thinning calls' intervals include their waits for the round counters and the counts",
              "not_measured": ["host-memory calls (uploads and read-backs)", "the Python wrappers and their holders", "meshes above 100,000 faces",
                               "thin_to_spacing on a depth camera's cloud", "a context shared with a running registration"],
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(out_path)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--restatement" in sys.argv:
        restatement(args[0] if args else os.path.join(ROOT, "profiles", "mesh_sample_restatement.json"))
    else:
        main(args[0] if args else os.path.join(ROOT, "profiles", "mesh_sample_time.json"))
