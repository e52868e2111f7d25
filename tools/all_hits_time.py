"""Time the all-hits queries on the bench frame and write profiles/all_hits_time.json.

    python tools/all_hits_time.py [--reps 30] [--warmup 5] [--parent-lib PATH/libpedp_hip.so] [--out profiles/all_hits_time.json]

Bench frame: the 368,640-ray resident set against the 100k-triangle torus.  Everything is timed in device memory, host
wall clock from a synchronised stream to the next synchronise, medians after warm-up:

    count / occlusion / list   the three queries of the ray set (the grid path)
    cast_rayset                the closest-hit cast of the same checkout
    parent cast_rayset         the same cast by the parent commit's library (--parent-lib), alternated with this checkout's
                               in blocks within this one process, so that both see the same machine
    exhaustive, 1,000 rays     count and list of 1,000 rays of scattered origins (every ray against every triangle)

Nothing here is a gate.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(sync, call, reps, warmup):
    for _ in range(warmup):
        call()
    sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "p90_ms": float(a[int(0.9 * (len(a) - 1))]), "reps": len(a)}


class ParentCast:
    """cast_rayset through another build of the library (the parent commit's), device memory."""

    def __init__(self, path, verts, tris, rays_ptr, n, outs):
        self.lib = C.CDLL(path)
        vp = C.c_void_p
        self.lib.pedp_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        self.lib.pedp_mesh_create.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(vp)]
        self.lib.pedp_rayset_create.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(vp)]
        self.lib.pedp_raycast_rayset.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
        self.lib.pedp_ctx_synchronize.argtypes = [vp]
        self.ctx, self.mesh, self.rays = vp(), vp(), vp()
        v = np.ascontiguousarray(verts, np.float32)
        t = np.ascontiguousarray(tris, np.uint32)
        assert self.lib.pedp_ctx_create(0, None, C.byref(self.ctx)) == 0
        assert self.lib.pedp_mesh_create(self.ctx, v.ctypes.data, len(v), t.ctypes.data, len(t), C.byref(self.mesh)) == 0
        assert self.lib.pedp_rayset_create(self.ctx, rays_ptr, n, 1, C.byref(self.rays)) == 0
        self.outs = outs

    def cast(self):
        assert self.lib.pedp_raycast_rayset(self.ctx, self.mesh, self.rays, 1, *self.outs) == 0

    def sync(self):
        self.lib.pedp_ctx_synchronize(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "all_hits_time.json"))
    a = ap.parse_args()

    import torch
    from pedp_hip import _lib, synth

    f = synth.Frame("bench_100k")
    ctx = _lib.Context(0)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    n = f.n_rays
    d_rays = torch.from_numpy(f.rays6).cuda()
    rs = _lib.RaySet(ctx, device_ptr=d_rays.data_ptr(), n=n)
    t, ids, uv = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, 2), device="cuda")
    counts, occ = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    vp = C.c_void_p
    total = C.c_int64()

    def make_list(rays_handle, n_rays, by_set, cap):
        bufs = [torch.empty(n_rays + 1, dtype=torch.int64, device="cuda"), torch.empty(max(cap, 1), dtype=torch.int64, device="cuda"),
                torch.empty(max(cap, 1), device="cuda"), torch.empty(max(cap, 1), dtype=torch.int32, device="cuda"),
                torch.empty((max(cap, 1), 2), device="cuda")]
        ptrs = [vp(b.data_ptr()) for b in bufs]

        def call():
            if by_set:
                rc = lib.pedp_list_intersections_rayset(ctx._h, mesh._h, rays_handle, _lib.DEVICE, cap, *ptrs, C.byref(total))
            else:
                rc = lib.pedp_list_intersections(ctx._h, mesh._h, vp(rays_handle), n_rays, _lib.DEVICE, cap, *ptrs, C.byref(total))
            assert rc == 0 or cap == 0
        call.bufs = bufs
        return call

    make_list(rs._h, n, True, 0)()             # sizes the list
    m_set = total.value
    out = {"frame": "bench_100k", "rays": int(n), "triangles": int(f.n_tris), "list_entries": int(m_set), "timing": "host wall clock, "
           "synchronised stream to synchronise, device memory", "queries": {}}
    this_cast = lambda: mesh.cast_rayset_device(rs, t.data_ptr(), ids.data_ptr(), uv.data_ptr())   # noqa: E731
    jobs = {"count_intersections": lambda: mesh.count_intersections_rayset_device(rs, counts.data_ptr()),
            "test_occlusions": lambda: mesh.test_occlusions_rayset_device(rs, occ.data_ptr()),
            "list_intersections": make_list(rs._h, n, True, m_set),
            "cast_rayset": this_cast}
    for name, call in jobs.items():
        out["queries"][name] = stats(timed(ctx.synchronize, call, a.reps, a.warmup))
        out["queries"][name]["path"] = list(_lib.intersections_last_path(ctx)) if name != "cast_rayset" else list(rs.last_variant())
    out["rays_hit"] = int((counts > 0).sum().item())
    out["max_count"] = int(counts.max().item())

    if a.parent_lib:
        pt, pid, puv = torch.empty_like(t), torch.empty_like(ids), torch.empty_like(uv)
        parent = ParentCast(a.parent_lib, f.verts_posed, f.tris, vp(d_rays.data_ptr()), n, [vp(pt.data_ptr()), vp(pid.data_ptr()), vp(puv.data_ptr())])
        blocks = {"parent": [], "this": []}
        for _ in range(4):                       # parent, this, parent, this, ...
            blocks["parent"].append(stats(timed(parent.sync, parent.cast, a.reps, a.warmup))["median_ms"])
            blocks["this"].append(stats(timed(ctx.synchronize, this_cast, a.reps, a.warmup))["median_ms"])
        same = bool(torch.equal(pt.view(torch.int32), t.view(torch.int32)) and torch.equal(pid, ids) and
                    torch.equal(puv.view(torch.int32), uv.view(torch.int32)))
        out["cast_rayset_alternated"] = {"parent_block_medians_ms": blocks["parent"], "this_block_medians_ms": blocks["this"],
                                         "parent_spread_ms": float(max(blocks["parent"]) - min(blocks["parent"])),
                                         "this_minus_parent_ms": float(np.median(blocks["this"]) - np.median(blocks["parent"])),
                                         "same_bits": same}

    rng = np.random.default_rng(5)
    centre = f.verts_posed.mean(axis=0)
    k = 1000
    scattered = np.empty((k, 6), np.float32)
    scattered[:, :3] = centre + rng.normal(0, 1, (k, 3)) * 300.0
    scattered[:, 3:] = centre + rng.normal(0, 40.0, (k, 3)) - scattered[:, :3]
    d_sc = torch.from_numpy(scattered).cuda()
    sc_counts = torch.empty(k, dtype=torch.int32, device="cuda")
    make_list(d_sc.data_ptr(), k, False, 0)()
    m_sc = total.value
    ex = {"count_intersections": lambda: mesh.count_intersections_device(d_sc.data_ptr(), k, sc_counts.data_ptr()),
          "list_intersections": make_list(d_sc.data_ptr(), k, False, m_sc)}
    out["exhaustive_1000_scattered"] = {"list_entries": int(m_sc)}
    for name, call in ex.items():
        out["exhaustive_1000_scattered"][name] = stats(timed(ctx.synchronize, call, a.reps, a.warmup))
        out["exhaustive_1000_scattered"][name]["path"] = list(_lib.intersections_last_path(ctx))

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
