"""Times of next-best-view planning on cuda:0 -> profiles/view_plan_time.json (or the path given).

    python tools/view_plan_time.py [OUT.json]

The 100,000-triangle bumpy torus, a 640 x 576 camera, 42 and 162 candidate poses on a sphere around the part
(orbit_views), a coverage map that has taken two real views:

    add_candidates   ViewPlanner.add_candidates of all V poses (set_pose + cast + observe each, nothing waits), per candidate
    score            ViewPlanner.score(): all V gains against the working state, with the download of the 2 V numbers
    select_8         ViewPlanner.select(8): reset, eight rounds of score / choose / merge, the totals, one wait
    replay_loop      the only way to the same V numbers without the planner: per candidate, clear a scratch CoverageMap,
                     replay the two views of the history, add_view at the candidate's pose, summary.  It alternates call
                     by call with `score` in the same process; its covered-face gains are checked against score's

Every time is the median of hipEvent intervals on the stream the context shares with torch, after WARM unmeasured calls.
Nothing falls back: without a GPU the first call raises."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pedp_hip import CoverageMap, ViewPlanner, _lib, orbit_views, synth  # noqa: E402

WARM = 1
REPS = 7


def timed(stream, calls, reps=REPS):
    """calls: name -> function; they alternate call by call.  name -> dict of its hipEvent intervals' median and minimum."""
    ev = {k: [] for k in calls}
    for rep in range(WARM + reps):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            stream.synchronize()
            if rep >= WARM:
                ev[name].append(e0.elapsed_time(e1))
    return {k: {"reps": reps, "event_ms_median": float(np.median(v)), "event_ms_min": float(min(v))} for k, v in ev.items()}


def case(ctx, stream, f, n_views):
    model = (f.verts.astype(np.float64), f.tris)
    centre = model[0].mean(axis=0)
    radius = float(np.linalg.norm(f.verts_posed.astype(np.float64).mean(axis=0)))          # the benchmark pose's distance
    poses = orbit_views(centre, radius, n_views)
    V, shape = len(poses), (f.height, f.width)
    history = [poses[0], poses[V // 2]]
    with torch.cuda.stream(stream):
        cov, scratch = CoverageMap(model, ctx), CoverageMap(model, ctx)
        mesh = _lib.Mesh(ctx, model[0], model[1], posable=True)
        for T in history:
            cov.add_view(mesh.set_pose(T), f.K, shape)
        planner = ViewPlanner(cov, model, f.K, shape, capacity=V)
        before = cov.summary()
        replayed = {}

        def add_candidates():
            planner.clear()
            planner.add_candidates(poses)

        def replay_loop():
            faces = np.empty(V, np.int64)
            for v, T in enumerate(poses):
                scratch.clear()
                for past in history:
                    scratch.add_view(mesh.set_pose(past), f.K, shape)
                scratch.add_view(mesh.set_pose(T), f.K, shape)
                faces[v] = scratch.summary()["covered_faces"] - before["covered_faces"]
            replayed["gain_faces"] = faces

        r = timed(stream, {"add_candidates": add_candidates})
        r["add_candidates"]["per_candidate_ms_median"] = r["add_candidates"]["event_ms_median"] / V
        planner.reset()
        r.update(timed(stream, {"score": planner.score, "replay_loop": replay_loop}))
        r.update(timed(stream, {"select_8": lambda: planner.select(8)}))
        planner.reset()
        gains, picked = planner.score(), planner.select(8)
    r["candidates"] = V
    r["agree"] = bool(np.array_equal(gains["gain_faces"], replayed["gain_faces"]))
    r["select_8"].update(order=[int(v) for v in picked["order"]], fraction_before=before["fraction"], fraction_after=picked["fraction"])
    r["replay_over_score"] = r["replay_loop"]["event_ms_median"] / r["score"]["event_ms_median"]
    for h in (planner, mesh, scratch, cov):
        h.close()
    return r


def main(out_path):
    assert torch.cuda.is_available(), "view_plan_time.py measures on a GPU"
    stream = torch.cuda.Stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)
    f = synth.Frame("bench_100k")
    result = {"device": torch.cuda.get_device_name(0),
              "what": f"median / minimum hipEvent interval (ms) of {REPS} calls after {WARM} on the stream the context shares with torch; "
                      "score and replay_loop alternate call by call in one process",
              "frame": {"width": f.width, "height": f.height, "F": int(len(f.tris))}}
    for n_views in (42, 162):
        result[f"candidates_{n_views}"] = case(ctx, stream, f, n_views)
        print(json.dumps(result[f"candidates_{n_views}"]), flush=True)
    result["not_measured"] = ["candidates observed from host memory (pedp_view_plan_observe with PEDP_HOST)", "planning under a concurrent registration",
                              "the 1,000,000-triangle torus", "criteria other than the defaults", "more than 162 candidates",
                              "kernel time by rocprofv3 (the intervals hold the launch gaps of the calls they span)"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(out_path)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else os.path.join(ROOT, "profiles", "view_plan_time.json"))
