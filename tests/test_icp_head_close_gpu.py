"""Steady ICP passes closed at the head of the next launch (GPU).

A steady pass of a single fused registration ends with its partial sums; every workgroup of the next launch sums them,
solves and updates the pose before it transforms its chunk (csrc/icp/fused_close.h).  Rebuild passes and
the last pass close in their own launch.  Every workgroup runs the float64 sequence the in-launch close runs, so the
bound is the strictest there is: the raw bytes of transformation, fitness, rmse, iteration count, trace and
correspondences equal those of
  PEDP_ICP_HEAD_CLOSE=0     every pass closed in its own launch
  PEDP_ICP_SERIAL_CLOSE=1   the close on one lane (which also keeps every close in its launch)
The switches are read once per process: one child process per setting.  pedp_icp_last_head_closed shows that the path
under test ran: passes - rebuild passes - 1 head closes by default (a registration that its criteria stop has no last
in-launch pass: passes - rebuild passes), none with either switch.

The library replays captured graphs only for registrations on the segmented path (uniform batches beyond the fused
pass's radius); that case is here as one of the paths that keep today's close -- two start poses, one capture."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RADIUS = 10.0

_PROBE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle")
from pedp_hip import _lib, synth
ctx = _lib.Context(0)
picked = dict(np.load(sys.argv[3]))
out = {}
FIXED = dict(relative_fitness=-1, relative_rmse=-1)

def put(name, r, c=ctx):
    for k in ("T", "trace", "corr"):
        out[name + "_" + k] = r[k]
    out[name + "_fit"] = np.float64(r["fitness"]); out[name + "_rmse"] = np.float64(r["inlier_rmse"]); out[name + "_iters"] = np.int64(r["iters"])
    head, rebuilds, launches = _lib.icp_last_head_closed(c, rebuilds=True)
    out[name + "_path_head"] = np.int64(head); out[name + "_path_rebuilds"] = np.int64(rebuilds); out[name + "_path_launches"] = np.int64(launches)
    out[name + "_path_wide"] = np.int64(_lib.icp_last_serial_path(c)[0])

for config in ("parity", "tiny"):
    f = synth.Frame(config)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    init = f.icp_init()
    kw = dict(want_corr=True, want_trace=True)
    put(config + "_icp", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=20, **kw, **FIXED))
    _lib.icp_begin(ctx, src, tgt, 10.0, init, max_iteration=20, want_trace=True, **FIXED)
    put(config + "_beginend", _lib.icp_end(ctx, want_corr=True))
    for m in (0, 1, 2):
        put(config + "_max%d" % m, _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=m, **kw, **FIXED))
    # criteria that stop the registration long before the limit: launches behind the stop are no-ops, the final state arrives
    put(config + "_early", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=60, relative_fitness=1e-2, relative_rmse=1e-2, **kw))
    _lib.icp_begin(ctx, src, tgt, 10.0, init, max_iteration=60, relative_fitness=1e-2, relative_rmse=1e-2, want_trace=True)
    put(config + "_early_beginend", _lib.icp_end(ctx, want_corr=True))
    put(config + "_p2p", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=6, estimator=_lib.POINT_TO_POINT, **kw, **FIXED))
    # no point of the scene comes near the target: no live chunk in any pass
    nowhere = np.eye(4); nowhere[:3, 3] = 1e4
    put(config + "_nolive", _lib.icp(ctx, src, tgt, 1.0, nowhere, max_iteration=4, **kw, **FIXED))
    # back to back on one context, different iteration limits
    put(config + "_b2b_7", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=7, **kw, **FIXED))
    put(config + "_b2b_12", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=12, **kw, **FIXED))
    # a start pose picked on the CPU: the motion bound asks for a rebuild behind head-closed passes
    if config + "_init" in picked:
        put(config + "_late_rebuild", _lib.icp(ctx, src, tgt, 10.0, picked[config + "_init"], max_iteration=12, **kw, **FIXED))
    if config == "parity":
        # a single registration right behind a fused batch on the same context
        inits = np.stack([np.linalg.inv(T) for T in synth.batched_start_poses(5)])
        T, fit, rmse, its = _lib.icp_batched_ex(ctx, src, tgt, np.full(5, 8.0), inits, max_iteration=15)
        out["batch_T"], out["batch_fit"], out["batch_rmse"], out["batch_its"] = T, fit, rmse, its
        put("after_batch", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=9, **kw, **FIXED))
        # a replayed graph (segmented path: keeps its close): two start poses, one after the other, one capture
        c2 = _lib.Context(0)
        s2, t2 = _lib.Cloud(c2, scene), _lib.Cloud(c2, f.model_points, f.normals)
        for q in range(2):
            T, fit, rmse, its = _lib.icp_batched_ex(c2, s2, t2, np.full(1, 500.0), inits[q:q + 1], max_iteration=6)
            out["graph%d_T" % q], out["graph%d_fit" % q], out["graph%d_rmse" % q], out["graph%d_its" % q] = T, fit, rmse, its
        out["graph_path_captures"] = np.int64(_lib.icp_graph_captures(c2))
np.savez(sys.argv[2], **out)
"""

_SETTINGS = {
    "default": {},
    "head_off": {"PEDP_ICP_HEAD_CLOSE": "0"},
    "serial_close": {"PEDP_ICP_SERIAL_CLOSE": "1"},
}
_SWITCHES = ("PEDP_ICP_HEAD_CLOSE", "PEDP_ICP_SERIAL_CLOSE", "PEDP_ICP_COPY_BRACKET", "PEDP_ICP_UNFUSED_FINISH")


def rebuild_requests(trace, r, lo, hi):
    """Passes of an oracle trace whose close asks for a rebuild, by the motion bound of fused_close.h: the sums of
    |R - I|_F and of |t + (R - I) c| over the updates since the last rebuild, c the centre of the target's box, against
    0.95 x margin (margin = 2 r, reach E = r + margin + the box's half diagonal).  Also mu / (0.95 margin) per pass."""
    margin = 2.0 * r
    c = 0.5 * (lo + hi)
    reach = r + margin + np.sqrt((0.25 * (hi - lo) ** 2).sum())
    th = ta = 0.0
    asked, ratio = [], []
    for p in range(len(trace) - 1):
        U = trace[p + 1, 2:].reshape(4, 4) @ np.linalg.inv(trace[p, 2:].reshape(4, 4))
        D = U[:3, :3] - np.eye(3)
        th += np.sqrt((D * D).sum())
        ta += np.linalg.norm(U[:3, 3] + D @ c)
        ratio.append((th * reach + ta) / (0.95 * margin))
        if not ratio[-1] < 1.0:
            asked.append(p)
            th = ta = 0.0
    return asked, ratio


def pick_late_rebuild(config, oracle):
    """A start pose whose registration (12 iterations) asks for a rebuild at the close of a pass >= 2 -- the rebuild
    pass is >= 3 and follows a head-closed pass -- and not at the last two passes.  No decision of the bound up to
    there is closer than 10 % to its threshold: the device's trace differs from the oracle's by rounding only.
    (An oracle registration of these frames takes about 10 ms: the whole search stays near a second.)"""
    from pedp_hip import synth

    f = synth.Frame(config)
    scene = f.scene(oracle.raycast(f.verts_posed, f.tris, f.rays6)["t_hit"])
    lo, hi = f.model_points.min(0), f.model_points.max(0)
    for d in ((6.0, -5.0, 4.0), (-3.0, 7.0, 2.0), (5.0, 5.0, -6.0), (1.0, -8.0, -3.0)):
        d = np.asarray(d) / np.linalg.norm(d)
        for s in range(6, 61, 2):
            init = f.icp_init().copy()
            init[:3, 3] += s * d
            ro = oracle.icp(scene, f.model_points, f.normals, RADIUS, init, max_iter=12, rel_fitness=-1, rel_rmse=-1)
            asked, ratio = rebuild_requests(ro["trace"], RADIUS, lo, hi)
            late = [p for p in asked if 2 <= p <= 9]
            if late and all(abs(v - 1.0) > 0.1 for v in ratio[: late[0] + 1]):
                return init, asked
    return None, None


@pytest.fixture(scope="module")
def probes(tmp_path_factory, oracle):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("head_close")
    picked, asked = {}, {}
    for config in ("parity", "tiny"):
        init, a = pick_late_rebuild(config, oracle)
        if init is not None:
            picked[config + "_init"], asked[config] = init, a
    np.savez(str(tmp / "picked.npz"), **picked)
    res = {"asked": asked}
    for name, extra in _SETTINGS.items():
        out = str(tmp / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", _PROBE, root, out, str(tmp / "picked.npz")], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        res[name] = dict(np.load(out))
    return res


@pytest.mark.parametrize("setting", ["head_off", "serial_close"])
def test_every_bit_equals_the_in_launch_close(probes, setting):
    new, old = probes["default"], probes[setting]
    assert set(new) == set(old)
    compared = 0
    for k in sorted(new):
        if "_path_" in k:
            continue
        a, b = np.ascontiguousarray(new[k]), np.ascontiguousarray(old[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
        compared += 1
    assert compared >= 2 * 12 * 6 + 6 + 4 + 8
    assert new["parity_icp_trace"].shape == (21, 18) and new["tiny_icp_trace"].shape == (21, 18)


_FIXED = ["icp", "beginend", "max0", "max1", "max2", "p2p", "nolive", "b2b_7", "b2b_12"]
_LIMIT = {"icp": 20, "beginend": 20, "max0": 0, "max1": 1, "max2": 2, "p2p": 6, "nolive": 4, "b2b_7": 7, "b2b_12": 12, "late_rebuild": 12}


def _box(config, _cache={}):
    from pedp_hip import synth

    if config not in _cache:
        m = synth.Frame(config).model_points
        _cache[config] = (m.min(0), m.max(0))
    return _cache[config]


def test_the_head_close_was_in_force(probes):
    """Head-closed passes = passes - rebuild passes - 1 (rebuild passes: pass 0 and the pass behind every rebuild asked
    for; the last pass closes in its launch -- where it is a rebuild pass itself it counts once) wherever the
    registration runs to its limit; every pass was closed by the wide close; none at a head with either switch set."""
    d = probes["default"]
    names = [c + "_" + n for c in ("parity", "tiny") for n in _FIXED] + ["after_batch"]
    for name in names:
        limit = 9 if name == "after_batch" else _LIMIT[name.split("_", 1)[1]]
        passes, rebuilds = int(d[name + "_iters"]) + 1, int(d[name + "_path_rebuilds"])
        assert passes == limit + 1, name
        config = "parity" if name == "after_batch" else name.split("_", 1)[0]
        asked, _ = rebuild_requests(d[name + "_trace"], 1.0 if name.endswith("nolive") else RADIUS, *_box(config))
        assert len(asked) == rebuilds, (name, asked, rebuilds)
        in_launch = {0, passes - 1} | {p + 1 for p in asked}
        assert int(d[name + "_path_head"]) == passes - len(in_launch), (name, passes, asked, int(d[name + "_path_head"]))
        assert int(d[name + "_path_wide"]) == passes, name
        for off in ("head_off", "serial_close"):
            assert int(probes[off][name + "_path_head"]) == 0, (off, name)
            assert int(probes[off][name + "_path_rebuilds"]) == rebuilds, (off, name)
    assert int(d["parity_icp_path_head"]) >= 15 and int(d["tiny_nolive_path_head"]) == 3 and int(d["parity_nolive_path_head"]) == 3
    assert int(d["parity_max0_path_head"]) == 0 and int(d["parity_max1_path_head"]) == 0


def test_a_head_close_ends_the_registration(probes):
    """Criteria of 1e-2: the close that meets them is a head close (or a rebuild pass's own) -- there is no last
    in-launch pass, the launches behind it do nothing and the final state still arrives."""
    d = probes["default"]
    for config in ("parity", "tiny"):
        for name in (config + "_early", config + "_early_beginend"):
            passes, rebuilds = int(d[name + "_iters"]) + 1, int(d[name + "_path_rebuilds"])
            assert 2 <= passes < 60, name
            assert int(d[name + "_path_head"]) == passes - (1 + rebuilds), (name, passes, rebuilds)
            assert int(probes["head_off"][name + "_path_head"]) == 0
        # pedp_icp looks at `done` behind every 8th launch (both state slots) and stops enqueuing: the stop of pass s is
        # made in launch s + 1 at the latest, the first look behind it is at most 8 launches on -- with or without the
        # head close.  pedp_icp_begin enqueues everything.
        for s in _SETTINGS:
            p = probes[s]
            assert int(p[config + "_early_path_launches"]) <= int(p[config + "_early_iters"]) + 1 + 8 < 61, (s, config)
            assert int(p[config + "_early_beginend_path_launches"]) == 61, (s, config)
    assert int(d["parity_early_path_head"]) >= 1


def test_a_rebuild_behind_head_closed_passes(probes):
    """The start pose picked on the CPU: the registration asked for a rebuild at a pass >= 2 (so the rebuild pass ran in
    the launch whose head closed the pass before it), and the read-outs show it."""
    asked = probes["asked"]
    assert asked, "no start pose with a late rebuild was found on the CPU"
    d = probes["default"]
    for config, a in asked.items():
        name = config + "_late_rebuild"
        passes, rebuilds = int(d[name + "_iters"]) + 1, int(d[name + "_path_rebuilds"])
        assert passes == 13
        assert rebuilds == len(a) and rebuilds >= 1, (config, a, rebuilds)
        assert int(d[name + "_path_head"]) == passes - (1 + rebuilds) - 1, (config, a)
        # the device's own trace asks at the same passes
        from pedp_hip import synth
        f = synth.Frame(config)
        got, _ = rebuild_requests(d[name + "_trace"], RADIUS, f.model_points.min(0), f.model_points.max(0))
        assert got == a and any(p >= 2 for p in got), (config, got, a)
        assert int(probes["head_off"][name + "_path_head"]) == 0 and int(probes["serial_close"][name + "_path_head"]) == 0


def test_segmented_path_graph_untouched_by_the_switches(probes):
    """Runs no code of the head close: the library replays graphs only for registrations that are not fused-eligible.
    It only pins that the switches leave that path alone (bytes, above) and that two poses share one capture."""
    for s in _SETTINGS:
        assert int(probes[s]["graph_path_captures"]) == 1, s
