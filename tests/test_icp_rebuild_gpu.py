"""The head and the close of ICP rebuild passes (GPU).

A rebuild pass decides from the chunks' run spheres which chunks to visit, eight chunks a round with a lane per sphere
(csrc/icp/fused_pass.h), withdraws the correspondences of the chunks it leaves out over all eight waves, and its close
lists the live chunks by a wave scan (csrc/icp/live_list.h).  None of that may move a bit: the raw bytes of
transformation, fitness, rmse, iteration count, trace and correspondences are compared

  * with the CPU oracle (correspondences and fitness exactly, poses and rmse within the bounds tests/test_icp_gpu.py
    holds the registration to);
  * between the default grid and PEDP_ICP_PASS_GRID = 1, 2, 3, 8 on `tiny` (15 chunks: a workgroup owns 15, 8 / 7, 5 and
    2 / 1 of them -- two rounds with a short second one, a full round and a round of seven, lanes without a chunk) and
    1, 7, 64 on `parity` (180 chunks, three mask words);
  * with PEDP_ICP_UNFUSED_FINISH=1: the finish kernel's listing on 1,024 threads;
  * between a 5-pose batch on `parity` and its five single registrations (the batch kernel's rebuild head).

The switches are read once per process: one child process per setting, all started together.  Both frames rebuild more
than once (tools/icp_certificate_model.rebuild_passes on the oracle's trace at r = 10: `parity` in passes 0 and 1, `tiny`
in passes 0, 1 and 4); the read-out of the rebuilds asked for after pass 0 must say 1 and 2.

Further cases, in every child: correspondences left by an earlier registration on the same handles are withdrawn by a
registration that visits no chunk (pass 0's withdrawals); `tiny` less its last 37 points (a point count that is no
multiple of 128, run spheres of radius < 0 in the last chunk); a scene with a NaN coordinate (a Cloud takes such rows
and leaves them out of its box: the sphere of the point's run is NaN, and the chunk is visited)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-5
RADIUS = 10.0

_PROBE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle")
from pedp_hip import _lib, synth
ctx = _lib.Context(0)
out = {}
FIXED = dict(relative_fitness=-1, relative_rmse=-1)
KW = dict(want_corr=True, want_trace=True)

def put(name, r):
    for k in ("T", "trace", "corr"):
        out[name + "_" + k] = r[k]
    out[name + "_fit"] = np.float64(r["fitness"]); out[name + "_rmse"] = np.float64(r["inlier_rmse"]); out[name + "_iters"] = np.int64(r["iters"])
    out[name + "_path_rebuilds"] = np.int64(_lib.icp_last_head_closed(ctx, rebuilds=True)[1])

for config in sys.argv[3].split(","):
    f = synth.Frame(config)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    out[config + "_scene"] = scene
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    init = f.icp_init()
    put(config + "_icp", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=20, **KW, **FIXED))
    # stale correspondences: the same handles, a start pose 1e4 away, no iteration -- pass 0 visits no chunk
    far = init.copy(); far[:3, 3] += 1e4
    put(config + "_far", _lib.icp(ctx, src, tgt, 10.0, far, max_iteration=0, **KW, **FIXED))
    if config == "tiny":
        put("tiny_short", _lib.icp(ctx, _lib.Cloud(ctx, scene[:-37]), tgt, 10.0, init, max_iteration=20, **KW, **FIXED))
        bad = scene.copy(); bad[len(bad) // 2, 1] = np.nan
        put("tiny_nan", _lib.icp(ctx, _lib.Cloud(ctx, bad), tgt, 10.0, init, max_iteration=20, **KW, **FIXED))
    if config == "parity":
        inits = np.stack([np.linalg.inv(T) for T in synth.batched_start_poses(5)])
        T, fit, rmse, its = _lib.icp_batched_ex(ctx, src, tgt, np.full(5, 8.0), inits, max_iteration=15)
        out["batch_T"], out["batch_fit"], out["batch_rmse"], out["batch_its"] = T, fit, rmse, its
        for b in range(5):
            one = _lib.icp(ctx, src, tgt, 8.0, inits[b], max_iteration=15)
            out["single%d_T" % b] = one["T"]; out["single%d_fit" % b] = np.float64(one["fitness"])
            out["single%d_rmse" % b] = np.float64(one["inlier_rmse"]); out["single%d_its" % b] = np.int32(one["iters"])
np.savez(sys.argv[2], **out)
"""

_BOTH = "parity,tiny"
_SETTINGS = {
    "default": ({}, _BOTH),
    "grid1": ({"PEDP_ICP_PASS_GRID": "1"}, _BOTH),
    "grid2": ({"PEDP_ICP_PASS_GRID": "2"}, "tiny"),
    "grid3": ({"PEDP_ICP_PASS_GRID": "3"}, "tiny"),
    "grid8": ({"PEDP_ICP_PASS_GRID": "8"}, "tiny"),
    "grid7": ({"PEDP_ICP_PASS_GRID": "7"}, "parity"),
    "grid64": ({"PEDP_ICP_PASS_GRID": "64"}, "parity"),
    "unfused": ({"PEDP_ICP_UNFUSED_FINISH": "1"}, _BOTH),
}
_SWITCHES = ("PEDP_ICP_PASS_GRID", "PEDP_ICP_UNFUSED_FINISH", "PEDP_ICP_HEAD_CLOSE", "PEDP_ICP_SERIAL_CLOSE", "PEDP_ICP_COPY_BRACKET",
             "PEDP_ICP_STEADY", "PEDP_ICP_STEADY_GRID", "PEDP_ICP_CERT", "PEDP_ICP_LANE_SOLVE")
_REBUILDS_AFTER_PASS_0 = {"parity": 1, "tiny": 2}


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("rebuild")
    running = {}
    for name, (extra, frames) in _SETTINGS.items():
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(extra)
        running[name] = subprocess.Popen([sys.executable, "-c", _PROBE, root, str(tmp / f"{name}.npz"), frames], env=env,
                                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    res = {}
    for name, p in running.items():
        text, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (name, text.decode())
        res[name] = dict(np.load(str(tmp / f"{name}.npz")))
    return res


def _same_bytes(new, old, prefixes):
    compared = 0
    for k in sorted(new):
        if not k.startswith(prefixes) or "_path_" in k:
            continue
        a, b = np.ascontiguousarray(new[k]), np.ascontiguousarray(old[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
        compared += 1
    return compared


@pytest.mark.parametrize("setting", [s for s in _SETTINGS if s != "default"])
def test_every_bit_equals_the_default_grid(probes, setting):
    frames = _SETTINGS[setting][1].split(",")
    n = _same_bytes(probes[setting], probes["default"], tuple(frames) + (("batch", "single") if "parity" in frames else ()))
    # per frame: the scene, six results of the registration and six of the far one; tiny: the short and the NaN scene; parity: the batch
    assert n == 13 * len(frames) + (12 if "tiny" in frames else 0) + (24 if "parity" in frames else 0)


@pytest.mark.parametrize("setting", list(_SETTINGS))
def test_rebuild_passes_ran(probes, setting):
    """More than one rebuild per registration, so a later rebuild's sphere round (a mask of the rebuild before it to
    read, withdrawals only where a chunk left the live set) ran under every setting."""
    d = probes[setting]
    for config in _SETTINGS[setting][1].split(","):
        assert int(d[config + "_icp_iters"]) == 20
        assert int(d[config + "_icp_path_rebuilds"]) == _REBUILDS_AFTER_PASS_0[config], (setting, config)


def _against_oracle(oracle, res, name, scene, f):
    ref = oracle.icp(scene, f.model_points, f.normals, RADIUS, f.icp_init(), max_iter=20, rel_fitness=-1, rel_rmse=-1)
    assert int(res[name + "_iters"]) == ref["iters"] == 20
    assert np.array_equal(res[name + "_corr"], ref["corr"])
    assert float(res[name + "_fit"]) == ref["fitness"]
    assert abs(float(res[name + "_rmse"]) - ref["inlier_rmse"]) < 1e-9
    assert np.abs(res[name + "_T"] - ref["T"]).max() < POSE_TOL
    assert np.abs(res[name + "_trace"][:, :2] - ref["trace"][:, :2]).max() < 1e-9
    assert np.abs(res[name + "_trace"][:, 2:] - ref["trace"][:, 2:]).max() < POSE_TOL


@pytest.mark.parametrize("setting,config", [("default", "parity"), ("default", "tiny"), ("grid1", "parity"), ("grid1", "tiny"),
                                            ("unfused", "parity"), ("unfused", "tiny")])
def test_trace_and_correspondences_match_the_oracle(probes, oracle, setting, config):
    from pedp_hip import synth

    d = probes[setting]
    _against_oracle(oracle, d, config + "_icp", d[config + "_scene"], synth.Frame(config))


def test_short_last_chunk_matches_the_oracle_on_one_workgroup(probes, oracle):
    """tiny less its last 37 points: the point count is no multiple of 128 and the last chunk's trailing run spheres have
    radius < 0.  One workgroup (PEDP_ICP_PASS_GRID=1) owns every chunk."""
    from pedp_hip import synth

    d = probes["grid1"]
    scene = d["tiny_scene"][:-37]
    assert len(scene) % 128 != 0 and (len(scene) % 128) <= 128 - 16
    _against_oracle(oracle, d, "tiny_short", scene, synth.Frame("tiny"))


@pytest.mark.parametrize("setting", list(_SETTINGS))
def test_stale_correspondences_are_withdrawn(probes, setting):
    """A registration from a pose 1e4 away, no iteration, on the handles of a registration that left correspondences: pass 0
    visits no chunk and withdraws every one of them."""
    d = probes[setting]
    for config in _SETTINGS[setting][1].split(","):
        assert (d[config + "_icp_corr"] >= 0).sum() > 100
        far = d[config + "_far_corr"]
        assert far.dtype == np.int32 and len(far) == len(d[config + "_scene"])
        assert (far == -1).all(), (setting, config, int((far != -1).sum()))
        assert int(d[config + "_far_iters"]) == 0 and float(d[config + "_far_fit"]) == 0.0


def test_nan_coordinate_is_accepted_and_its_chunk_decided_alike(probes, oracle):
    """A Cloud takes a row with a NaN coordinate (it is left out of the box and never has a neighbour).  The run sphere
    that holds it is NaN: the sphere test says "visit" ("also when anything is NaN").  Every grid gives the default grid's
    bits (test_every_bit_equals_the_default_grid compares tiny_nan_*); here: the point has no correspondence, and every
    other point's is what the registration of the scene without that row finds -- up to the index shift."""
    d = probes["default"]
    scene = d["tiny_scene"]
    at = len(scene) // 2
    corr = d["tiny_nan_corr"]
    assert corr[at] == -1
    from pedp_hip import synth

    f = synth.Frame("tiny")
    ref = oracle.icp(np.delete(scene, at, axis=0), f.model_points, f.normals, RADIUS, f.icp_init(), max_iter=20, rel_fitness=-1, rel_rmse=-1)
    assert np.array_equal(np.delete(corr, at), ref["corr"])
    assert np.abs(d["tiny_nan_T"] - ref["T"]).max() < POSE_TOL


def test_batch_equals_its_single_registrations(probes):
    """The batch kernel's rebuild head: five poses in one launch against the five single registrations, bit for bit."""
    for setting in ("default", "grid1", "grid7", "grid64", "unfused"):
        d = probes[setting]
        for b in range(5):
            assert np.array_equal(d["batch_T"][b].view(np.uint8), d["single%d_T" % b].view(np.uint8)), (setting, b)
            assert d["batch_fit"][b].tobytes() == d["single%d_fit" % b].tobytes() and d["batch_rmse"][b].tobytes() == d["single%d_rmse" % b].tobytes()
            assert int(d["batch_its"][b]) == int(d["single%d_its" % b])
