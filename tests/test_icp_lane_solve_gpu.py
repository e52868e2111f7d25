"""The close's 6x6 solve with a row per lane of the closing wave (GPU; csrc/icp/solve_lanes.h).

PEDP_ICP_LANE_SOLVE (read once per process) picks the form: 0 the pivoted LDLT on one lane, as it was; 1 (default)
lane i < 6 of the closing wave holds row i.  Either way each output is computed by the oracle's sequence of float64
operations, so the bound is the strictest there is: raw bytes.

1. The solve alone (pedp_debug_solve6): both device forms on the 2,004 systems of tests/_lane_solve_cases.py -- every
   (k, p) pivot choice, exactly zero pivots, ties, the zero matrix, a NaN and an infinite entry -- against each other
   and against oracle.solve6.
2. Registrations: one child process per setting; transformation, fitness, rmse, iteration count, every trace row and
   every correspondence compared byte for byte, and the read-out pedp_icp_last_lane_solves asserted on each side (a
   comparison that passes because the lane solve never ran is no comparison)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _lane_solve_cases as cases
import _nn_cases  # noqa: F401  (the probe imports it by the same name)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the solve alone

@pytest.fixture(scope="module")
def solved(ctx, oracle):
    from pedp_hip import _lib

    A, b, n_finite = cases.systems()
    dev = _lib.debug_solve6(ctx, A, b)
    ref = [oracle.solve6(A[s], b[s]) for s in range(len(A))]
    return A, b, n_finite, dev, np.array([bool(ok) for ok, _ in ref]), np.array([np.asarray(x, np.float64) for _, x in ref])


def test_the_systems_cover_every_pivot_choice_and_zero_pivots(solved):
    A, b, n_finite, *_ = solved
    pairs, zeros = cases.coverage(A, b, 2000)
    assert pairs == {(k, p) for k in range(6) for p in range(k, 6)} and len(pairs) == 21
    assert zeros >= 1


def test_lane_form_equals_one_lane_form_in_raw_bytes(solved):
    A, b, n_finite, dev, ok_o, x_o = solved
    assert len(A) == 2004
    assert np.array_equal(dev["ok_lanes"], dev["ok_one"])
    diff = np.nonzero((dev["x_lanes"].view(np.uint64) != dev["x_one"].view(np.uint64)).any(1))[0]
    assert len(diff) == 0, (diff[:10], dev["x_lanes"][diff[:3]], dev["x_one"][diff[:3]])


def test_both_forms_equal_the_oracle(solved):
    A, b, n_finite, dev, ok_o, x_o = solved
    assert ok_o[:n_finite].all() and not ok_o[n_finite:].any()
    for form in ("lanes", "one"):
        assert np.array_equal(dev["ok_" + form] != 0, ok_o), form   # (the two non-finite systems: ok alone)
        diff = np.nonzero((dev["x_" + form][:n_finite].view(np.uint64) != x_o[:n_finite].view(np.uint64)).any(1))[0]
        assert len(diff) == 0, (form, diff[:10])
    # ties keep the identity permutation: x = b / 3; the zero matrix solves to zero
    assert np.array_equal(dev["x_lanes"][2000], b[2000] / 3.0) and not dev["x_lanes"][2001].any()


# ---------------------------------------------------------------- 2. registrations

_PROBE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle"); sys.path.insert(0, sys.argv[1] + "/tests")
from pedp_hip import _lib, synth
import _nn_cases as cases
ctx = _lib.Context(0)
out = {}
FIXED = dict(relative_fitness=-1, relative_rmse=-1)
KW = dict(want_corr=True, want_trace=True)

def put(name, r):
    for k in ("T", "trace", "corr"):
        out[name + "_" + k] = r[k]
    out[name + "_fit"] = np.float64(r["fitness"]); out[name + "_rmse"] = np.float64(r["inlier_rmse"]); out[name + "_iters"] = np.int64(r["iters"])
    out[name + "_path_lane"] = np.int64(_lib.icp_last_lane_solves(ctx))
    out[name + "_path_wide"] = np.int64(_lib.icp_last_serial_path(ctx)[0])
    out[name + "_path_steady"] = np.int64(_lib.icp_last_steady(ctx)[0])
    out[name + "_path_followers"] = np.int64(_lib.icp_last_steady_followers(ctx))

if sys.argv[3] == "main":
    f = synth.Frame("parity")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    init = f.icp_init()
    put("parity_icp", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=20, **KW, **FIXED))
    _lib.icp_begin(ctx, src, tgt, 10.0, init, max_iteration=20, want_trace=True, **FIXED)
    put("parity_beginend", _lib.icp_end(ctx, want_corr=True))
    # a start that is far off: the live set is rebuilt in the first passes
    far = init.copy(); far[:3, 3] += np.array([6.0, -5.0, 4.0])
    put("parity_far", _lib.icp(ctx, src, tgt, 10.0, far, max_iteration=12, **KW, **FIXED))
    # a stop by criteria: the solve of the stopping pass is not run
    put("parity_early", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=60, relative_fitness=1e-2, relative_rmse=1e-2, **KW))
    # point-to-point: no 6x6 system
    put("p2p", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=6, estimator=_lib.POINT_TO_POINT, **KW, **FIXED))
    # the fused batch, whose kernel shares the close
    inits = np.stack([np.linalg.inv(T) for T in synth.batched_start_poses(5)])
    T, fit, rmse, its = _lib.icp_batched_ex(ctx, src, tgt, np.full(5, 8.0), inits, max_iteration=15)
    out["batch_T"], out["batch_fit"], out["batch_rmse"], out["batch_its"] = T, fit, rmse, its
    out["batch_path_lane"] = np.int64(_lib.icp_last_lane_solves(ctx))
    # 256 source points (two chunks), 1,024 target rows (one mask word), 7 passes
    rng = np.random.default_rng(7)
    uv = rng.uniform(-50.0, 50.0, (1024, 2))
    model = np.c_[uv, 0.01 * (uv[:, 0] ** 2 - uv[:, 1] ** 2)]
    nrm = np.c_[-0.02 * uv[:, 0], 0.02 * uv[:, 1], np.ones(1024)]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    put("small", _lib.icp(ctx, _lib.Cloud(ctx, model[::4] - np.array([0.5, -0.4, 0.3])), _lib.Cloud(ctx, model, nrm), 5.0, np.eye(4),
                          max_iteration=6, **KW, **FIXED))
    # a planar scene on a planar model: J = (s x n, n) with n = e_z has three zero columns -- a system of rank 3, exactly
    # zero pivots and the <= DBL_MIN guard of the diagonal inside a registration
    g = np.stack(np.meshgrid(np.arange(40.0), np.arange(40.0)), -1).reshape(-1, 2)
    plane = np.c_[g, np.zeros(len(g))]
    up = np.tile([0.0, 0.0, 1.0], (len(g), 1))
    tilt = np.eye(4); tilt[:3, :3] = synth.axis_angle([1.0, 0.5, 0.0], np.deg2rad(1.5)); tilt[:3, 3] = (0.0, 0.0, 0.4)
    sp = plane[::3] + np.array([0.2, 0.1, 0.0])
    put("planar", _lib.icp(ctx, _lib.Cloud(ctx, sp), _lib.Cloud(ctx, plane, up), 3.0, tilt, max_iteration=8, **KW, **FIXED))
else:
    # five chunks under PEDP_ICP_STEADY_GROUPS=2 PEDP_ICP_STEADY_CLOSERS=1: the close on 1,024 threads and workgroups that
    # follow it -- the instantiations the bench frame takes
    s, t, n = cases.blob(600, 2100, 11)
    c = t[np.isfinite(t).all(1)].mean(0)
    init = np.eye(4); init[:3, :3] = synth.axis_angle([0.3, -1.0, 0.5], np.deg2rad(2.0)); init[:3, 3] = c - init[:3, :3] @ c
    put("five", _lib.icp(ctx, _lib.Cloud(ctx, s), _lib.Cloud(ctx, t, n), 0.1 * cases.extent(t), init, max_iteration=20, **KW, **FIXED))
np.savez(sys.argv[2], **out)
"""

_SWITCHES = ("PEDP_ICP_LANE_SOLVE", "PEDP_ICP_SERIAL_CLOSE", "PEDP_ICP_COPY_BRACKET", "PEDP_ICP_HEAD_CLOSE", "PEDP_ICP_CERT", "PEDP_ICP_STEADY",
             "PEDP_ICP_STEADY_FROM", "PEDP_ICP_STEADY_GRID", "PEDP_ICP_STEADY_CLOSERS", "PEDP_ICP_STEADY_GROUPS", "PEDP_ICP_UNFUSED_FINISH")
_BLOB = {"PEDP_ICP_STEADY_GROUPS": "2", "PEDP_ICP_STEADY_CLOSERS": "1"}
# side: (which cases, switches)
_SIDES = {"lane0": ("main", {"PEDP_ICP_LANE_SOLVE": "0"}), "lane1": ("main", {"PEDP_ICP_LANE_SOLVE": "1"}),
          "serial": ("main", {"PEDP_ICP_SERIAL_CLOSE": "1"}),
          "blob0": ("blob", dict(_BLOB, PEDP_ICP_LANE_SOLVE="0")), "blob1": ("blob", dict(_BLOB, PEDP_ICP_LANE_SOLVE="1"))}
_P2PLANE = ("parity_icp", "parity_beginend", "parity_far", "parity_early", "small", "planar")


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("lane_solve")
    res = {}
    for name, (which, extra) in _SIDES.items():
        out = str(tmp / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", _PROBE, root, out, which], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, (name, p.stdout.decode())
        res[name] = dict(np.load(out))
    return res


@pytest.mark.parametrize("new, old", [("lane1", "lane0"), ("serial", "lane0"), ("blob1", "blob0")])
def test_every_bit_equals_the_one_lane_solve(probes, new, old):
    a, b = probes[new], probes[old]
    assert set(a) == set(b)
    compared = 0
    for k in sorted(a):
        if "_path_" in k:
            continue
        u, v = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert u.dtype == v.dtype and u.shape == v.shape, k
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), k
        compared += 1
    assert compared >= (6 * 7 + 4 if old == "lane0" else 6)


def test_the_expected_form_ran(probes):
    """A point-to-plane pass that has correspondences and does not stop solves: every pass but the last one.  The lane
    form ran them all with the switch at 1 (the default: tests/test_icp_lane_solve_cpu.py), none with the switch at 0 or
    with the close on one lane."""
    for side in ("lane1",):
        r = probes[side]
        for name in _P2PLANE:
            assert int(r[name + "_path_lane"]) == int(r[name + "_iters"]) > 0, (side, name)
            assert int(r[name + "_path_wide"]) == int(r[name + "_iters"]) + 1, (side, name)
        assert int(r["p2p_path_lane"]) == 0 and int(r["p2p_iters"]) == 6
        assert int(r["batch_path_lane"]) == int(r["batch_its"].sum()) > 0
        assert int(r["parity_early_iters"]) < 60 and int(r["parity_icp_iters"]) == 20
    for side in ("lane0", "serial"):
        r = probes[side]
        for name in _P2PLANE + ("p2p", "batch"):
            assert int(r[name + "_path_lane"]) == 0, (side, name)
    assert int(probes["serial"]["parity_icp_path_wide"]) == 0 and int(probes["lane0"]["parity_icp_path_wide"]) == 21
    # the planar registration kept its correspondences (a solve per pass on a rank-3 system) and stayed finite
    assert np.isfinite(probes["lane1"]["planar_T"]).all() and float(probes["lane1"]["planar_fit"]) > 0.5


def test_the_blob_reached_the_wide_steady_close_and_a_follower(probes):
    for side, lane in (("blob1", 20), ("blob0", 0)):
        r = probes[side]
        assert int(r["five_iters"]) == 20 and int(r["five_path_lane"]) == lane, side
        assert int(r["five_path_steady"]) > 0 and int(r["five_path_followers"]) > 0, side
