"""The serial part of an ICP pass and a registration's fixed cost (GPU).

Two switches restore the earlier behaviour, each read once per process, so every comparison runs one child process
per setting:
  PEDP_ICP_SERIAL_CLOSE=1   the close of a pass on one lane, the sign-off counters looked at after the sums
  PEDP_ICP_COPY_BRACKET=1   host-to-device copy + fill in front of pass 0, device-to-host copy behind the last pass
The new default only moves WHEN loads are issued and WHICH lane computes an output; every output is computed by the
same sequence of float64 operations.  So the bound is the strictest there is: the raw bytes are equal.  And the
read-out of pedp_icp_last_serial_path shows that the new path really was in force (a comparison that passes because
the fast path never ran is no comparison).

Not provoked on a card: a sign-off spin that runs out (done = -1).  Its bound is unchanged; the closing workgroup
writes -1 to the page-locked block where icp_collect looks (reviewed in the source)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PEDP_ERR_BAD_ARG = -1   # include/pedp.h

_PROBE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle")
from pedp_hip import _lib, synth
ctx = _lib.Context(0)
out = {}
FIXED = dict(relative_fitness=-1, relative_rmse=-1)

def put(name, r):
    for k in ("T", "trace", "corr"):
        if k in r:
            out[name + "_" + k] = r[k]
    out[name + "_fit"] = np.float64(r["fitness"]); out[name + "_rmse"] = np.float64(r["inlier_rmse"]); out[name + "_iters"] = np.int64(r["iters"])
    wide, bracket = _lib.icp_last_serial_path(ctx)
    out[name + "_path_wide"] = np.int64(wide); out[name + "_path_bracket"] = np.int64(bracket)

for config in ("parity", "bench_100k"):
    f = synth.Frame(config)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    init = f.icp_init()
    # the bench's registration: 20 iterations, 21 passes, no early exit -- blocking, and enqueued whole
    put(config + "_icp", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=20, want_corr=True, want_trace=True, **FIXED))
    _lib.icp_begin(ctx, src, tgt, 10.0, init, max_iteration=20, want_trace=True, **FIXED)
    put(config + "_beginend", _lib.icp_end(ctx, want_corr=True))
    # `done` is set before max_iter, the launches behind it are no-ops.  (The default criteria, 1e-6, do not stop
    # these two frames within 200 iterations -- a few correspondences keep flipping -- so the criteria are 1e-2.)
    put(config + "_early", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=60, relative_fitness=1e-2, relative_rmse=1e-2,
                                    want_corr=True, want_trace=True))
    # a start that is far off: large updates, the live set is rebuilt in the first passes
    far = init.copy(); far[:3, 3] += np.array([6.0, -5.0, 4.0])
    put(config + "_far", _lib.icp(ctx, src, tgt, 10.0, far, max_iteration=12, want_corr=True, want_trace=True, **FIXED))
    if config == "parity":
        # the update of the point-to-point estimator does not come from angles: it is handed over whole
        put("p2p", _lib.icp(ctx, src, tgt, 10.0, init, max_iteration=6, estimator=_lib.POINT_TO_POINT, want_corr=True, want_trace=True, **FIXED))
        # a radius beyond the fused pass: uniform batches replay one captured graph per pose on sub-contexts
        inits = np.stack([np.linalg.inv(T) for T in synth.batched_start_poses(3)])
        T, fit, rmse, its = _lib.icp_batched_ex(ctx, src, tgt, np.full(3, 500.0), inits, max_iteration=6)
        out["graph_T"], out["graph_fit"], out["graph_rmse"], out["graph_its"] = T, fit, rmse, its
        # ... and a fused batch, whose kernel shares the close
        T, fit, rmse, its = _lib.icp_batched_ex(ctx, src, tgt, np.full(5, 8.0), np.stack([np.linalg.inv(T) for T in synth.batched_start_poses(5)]), max_iteration=15)
        out["batch_T"], out["batch_fit"], out["batch_rmse"], out["batch_its"] = T, fit, rmse, its
# a small registration whose path the library's decision function predicts: 256 source points (two chunks), 1,024 target
# rows (one mask word), point-to-plane, 7 passes
rng = np.random.default_rng(7)
uv = rng.uniform(-50.0, 50.0, (1024, 2))
model = np.c_[uv, 0.01 * (uv[:, 0] ** 2 - uv[:, 1] ** 2)]
nrm = np.c_[-0.02 * uv[:, 0], 0.02 * uv[:, 1], np.ones(1024)]
nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
shift = np.eye(4); shift[:3, 3] = (0.5, -0.4, 0.3)
put("small", _lib.icp(ctx, _lib.Cloud(ctx, model[::4] - shift[:3, 3]), _lib.Cloud(ctx, model, nrm), 5.0, np.eye(4), max_iteration=6,
                      want_corr=True, want_trace=True, **FIXED))
out["small_path_head"] = np.int64(_lib.icp_last_head_closed(ctx))
want = _lib.icp_path(None, n_source=256, n_target=1024, radius=5.0, unit_size=1, poses=1, timed_pass=-1, resident=True)
for k, v in want.items():
    out["small_path_want_" + k] = np.int64(v)
np.savez(sys.argv[2], **out)
"""

_SETTINGS = {
    "default": {},
    "serial_close": {"PEDP_ICP_SERIAL_CLOSE": "1"},
    "copy_bracket": {"PEDP_ICP_COPY_BRACKET": "1"},
    "all_off": {"PEDP_ICP_SERIAL_CLOSE": "1", "PEDP_ICP_COPY_BRACKET": "1"},
}


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("serial_path")
    res = {}
    for name, extra in _SETTINGS.items():
        out = str(tmp / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in ("PEDP_ICP_SERIAL_CLOSE", "PEDP_ICP_COPY_BRACKET")}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", _PROBE, root, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        res[name] = dict(np.load(out))
    return res


@pytest.mark.parametrize("setting", ["serial_close", "copy_bracket", "all_off"])
def test_every_bit_equals_the_switched_off_path(probes, setting):
    """Transformation, fitness, rmse, iteration count, every row of the trace and every correspondence: the raw bytes
    of the new default equal those of the path with one switch, or all of them, set."""
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
    assert compared >= 9 * 6 + 8
    assert new["parity_icp_trace"].shape == (21, 18) and new["bench_100k_icp_trace"].shape == (21, 18)


def test_the_new_paths_were_in_force(probes):
    """The wide close closed every pass of every fused registration of the default run and none with the switch set;
    the start kernel and the closing workgroup's own write of the final state bracketed them, or the copies did."""
    for name in ("parity_icp", "parity_beginend", "parity_early", "parity_far", "p2p", "bench_100k_icp", "bench_100k_beginend",
                 "bench_100k_early", "bench_100k_far"):
        passes = int(probes["default"][name + "_iters"]) + 1
        assert int(probes["default"][name + "_path_wide"]) == passes, name
        assert int(probes["default"][name + "_path_bracket"]) == 3, name
        assert int(probes["serial_close"][name + "_path_wide"]) == 0 and int(probes["serial_close"][name + "_path_bracket"]) == 3, name
        assert int(probes["copy_bracket"][name + "_path_wide"]) == passes and int(probes["copy_bracket"][name + "_path_bracket"]) == 0, name
        assert int(probes["all_off"][name + "_path_wide"]) == 0 and int(probes["all_off"][name + "_path_bracket"]) == 0, name
    # the registrations meant to end early, and to run all their passes, did
    for config in ("parity", "bench_100k"):
        assert int(probes["default"][config + "_early_iters"]) < 60 and int(probes["default"][config + "_icp_iters"]) == 20


def test_the_decision_function_predicts_the_path_that_ran(probes):
    """Bracket bits and head closes of a small registration are what pedp_debug_icp_path says for the process's switches:
    in the default process, and with PEDP_ICP_SERIAL_CLOSE=1 PEDP_ICP_COPY_BRACKET=1."""
    for setting, dev_result, head in (("default", 1, 1), ("all_off", 0, 0)):
        r = probes[setting]
        want = {k[len("small_path_want_"):]: int(v) for k, v in r.items() if k.startswith("small_path_want_")}
        assert want["fused"] == 1 and want["dev_result"] == dev_result and want["head"] == head, setting
        assert want["copy_bracket"] == want["serial_close"] == 1 - dev_result, setting
        assert int(r["small_iters"]) == 6
        assert int(r["small_path_bracket"]) == (0 if want["copy_bracket"] else 1) + (2 if want["dev_result"] else 0), setting
        assert (int(r["small_path_head"]) > 0) == bool(want["head"]), setting


def _scene(ctx, config):
    from pedp_hip import _lib, synth

    f = synth.Frame(config)
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    return f, f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])


def _same(a, b):
    return (np.array_equal(a["T"].view(np.uint8), b["T"].view(np.uint8)) and a["fitness"] == b["fitness"] and a["inlier_rmse"] == b["inlier_rmse"]
            and a["iters"] == b["iters"] and np.array_equal(a["corr"], b["corr"]) and np.array_equal(a["trace"].view(np.uint8), b["trace"].view(np.uint8)))


def test_back_to_back_registrations_equal_fresh_contexts(ctx):
    """Two registrations of different sizes on one context (the workspace is carved anew, the page-locked block and the
    visit plan are used again) with a pedp_nn between them give the bits of fresh contexts."""
    from pedp_hip import _lib

    f, scene = _scene(ctx, "parity")
    small = np.ascontiguousarray(scene[::3])
    kw = dict(max_iteration=10, relative_fitness=-1, relative_rmse=-1, want_corr=True, want_trace=True)

    def run(c, pts, radius):
        return _lib.icp(c, _lib.Cloud(c, pts), _lib.Cloud(c, f.model_points, f.normals), radius, f.icp_init(), **kw)

    first = run(ctx, scene, 10.0)
    idx, d2 = _lib.nn(ctx, _lib.Cloud(ctx, small), _lib.Cloud(ctx, f.model_points, f.normals), f.icp_init())
    second = run(ctx, small, 7.0)
    third = run(ctx, scene, 10.0)
    fresh_a, fresh_b = _lib.Context(0), _lib.Context(0)
    assert _same(first, run(fresh_a, scene, 10.0))
    assert _same(second, run(fresh_b, small, 7.0))
    assert _same(third, first)
    idx2, d22 = _lib.nn(fresh_b, _lib.Cloud(fresh_b, small), _lib.Cloud(fresh_b, f.model_points, f.normals), f.icp_init())
    assert np.array_equal(idx, idx2) and np.array_equal(d2.view(np.uint64), d22.view(np.uint64))


def test_pending_registration_keeps_its_block(ctx):
    """While a registration is pending the device writes the page-locked block at a time of its own: pedp_nn,
    pedp_icp_configure and pedp_ransac_hypotheses return PEDP_ERR_BAD_ARG, and the registration ends with the right pose."""
    from pedp_hip import _lib

    f, scene = _scene(ctx, "parity")
    src, tgt = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    kw = dict(max_iteration=12, relative_fitness=-1, relative_rmse=-1)
    one = _lib.icp(ctx, src, tgt, 10.0, f.icp_init(), want_corr=True, want_trace=True, **kw)
    lib = _lib.load()
    M = np.ascontiguousarray(f.icp_init(), np.float64)
    idx, d2 = np.empty(src.N, np.int32), np.empty(src.N, np.float64)
    corr = np.zeros(src.N, np.int32)
    ok, T = np.empty(16, np.uint8), np.empty((16, 4, 4), np.float64)
    _lib.icp_begin(ctx, src, tgt, 10.0, f.icp_init(), want_trace=True, **kw)
    import ctypes as C
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.pedp_nn(ctx._h, src._h, tgt._h, p(M), p(idx), p(d2)) == PEDP_ERR_BAD_ARG
    assert lib.pedp_icp_configure(ctx._h, 1, -1) == PEDP_ERR_BAD_ARG
    assert lib.pedp_ransac_hypotheses(ctx._h, src._h, tgt._h, p(corr), C.c_uint64(1), 0, 16, 0.9, 4.0, 0.6, p(ok), p(T)) == PEDP_ERR_BAD_ARG
    two = _lib.icp_end(ctx, want_corr=True)
    assert _same(one, two)
    assert _lib.icp_last_serial_path(ctx) == (13, 3)
