"""Fully certified ICP passes in one resident launch (GPU).

From pass PEDP_ICP_STEADY_FROM on (default 5) a single fused registration runs its passes inside one launch of
icp_steady_kernel: a bounded device-wide hand-over of the partial sums per pass instead of a launch boundary, every
workgroup closes the pass itself, a slot without a certificate runs the exact search, and the launch hands the
registration back when a close asks for a rebuild or too many slots search (csrc/icp/steady_pass.h).  Every
float64 sequence is the generic pass kernel's, so the bound is the strictest there is: the raw bytes of transformation,
fitness, rmse, iteration count, trace and correspondences equal those of PEDP_ICP_STEADY=0 -- and those of a launch
capped at two workgroups (PEDP_ICP_STEADY_GRID=2), where a workgroup has several chunks.  The switches are read once per
process: one child process per side, each runs every case once.  pedp_icp_last_steady shows that the kernel ran, that the
switch turns it off, and that the rebuild case was handed back.

The start pose of the rebuild case is the one test_icp_head_close_gpu.py picks on the CPU; its registration asks for the
late rebuild at the close of a pass in 2..9 -- pass 2 for the parity frame, in front of the default take-over at pass 5,
where the steady launch never sees it.  A fourth side therefore takes over at that very pass (PEDP_ICP_STEADY_FROM): there
the steady launch runs the pass, its close asks for the rebuild, the launch hands back and the host continues.

Shapes: 300 scene points are two full chunks and one of 44; 2,100 target rows are three mask words."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _nn_cases as cases
import test_icp_head_close_gpu as head_close

pytestmark = pytest.mark.gpu

F = 5  # the default of PEDP_ICP_STEADY_FROM

_PROBE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle"); sys.path.insert(0, sys.argv[1] + "/tests")
from pedp_hip import _lib, synth
import _nn_cases as cases
ctx = _lib.Context(0)
picked = dict(np.load(sys.argv[3]))
F = int(sys.argv[4])
out = {}
FIXED = dict(relative_fitness=-1, relative_rmse=-1)
KW = dict(want_corr=True, want_trace=True)

def put(name, r):
    for k in ("T", "trace", "corr"):
        out[name + "_" + k] = r[k]
    out[name + "_fit"] = np.float64(r["fitness"]); out[name + "_rmse"] = np.float64(r["inlier_rmse"]); out[name + "_iters"] = np.int64(r["iters"])
    passes, handbacks = _lib.icp_last_steady(ctx)
    out[name + "_path_steady"] = np.int64(passes); out[name + "_path_handbacks"] = np.int64(handbacks)
    head, rebuilds, launches = _lib.icp_last_head_closed(ctx, rebuilds=True)
    out[name + "_path_head"] = np.int64(head); out[name + "_path_rebuilds"] = np.int64(rebuilds); out[name + "_path_launches"] = np.int64(launches)
    out[name + "_path_wide"] = np.int64(_lib.icp_last_serial_path(ctx)[0])

def rot(tgt, deg=2.0):
    c = tgt[np.isfinite(tgt).all(1)].mean(0)
    T = np.eye(4)
    T[:3, :3] = synth.axis_angle([0.3, -1.0, 0.5], np.deg2rad(deg))
    T[:3, 3] = c - T[:3, :3] @ c
    return T

# the smallest shape with every boundary: both estimators, both entry points, a second time on the context, NaN points
src, tgt, nrm = cases.blob(300, 2100, 11)
r = 0.1 * cases.extent(tgt)
S, G = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
init = rot(tgt)
put("small_icp", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
_lib.icp_begin(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, want_trace=True, **FIXED)
put("small_beginend", _lib.icp_end(ctx, want_corr=True))
put("small_again", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
put("small_p2p", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_POINT, max_iteration=20, **KW, **FIXED))
bad = src.copy()
bad[[3, 130, 131, 299], [0, 1, 2, 0]] = np.nan
put("small_nan", _lib.icp(ctx, _lib.Cloud(ctx, bad), G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
# criteria that stop the registration: the steady launch ends it itself (icp_begin enqueues everything)
_lib.icp_begin(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=60, relative_fitness=1e-2, relative_rmse=1e-2, want_trace=True)
put("small_early", _lib.icp_end(ctx, want_corr=True))

# the boundary of the take-over; a rebuild in mid-run: a hand-back and the host's continuation
f = synth.Frame("parity")
mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
Sp, Gp = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
for m in (F - 1, F, F + 1, 20):
    put("parity_max%d" % m, _lib.icp(ctx, Sp, Gp, 10.0, f.icp_init(), max_iteration=m, **KW, **FIXED))
_lib.icp_begin(ctx, Sp, Gp, 10.0, f.icp_init(), max_iteration=60, relative_fitness=1e-2, relative_rmse=1e-2, want_trace=True)
put("parity_early", _lib.icp_end(ctx, want_corr=True))
if "parity_init" in picked:
    put("rebuild_full", _lib.icp(ctx, Sp, Gp, 10.0, picked["parity_init"], max_iteration=12, **KW, **FIXED))

# exact ties: a tied slot never certifies -- the in-kernel exact search runs in every pass
src, tgt, nrm = cases.lattice(1000, 512, 7)
Sl, Gl = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
put("lattice_max20", _lib.icp(ctx, Sl, Gl, 1.8, np.eye(4), estimator=_lib.POINT_TO_POINT, max_iteration=20, **KW, **FIXED))
np.savez(sys.argv[2], **out)
"""

_SWITCHES = ("PEDP_ICP_STEADY", "PEDP_ICP_STEADY_FROM", "PEDP_ICP_STEADY_GRID", "PEDP_ICP_CERT", "PEDP_ICP_HEAD_CLOSE",
             "PEDP_ICP_SERIAL_CLOSE", "PEDP_ICP_COPY_BRACKET", "PEDP_ICP_UNFUSED_FINISH")
_SIDES = (("default", {}), ("off", {"PEDP_ICP_STEADY": "0"}), ("grid2", {"PEDP_ICP_STEADY_GRID": "2"}), ("at_rebuild", None))
_NEW = ("default", "grid2", "at_rebuild")
_SMALL = ["small_icp", "small_beginend", "small_again", "small_p2p", "small_nan"]
_PARITY = ["parity_max%d" % m for m in (F - 1, F, F + 1, 20)]


@pytest.fixture(scope="module")
def probes(tmp_path_factory, oracle):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("steady")
    picked = {}
    init, asked = head_close.pick_late_rebuild("parity", oracle)
    if init is not None:
        picked["parity_init"] = init
    np.savez(str(tmp / "picked.npz"), **picked)
    res = {"picked": picked, "asked": asked}
    late = [p for p in (asked or []) if 2 <= p <= 9]
    res["from"] = {"default": F, "grid2": F, "at_rebuild": late[0] if late else 2}
    for name, extra in _SIDES:
        if extra is None:  # the take-over at the pass whose close asks for the late rebuild
            extra = {"PEDP_ICP_STEADY_FROM": str(late[0] if late else 2)}
        out = str(tmp / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", _PROBE, root, out, str(tmp / "picked.npz"), str(F)], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        res[name] = dict(np.load(out))
    return res


def _same_bytes(probes, names):
    ref = probes["off"]
    for side in _NEW:
        new = probes[side]
        for name in names:
            keys = [k for k in sorted(new) if k.startswith(name + "_") and "_path_" not in k]
            assert len(keys) == 6, (name, keys)
            for k in keys:
                a, b = np.ascontiguousarray(new[k]), np.ascontiguousarray(ref[k])
                assert a.dtype == b.dtype and a.shape == b.shape, (side, k)
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (side, k)
    for name in names:
        assert int(ref[name + "_path_steady"]) == 0 and int(ref[name + "_path_handbacks"]) == 0, name  # the switch is a switch


def _show(probes, names):
    for name in names:
        print(name, {s: (int(probes[s][name + "_path_steady"]), int(probes[s][name + "_path_handbacks"])) for s, _ in _SIDES},
              "passes", int(probes["default"][name + "_iters"]) + 1)


def test_smallest_shape_with_every_boundary(probes):
    """Both estimators, through icp and through icp_begin / icp_end, a second time on the same context (the counters'
    bases carried over), four NaN source points -- with one chunk per workgroup and with two workgroups for three chunks."""
    _same_bytes(probes, _SMALL)
    _show(probes, _SMALL)
    for side in ("default", "grid2"):
        d = probes[side]
        for name in _SMALL:
            assert d[name + "_trace"].shape == (21, 18)
            assert int(d[name + "_path_steady"]) > 0, (side, name)
            # the read-outs the other tests pin keep their meaning: every pass closed by the wide close, the passes behind
            # pass 0 that are no rebuild passes and not the last at a head, the passes an enqueue covers
            assert int(d[name + "_path_wide"]) == 21 and int(d[name + "_path_launches"]) == 21, (side, name)
            assert int(d[name + "_path_head"]) == int(probes["off"][name + "_path_head"]), (side, name)
            assert int(d[name + "_path_rebuilds"]) == int(probes["off"][name + "_path_rebuilds"]), (side, name)
        assert int(d["small_again_path_steady"]) == int(d["small_icp_path_steady"]) == int(d["small_beginend_path_steady"])


def test_the_boundary_of_the_take_over(probes):
    """max_iteration F - 1 leaves the registration to the generic launches; F, F + 1 and 20 end inside the steady launch."""
    _same_bytes(probes, _PARITY)
    _show(probes, _PARITY)
    for side in ("default", "grid2"):
        d = probes[side]
        assert int(d["parity_max%d_path_steady" % (F - 1)]) == 0
        for m in (F, F + 1, 20):
            name = "parity_max%d" % m
            assert int(d[name + "_iters"]) == m
            assert int(d[name + "_path_steady"]) > 0, (side, name)
            assert int(d[name + "_path_head"]) == int(probes["off"][name + "_path_head"]), (side, name)
        # without a hand-back every pass from F on ran inside the one launch
        if int(d["parity_max20_path_handbacks"]) == 0:
            assert int(d["parity_max20_path_steady"]) == 20 - F + 1


def test_a_rebuild_hands_back_and_the_host_continues(probes):
    """The start pose test_icp_head_close_gpu.py picks: a close asks for a rebuild in mid-run.  Where that happens behind
    pass F - 1 the steady launch hands back, the host runs the rebuild pass in a generic launch and starts the steady
    launch again."""
    assert "parity_init" in probes["picked"], "no start pose with a late rebuild was found on the CPU"
    _same_bytes(probes, ["rebuild_full"])
    _show(probes, ["rebuild_full"])
    print("rebuilds asked for at the close of passes", probes["asked"])
    assert int(probes["at_rebuild"]["rebuild_full_path_handbacks"]) >= 1
    for side in _NEW:
        d = probes[side]
        assert int(d["rebuild_full_path_steady"]) > 0, side
        assert int(d["rebuild_full_path_rebuilds"]) == int(probes["off"]["rebuild_full_path_rebuilds"]) >= 1
        assert int(d["rebuild_full_path_head"]) == int(probes["off"]["rebuild_full_path_head"]), side


def test_exact_ties_search_inside_the_launch(probes):
    """On the lattice tied slots never certify: the exact search of the steady kernel runs in every pass it has, and the
    launch hands back when more than 1/8 of the slots searched."""
    _same_bytes(probes, ["lattice_max20"])
    _show(probes, ["lattice_max20"])
    for side in ("default", "grid2"):
        assert int(probes[side]["lattice_max20_path_steady"]) > 0, side


def test_criteria_end_the_registration_inside_the_launch(probes):
    """Criteria of 1e-2 through icp_begin / icp_end: everything is enqueued.  They are met after a few passes -- in front of
    the default take-over, where the steady launch finds the registration over and leaves, and behind the early take-over
    of the fourth side, where the close that meets them is the steady launch's: it writes the final state itself."""
    names = ["small_early", "parity_early"]
    _same_bytes(probes, names)
    _show(probes, names)
    for side in _NEW:
        d, frm = probes[side], probes["from"][side]
        for name in names:
            passes = int(d[name + "_iters"]) + 1
            assert 2 <= passes < 60, name
            assert int(d[name + "_path_launches"]) == 61, name
            assert int(d[name + "_path_head"]) == int(probes["off"][name + "_path_head"]), (side, name)
            if int(d[name + "_path_handbacks"]) == 0:  # every pass from the take-over on ran inside the one launch
                assert int(d[name + "_path_steady"]) == max(0, passes - frm), (side, name, passes)
    d, frm = probes["at_rebuild"], probes["from"]["at_rebuild"]
    assert int(d["small_early_iters"]) >= frm and int(d["small_early_path_steady"]) > 0 and int(d["small_early_path_handbacks"]) == 0, \
        "no registration was ended by the steady launch"
