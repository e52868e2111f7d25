"""Two wave groups per workgroup of a steady ICP launch (GPU).

icp_steady_kernel<2> runs two ranks in one workgroup of sixteen waves: wave group g (waves 8 g .. 8 g + 7) works on unit
b + (2 it + g) G exactly as the eight waves of icp_steady_kernel<1> work on theirs, the workgroup closes a pass once on all its
threads, and the second group goes on from the state that close -- or the copy of a closer's record -- left in the workgroup's
LDS (csrc/icp/steady_pass.h).  The library takes two groups by itself only for a scene with more chunks than the
device has CUs; PEDP_ICP_STEADY_GROUPS forces the choice, PEDP_ICP_STEADY_GRID caps the workgroups:

    groups1                    the kernel as it was
    groups2                    two groups, a workgroup per CU: at these sizes every second group idles through the barriers
    groups2_grid1              one workgroup: group 0 owns units 0, 2, 4, group 1 units 1, 3; on three chunks group 1 idles
                               in the second round, on five in the third
    groups2_grid2              two workgroups, both closing; on five chunks only group 0 of workgroup 0 loops to the fifth
    groups2_grid2_closers1     workgroup 1 FOLLOWS workgroup 0: a second group in a following workgroup
    groups2_grid2_closers1_rebuild   the same with the take-over at the pass whose close asks for the late rebuild
                               (test_icp_head_close_gpu.pick_late_rebuild): a hand-back, the host's continuation, and a
                               stop by criteria inside the launch
    default                    no switch: the bench_100k frame only -- the one shape here with more chunks than CUs

A chunk's sum tree, its rank and the index of its partial sums are those of one group, so the bound is the strictest there is:
the raw bytes of transformation, fitness, rmse, iteration count, trace and correspondences equal those of PEDP_ICP_STEADY=0.
The switches are read once per process: one child process per side, each runs every case once.  The read-outs
pedp_icp_last_steady / pedp_icp_last_steady_followers (ranks that closed no pass themselves: ranks minus closing workgroups)
show that the path under test ran.

The failure path of the bounded poll is not provoked here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _nn_cases as cases  # noqa: F401  (the probe imports it by the same name)
import test_icp_head_close_gpu as head_close

pytestmark = pytest.mark.gpu

F = 5  # the default of PEDP_ICP_STEADY_FROM

_PROBE = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle"); sys.path.insert(0, sys.argv[1] + "/tests")
from pedp_hip import _lib, synth
import _nn_cases as cases
ctx = _lib.Context(0)
picked = dict(np.load(sys.argv[3]))
F = int(sys.argv[4])
SMALL, BENCH = sys.argv[5] == "1", sys.argv[6] == "1"
out = {}
FIXED = dict(relative_fitness=-1, relative_rmse=-1)
KW = dict(want_corr=True, want_trace=True)

def put(name, r):
    for k in ("T", "trace", "corr"):
        out[name + "_" + k] = r[k]
    out[name + "_fit"] = np.float64(r["fitness"]); out[name + "_rmse"] = np.float64(r["inlier_rmse"]); out[name + "_iters"] = np.int64(r["iters"])
    passes, handbacks = _lib.icp_last_steady(ctx)
    out[name + "_path_steady"] = np.int64(passes); out[name + "_path_handbacks"] = np.int64(handbacks)
    out[name + "_path_followers"] = np.int64(_lib.icp_last_steady_followers(ctx))

def rot(tgt, deg=2.0):
    c = tgt[np.isfinite(tgt).all(1)].mean(0)
    T = np.eye(4)
    T[:3, :3] = synth.axis_angle([0.3, -1.0, 0.5], np.deg2rad(deg))
    T[:3, 3] = c - T[:3, :3] @ c
    return T

def blob_cases(tag, ns, nan_rows):
    src, tgt, nrm = cases.blob(ns, 2100, 11)
    r = 0.1 * cases.extent(tgt)
    S, G = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    init = rot(tgt)
    put(tag + "_icp", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
    put(tag + "_p2p", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_POINT, max_iteration=20, **KW, **FIXED))
    # the same call behind a different registration: a record with equal pass numbers lies in the slot
    put(tag + "_again", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
    _lib.icp_begin(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, want_trace=True, **FIXED)
    put(tag + "_beginend", _lib.icp_end(ctx, want_corr=True))
    bad = src.copy()
    bad[nan_rows, [0, 1, 2, 0]] = np.nan
    put(tag + "_nan", _lib.icp(ctx, _lib.Cloud(ctx, bad), G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
    # criteria that stop the registration: the steady launch ends it itself where the take-over comes early enough
    _lib.icp_begin(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=60, relative_fitness=1e-2, relative_rmse=1e-2, want_trace=True)
    put(tag + "_early", _lib.icp_end(ctx, want_corr=True))

if SMALL:
    blob_cases("small", 300, [3, 130, 131, 299])  # three chunks, the last one of 44 points
    blob_cases("five", 600, [3, 130, 300, 599])   # five chunks, the last one of 88 points

    f = synth.Frame("parity")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    Sp, Gp = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    for m in (F - 1, F, F + 1, 20):
        put("parity_max%d" % m, _lib.icp(ctx, Sp, Gp, 10.0, f.icp_init(), max_iteration=m, **KW, **FIXED))
    if "parity_init" in picked:
        put("rebuild_full", _lib.icp(ctx, Sp, Gp, 10.0, picked["parity_init"], max_iteration=12, **KW, **FIXED))

    # exact ties: tied slots search in every pass -- in a second group, too -- and the launch hands back by the searched share
    src, tgt, nrm = cases.lattice(1000, 512, 7)
    Sl, Gl = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
    put("lattice_max20", _lib.icp(ctx, Sl, Gl, 1.8, np.eye(4), estimator=_lib.POINT_TO_POINT, max_iteration=20, **KW, **FIXED))

if BENCH:
    f = synth.Frame("bench_100k")
    mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
    scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
    Sb, Gb = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
    put("bench", _lib.icp(ctx, Sb, Gb, 10.0, f.icp_init(), max_iteration=20, **KW, **FIXED))
    n_cu = C.c_int(0)
    if C.CDLL("libamdhip64.so").hipDeviceGetAttribute(C.byref(n_cu), 63, 0) != 0:  # hipDeviceAttributeMultiprocessorCount
        n_cu = C.c_int(0)
    out["n_cu"] = np.int64(n_cu.value)
np.savez(sys.argv[2], **out)
"""

_SWITCHES = ("PEDP_ICP_STEADY", "PEDP_ICP_STEADY_FROM", "PEDP_ICP_STEADY_GRID", "PEDP_ICP_STEADY_CLOSERS", "PEDP_ICP_STEADY_GROUPS",
             "PEDP_ICP_CERT", "PEDP_ICP_HEAD_CLOSE", "PEDP_ICP_SERIAL_CLOSE", "PEDP_ICP_COPY_BRACKET", "PEDP_ICP_UNFUSED_FINISH")
_G2 = {"PEDP_ICP_STEADY_GROUPS": "2"}
# side: (switches -- None: filled in by the fixture --, runs the small cases, runs the bench frame)
_SIDES = (("off", {"PEDP_ICP_STEADY": "0"}, True, True), ("groups1", {"PEDP_ICP_STEADY_GROUPS": "1"}, True, True),
          ("groups2", dict(_G2), True, False),
          ("groups2_grid1", dict(_G2, PEDP_ICP_STEADY_GRID="1"), True, False),
          ("groups2_grid2", dict(_G2, PEDP_ICP_STEADY_GRID="2"), True, False),
          ("groups2_grid2_closers1", dict(_G2, PEDP_ICP_STEADY_GRID="2", PEDP_ICP_STEADY_CLOSERS="1"), True, False),
          ("groups2_grid2_closers1_rebuild", None, True, False),
          ("default", {}, False, True))
_NEW = tuple(s for s, _, small, _ in _SIDES if s != "off" and small)
_CAPPED = ("groups2_grid1", "groups2_grid2", "groups2_grid2_closers1", "groups2_grid2_closers1_rebuild")
_BLOB = ("icp", "p2p", "again", "beginend", "nan")
_PARITY = ["parity_max%d" % m for m in (F - 1, F, F + 1, 20)]
# ranks that close no pass = min(live chunks, groups x grid) - min(closers, live chunks, grid); every chunk of both blobs is live
_FOLLOWERS = {"small": {"groups1": 0, "groups2": 0, "groups2_grid1": 2 - 1, "groups2_grid2": 3 - 2, "groups2_grid2_closers1": 3 - 1,
                        "groups2_grid2_closers1_rebuild": 3 - 1},
              "five": {"groups1": 0, "groups2": 0, "groups2_grid1": 2 - 1, "groups2_grid2": 4 - 2, "groups2_grid2_closers1": 4 - 1,
                       "groups2_grid2_closers1_rebuild": 4 - 1}}


@pytest.fixture(scope="module")
def probes(tmp_path_factory, oracle):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("groups")
    picked = {}
    init, asked = head_close.pick_late_rebuild("parity", oracle)
    if init is not None:
        picked["parity_init"] = init
    np.savez(str(tmp / "picked.npz"), **picked)
    late = [p for p in (asked or []) if 2 <= p <= 9]
    res = {"picked": picked, "asked": asked, "from": late[0] if late else 2}
    for name, extra, small, bench in _SIDES:
        if extra is None:  # the take-over at the pass whose close asks for the late rebuild
            extra = dict(_G2, PEDP_ICP_STEADY_GRID="2", PEDP_ICP_STEADY_CLOSERS="1", PEDP_ICP_STEADY_FROM=str(res["from"]))
        out = str(tmp / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", _PROBE, root, out, str(tmp / "picked.npz"), str(F), "1" if small else "0",
                            "1" if bench else "0"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, (name, p.stdout.decode())
        res[name] = dict(np.load(out))
    return res


def _same_bytes(probes, names, sides=_NEW):
    ref = probes["off"]
    for side in sides:
        new = probes[side]
        for name in names:
            keys = [k for k in sorted(new) if k.startswith(name + "_") and "_path_" not in k]
            assert len(keys) == 6, (name, keys)
            for k in keys:
                a, b = np.ascontiguousarray(new[k]), np.ascontiguousarray(ref[k])
                assert a.dtype == b.dtype and a.shape == b.shape, (side, k)
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (side, k)
    for name in names:
        assert int(ref[name + "_path_steady"]) == 0 and int(ref[name + "_path_followers"]) == 0, name


def _show(probes, names, sides=_NEW):
    for name in names:
        print(name, {s: tuple(int(probes[s][name + "_path_" + k]) for k in ("steady", "handbacks", "followers")) for s in sides},
              "passes", int(probes[sides[0]][name + "_iters"]) + 1)


@pytest.mark.parametrize("shape", ["small", "five"])
def test_blobs_both_estimators_both_entry_points_again_and_nan(probes, shape):
    """Three chunks and five: both estimators, icp and icp_begin / icp_end, the same call again behind a different
    registration, four NaN points.  The read-out is ranks minus closing workgroups on every side, and no byte differs."""
    names = [shape + "_" + c for c in _BLOB]
    _same_bytes(probes, names)
    _show(probes, names)
    for side in _NEW:
        d = probes[side]
        for name in names:
            assert int(d[name + "_path_steady"]) > 0, (side, name)
            assert int(d[name + "_path_followers"]) == _FOLLOWERS[shape][side], (side, name)
        assert int(d[shape + "_again_path_steady"]) == int(d[shape + "_icp_path_steady"]) == int(d[shape + "_beginend_path_steady"])


def test_the_boundary_of_the_take_over(probes):
    """max_iteration F - 1 never reaches the steady launch; F closes one pass at the launch's entry, from the generic
    launch's partial sums; F + 1 and 20 close passes of the launch itself."""
    _same_bytes(probes, _PARITY)
    _show(probes, _PARITY)
    for side in ("groups1", "groups2", "groups2_grid1", "groups2_grid2", "groups2_grid2_closers1"):
        d = probes[side]
        assert int(d["parity_max%d_path_steady" % (F - 1)]) == 0 and int(d["parity_max%d_path_followers" % (F - 1)]) == 0, side
        for m in (F, F + 1, 20):
            name = "parity_max%d" % m
            assert int(d[name + "_iters"]) == m
            assert int(d[name + "_path_steady"]) > 0, (side, name)
            if side in _CAPPED:
                assert int(d[name + "_path_followers"]) >= 1, (side, name)
        if int(d["parity_max20_path_handbacks"]) == 0:
            assert int(d["parity_max20_path_steady"]) == 20 - F + 1


def test_a_stop_by_criteria_inside_the_launch(probes):
    """Criteria of 1e-2 through icp_begin / icp_end.  With the early take-over the close that meets them is the steady
    launch's: both groups of both workgroups leave on it, and the last closer writes the final state."""
    names = ["small_early", "five_early"]
    _same_bytes(probes, names)
    _show(probes, names)
    d, frm = probes["groups2_grid2_closers1_rebuild"], probes["from"]
    for shape in ("small", "five"):
        name = shape + "_early"
        assert int(d[name + "_iters"]) >= frm and int(d[name + "_path_steady"]) > 0 and int(d[name + "_path_handbacks"]) == 0, \
            "no registration was ended by the steady launch"
        assert int(d[name + "_path_followers"]) == _FOLLOWERS[shape]["groups2_grid2_closers1_rebuild"]


def test_second_groups_through_a_hand_back_for_a_rebuild(probes):
    """The start pose test_icp_head_close_gpu.py picks; the take-over at the pass whose close asks for the rebuild: the
    workgroups hand back with both their groups, the host runs the rebuild pass in a generic launch and starts the steady
    launch again."""
    assert "parity_init" in probes["picked"], "no start pose with a late rebuild was found on the CPU"
    _same_bytes(probes, ["rebuild_full"])
    _show(probes, ["rebuild_full"])
    print("rebuilds asked for at the close of passes", probes["asked"])
    d = probes["groups2_grid2_closers1_rebuild"]
    assert int(d["rebuild_full_path_handbacks"]) >= 1 and int(d["rebuild_full_path_steady"]) > 0
    assert int(d["rebuild_full_path_followers"]) >= 1
    for side in _NEW:
        assert int(probes[side]["rebuild_full_path_steady"]) > 0, side


def test_a_searching_second_group_hands_back_by_the_search_share(probes):
    """On the lattice tied slots never certify and search in every pass; more than 1/8 of them searching hands the launch
    back, as often as with one group."""
    _same_bytes(probes, ["lattice_max20"])
    _show(probes, ["lattice_max20"])
    for side in _NEW:
        assert int(probes[side]["lattice_max20_path_steady"]) > 0, side
        if not side.endswith("_rebuild"):  # (that side takes over at another pass)
            assert int(probes[side]["lattice_max20_path_handbacks"]) == int(probes["groups1"]["lattice_max20_path_handbacks"]), side
    for side in _CAPPED:
        assert int(probes[side]["lattice_max20_path_followers"]) >= 1, side


def test_the_bench_frame_where_the_default_takes_two_groups(probes):
    """One registration of the bench_100k frame: more chunks than CUs, so the default is two groups and the ranks beyond the
    CU count are second groups.  The read-out is the one a second workgroup per CU gave (25 at 256 CUs)."""
    sides = ("groups1", "default")
    _same_bytes(probes, ["bench"], sides)
    _show(probes, ["bench"], sides)
    for side in sides:
        assert int(probes[side]["bench_path_steady"]) > 0, side
    assert int(probes["default"]["bench_path_followers"]) == int(probes["groups1"]["bench_path_followers"])
    if int(probes["default"]["n_cu"]) == 256:
        assert int(probes["default"]["bench_path_followers"]) == 25
        assert int(probes["groups1"]["bench_path_followers"]) == 25
