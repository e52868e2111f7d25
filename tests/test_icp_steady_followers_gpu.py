"""Closers and followers of a steady ICP launch (GPU).

Inside icp_steady_kernel the ranks below C = min(ranks, closers) close a pass themselves; the other ranks follow: they poll
the tag of the record closer `rank % C` publishes, copy the closed state from it and take the branches the closer took
(csrc/icp/steady_pass.h).  `closers` is the device's CU count, so at these sizes -- a handful of chunks -- the
default has no follower at all; PEDP_ICP_STEADY_CLOSERS makes some:

    default            no follower; reads 0
    closers1           ranks 1 and 2 of the three-chunk shape follow rank 0
    closers2           one follower there, an uneven map (rank 2 follows rank 0, rank 1 has none)
    closers1_grid2     PEDP_ICP_STEADY_GRID=2: a follower that owns several chunks
    every              closers at least the grid: every rank closes, as before followers existed; reads 0
    closers1_rebuild   closers1 with the take-over at the pass whose close asks for the late rebuild
                       (test_icp_head_close_gpu.pick_late_rebuild, as test_icp_steady_gpu.py uses it): followers through a
                       hand-back and the host's continuation, and through a stop by criteria inside the launch

Every float64 sequence is the same on every side, so the bound is the strictest there is: the raw bytes of transformation,
fitness, rmse, iteration count, trace and correspondences equal those of PEDP_ICP_STEADY=0.  The switches are read once per
process: one child process per side, each runs every case once.  pedp_icp_last_steady_followers is asserted on each side.

The order of the small cases matters: the same call comes a second time on the context with a different registration in
between (the other estimator), so a record the first call left in a slot lies there, with the same pass numbers, when the
second polls -- the registration's nonce in the tag keeps it from matching.

The failure path of the bounded poll (a closer that never publishes) is not provoked here."""
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
    out[name + "_path_followers"] = np.int64(_lib.icp_last_steady_followers(ctx))

def rot(tgt, deg=2.0):
    c = tgt[np.isfinite(tgt).all(1)].mean(0)
    T = np.eye(4)
    T[:3, :3] = synth.axis_angle([0.3, -1.0, 0.5], np.deg2rad(deg))
    T[:3, 3] = c - T[:3, :3] @ c
    return T

# three chunks, the last one of 44 points, three mask words
src, tgt, nrm = cases.blob(300, 2100, 11)
r = 0.1 * cases.extent(tgt)
S, G = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
init = rot(tgt)
put("small_icp", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
put("small_p2p", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_POINT, max_iteration=20, **KW, **FIXED))
put("small_again", _lib.icp(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
_lib.icp_begin(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, want_trace=True, **FIXED)
put("small_beginend", _lib.icp_end(ctx, want_corr=True))
bad = src.copy()
bad[[3, 130, 131, 299], [0, 1, 2, 0]] = np.nan
put("small_nan", _lib.icp(ctx, _lib.Cloud(ctx, bad), G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=20, **KW, **FIXED))
# criteria that stop the registration: the steady launch ends it itself where the take-over comes early enough
_lib.icp_begin(ctx, S, G, r, init, estimator=_lib.POINT_TO_PLANE, max_iteration=60, relative_fitness=1e-2, relative_rmse=1e-2, want_trace=True)
put("small_early", _lib.icp_end(ctx, want_corr=True))

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

# exact ties: tied slots search in every pass, and the launch hands back by the searched share -- read from the record
src, tgt, nrm = cases.lattice(1000, 512, 7)
Sl, Gl = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
put("lattice_max20", _lib.icp(ctx, Sl, Gl, 1.8, np.eye(4), estimator=_lib.POINT_TO_POINT, max_iteration=20, **KW, **FIXED))
np.savez(sys.argv[2], **out)
"""

_SWITCHES = ("PEDP_ICP_STEADY", "PEDP_ICP_STEADY_FROM", "PEDP_ICP_STEADY_GRID", "PEDP_ICP_STEADY_CLOSERS", "PEDP_ICP_CERT",
             "PEDP_ICP_HEAD_CLOSE", "PEDP_ICP_SERIAL_CLOSE", "PEDP_ICP_COPY_BRACKET", "PEDP_ICP_UNFUSED_FINISH")
_EVERY = 1 << 20  # more closers than any grid has workgroups
_SIDES = (("off", {"PEDP_ICP_STEADY": "0"}), ("default", {}), ("closers1", {"PEDP_ICP_STEADY_CLOSERS": "1"}),
          ("closers2", {"PEDP_ICP_STEADY_CLOSERS": "2"}),
          ("closers1_grid2", {"PEDP_ICP_STEADY_CLOSERS": "1", "PEDP_ICP_STEADY_GRID": "2"}),
          ("every", {"PEDP_ICP_STEADY_CLOSERS": str(_EVERY)}), ("closers1_rebuild", None))
_NEW = tuple(s for s, _ in _SIDES if s != "off")
_FOLLOWING = ("closers1", "closers2", "closers1_grid2", "closers1_rebuild")
_SMALL = ["small_icp", "small_p2p", "small_again", "small_beginend", "small_nan"]
_PARITY = ["parity_max%d" % m for m in (F - 1, F, F + 1, 20)]
# the three-chunk shape: ranks = min(live chunks, grid) = 3, or 2 under the grid cap; followers = ranks - min(ranks, closers)
_SMALL_FOLLOWERS = {"default": 0, "closers1": 2, "closers2": 1, "closers1_grid2": 1, "every": 0, "closers1_rebuild": 2}


@pytest.fixture(scope="module")
def probes(tmp_path_factory, oracle):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("followers")
    picked = {}
    init, asked = head_close.pick_late_rebuild("parity", oracle)
    if init is not None:
        picked["parity_init"] = init
    np.savez(str(tmp / "picked.npz"), **picked)
    late = [p for p in (asked or []) if 2 <= p <= 9]
    res = {"picked": picked, "asked": asked, "from": late[0] if late else 2}
    for name, extra in _SIDES:
        if extra is None:  # the take-over at the pass whose close asks for the late rebuild
            extra = {"PEDP_ICP_STEADY_CLOSERS": "1", "PEDP_ICP_STEADY_FROM": str(res["from"])}
        out = str(tmp / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", _PROBE, root, out, str(tmp / "picked.npz"), str(F)], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, (name, p.stdout.decode())
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
        assert int(ref[name + "_path_steady"]) == 0 and int(ref[name + "_path_followers"]) == 0, name


def _show(probes, names):
    for name in names:
        print(name, {s: tuple(int(probes[s][name + "_path_" + k]) for k in ("steady", "handbacks", "followers")) for s in _NEW},
              "passes", int(probes["default"][name + "_iters"]) + 1)


def _no_follower_where_every_rank_closes(probes, names):
    for side in ("default", "every"):
        for name in names:
            assert int(probes[side][name + "_path_followers"]) == 0, (side, name)


def test_three_chunks_both_estimators_both_entry_points_again_and_nan(probes):
    """Both estimators, icp and icp_begin / icp_end, the same call again behind a different registration, four NaN points:
    the follower counts are the ones the shape and the switches give, and no byte differs."""
    _same_bytes(probes, _SMALL)
    _show(probes, _SMALL)
    for side in _NEW:
        d = probes[side]
        for name in _SMALL:
            assert int(d[name + "_path_steady"]) > 0, (side, name)
            assert int(d[name + "_path_followers"]) == _SMALL_FOLLOWERS[side], (side, name)
        assert int(d["small_again_path_steady"]) == int(d["small_icp_path_steady"]) == int(d["small_beginend_path_steady"])


def test_the_boundary_of_the_take_over(probes):
    """max_iteration F - 1 never reaches the steady launch; F closes one pass at the launch's entry -- from the generic
    launch's partial sums, which a follower follows too -- F + 1 and 20 close passes of the launch itself."""
    _same_bytes(probes, _PARITY)
    _show(probes, _PARITY)
    _no_follower_where_every_rank_closes(probes, _PARITY)
    for side in ("default", "closers1", "closers2", "closers1_grid2", "every"):
        d = probes[side]
        assert int(d["parity_max%d_path_steady" % (F - 1)]) == 0 and int(d["parity_max%d_path_followers" % (F - 1)]) == 0, side
        for m in (F, F + 1, 20):
            name = "parity_max%d" % m
            assert int(d[name + "_iters"]) == m
            assert int(d[name + "_path_steady"]) > 0, (side, name)
            if side in _FOLLOWING:
                assert int(d[name + "_path_followers"]) >= 1, (side, name)
        if int(d["parity_max20_path_handbacks"]) == 0:
            assert int(d["parity_max20_path_steady"]) == 20 - F + 1


def test_followers_leave_on_the_closers_stop(probes):
    """Criteria of 1e-2 through icp_begin / icp_end.  With the early take-over the close that meets them is the steady
    launch's: the closers stop, the followers read `done` out of the record and leave with them, and the last closer
    writes the final state."""
    names = ["small_early", "parity_early"]
    _same_bytes(probes, names)
    _show(probes, names)
    _no_follower_where_every_rank_closes(probes, names)
    d, frm = probes["closers1_rebuild"], probes["from"]
    assert int(d["small_early_iters"]) >= frm and int(d["small_early_path_steady"]) > 0 and int(d["small_early_path_handbacks"]) == 0, \
        "no registration was ended by the steady launch"
    assert int(d["small_early_path_followers"]) == 2


def test_followers_through_a_hand_back_for_a_rebuild(probes):
    """The start pose test_icp_head_close_gpu.py picks; the take-over at the pass whose close asks for the rebuild: closers
    and followers hand back together, the host runs the rebuild pass in a generic launch and starts the steady launch
    again, with followers again."""
    assert "parity_init" in probes["picked"], "no start pose with a late rebuild was found on the CPU"
    _same_bytes(probes, ["rebuild_full"])
    _show(probes, ["rebuild_full"])
    print("rebuilds asked for at the close of passes", probes["asked"])
    _no_follower_where_every_rank_closes(probes, ["rebuild_full"])
    d = probes["closers1_rebuild"]
    assert int(d["rebuild_full_path_handbacks"]) >= 1 and int(d["rebuild_full_path_steady"]) > 0
    assert int(d["rebuild_full_path_followers"]) >= 1
    for side in _FOLLOWING:
        assert int(probes[side]["rebuild_full_path_steady"]) > 0, side


def test_followers_hand_back_by_the_published_search_share(probes):
    """On the lattice tied slots never certify and search in every pass; more than 1/8 of them searching hands the launch
    back -- a follower decides that from the word in the record."""
    _same_bytes(probes, ["lattice_max20"])
    _show(probes, ["lattice_max20"])
    _no_follower_where_every_rank_closes(probes, ["lattice_max20"])
    for side in _NEW:
        assert int(probes[side]["lattice_max20_path_steady"]) > 0, side
    for side in ("closers1", "closers2", "closers1_grid2"):
        assert int(probes[side]["lattice_max20_path_followers"]) >= 1, side
        assert int(probes[side]["lattice_max20_path_handbacks"]) == int(probes["every"]["lattice_max20_path_handbacks"]), side
