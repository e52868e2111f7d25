"""Nearest-neighbour certificates of the fused ICP pass (GPU).

A pass leaves, per scene point, a lower bound on the distance to every target point other than the neighbour it found;
while the point's motion since keeps that neighbour strictly inside the bound, the next pass takes it over without a
search (csrc/icp/fused_pass.h).  The certificate only ever replaces a search whose answer is proven, so the
bound is the strictest there is: the raw bytes of transformation, fitness, rmse, iteration count, trace and
correspondences equal those of PEDP_ICP_CERT=0, which restores the search in every pass (and its uninflated radius).
The switch is read once per process: one child process per side.  pedp_icp_last_certified shows that the path under
test ran (slots certified > 0, and fewer pairs swept than the switched-off side), and that the switch turns it off.

Shapes: 300 scene points are two full chunks and one of 44; 2,100 target rows are three mask words."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _nn_cases as cases
import test_icp_head_close_gpu as head_close

pytestmark = pytest.mark.gpu

_PROBE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/oracle"); sys.path.insert(0, sys.argv[1] + "/tests")
from pedp_hip import _lib, synth
import _nn_cases as cases
ctx = _lib.Context(0)
picked = dict(np.load(sys.argv[3]))
out = {}
FIXED = dict(relative_fitness=-1, relative_rmse=-1)
KW = dict(want_corr=True, want_trace=True)

def put(name, r):
    for k in ("T", "trace", "corr"):
        out[name + "_" + k] = r[k]
    out[name + "_fit"] = np.float64(r["fitness"]); out[name + "_rmse"] = np.float64(r["inlier_rmse"]); out[name + "_iters"] = np.int64(r["iters"])
    cert, searched = _lib.icp_last_certified(ctx)
    out[name + "_path_cert"] = np.int64(cert); out[name + "_path_searched"] = np.int64(searched)
    out[name + "_path_pairs"] = np.int64(_lib.icp_last_stats(ctx)[1])

def rot(tgt, deg=2.0):
    c = tgt[np.isfinite(tgt).all(1)].mean(0)
    T = np.eye(4)
    T[:3, :3] = synth.axis_angle([0.3, -1.0, 0.5], np.deg2rad(deg))
    T[:3, 3] = c - T[:3, :3] @ c
    return T

# 1. the smallest shape with every boundary; 4. the other estimator, and NaN source points
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

# 2. the passes in which some neighbours still change while others are certified; 5. a rebuild in mid-run
f = synth.Frame("parity")
mesh = _lib.Mesh(ctx, f.verts_posed, f.tris)
scene = f.scene(mesh.cast_rays(f.rays6, want_uv=False)["t_hit"])
Sp, Gp = _lib.Cloud(ctx, scene), _lib.Cloud(ctx, f.model_points, f.normals)
for m in (2, 3, 4, 6, 20):
    put("parity_max%d" % m, _lib.icp(ctx, Sp, Gp, 10.0, f.icp_init(), max_iteration=m, **KW, **FIXED))
if "parity_init" in picked:
    put("rebuild_full", _lib.icp(ctx, Sp, Gp, 10.0, picked["parity_init"], max_iteration=12, **KW, **FIXED))
    put("rebuild_upto", _lib.icp(ctx, Sp, Gp, 10.0, picked["parity_init"], max_iteration=int(picked["parity_rebuild_pass"]), **KW, **FIXED))

# 3. exact ties: a tied slot's bound equals its neighbour's distance and can never certify
src, tgt, nrm = cases.lattice(1000, 512, 7)
Sl, Gl = _lib.Cloud(ctx, src), _lib.Cloud(ctx, tgt, nrm)
for m in (1, 2, 20):
    put("lattice_max%d" % m, _lib.icp(ctx, Sl, Gl, 1.8, np.eye(4), estimator=_lib.POINT_TO_POINT, max_iteration=m, **KW, **FIXED))
np.savez(sys.argv[2], **out)
"""

_SWITCHES = ("PEDP_ICP_CERT", "PEDP_ICP_HEAD_CLOSE", "PEDP_ICP_SERIAL_CLOSE", "PEDP_ICP_COPY_BRACKET", "PEDP_ICP_UNFUSED_FINISH")


@pytest.fixture(scope="module")
def probes(tmp_path_factory, oracle):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("certificate")
    picked = {}
    init, asked = head_close.pick_late_rebuild("parity", oracle)
    if init is not None:
        picked["parity_init"] = init
        picked["parity_rebuild_pass"] = np.int64([p for p in asked if 2 <= p <= 9][0] + 1)
    np.savez(str(tmp / "picked.npz"), **picked)
    res = {"picked": picked}
    for name, extra in (("default", {}), ("off", {"PEDP_ICP_CERT": "0"})):
        out = str(tmp / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", _PROBE, root, out, str(tmp / "picked.npz")], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        res[name] = dict(np.load(out))
    return res


def _same_bytes(probes, names):
    new, old = probes["default"], probes["off"]
    for name in names:
        keys = [k for k in sorted(new) if k.startswith(name + "_") and "_path_" not in k]
        assert len(keys) == 6, (name, keys)
        for k in keys:
            a, b = np.ascontiguousarray(new[k]), np.ascontiguousarray(old[k])
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
        assert int(old[name + "_path_cert"]) == 0, name  # the switch is a switch


def test_smallest_shape_with_every_boundary(probes):
    """Through icp, through icp_begin / icp_end, and a second time on the same context."""
    names = ["small_icp", "small_beginend", "small_again"]
    _same_bytes(probes, names)
    d, o = probes["default"], probes["off"]
    for name in names:
        print(name, "certified", int(d[name + "_path_cert"]), "searched", int(d[name + "_path_searched"]), "pairs", int(d[name + "_path_pairs"]),
              "pairs, switched off", int(o[name + "_path_pairs"]))
        assert d[name + "_trace"].shape == (21, 18)
        assert int(d[name + "_path_cert"]) > 0, name
        assert int(d[name + "_path_pairs"]) < int(o[name + "_path_pairs"]), name
        assert int(d[name + "_path_cert"]) == int(d["small_icp_path_cert"]) and int(d[name + "_path_pairs"]) == int(d["small_icp_path_pairs"])


def test_parity_frame_while_neighbours_still_change(probes):
    _same_bytes(probes, ["parity_max%d" % m for m in (2, 3, 4, 6, 20)])
    d = probes["default"]
    cert = [int(d["parity_max%d_path_cert" % m]) for m in (2, 3, 4, 6, 20)]
    print("certified slots by iteration limit", cert)
    assert cert == sorted(cert) and cert[-1] > 0


def test_exact_ties_never_certify_wrongly(probes):
    _same_bytes(probes, ["lattice_max%d" % m for m in (1, 2, 20)])
    # identity start on the lattice: pass 0 (a rebuild pass) certifies nothing, and every query of pass 1 that has not
    # moved still ties -- its bound is no larger than its neighbour's distance
    d = probes["default"]
    print("lattice: certified", [int(d["lattice_max%d_path_cert" % m]) for m in (1, 2, 20)])


def test_point_to_point_and_nan_source_points(probes):
    _same_bytes(probes, ["small_p2p", "small_nan"])
    d = probes["default"]
    assert int(d["small_p2p_path_cert"]) > 0 and int(d["small_nan_path_cert"]) > 0


def test_a_rebuild_in_mid_run(probes):
    """The start pose test_icp_head_close_gpu.py picks: a rebuild pass behind certified passes drops every certificate
    (its points are recomputed through the history) and writes new ones, which the passes behind it use."""
    assert "parity_init" in probes["picked"], "no start pose with a late rebuild was found on the CPU"
    _same_bytes(probes, ["rebuild_full", "rebuild_upto"])
    d = probes["default"]
    full, upto = int(d["rebuild_full_path_cert"]), int(d["rebuild_upto_path_cert"])
    print("certified over the run", full, "up to and including the rebuild pass", upto)
    assert full - upto > 0
