"""Writes tests/golden/g10_reference.npz from the reference's own numpy / torch functions.

    python tests/golden/make_reference_golden.py /path/to/reference

Runs only where the reference tree exists; no test calls it.  The named function (or method) definitions are taken out
of Utils.py, estimater.py, src/defect_projection.py and src/pose_estimation.py with `ast`, so the files' imports
(open3d, pytorch3d, nvdiffrast, warp, cv2) never execute, and run on the CPU against the installed numpy / torch / scipy
/ sklearn.  The fixture holds names and numbers only: every input the functions were given and every output they gave.

Stand-ins, all of them here: `torch.Tensor.cuda` returns the tensor, `torch.set_default_tensor_type` does nothing, a
bare object with `debug = 0` is guess_translation's `self`, an object with `.intrinsic_matrix` is the camera.  One
observer: guess_translation returns only the centre, so the `np` it sees is numpy itself with `where`, `median` and
`asarray` passed through and their values noted; from these come n_pos and the box (the arrays `np.where(mask>0)` gave),
n_med and the median (np.median's argument and result), uc and vc (the vector given to np.asarray).  Two fields are not
reference values and are marked so: `n_valid` is the generator's count of `(mask>0) & (depth>=0.001)`, the two
comparisons the reference makes, combined as the product's record combines them; where the reference returns before it
forms the median, n_med is 0 with a NaN median if it found `valid` empty, and -1 (not known) if `mask>0` was empty.

Crop windows: the reference's float32 `K @ pts` is a matmul whose last bit depends on the device, so a window edge
within an ulp of a half-integer rounds either way.  The generator forms each unrounded edge in float64 and leaves out
the poses with an edge within 1e-3 px of a half-integer; `crop/d<i>/keep` holds the kept indices.

Not pinned because not executable this way (pytorch3d is not installed): so3_exp_map and rotation_6d_to_matrix, the maps
from the refiner's output to `rot_mat_delta`; only the composition after them (egocentric_delta_pose_to_pose) is.
Every listed function ran.

Layout (keys `<group>/...`): xyz (depth2xyzmap), xyzb (depth2xyzmap_batch), gt (guess_translation), crop
(compute_crop_window_tf_batch, box_3d), pose (egocentric_delta_pose_to_pose), diam (compute_mesh_diameter), proj
(projection_matrix_from_intrinsics), heat (heatmap_to_points, compute_rays), p3d (heatmap_to_point3d,
calc_coordinates), flip (flip_plane_normal_if_needed).  tests/test_reference_cpu.py states the keys and shapes.
"""
import ast
import logging
import os
import sys

import numpy as np
import scipy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

F32 = np.float32
CAMERAS = {"tiny": (38.0, 23.5, 19.5), "parity": (126.0, 79.5, 71.5)}       # synth.CONFIGS: f, cx, cy


# ---------------------------------------------------------------- the reference's definitions

def take(ref_root, rel, names, ns):
    """The FunctionDef nodes called `names` (module level or methods) of ref_root/rel, executed in ns."""
    path = os.path.join(ref_root, rel)
    tree = ast.parse(open(path).read(), path)
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in names and node.name not in found:
            found[node.name] = node
    missing = set(names) - set(found)
    if missing:
        raise SystemExit(f"{rel}: no definition of {sorted(missing)}")
    mod = ast.Module(body=[found[n] for n in names], type_ignores=[])
    exec(compile(mod, path, "exec"), ns)
    return [ns[n] for n in names]


class Noted:
    """numpy, with the values that pass through where / median / asarray kept."""

    def __init__(self):
        self.seen = {}

    def __getattr__(self, name):
        fn = getattr(np, name)
        if name not in ("where", "median", "asarray"):
            return fn

        def call(*a, **k):
            out = fn(*a, **k)
            self.seen[name] = (a, out)
            return out
        return call


class Self:
    debug = 0


class Camera:
    def __init__(self, K):
        self.intrinsic_matrix = np.asarray(K, np.float64)


def cpu_shims():
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.set_default_tensor_type = lambda *a, **k: None


# ---------------------------------------------------------------- inputs

def sprinkle(a, rng, values, each):
    """`each` entries of every value of `values` at distinct random places of a (in place); returns a."""
    flat = a.reshape(-1)
    where = rng.choice(flat.size, size=each * len(values), replace=False)
    for i, v in enumerate(values):
        flat[where[i * each:(i + 1) * each]] = v
    return a


def rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


# ---------------------------------------------------------------- the groups

def group_xyz(out, ref):
    rng = np.random.default_rng(1001)
    K = np.array([[615.3, 0, 31.7], [0, 614.9, 8.3], [0, 0, 1]])
    d = rng.uniform(0.2, 1.5, (17, 65)).astype(F32)
    sprinkle(d, rng, [0.0, 0.000999, 0.001, -0.5, np.nan, np.inf], 10)
    uv = np.empty((64, 2))
    uv[:, 0] = rng.uniform(0, 63.4, 64)
    uv[:, 1] = rng.uniform(0, 15.4, 64)
    uv[0:8, 0] = 2 * rng.integers(0, 31, 8) + 0.5            # even floor, .5: half-even stays, half-away goes up
    uv[8:16, 0] = 2 * rng.integers(0, 31, 8) + 1.5           # odd floor, .5: both go up
    uv[16:22, 1] = 2 * rng.integers(0, 7, 6) + 0.5
    uv[22:28, 1] = 2 * rng.integers(0, 7, 6) + 1.5
    uv[28:32] = uv[0:4] - [0.25, 0.0]                        # duplicates after rounding: (e + .25, v) goes to e like (e + .5, v)
    special = np.argwhere(~(d >= 0.001) | np.isinf(d))[:12]  # some listed pixels are invalid / NaN / inf ones
    uv[32:44] = special[:, ::-1] + rng.uniform(-0.4, 0.4, (12, 2))
    uv = np.clip(uv, 0, [63.9, 15.9])
    out["xyz/K"], out["xyz/depth"], out["xyz/uvs"] = K, d, uv
    out["xyz/out"] = ref["depth2xyzmap"](d.copy(), K)
    out["xyz/out_uvs"] = ref["depth2xyzmap"](d.copy(), K, uvs=uv.copy())
    d1 = np.array([[0.75]], F32)
    out["xyz/depth1"], out["xyz/out1"] = d1, ref["depth2xyzmap"](d1.copy(), K)
    away = np.floor(np.abs(uv) + 0.5)
    print(f"xyz: 17x65 and 1x1; {int((np.round(uv) != away).any(1).sum())} uvs where half-even and half-away differ, "
          f"{int(((uv % 1) == 0.5).any(1).sum())} with a .5, "
          f"{64 - len(np.unique(np.round(uv), axis=0))} duplicates after rounding")


def group_xyzb(out, ref):
    rng = np.random.default_rng(1002)
    z8 = F32(0.8)
    d = rng.uniform(0.2, 1.2, (3, 17, 65)).astype(F32)
    d[rng.random(d.shape) < 0.45] = 0                         # holes, as a sensor leaves them (and a smaller fixture)
    sprinkle(d, rng, [z8, np.nextafter(z8, F32(1)), np.nextafter(z8, F32(0)), np.nan, -0.3, 0.0, 0.000999, 0.001, np.inf], 24)
    Ks = np.array([[[615.3, 0, 31.7], [0, 614.9, 8.3], [0, 0, 1]], [[300.0, 0, 32.5], [0, 310.0, 7.5], [0, 0, 1]],
                   [[912.25, 0, 40.125], [0, 911.5, 3.875], [0, 0, 1]]], F32)
    clean = np.where((d >= F32(0.001)) & (d < F32(100)), d, F32(0)).astype(F32)
    out["xyzb/depths"], out["xyzb/Ks"], out["xyzb/clean"] = d, Ks, clean[:1]
    out["xyzb/zfars"] = np.array([np.inf, 0.8])
    for tag, zfar in (("inf", np.inf), ("0.8", 0.8)):
        out[f"xyzb/out_{tag}"] = ref["depth2xyzmap_batch"](torch.from_numpy(d.copy()), torch.from_numpy(Ks.copy()), zfar).numpy()
    # what the two depth filters at radius 0 leave of image 0 (values in [0.001, 100), else 0), for depth_to_scene's xyz map
    out["xyzb/clean_out_0.8"] = ref["depth2xyzmap_batch"](torch.from_numpy(clean[:1].copy()), torch.from_numpy(Ks[:1].copy()), 0.8).numpy()
    kept = (out["xyzb/out_0.8"][..., 2].view(np.uint32) == z8.view(np.uint32)).sum()
    print(f"xyzb: 3x17x65; {int((d == z8).sum())} entries equal to zfar, {int(kept)} of them kept; "
          f"{int((d == np.nextafter(z8, F32(1))).sum())} one ulp above")


def gt_depth(h, w, rng, quantised):
    d = rng.uniform(0.3, 1.6, (h, w)).astype(F32)
    if quantised:
        d = (np.round(d * quantised) / quantised).astype(F32)     # centimetres or millimetres: ties
    r = rng.random((h, w))
    for lo, hi, v in ((0, .10, 0), (.10, .13, -0.4), (.13, .15, np.nan), (.15, .16, np.inf), (.16, .17, 0.000999), (.17, .18, 0.001)):
        d[(r >= lo) & (r < hi)] = v
    return d


def gt_mask(h, w, rng, kind):
    yy, xx = np.mgrid[:h, :w]
    blob = ((yy - 0.45 * h) ** 2 / max(0.09 * h * h, 1) + (xx - 0.55 * w) ** 2 / max(0.06 * w * w, 1)) <= 1
    blob &= rng.random((h, w)) < 0.9
    if kind == "bool":
        return blob
    if kind == "uint8":
        return (blob * rng.choice(np.array([1, 2, 255], np.uint8), (h, w))).astype(np.uint8)
    m = np.where(blob, rng.uniform(0.1, 2.0, (h, w)), 0).astype(F32)
    r = rng.random((h, w))
    m[r < 0.03] = -1.5                 # truthy, not positive: in the median, not in the box
    m[(r >= 0.03) & (r < 0.05)] = np.nan
    m[(r >= 0.05) & (r < 0.07)] = -0.0
    return m


def group_gt(out, ref):
    rng = np.random.default_rng(1003)
    K = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]])
    out["gt/K"] = K
    cases = {}
    for h, w in ((37, 53), (64, 96)):
        # continuous (c) and centimetre (q) depths; the larger frame has one image, in millimetres, for all its masks
        for dk, q in ((("c", 0), ("q", 100)) if h == 37 else (("q", 1000),)):
            out[f"gt/depth/{h}x{w}_{dk}"] = gt_depth(h, w, rng, q)
        for dk, kind, parity in (("c", "bool", 1), ("q", "uint8", 0), ("c", "float32", 0), ("q", "float32", 1)):
            dk = dk if h == 37 else "q"
            depth = out[f"gt/depth/{h}x{w}_{dk}"]
            mask = gt_mask(h, w, rng, kind)
            with np.errstate(invalid="ignore"):
                chosen = mask.astype(bool) & (depth >= 0.001)
            if chosen.sum() % 2 != parity:                        # an odd and an even count of each kind
                v, u = np.argwhere(chosen & (mask > 0))[len(chosen) // 2]
                mask[v, u] = 0
            cases[f"{h}x{w}_{dk}_{kind}_{'odd' if parity else 'even'}"] = (f"{h}x{w}_{dk}", mask)
    out["gt/depth/1x1_a"] = np.array([[0.5]], F32)
    out["gt/depth/1x1_b"] = np.array([[0.001]], F32)
    cases["1x1_bool"] = ("1x1_a", np.array([[True]]))
    cases["1x1_uint8"] = ("1x1_b", np.array([[255]], np.uint8))
    cases["1x1_negative"] = ("1x1_a", np.array([[-1.0]], F32))    # truthy but not positive: "mask is all zero"
    cases["zero_mask"] = ("37x53_c", np.zeros((37, 53), np.uint8))
    d = out["gt/depth/37x53_q"].copy()
    m = gt_mask(37, 53, rng, "uint8")
    d[(m > 0) & (d >= 0.001)] = 0.000999
    out["gt/depth/37x53_none"] = d
    cases["no_valid"] = ("37x53_none", m)
    out["gt/cases"] = np.array(list(cases))
    for name, (dk, mask) in cases.items():
        depth = out[f"gt/depth/{dk}"]
        noted = Noted()
        ref["guess_translation"].__globals__["np"] = noted
        with np.errstate(invalid="ignore", over="ignore"):
            center = ref["guess_translation"](Self(), depth=depth.copy(), mask=mask.copy(), K=K.copy())
            positive = mask > 0
        (_, (vs, us)) = noted.seen["where"]
        rec = {"n_pos": len(us), "n_med": 0 if len(us) else -1, "median": F32(np.nan), "uc": np.nan, "vc": np.nan}
        rec.update(zip(("umin", "umax", "vmin", "vmax"), (us.min(), us.max(), vs.min(), vs.max()) if len(us) else (-1,) * 4))
        if "median" in noted.seen:
            (picked,), med = noted.seen["median"]
            rec["n_med"], rec["median"] = picked.size, med
            assert isinstance(med, F32)
            rec["uc"], rec["vc"] = (float(v) for v in noted.seen["asarray"][0][0][:2])
        rec["n_valid"] = int((positive & (depth >= 0.001)).sum())          # the generator's, see the docstring
        out[f"gt/{name}/depth"] = np.array(dk)
        out[f"gt/{name}/mask"] = mask
        out[f"gt/{name}/center"] = np.asarray(center, np.float64)
        for k, v in rec.items():
            out[f"gt/{name}/{k}"] = np.asarray(v)
        with np.errstate(invalid="ignore"):
            odd = int((mask.astype(bool) & ~positive).sum())
        print(f"gt/{name}: {mask.dtype} n_pos {rec['n_pos']} n_med {rec['n_med']} median {rec['median']!r} "
              f"truthy-not-positive {odd} center {center}")
    ref["guess_translation"].__globals__["np"] = np


def group_crop(out, ref):
    rng = np.random.default_rng(1004)
    n = 2000
    t = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.25, 0.25, n), rng.uniform(0.3, 1.5, n)], 1)
    t = (np.round(t * 8192) / 8192).astype(F32)               # an eighth of a millimetre: the inputs pack smaller
    K = np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]], F32)
    poses = np.tile(np.eye(4, dtype=F32), (n, 1, 1))
    poses[:, :3, 3] = t
    out["crop/trans"], out["crop/K"] = t, K
    out["crop/diameters"], out["crop/crop_ratio"] = np.array([0.1, 0.137, 0.3]), np.array(1.2)
    out["crop/out_sizes"] = np.array([[160, 160], [32, 48]])
    t64 = t.astype(np.float64)
    for di, diam in enumerate(out["crop/diameters"].tolist()):
        r = float(F32(diam * 1.2 / 2))
        cu, cv = 600.0 * t64[:, 0] / t64[:, 2] + 319.5, 600.0 * t64[:, 1] / t64[:, 2] + 239.5
        rad = 600.0 * r / t64[:, 2]
        edges = np.stack([cu - rad, cu + rad, cv - rad, cv + rad], 1)
        keep = np.nonzero((np.abs(edges - np.floor(edges) - 0.5) >= 1e-3).all(1))[0]
        out[f"crop/d{di}/keep"] = keep.astype(np.int32)
        for oi, size in enumerate(out["crop/out_sizes"].tolist()):
            if oi == 1 and di != 1:
                continue                                          # the second out_size differs by one product: one diameter
            tf = ref["compute_crop_window_tf_batch"](poses=torch.from_numpy(poses.copy()), K=torch.from_numpy(K.copy()),
                                                     crop_ratio=1.2, out_size=tuple(size), method="box_3d", mesh_diameter=diam)
            tf = tf.numpy()
            rest = tf.copy()
            rest[:, [0, 0, 1, 1], [0, 2, 1, 2]] = 0
            assert (rest.view(np.uint32) == np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], F32).view(np.uint32)).all()
            # the five other entries are +0 and 1 in every pose (asserted above): the four that vary, one array each
            for name, (i, j) in (("sx", (0, 0)), ("tx", (0, 2)), ("sy", (1, 1)), ("ty", (1, 2))):
                out[f"crop/d{di}_o{oi}/{name}"] = np.ascontiguousarray(tf[:, i, j])
        print(f"crop: diameter {diam}: {n - len(keep)} of {n} poses left out ({100 * (n - len(keep)) / n:.2f} %)")
    # Edges at exactly a half-integer, which the 2,000 poses above cannot keep: translations in 64ths at depths 0.5, 1
    # and 2 with a radius of exactly 1 / 16 (float32 of 0.125 * 1.0 / 2).  Every product, sum and quotient of the
    # projection is then exact in float32 in any order, with or without FMA, so the rounding alone decides.
    half, floors = [], []
    for z in (0.5, 1.0, 2.0):
        for kx in range(-12, 13):
            for ky in range(-10, 11):
                cu, cv, rad = 600.0 * (kx / 64) / z + 319.5, 600.0 * (ky / 64) / z + 239.5, 600.0 * 0.0625 / z
                edges = np.array([cu - rad, cu + rad, cv - rad, cv + rad])
                if (edges % 1 == 0.5).all() and (np.floor(edges) % 2 == 0).any():
                    half.append([kx / 64, ky / 64, z])
                    floors.append(np.floor(edges) % 2)
    pick = np.random.default_rng(1009).permutation(len(half))[:24]
    t = np.array(half, F32)[pick]
    poses = np.tile(np.eye(4, dtype=F32), (len(t), 1, 1))
    poses[:, :3, 3] = t
    out["crop/half/trans"], out["crop/half/diameter"], out["crop/half/crop_ratio"] = t, np.array(0.125), np.array(1.0)
    out["crop/half/tf"] = ref["compute_crop_window_tf_batch"](poses=torch.from_numpy(poses.copy()), K=torch.from_numpy(K.copy()),
                                                              crop_ratio=1.0, out_size=(160, 160), method="box_3d", mesh_diameter=0.125).numpy()
    print(f"crop/half: {len(t)} poses with every edge at a half-integer, {int((np.array(floors)[pick] == 0).sum())} edges with an even floor")


def group_pose(out, ref):
    rng = np.random.default_rng(1005)
    n = 300
    A = np.tile(np.eye(4, dtype=F32), (n, 1, 1))
    A[:, :3, :3] = rotations(rng, n)
    A[:, :3, 3] = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.3, 1.5, n)], 1)
    R = rotations(rng, n).astype(F32)                         # the 6d rows b1, b2 (orthonormal up to float32 rounding)
    td = rng.uniform(-0.05, 0.05, (n, 3)).astype(F32)
    Rd = np.ascontiguousarray(R.transpose(0, 2, 1))           # the kernel emits the transposed map as rot_mat_delta
    out["pose/A"], out["pose/td"], out["pose/Rd"] = A, td, Rd
    out["pose/B"] = ref["egocentric_delta_pose_to_pose"](torch.from_numpy(A.copy()), torch.from_numpy(td.copy()),
                                                         torch.from_numpy(Rd.copy())).numpy()
    print(f"pose: {n} triples")


def group_diam(out, ref):
    rng = np.random.default_rng(1006)

    def cloud(k):
        return rng.standard_normal((k, 3)).astype(F32).astype(np.float64)      # float32 values: they pack smaller
    clouds = {str(k): cloud(k) for k in (1, 2, 255, 256, 257, 513)}
    clouds["equal"] = np.tile(cloud(1), (257, 1))
    far = cloud(300) * 0.1
    far[5], far[290] = [-7.25, 3.5, 1.125], [6.5, -2.75, -3.0625]             # the extreme pair, in two tiles
    clouds["far"] = far
    out["diam/cases"] = np.array(list(clouds))
    for name, p in clouds.items():
        out[f"diam/{name}/pts"] = p
        out[f"diam/{name}/out"] = np.float64(ref["compute_mesh_diameter"](model_pts=p.copy(), n_sample=None))
        print(f"diam/{name}: {len(p)} points, {float(out[f'diam/{name}/out'])!r}")


def group_proj(out, ref):
    sets = [(np.array([[600.0, 0, 319.5], [0, 600.0, 239.5], [0, 0, 1]]), 480, 640, 0.001, 100),        # the renderer's defaults
            (np.array([[615.3, 0.7, 31.7], [0, 614.9, 8.3], [0, 0, 1]]), 17, 65, 0.1, 10.0),
            (np.array([[126.0, 0, 79.5], [0, 126.0, 71.5], [0, 0, 1]]), 144, 160, 0.05, 3)]
    out["proj/n"] = np.array(len(sets))
    for i, (K, h, w, near, far) in enumerate(sets):
        out[f"proj/{i}/K"], out[f"proj/{i}/hw"], out[f"proj/{i}/near_far"] = K, np.array([h, w]), np.array([near, far], np.float64)
        for wc in ("y_down", "y_up"):
            out[f"proj/{i}/{wc}"] = ref["projection_matrix_from_intrinsics"](K.copy(), h, w, near, far, window_coords=wc)
    print(f"proj: {len(sets)} sets x 2 window_coords")


def points_arrays(pts, dtype):
    """The reference's list of (x, y, intensity) tuples as arrays (x and y are numpy integers, intensity the map's type)."""
    xy = np.array([[p[0], p[1]] for p in pts], np.int64).reshape(-1, 2)
    return xy, np.array([p[2] for p in pts], dtype)


def group_heat(out, ref):
    rng = np.random.default_rng(1007)
    h9 = rng.uniform(-0.5, 1.0, (9, 11))
    sprinkle(h9, rng, [0.5, np.nan, -0.25, 0.3], 6)
    t3 = F32(0.3)                                             # float32(0.3) > 0.3: numpy compares a float32 map in float32
    h48 = (rng.integers(-32, 65, (48, 64)) / 64).astype(F32)
    h48[rng.random((48, 64)) < 0.75] -= F32(0.5)              # most pixels cold
    sprinkle(h48, rng, [0.5, np.nan, -0.25, t3, np.nextafter(t3, F32(1)), np.nextafter(t3, F32(0))], 40)
    out["heat/h9"], out["heat/h48"] = h9, h48
    out["heat/thresholds"] = np.array([0.5, 0.3, -0.25])
    for cam, (f, cx, cy) in CAMERAS.items():
        out[f"heat/K_{cam}"] = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])
    for name, h in (("h9", h9), ("h48", h48)):
        for ti, thr in enumerate(out["heat/thresholds"].tolist()):
            with np.errstate(invalid="ignore"):
                pts = ref["heatmap_to_points"](h.copy(), thr)
            xy, inten = points_arrays(pts, h.dtype)
            out[f"heat/{name}_t{ti}/xy"], out[f"heat/{name}_t{ti}/intensity"] = xy, inten
            with np.errstate(invalid="ignore"):
                print(f"heat/{name} threshold {thr}: {len(pts)} points, {int((h == h.dtype.type(thr)).sum())} entries equal to it")
            if ti == 0:
                for cam in CAMERAS:
                    rays, iv = ref["compute_rays"](pts, Camera(out[f"heat/K_{cam}"]))
                    out[f"heat/{name}_t{ti}/rays_{cam}"] = rays
                    assert np.array_equal(iv, inten)
    with np.errstate(invalid="ignore"):
        empty = ref["compute_rays"](ref["heatmap_to_points"](h9.copy(), 5.0), Camera(out["heat/K_tiny"]))
    out["heat/empty_rays_shape"] = np.array(np.asarray(empty[0]).shape + np.asarray(empty[1]).shape)


def group_p3d(out, ref):
    rng = np.random.default_rng(1008)
    heat = rng.uniform(0, 1.0, (9, 11))
    heat[4, 5] = 2.0                                          # the maximum: intensities are heat / 2
    heat[2, 3:7] = 0.2                                        # 0.2 / 2 equals the threshold 0.1: not above it
    depth = rng.uniform(300, 900, (9, 11)).astype(F32)
    sprinkle(depth, rng, [0.0, -5.0], 8)
    d16 = np.where(depth > 0, depth, 0).astype(np.uint16)
    cam = Camera([[38.0, 0, 23.5], [0, 38.0, 19.5], [0, 0, 1]])
    out["p3d/K"], out["p3d/heat"] = cam.intrinsic_matrix, heat
    out["p3d/thresholds"] = np.array([0.1, 0.45])
    pts = rng.permutation(np.argwhere(depth > 0))[:12, ::-1].copy()      # integer (x, y) pixels
    pts[3] = np.argwhere(depth == 0)[0][::-1]                 # one point at zero depth: skipped
    pts[7] = np.argwhere(depth < 0)[0][::-1]                  # one at a negative depth: kept
    out["p3d/points"] = pts
    for name, d in (("f32", depth), ("u16", d16), ("small", depth[:7, :9].copy())):
        out[f"p3d/depth_{name}"] = d
        for ti, thr in enumerate(out["p3d/thresholds"].tolist()):
            out[f"p3d/{name}_t{ti}/out"] = ref["heatmap_to_point3d"](heat.copy(), d.copy(), cam, thr)
            print(f"p3d/{name} threshold {thr}: {len(out[f'p3d/{name}_t{ti}/out'])} points")
        if name != "small":
            out[f"p3d/{name}/coords"] = ref["calc_coordinates"](d.copy(), pts.copy(), cam)
    out["p3d/equal_to_threshold"] = np.array(int((heat / heat.max() == 0.1).sum()))


def group_flip(out, ref):
    planes = np.array([[0.0, 0.0, 2.0, -5.0], [0.0, 0.0, 2.0, -5.0], [1.0, -2.0, 0.5, 3.0], [1.0, -2.0, 0.5, 3.0],
                       [0.0, 3.0, 0.0, 1.0], [-0.3, 0.4, -1.2, 0.25]])
    normals = np.array([[0.1, 0.2, 0.9], [0.1, 0.2, -0.9], [-0.5, 0.5, 0.1], [0.5, -0.5, 0.1],
                        [1.0, 0.0, 0.0], [0.2, -0.1, 0.7]])      # the fifth: dot product exactly 0, not flipped
    out["flip/planes"], out["flip/normals"] = planes, normals
    res = [ref["flip_plane_normal_if_needed"](list(p), n.copy()) for p, n in zip(planes.copy(), normals)]
    out["flip/out_planes"] = np.array([np.asarray(m, np.float64) for m, _ in res])
    out["flip/out_normals"] = np.array([n for _, n in res])
    print(f"flip: {int((out['flip/out_planes'][:, 3] != planes[:, 3]).sum())} of {len(planes)} flipped")


def main(ref_root):
    cpu_shims()
    ns = {"np": np, "torch": torch, "scipy": scipy, "logging": logging}
    ref = {}
    for rel, names in (("Utils.py", ["depth2xyzmap", "depth2xyzmap_batch", "compute_crop_window_tf_batch",
                                     "egocentric_delta_pose_to_pose", "compute_mesh_diameter",
                                     "projection_matrix_from_intrinsics"]),
                       ("estimater.py", ["guess_translation"]),
                       ("src/defect_projection.py", ["heatmap_to_points", "compute_rays", "heatmap_to_point3d", "calc_coordinates"]),
                       ("src/pose_estimation.py", ["flip_plane_normal_if_needed"])):
        ref.update(zip(names, take(ref_root, rel, names, dict(ns))))
    out = {}
    for group in (group_xyz, group_xyzb, group_gt, group_crop, group_pose, group_diam, group_proj, group_heat, group_p3d,
                  group_flip):
        group(out, ref)
    path = os.path.join(HERE, "g10_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
