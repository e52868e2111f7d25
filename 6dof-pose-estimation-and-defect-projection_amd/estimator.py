"""FoundationPose's first stage over the package's kernels: the estimator (estimater.py) and the two predictors' loops
(learning/training/predict_pose_refine.py:93-295, predict_score.py:117-226).

    mask_depth_stats        counts, box and exact median of a mask over a depth frame in one library call
                            (pedp_mask_depth_stats, csrc/pedp_estimator.hip)
    guess_translation       estimater.py:135-154 on that record; the last step is the reference's numpy expression
    set_seed, euler_matrix, sample_views_icosphere, compute_mesh_diameter      Utils.py:222-229, :483-507, :559-574
    rotation_grid           estimater.py:104-121 as a function (views x in-plane steps, inverted, clustered)
    PoseRefinePredictor, ScorePredictor     the loops around the caller's networks
    FoundationPose          reset_object, make_rotation_grid, register, track_one, ...

The networks are the caller's torch modules (`model(A, B) -> {'trans', 'rot'}`, `model(A, B, L=) -> {'score_logit'}`):
their definitions, weights and checkpoint loading are not part of this package.  Between the frame going up and the pose
coming back nothing leaves the device except the statistics record (32 bytes) in `register`.  The contract, and what is
unpinned (the icosphere's vertex order, ties in the score sort, autocast numerics), is DESIGN.md s4.11.
"""
import copy
import ctypes as C
import logging
import os
import random

import numpy as np

from . import _lib, cloud_ops
from ._bridge import device_of, is_torch, launch, ptr, to_device
from .crop import _crop_batch, _source
from .depth_filters import bilateral_filter_depth, depth2xyzmap, depth2xyzmap_batch, erode_depth
from .pose import max_pair_distance, pose_update, update_params
from .render import RasterizeCudaContext, make_mesh_tensors


# ---------------------------------------------------------------- mask / depth statistics

def _host(x):
    return x.detach().cpu().numpy() if is_torch(x) else np.asarray(x)


def _dtype_name(x):
    return str(x.dtype).replace("torch.", "")


def _kernel_reads(depth, mask):
    """The kernel takes this pair as it is: a float32 depth and a bool / uint8 / float32 mask."""
    return (hasattr(depth, "dtype") and hasattr(mask, "dtype") and _dtype_name(depth) == "float32"
            and _dtype_name(mask) in ("bool", "uint8", "float32"))


def mask_depth_stats(depth, mask):
    """depth H x W float32, mask H x W bool / uint8 / float32 (numpy, CPU or CUDA tensors; if either is on a GPU the call
    runs there on the caller's current stream) -> dict(n_pos, n_valid, n_med, umin, umax, vmin, vmax, median):
    the count and box of `mask > 0`, the count of `(depth >= 0.001) & (mask > 0)`, and the count and np.median (bit for
    bit, an np.float32) of `depth[mask.astype(bool) & (depth >= 0.001)]`.  The box is -1 for an empty mask, the median NaN
    for an empty set.  The call waits for the record."""
    if not hasattr(depth, "shape") or not hasattr(mask, "shape"):
        raise _lib.PedpError("mask_depth_stats: depth and mask must be arrays or tensors")
    ds, ms = tuple(depth.shape), tuple(mask.shape)
    if len(ds) != 2 or ds != ms:
        raise _lib.PedpError(f"mask_depth_stats: depth and mask must be the same H x W, got {ds} and {ms}")
    if not _kernel_reads(depth, mask):
        raise _lib.PedpError(f"mask_depth_stats: float32 depth and bool / uint8 / float32 mask, got {_dtype_name(depth)} "
                             f"and {_dtype_name(mask)}")
    H, W = int(ds[0]), int(ds[1])
    if H <= 0 or W <= 0 or H * W > 4096 * 4096:
        raise _lib.PedpError(f"mask_depth_stats: {H} x {W} frame (1 to 4096 x 4096 pixels)")
    dev = device_of(depth, mask)
    if dev is not None:
        import torch

        d = to_device(depth, dev).contiguous()
        m = mask if is_torch(mask) else torch.from_numpy(np.ascontiguousarray(mask))
        if not m.is_cuda:
            m = m.contiguous().pin_memory().to(dev, non_blocking=True)
        m = (m if m.device == dev else m.to(dev)).contiguous()
        f32 = m.dtype == torch.float32
    else:
        d = np.ascontiguousarray(_host(depth))
        m = np.ascontiguousarray(_host(mask))
        f32 = m.dtype == np.float32
    rec = _lib.MaskDepthStats()
    launch(dev, "pedp_mask_depth_stats", lambda lib, h, mem: lib.pedp_mask_depth_stats(
        h, ptr(d), ptr(m), _lib.F32 if f32 else _lib.U8, H, W, mem, C.byref(rec)))
    out = {k: int(getattr(rec, k)) for k in ("n_pos", "n_valid", "n_med", "umin", "umax", "vmin", "vmax")}
    out["median"] = np.float32(rec.median)
    return out


def _host_stats(depth, mask):
    """The same record from numpy, for the dtypes the kernel does not read."""
    depth, mask = _host(depth), _host(mask)
    rows, cols = np.nonzero(mask > 0)
    near = depth >= 0.001
    picked = depth[mask.astype(bool) & near]
    box = (int(cols.min()), int(cols.max()), int(rows.min()), int(rows.max())) if len(cols) else (-1,) * 4
    return {"n_pos": len(cols), "n_valid": int((near & (mask > 0)).sum()), "n_med": int(picked.size),
            "umin": box[0], "umax": box[1], "vmin": box[2], "vmax": box[3],
            "median": np.median(picked) if picked.size else np.float32(np.nan)}


def _stats(depth, mask):
    return mask_depth_stats(depth, mask) if _kernel_reads(depth, mask) else _host_stats(depth, mask)


def _center_from(rec, K):
    """estimater.py:137-154 from the record: the box midpoint back-projected to the median depth, in numpy on the host."""
    if rec["n_pos"] == 0:
        logging.info("mask is all zero")
        return np.zeros((3))
    uc = (rec["umin"] + rec["umax"]) / 2.0
    vc = (rec["vmin"] + rec["vmax"]) / 2.0
    if rec["n_med"] == 0:
        logging.info("valid is empty")
        return np.zeros((3))
    zc = rec["median"]
    center = (np.linalg.inv(_host(K)) @ np.asarray([uc, vc, 1]).reshape(3, 1)) * zc
    return center.reshape(3)


def guess_translation(depth, mask, K):
    """The translation every pose hypothesis starts from: the mask's box midpoint at the median of the masked depths
    (>= 0.001), through inv(K).  np.zeros(3) for an empty mask or no such depth.  A float32 depth with a bool / uint8 /
    float32 mask is reduced by the kernel (host or device memory); any other dtype by the same expressions in numpy."""
    return _center_from(_stats(depth, mask), K)


# ---------------------------------------------------------------- helpers of Utils.py

def set_seed(random_seed):
    """Utils.py:222-229: numpy's and Python's global generators, torch's CPU and device generators, cudnn's switches."""
    import torch

    np.random.seed(random_seed)
    random.seed(random_seed)
    torch.manual_seed(random_seed)
    torch.cuda.manual_seed_all(random_seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False


def euler_matrix(ai, aj, ak, axes="sxyz"):
    """transformations.euler_matrix for static x-y-z axes (the only convention the rotation grid uses): a 4 x 4 float64
    Rz(ak) Ry(aj) Rx(ai)."""
    if axes != "sxyz":
        raise NotImplementedError(f"euler_matrix: axes {axes!r} (sxyz only)")
    si, sj, sk = np.sin(ai), np.sin(aj), np.sin(ak)
    ci, cj, ck = np.cos(ai), np.cos(aj), np.cos(ak)
    M = np.identity(4)
    M[0, :3] = cj * ck, sj * si * ck - ci * sk, sj * ci * ck + si * sk
    M[1, :3] = cj * sk, sj * si * sk + ci * ck, sj * ci * sk - si * ck
    M[2, :3] = -sj, cj * si, cj * ci
    return M


_ICO_FACES = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
              (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
              (9, 8, 1)]


def icosphere(subdivisions=1, radius=1.0):
    """Unit icosahedron, each subdivision adding the edge midpoints pushed out to the sphere -> (vertices V x 3 float64,
    faces F x 3).  Vertex order: the 12 icosahedron vertices, then each level's midpoints in the order its faces meet
    them (trimesh's order is not reproduced; the set of vertices is the same)."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    verts = [np.asarray(p, np.float64) / np.sqrt(1.0 + t * t) for p in v]
    faces = list(_ICO_FACES)
    for _ in range(int(subdivisions)):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = (verts[a] + verts[b]) / 2.0
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return np.asarray(verts) * radius, np.asarray(faces, np.int64)


def sample_views_icosphere(n_views, subdivisions=None, radius=1):
    """Utils.py:483-507: one camera per icosphere vertex, looking at the origin (z towards it, x = up x z with up = +z,
    (1, 0, 0) at the poles), as cam_in_ob N x 4 x 4 float64.  Without `subdivisions` the first level with at least n_views
    vertices (12, 42, 162, ...)."""
    if subdivisions is None:
        subdivisions = 1
        while 10 * 4 ** subdivisions + 2 < n_views:
            subdivisions += 1
    verts, _ = icosphere(subdivisions, radius)
    cams = np.tile(np.eye(4)[None], (len(verts), 1, 1))
    cams[:, :3, 3] = verts
    z = -cams[:, :3, 3]
    z /= np.linalg.norm(z, axis=-1).reshape(-1, 1)
    x = np.cross(np.array([0, 0, 1]).reshape(1, 3), z)
    x[(x == 0).all(axis=-1)] = [1, 0, 0]
    x /= np.linalg.norm(x, axis=-1).reshape(-1, 1)
    y = np.cross(z, x)
    y /= np.linalg.norm(y, axis=-1).reshape(-1, 1)
    cams[:, :3, 0], cams[:, :3, 1], cams[:, :3, 2] = x, y, z
    return cams


def compute_mesh_diameter(model_pts=None, mesh=None, n_sample=1000):
    """Utils.py:559-574.  model_pts: the largest distance between two of (at most n_sample) points, drawn with
    np.random.choice from numpy's global generator as the reference draws them, the maximum on the device
    (max_pair_distance).  mesh: the reference's SVD branch as it is written there (it needs scipy)."""
    if mesh is not None:
        import scipy.linalg

        u, s, _ = scipy.linalg.svd(np.asarray(mesh.vertices), full_matrices=False)
        pts = u @ s
        return float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    model_pts = _host(model_pts)
    if n_sample is None:
        pts = model_pts
    else:
        ids = np.random.choice(len(model_pts), size=min(n_sample, len(model_pts)), replace=False)
        pts = model_pts[ids]
    return max_pair_distance(pts)


def rotation_grid(min_n_views=40, inplane_step=60, symmetry_tfs=None):
    """estimater.py:104-121: every icosphere view turned about its optical axis in steps of inplane_step degrees,
    inverted to ob_in_cam, then cluster_poses(30 degrees, 99999) under the symmetries -> n x 4 x 4 float32 (host)."""
    from .compat import cluster_poses

    grid = []
    for cam_in_ob in sample_views_icosphere(n_views=min_n_views):
        for inplane in np.deg2rad(np.arange(0, 360, inplane_step)):
            grid.append(np.linalg.inv(cam_in_ob @ euler_matrix(0, 0, inplane)))
    sym = np.eye(4, dtype=np.float32)[None] if symmetry_tfs is None else np.asarray(_host(symmetry_tfs), np.float32)
    return np.asarray(cluster_poses(30, 99999, np.asarray(grid), sym.reshape(-1, 4, 4)), dtype=np.float32).reshape(-1, 4, 4)


# ---------------------------------------------------------------- predictors

class Config(dict):
    """A predictor's settings: a dict whose keys also read as attributes (the reference uses both spellings)."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None

    def __setattr__(self, key, value):
        self[key] = value


_REFINER_DEFAULTS = {"use_normal": False, "use_mask": False, "use_BN": False, "c_in": 4, "crop_ratio": 1.2, "n_view": 1,
                     "trans_rep": "tracknet", "rot_rep": "axis_angle", "zfar": 3, "normalize_xyz": False,
                     "normal_uint8": False}
_SCORER_DEFAULTS = {"use_normal": False, "use_BN": False, "zfar": np.inf, "c_in": 4, "normalize_xyz": False,
                    "crop_ratio": 1.2}


def _config(cfg, defaults, required, who):
    """cfg (a mapping or an object with attributes) with the reference's defaults filled in."""
    out = Config()
    if cfg is not None:
        out.update({k: cfg[k] for k in cfg.keys()} if hasattr(cfg, "keys") else
                   {k: v for k, v in vars(cfg).items() if not k.startswith("_")})
    for k, v in defaults.items():
        if k not in out or (k == "crop_ratio" and out[k] is None):
            out[k] = v
    if isinstance(out["zfar"], str) and "inf" in out["zfar"].lower():
        out["zfar"] = np.inf
    missing = [k for k in required if out.get(k) is None]
    if missing:
        raise KeyError(f"{who}: cfg lacks {', '.join(missing)}")
    out["enable_amp"] = True
    return out


def _need_model(model, who, outputs):
    if model is None or not callable(model):
        raise ValueError(f"{who}: pass the network as model= (a torch module returning {outputs}); network definitions, "
                         "weights and checkpoint loading are not part of this package")
    return model.eval() if hasattr(model, "eval") else model


def _no_vis(get_vis):
    if get_vis:
        raise NotImplementedError("get_vis=True draws with cv2 / torchvision, which this package does not use")


def _frame_device(*xs):
    import torch

    dev = device_of(*xs)
    return dev if dev is not None else torch.device("cuda", torch.cuda.current_device())


class PoseRefinePredictor:
    """predict_pose_refine.py:93-295 around the caller's network.  cfg needs input_resize, trans_normalizer and
    rot_normalizer; the rest takes the reference's defaults.  `dataset` holds the cfg, as the crop batch reads it."""

    CHUNK = 1024  # poses per forward pass (predict_pose_refine.py:167)

    def __init__(self, model=None, cfg=None, amp=True):
        self.model = _need_model(model, "PoseRefinePredictor", "{'trans', 'rot'}")
        self.amp = amp
        self.cfg = _config(cfg, _REFINER_DEFAULTS, ("input_resize", "trans_normalizer", "rot_normalizer"), "PoseRefinePredictor")
        if self.cfg["trans_rep"] == "deepim":
            raise NotImplementedError("trans_rep 'deepim' is not supported")
        self.last_trans_update = None
        self.last_rot_update = None

    def predict(self, rgb, depth, K, ob_in_cams, xyz_map, normal_map=None, get_vis=False, mesh=None, mesh_tensors=None,
                glctx=None, mesh_diameter=None, iteration=5):
        """rgb H x W x 3, depth H x W, xyz_map H x W x 3, ob_in_cams N x 4 x 4 (numpy or tensors; device tensors are used
        where they are) -> (poses N x 4 x 4 float32 on the device, None).  Each iteration is one packed crop batch, the
        network in chunks of 1024 poses under autocast, and pose_update; the poses stay on the device throughout."""
        import torch

        _no_vis(get_vis)
        cfg = self.cfg
        dev = _frame_device(ob_in_cams, rgb, depth, xyz_map)
        if not cfg["use_normal"]:
            normal_map = None
        if mesh_tensors is None:
            mesh_tensors = make_mesh_tensors(mesh)
        tn = cfg["trans_normalizer"]
        prm = update_params(trans_rep=cfg["trans_rep"], rot_rep=cfg["rot_rep"], normalize_xyz=cfg["normalize_xyz"],
                            trans_normalizer=tn if isinstance(tn, (int, float)) else [float(v) for v in tn],
                            rot_normalizer=cfg["rot_normalizer"], mesh_diameter=mesh_diameter if mesh_diameter is not None else 1.0)
        with torch.inference_mode():
            poses = to_device(ob_in_cams, dev).reshape(-1, 4, 4).contiguous()
            rgb_d, depth_d, xyz_d = _source(rgb, dev), to_device(depth, dev), to_device(xyz_map, dev)   # up once
            n = int(poses.shape[0])
            for _ in range(int(iteration)):
                batch = _crop_batch(0, cfg["input_resize"], poses, mesh, rgb_d, depth_d, K, cfg["crop_ratio"], xyz_d, normal_map,
                                    mesh_diameter, cfg, glctx, mesh_tensors, None, None, packed=True)
                poses = torch.empty((n, 4, 4), dtype=torch.float32, device=dev)
                for b in range(0, n, self.CHUNK):
                    e = min(b + self.CHUNK, n)
                    with torch.autocast("cuda", enabled=bool(self.amp)):
                        output = self.model(batch.A[b:e], batch.B[b:e])
                    _, trans_delta, rot_mat_delta = pose_update(output["trans"].float(), output["rot"].float(), batch.poseA[b:e],
                                                                prm, out=poses[b:e], want_deltas=True)
                    self.last_trans_update, self.last_rot_update = trans_delta, rot_mat_delta
        return poses, None


class ScorePredictor:
    """predict_score.py:117-226 around the caller's network.  cfg needs input_resize."""

    def __init__(self, model=None, cfg=None, amp=True):
        self.model = _need_model(model, "ScorePredictor", "{'score_logit'}")
        self.amp = amp
        self.cfg = _config(cfg, _SCORER_DEFAULTS, ("input_resize",), "ScorePredictor")

    def predict(self, rgb, depth, K, ob_in_cams, normal_map=None, get_vis=False, mesh=None, mesh_tensors=None, glctx=None,
                mesh_diameter=None):
        """-> (scores N float32 on the device, None).  The reference's selection loop takes the whole batch as its one
        chunk (`L = len(A)`), so its first round already leaves a single winner and every pose's score is its logit
        + 100 (predict_score.py:186-210)."""
        import torch

        _no_vis(get_vis)
        cfg = self.cfg
        dev = _frame_device(ob_in_cams, rgb, depth)
        if mesh_tensors is None:
            mesh_tensors = make_mesh_tensors(mesh)
        with torch.inference_mode():
            poses = to_device(ob_in_cams, dev).reshape(-1, 4, 4).contiguous()
            batch = _crop_batch(1, cfg["input_resize"], poses, mesh, rgb, depth, K, cfg["crop_ratio"], None, None, mesh_diameter,
                                cfg, glctx, mesh_tensors, None, None, packed=True)
            A, B = batch.A, batch.B
            global_ids = torch.arange(len(poses), device=dev, dtype=torch.long)
            scores_global = torch.zeros(len(poses), dtype=torch.float, device=dev)
            with torch.autocast("cuda", enabled=bool(self.amp)):
                output = self.model(A, B, L=len(A))
            scores = output["score_logit"].float().reshape(-1)
            scores_global[global_ids] = scores + 100
        return scores_global, None


# ---------------------------------------------------------------- the estimator

def _copy_mesh(mesh):
    return mesh.copy() if hasattr(mesh, "copy") else copy.deepcopy(mesh)


class FoundationPose:
    """estimater.py's FoundationPose.  `scorer` and `refiner` are this module's predictors (each around a network of the
    caller); `mesh` is trimesh-like (vertices, faces, vertex_normals, visual) or the package's TriangleMesh.  Debug
    dumps (debug >= 2) are not reproduced."""

    def __init__(self, model_pts, model_normals, symmetry_tfs=None, mesh=None, scorer=None, refiner=None, glctx=None, debug=0,
                 debug_dir="debug"):
        if scorer is None or refiner is None:
            raise ValueError("FoundationPose: pass scorer= and refiner= (ScorePredictor / PoseRefinePredictor around your "
                             "networks); this package holds no weights to build them from")
        if debug >= 2:
            raise NotImplementedError("debug >= 2 writes point clouds and images with open3d / cv2 / imageio")
        self.gt_pose = None     # a pose of the mesh as given (what register returns): switches the ADD lines of register on
        self.add_errs = None    # register's last ADD errors in the order of self.poses (only with gt_pose)
        self.ignore_normal_flip = True
        self.debug = debug
        self.debug_dir = debug_dir
        if debug > 0:
            os.makedirs(debug_dir, exist_ok=True)
        self.reset_object(model_pts, model_normals, symmetry_tfs=symmetry_tfs, mesh=mesh)
        self.make_rotation_grid(min_n_views=40, inplane_step=60)
        self.glctx = glctx
        self.scorer = scorer
        self.refiner = refiner
        self.pose_last = None   # for tracking; of the centred mesh

    def reset_object(self, model_pts, model_normals, symmetry_tfs=None, mesh=None):
        import torch

        if mesh is None:
            raise ValueError("FoundationPose: a mesh is required")
        verts = np.asarray(mesh.vertices)
        self.model_center = (verts.min(axis=0) + verts.max(axis=0)) / 2
        self.mesh_ori = _copy_mesh(mesh)
        mesh = _copy_mesh(mesh)
        mesh.vertices = np.asarray(mesh.vertices) - self.model_center.reshape(1, 3)
        model_pts = np.asarray(mesh.vertices)
        self.diameter = compute_mesh_diameter(model_pts=model_pts, n_sample=10000)
        self.vox_size = max(self.diameter / 20.0, 0.003)
        logging.info(f"self.diameter:{self.diameter}, vox_size:{self.vox_size}")
        self.dist_bin = self.vox_size / 2
        self.angle_bin = 20  # degrees
        pts, normals = cloud_ops.voxel_down_sample(model_pts, self.vox_size, normals=_host(model_normals))
        self.max_xyz = pts.max(axis=0)
        self.min_xyz = pts.min(axis=0)
        self.pts = torch.tensor(pts, dtype=torch.float32, device="cuda")
        self.normals = torch.nn.functional.normalize(torch.tensor(normals, dtype=torch.float32, device="cuda"), dim=-1)
        self.mesh_path = None   # the reference exports the mesh to a temporary file nothing reads
        self.mesh = mesh
        self.mesh_tensors = make_mesh_tensors(self.mesh)
        if symmetry_tfs is None:
            self.symmetry_tfs = torch.eye(4).float().cuda()[None]
        else:
            self.symmetry_tfs = torch.as_tensor(_host(symmetry_tfs), device="cuda", dtype=torch.float)
        logging.info("reset done")

    def get_tf_to_centered_mesh(self):
        import torch

        tf_to_center = torch.eye(4, dtype=torch.float, device="cuda")
        tf_to_center[:3, 3] = -torch.as_tensor(self.model_center, device="cuda", dtype=torch.float)
        return tf_to_center

    def make_rotation_grid(self, min_n_views=40, inplane_step=60):
        import torch

        grid = rotation_grid(min_n_views, inplane_step, self.symmetry_tfs.data.cpu().numpy())
        self.rot_grid = torch.as_tensor(grid, device="cuda", dtype=torch.float)
        logging.info(f"self.rot_grid: {self.rot_grid.shape}")

    def _hypotheses(self, center):
        import torch

        ob_in_cams = self.rot_grid.clone()
        ob_in_cams[:, :3, 3] = torch.as_tensor(center, device="cuda", dtype=torch.float).reshape(1, 3)
        return ob_in_cams

    def generate_random_pose_hypo(self, K, rgb, depth, mask, scene_pts=None):
        return self._hypotheses(self.guess_translation(depth=depth, mask=mask, K=K))

    def guess_translation(self, depth, mask, K):
        return guess_translation(depth, mask, K)

    def register(self, K, rgb, depth, ob_mask, ob_id=None, glctx=None, iteration=5):
        """The pose of the object in a first frame (4 x 4 numpy, of the mesh as given): every rotation of the grid at the
        guessed translation, refined and scored.  The frame goes up once; one 32-byte record comes back before the
        networks run, and the pose after them."""
        import torch

        set_seed(0)
        if self.glctx is None:
            self.glctx = glctx if glctx is not None else RasterizeCudaContext()
        dev = _frame_device(depth, rgb)
        depth = to_device(depth, dev)
        depth = erode_depth(depth, radius=2, device="cuda")
        depth = bilateral_filter_depth(depth, radius=2, device="cuda")
        rec = _stats(depth, ob_mask)
        center = _center_from(rec, K)
        if rec["n_valid"] < 4:
            logging.info("valid too small, return")
            pose = np.eye(4)
            pose[:3, 3] = center
            return pose
        self.H, self.W = (int(v) for v in depth.shape[:2])
        self.K = K
        self.ob_id = ob_id
        self.ob_mask = ob_mask
        poses = self._hypotheses(center)
        if self.gt_pose is not None:
            logging.info(f"after viewpoint, add_errs min:{self.compute_add_err_to_gt_pose(poses).min()}")
        xyz_map = depth2xyzmap(depth, K)
        poses, _ = self.refiner.predict(mesh=self.mesh, mesh_tensors=self.mesh_tensors, rgb=rgb, depth=depth, K=K, ob_in_cams=poses,
                                        normal_map=None, xyz_map=xyz_map, glctx=self.glctx, mesh_diameter=self.diameter,
                                        iteration=iteration, get_vis=False)
        scores, _ = self.scorer.predict(mesh=self.mesh, rgb=rgb, depth=depth, K=K, ob_in_cams=poses, normal_map=None,
                                        mesh_tensors=self.mesh_tensors, glctx=self.glctx, mesh_diameter=self.diameter,
                                        get_vis=False)
        ids = torch.as_tensor(scores).argsort(descending=True, stable=True)   # (the reference's sort leaves ties open)
        if self.gt_pose is not None:
            add_errs = self.compute_add_err_to_gt_pose(poses)
            logging.info(f"final, add_errs min:{add_errs.min()}")
            self.add_errs = add_errs[ids]
        scores = scores[ids]
        poses = poses[ids]
        best_pose = poses[0] @ self.get_tf_to_centered_mesh()
        self.pose_last = poses[0]
        self.best_id = ids[0]
        self.poses = poses
        self.scores = scores
        return best_pose.data.cpu().numpy()

    def compute_add_err_to_gt_pose(self, poses):
        """The ADD error (metres, float32 CUDA tensor, no host wait) of every pose of the centred mesh against
        self.gt_pose, minimised over self.symmetry_tfs; -1 for every pose while gt_pose is None (the reference's stub).
        gt_pose is a pose of the mesh as given: the ground truth of the centred mesh is gt_pose @ inv(tf_to_center),
        formed in float64 and rounded once to float32, the precision of the estimator's poses, so that a pose equal to
        it has the error 0.  The points are self.pts."""
        import torch

        if self.gt_pose is None:
            return -torch.ones(len(poses), device="cuda", dtype=torch.float)
        from .metrics import add_err_batch

        back = np.eye(4)
        back[:3, 3] = np.asarray(self.model_center, np.float32)       # inv(tf_to_center), exactly
        gt = (np.asarray(_host(self.gt_pose), np.float64).reshape(4, 4) @ back).astype(np.float32)
        poses = torch.as_tensor(poses, device="cuda", dtype=torch.float).reshape(-1, 4, 4)
        return add_err_batch(poses, gt, self.pts, symmetry_tfs=self.symmetry_tfs).float()

    def track_one(self, rgb, depth, K, iteration, extra={}):
        """The next frame's pose (4 x 4 numpy) from the last one: the depth filters, the refiner on pose_last, which
        stays on the device, and one read-back."""
        import torch

        if self.pose_last is None:
            raise RuntimeError("track_one: initialise the pose with register first")
        depth = torch.as_tensor(depth, device="cuda", dtype=torch.float) if not (is_torch(depth) and depth.is_cuda) \
            else depth.float()
        depth = erode_depth(depth, radius=2, device="cuda")
        depth = bilateral_filter_depth(depth, radius=2, device="cuda")
        Kf = np.asarray(_host(K), dtype=np.float32)
        xyz_map = depth2xyzmap_batch(depth[None], Kf[None], zfar=np.inf)[0]
        pose, _ = self.refiner.predict(mesh=self.mesh, mesh_tensors=self.mesh_tensors, rgb=rgb, depth=depth, K=K,
                                       ob_in_cams=self.pose_last.reshape(1, 4, 4), normal_map=None, xyz_map=xyz_map,
                                       mesh_diameter=self.diameter, glctx=self.glctx, iteration=iteration, get_vis=False)
        self.pose_last = pose
        return (pose @ self.get_tf_to_centered_mesh()).data.cpu().numpy().reshape(4, 4)
