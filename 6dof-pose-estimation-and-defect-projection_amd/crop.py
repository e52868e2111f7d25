"""Crop batches of FoundationPose's render-and-compare step, without kornia.

    warp_perspective                kornia.geometry.transform.warp_perspective (kornia 0.7.2), modes bilinear / nearest,
                                    padding 'zeros'; bound as `kornia = pedp_hip.compat.kornia`
    compute_crop_window_tf_batch    Utils.py:577-621, method 'box_3d'
    make_crop_data_batch            predict_pose_refine.py:26-88 with PoseRefinePairH5Dataset.transform_batch
                                    (h5_dataset.py:79-116, :210-218)
    make_score_crop_data_batch      predict_score.py:57-112 with TripletH5Dataset.transform_batch (h5_dataset.py:137-180)

The pixels come from libpedp_hip.so (csrc/pedp_crop.hip).  A crop batch is three library calls on the caller's stream
with no host wait: the crop windows (and the renderer's bbox2d), nvdiffrast_render at crop size, and one fused pass that
writes every observed-side map from the shared full-frame sources and normalises the rendered side.  The scorer's xyz
map follows its crop -> frame -> crop round trip pixel by pixel, with no frame-sized intermediate.

Torch CUDA tensors stay on their device and run on the caller's current stream, with no host wait (host arrays such
as a numpy frame are copied through page-locked memory on that stream; K is read on the host); warp_perspective and
compute_crop_window_tf_batch also take CPU tensors and numpy arrays (host memory).  The contract (maps in float64,
grid_sample's float32 sampling, the window's float32 order, K in float32) is DESIGN.md s4.9.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._bridge import as_array, as_kind, device_of, empty, is_torch, launch, ptr, to_device
from .render import nvdiffrast_render


class BatchPoseData:
    """Holder with the reference's BatchPoseData field names (learning/datasets/pose_dataset.py); pass `batch_cls` to
    make_crop_data_batch to get the reference's own class instead."""

    def __init__(self, rgbAs=None, rgbBs=None, depthAs=None, depthBs=None, normalAs=None, normalBs=None, maskAs=None,
                 maskBs=None, poseA=None, poseB=None, xyz_mapAs=None, xyz_mapBs=None, tf_to_crops=None, Ks=None,
                 crop_masks=None, model_pts=None, mesh_diameters=None, labels=None):
        self.rgbAs, self.rgbBs, self.depthAs, self.depthBs = rgbAs, rgbBs, depthAs, depthBs
        self.normalAs, self.normalBs, self.maskAs, self.maskBs = normalAs, normalBs, maskAs, maskBs
        self.poseA, self.poseB, self.xyz_mapAs, self.xyz_mapBs = poseA, poseB, xyz_mapAs, xyz_mapBs
        self.tf_to_crops, self.Ks, self.crop_masks, self.model_pts = tf_to_crops, Ks, crop_masks, model_pts
        self.mesh_diameters, self.labels = mesh_diameters, labels


# ---------------------------------------------------------------- image sources

def _source(x, dev):
    """An image source as a uint8 / float32 array on the call's side, its strides kept (expanded and permuted views
    go through without a copy)."""
    if dev is not None:
        t = to_device(x, dev, u8_ok=True)
        if any(s < 0 for s in t.stride()):
            t = t.contiguous()
        return t
    a = x.detach().cpu().numpy() if is_torch(x) else np.asarray(x)
    if a.dtype not in (np.uint8, np.float32):
        a = a.astype(np.float32)
    if any(s < 0 or s % a.itemsize for s in a.strides):
        a = np.ascontiguousarray(a)
    return a


def _strides(a):
    return tuple(a.stride()) if is_torch(a) else tuple(s // a.itemsize for s in a.strides)


def _image(a, dims):
    """pedp_image over `a`; dims names a's axes among 'NCHW' (missing ones have extent 1, stride 0)."""
    st = dict(zip(dims, _strides(a)))
    ext = dict(zip(dims, (int(v) for v in a.shape)))
    im = _lib.Image()
    im.data = ptr(a).value if ptr(a) is not None else None
    u8 = (str(a.dtype) == "torch.uint8") if is_torch(a) else a.dtype == np.uint8
    im.dtype = _lib.U8 if u8 else _lib.F32
    im.N, im.C, im.H, im.W = (ext.get(k, 1) for k in "NCHW")
    im.sn, im.sc, im.sy, im.sx = (st.get(k, 0) for k in "NCHW")
    return im


def _dsize(dsize):
    d = [int(v) for v in np.asarray(dsize).reshape(-1)]
    if len(d) != 2 or d[0] <= 0 or d[1] <= 0:
        raise _lib.PedpError(f"dsize must be (height, width) > 0, got {dsize}")
    return d[0], d[1]


# ---------------------------------------------------------------- warp_perspective

def warp_perspective(src, M, dsize, mode="bilinear", padding_mode="zeros", align_corners=True, fill_value=None):
    """kornia 0.7.2 warp_perspective: src N x C x H x W (N = B or 1; uint8 or float32, any non-negative strides),
    M B x 3 x 3 (source pixel -> destination pixel), dsize (h, w) -> B x C x h x w float32, contiguous."""
    if mode not in ("bilinear", "nearest"):
        raise NotImplementedError(f"warp_perspective: mode {mode!r}")
    if padding_mode != "zeros":
        raise NotImplementedError(f"warp_perspective: padding_mode {padding_mode!r}")
    if (is_torch(src) and src.requires_grad) or (is_torch(M) and M.requires_grad):
        raise NotImplementedError("warp_perspective: gradients are not supported")
    if len(getattr(src, "shape", ())) != 4:
        raise _lib.PedpError(f"warp_perspective: src must be N x C x H x W, got shape {tuple(getattr(src, 'shape', ()))}")
    dev = device_of(src, M)
    s = _source(src, dev)
    m = as_array(M, dev)
    if m.ndim != 3 or tuple(m.shape[1:]) != (3, 3):
        raise _lib.PedpError(f"warp_perspective: M must be B x 3 x 3, got shape {tuple(m.shape)}")
    B = int(m.shape[0])
    if int(s.shape[0]) not in (B, 1):
        raise _lib.PedpError(f"warp_perspective: {int(s.shape[0])} source images for {B} matrices")
    h, w = _dsize(dsize)
    im = _image(s, "NCHW")
    out = empty(dev, (B, int(s.shape[1]), h, w))
    launch(dev, "pedp_warp_perspective", lambda lib, hd, mem: lib.pedp_warp_perspective(
        hd, C.byref(im), ptr(m), B, h, w, 1 if mode == "nearest" else 0, int(bool(align_corners)), mem, ptr(out)))
    return as_kind(out, src)


class _Transform:
    warp_perspective = staticmethod(warp_perspective)


class _Geometry:
    transform = _Transform()


class _Kornia:
    """`import kornia` stand-in with only kornia.geometry.transform.warp_perspective: bind `kornia = pedp_hip.compat.kornia`."""
    geometry = _Geometry()


kornia = _Kornia()


# ---------------------------------------------------------------- crop windows

def _crop_window(poses, K, radius, out_w, out_h, corner, want_bbox):
    dev = device_of(poses)
    p = as_array(poses, dev).reshape(-1, 16)
    Kf = np.ascontiguousarray(np.asarray(K.detach().cpu().numpy() if is_torch(K) else K, dtype=np.float64), dtype=np.float32)
    if Kf.size != 9:
        raise _lib.PedpError("K must be 3 x 3")
    B = int(p.shape[0])
    tf = empty(dev, (B, 3, 3))
    bb = empty(dev, (B, 4)) if want_bbox else None
    launch(dev, "pedp_crop_window", lambda lib, hd, mem: lib.pedp_crop_window(
        hd, ptr(p), B, _lib._ptr(Kf), float(np.float32(radius)), int(out_w), int(out_h), float(corner[0]), float(corner[1]), mem,
        ptr(tf), ptr(bb)))
    return as_kind(tf, poses), (None if bb is None else as_kind(bb, poses))


def compute_crop_window_tf_batch(pts=None, H=None, W=None, poses=None, K=None, crop_ratio=1.2, out_size=None, rgb=None,
                                 uvs=None, method="min_box", mesh_diameter=None):
    """tf_to_crops B x 3 x 3 float32 for poses B x 4 x 4 (box_3d only): the crop square around the projected pose centre,
    radius mesh_diameter * crop_ratio / 2, scaled to out_size (w, h).  K enters as float32."""
    if method != "box_3d":
        raise NotImplementedError(f"compute_crop_window_tf_batch: method {method!r} (box_3d only)")
    if poses is None or K is None or out_size is None or mesh_diameter is None:
        raise _lib.PedpError("compute_crop_window_tf_batch: poses, K, out_size and mesh_diameter are required")
    radius = mesh_diameter * crop_ratio / 2
    tf, _ = _crop_window(poses, K, radius, out_size[0], out_size[1], (0, 0), False)
    return tf


# ---------------------------------------------------------------- crop batches

def _cfg(cfg, key, default=None):
    try:
        return cfg[key]
    except (KeyError, TypeError, AttributeError):
        return getattr(cfg, key, default)


def crop_pass(variant, tf_to_crops, poseA, K, mesh_diameter, rgb, rgb_r, xyz_r, xyz_map=None, normal_map=None, depth=None,
              normalize_xyz=False, use_normal=False, packed=False):
    """The fused pass alone (pedp_crop_batch): every B-side map and the A-side normalisation, given the windows and the
    renderer's crop-sized maps (rgb_r, xyz_r: B x h x w x 3 CUDA tensors).  Returns a dict of B x C x h x w tensors
    (rgbA, rgbB, xyzA, xyzB, normalB, depthB; None where the variant has none).  With `packed` (pedp_crop_batch_packed)
    the dict also holds the networks' inputs A = cat([rgbA, xyzA], 1) and B = cat([rgbB, xyzB], 1), B x 6 x h x w, and
    rgbA ... xyzB are views of them."""
    import torch

    scorer = variant == 1
    use_normal = bool(use_normal) and not scorer
    dev = rgb_r.device
    B, oh, ow = (int(v) for v in rgb_r.shape[:3])
    if tuple(xyz_r.shape) != (B, oh, ow, 3) or tuple(rgb_r.shape) != (B, oh, ow, 3):
        raise _lib.PedpError("rgb_r and xyz_r must be B x h x w x 3")
    rgb_r, xyz_r = as_array(rgb_r, dev), as_array(xyz_r, dev)
    tf, poseA = as_array(tf_to_crops, dev), as_array(poseA, dev)
    if tuple(tf.shape) != (B, 3, 3) or tuple(poseA.shape) != (B, 4, 4):
        raise _lib.PedpError("tf_to_crops must be B x 3 x 3 and poseA B x 4 x 4")
    s_rgb = _source(rgb, dev)
    if s_rgb.ndim != 3 or int(s_rgb.shape[2]) != 3:
        raise _lib.PedpError(f"rgb must be H x W x 3, got shape {tuple(s_rgb.shape)}")
    H, W = (int(v) for v in s_rgb.shape[:2])
    srcs = {"rgb": _image(s_rgb, "HWC")}
    keep = [s_rgb]

    def frame(name, x, C_):
        a = _source(x, dev)
        if tuple(a.shape) != ((H, W, C_) if C_ > 1 else (H, W)):
            raise _lib.PedpError(f"{name} must be {H} x {W}{' x 3' if C_ > 1 else ''}, got shape {tuple(a.shape)}")
        keep.append(a)
        srcs[name] = _image(a, "HWC" if C_ > 1 else "HW")

    if scorer:
        frame("depth", depth, 1)
    else:
        if xyz_map is None:
            raise _lib.PedpError("make_crop_data_batch: xyz_map is required")
        frame("xyz", xyz_map, 3)
        if use_normal:
            if normal_map is None:
                raise _lib.PedpError("make_crop_data_batch: cfg['use_normal'] needs normal_map")
            frame("normal", normal_map, 3)
    Kf = np.asarray(K.detach().cpu().numpy() if is_torch(K) else K, dtype=np.float64).astype(np.float32).reshape(9)
    prm = _lib.CropParams()
    prm.variant, prm.normalize_xyz, prm.use_normal, prm.B = variant, int(bool(normalize_xyz)), int(use_normal), B
    prm.H, prm.W, prm.out_h, prm.out_w = H, W, oh, ow
    prm.K[:] = Kf.tolist()
    prm.mesh_diameter = float(np.float32(mesh_diameter))
    if packed:
        out = {k: torch.empty((B, 6, oh, ow), dtype=torch.float32, device=dev) for k in ("A", "B")}
        for side in "AB":
            out["rgb" + side], out["xyz" + side] = out[side][:, :3], out[side][:, 3:]
    else:
        out = {k: torch.empty((B, 3, oh, ow), dtype=torch.float32, device=dev) for k in ("rgbA", "rgbB", "xyzA", "xyzB")}
    out["normalB"] = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=dev) if use_normal else None
    out["depthB"] = torch.empty((B, 1, oh, ow), dtype=torch.float32, device=dev) if scorer else None

    def img(k):
        return C.byref(srcs[k]) if k in srcs else None

    if packed:
        launch(dev, "pedp_crop_batch_packed", lambda lib, hd, mem: lib.pedp_crop_batch_packed(
            hd, C.byref(prm), ptr(tf), ptr(poseA), img("rgb"), img("xyz"), img("normal"), img("depth"), ptr(rgb_r),
            ptr(xyz_r), mem, ptr(out["A"]), ptr(out["B"]), ptr(out["normalB"]), ptr(out["depthB"])))
        return out
    launch(dev, "pedp_crop_batch", lambda lib, hd, mem: lib.pedp_crop_batch(
        hd, C.byref(prm), ptr(tf), ptr(poseA), img("rgb"), img("xyz"), img("normal"), img("depth"), ptr(rgb_r),
        ptr(xyz_r), mem, ptr(out["rgbA"]), ptr(out["rgbB"]), ptr(out["xyzA"]), ptr(out["xyzB"]), ptr(out["normalB"]),
        ptr(out["depthB"])))
    return out


def _crop_batch(variant, render_size, ob_in_cams, mesh, rgb, depth, K, crop_ratio, xyz_map, normal_map, mesh_diameter, cfg,
                glctx, mesh_tensors, dataset, batch_cls, packed=False):
    """The crop batch of either predictor; with `packed` the returned batch also carries the networks' inputs as `A` and
    `B` (B x 6 x h x w), of which rgbAs ... xyz_mapBs are views."""
    import torch

    if cfg is None or mesh_diameter is None:
        raise _lib.PedpError("make_crop_data_batch: cfg and mesh_diameter are required")
    ir = tuple(int(v) for v in _cfg(cfg, "input_resize"))
    rs = tuple(int(v) for v in render_size)
    if rs != ir:
        raise NotImplementedError(f"make_crop_data_batch: render size {rs} other than input_resize {ir}")
    oh, ow = rs
    use_normal = bool(_cfg(cfg, "use_normal", False))
    dcfg = getattr(dataset, "cfg", None) if dataset is not None else None
    normalize = bool(_cfg(dcfg if dcfg is not None else cfg, "normalize_xyz", False))
    H, W = (int(v) for v in depth.shape[:2])
    dev = device_of(ob_in_cams, rgb, depth, xyz_map)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    poseA = to_device(ob_in_cams, dev).reshape(-1, 4, 4).contiguous()
    B = int(poseA.shape[0])
    Kf = np.asarray(K.detach().cpu().numpy() if is_torch(K) else K, dtype=np.float64).astype(np.float32).reshape(3, 3)

    tf_to_crops, bbox2d = _crop_window(poseA, Kf, mesh_diameter * crop_ratio / 2, ow, oh, (ir[0] - 1, ir[1] - 1), True)
    extra = {}
    rgb_r, depth_r, normal_r = nvdiffrast_render(K=K, H=H, W=W, ob_in_cams=poseA, context="cuda", get_normal=use_normal,
                                                 glctx=glctx, mesh_tensors=mesh_tensors, mesh=mesh, output_size=ir,
                                                 bbox2d=bbox2d, use_light=True, extra=extra)
    xyz_r = extra["xyz_map"]

    scorer = variant == 1
    outs = crop_pass(variant, tf_to_crops, poseA, Kf, mesh_diameter, rgb, rgb_r, xyz_r, xyz_map=xyz_map, normal_map=normal_map,
                     depth=depth if scorer else None, normalize_xyz=normalize, use_normal=use_normal, packed=packed)
    rgbA, rgbB, xyzA, xyzB, normalB, depthB = (outs[k] for k in ("rgbA", "rgbB", "xyzA", "xyzB", "normalB", "depthB"))
    normalA = None
    if use_normal and not scorer:  # the reference warps the crop-sized render like a full frame (predict_pose_refine.py:74)
        normalA = warp_perspective(normal_r.permute(0, 3, 1, 2), tf_to_crops, dsize=rs, mode="nearest", align_corners=False)
    mesh_diameters = torch.ones(B, dtype=torch.float32, device=dev) * mesh_diameter
    Ks = to_device(Kf, dev).reshape(1, 3, 3)
    if scorer:
        Ks = Ks.expand(B, 3, 3)
    cls = batch_cls or BatchPoseData
    batch = cls(rgbAs=rgbA, rgbBs=rgbB, depthAs=depth_r.reshape(B, 1, oh, ow) if scorer else None, depthBs=depthB,
                normalAs=normalA, normalBs=normalB, poseA=poseA, xyz_mapAs=xyzA, xyz_mapBs=xyzB, tf_to_crops=tf_to_crops,
                Ks=Ks, mesh_diameters=mesh_diameters)
    if packed:
        batch.A, batch.B = outs["A"], outs["B"]
    return batch


def make_crop_data_batch(render_size, ob_in_cams, mesh, rgb, depth, K, crop_ratio, xyz_map, normal_map=None,
                         mesh_diameter=None, cfg=None, glctx=None, mesh_tensors=None, dataset=None, batch_cls=None):
    """The refiner's crop batch (predict_pose_refine.py:26-88) after dataset.transform_batch: rgbAs, rgbBs, xyz_mapAs,
    xyz_mapBs B x 3 x h x w, normalAs / normalBs under cfg['use_normal'], poseA, tf_to_crops, Ks, mesh_diameters.
    normalize_xyz comes from dataset.cfg (else cfg)."""
    return _crop_batch(0, render_size, ob_in_cams, mesh, rgb, depth, K, crop_ratio, xyz_map, normal_map, mesh_diameter, cfg,
                       glctx, mesh_tensors, dataset, batch_cls)


def make_score_crop_data_batch(render_size, ob_in_cams, mesh, rgb, depth, K, crop_ratio, normal_map=None, mesh_diameter=None,
                               glctx=None, mesh_tensors=None, dataset=None, cfg=None, batch_cls=None):
    """The scorer's crop batch (predict_score.py:57-112) after dataset.transform_batch: also depthAs / depthBs
    B x 1 x h x w, and xyz_mapBs through the depth round trip of TripletH5Dataset.transform_depth_to_xyzmap."""
    return _crop_batch(1, render_size, ob_in_cams, mesh, rgb, depth, K, crop_ratio, None, normal_map, mesh_diameter, cfg,
                       glctx, mesh_tensors, dataset, batch_cls)
